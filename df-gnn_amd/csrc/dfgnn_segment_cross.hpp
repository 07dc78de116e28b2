// dfgnn_segment_cross.hpp -- the SPLIT form of the segment cross attention pair (segment_cross.hip,
// include/dfgnn_segment_cross.h): few queries against many keys.
//
// The wide form is the three bodies of dfgnn_segment.hpp with the strip side (extent, bounds) and the tile side given apart.
// Its work item is a 128-row query window: one seed query per graph puts 128 graphs into a window, 1024 graphs with 4 heads
// make 32 workgroups, and each wave computes on the one graph in eight that its strip of the staged keys belongs to.
//
// Here a work item is ONE aligned 16-row query strip and a head, and the workgroup is kSplitWaves = 4 waves that ALL hold
// those 16 rows (and their dO rows in the dQ kernel) as register operands.  The workgroup stages tiles of K and V the way
// seg_tile_loop does -- hi / lo images, own power-of-two scales, the next tile's loads in flight -- at a height of
// kSplitTR = 32 kSplitWaves rows, so that wave w owns the 32-row k-block w of every tile: the block of dense_cols_mma.  A
// wave runs the ordinary per-block step on its share (S, mask, online softmax, O += V^T P^T into a private (m, l, O)); the
// tile loop has the two barriers per tile of seg_tile_loop and nothing else.  After the loop the waves' partial states go
// through LDS (the tile area is free by then) and wave 0 merges them in wave order: m = max_w m_w, one rescale by
// exp(m_w - m) per wave, the sums, one store of out and the statistics.
//
// dQ keeps the two passes of DESIGN.md 3.3k: pass 1 leaves a partial t_i per wave, summed in wave order through LDS and
// read back by every wave; pass 2 forms dS = P (dP - t) and a partial dQ per wave, merged like O (plain sums: P comes from
// the saved statistics, no running maximum is involved).  No atomics, and the summation order is fixed by the wave index.
#pragma once
#include "dfgnn_segment.hpp"

namespace dfgnn {

constexpr int kSplitWaves = 4, kSplitThreads = kSplitWaves * kWave;
constexpr int kSplitTR = 32 * kSplitWaves;        // tile rows: a 32-row k-block per wave
constexpr int kSplitFixedLds = 2 * kSplitWaves * 4;  // the two workgroup-maximum slots

template <int FR>
struct SplitCfg {
  static constexpr int F = FR < 32 ? 32 : FR;
  static constexpr int RS = DenseCfg<F>::RS, KT = DenseCfg<F>::KT, FT = DenseCfg<F>::FT;
  static constexpr int TR = kSplitTR, PLANE = TR * RS;
  static constexpr int PER = TR * (F / 8) / kSplitThreads;  // 8-float pieces per thread and staged matrix
  static constexpr int kLds = kSplitFixedLds + segment_tile_bytes(F, TR, 0);
  // the merge: per wave (m, l) and FT accumulator tiles of every lane, in the tile area
  static constexpr int kMergeFloats = kSplitWaves * (2 + 4 * FT) * kWave;
  static_assert(TR * (F / 8) % kSplitThreads == 0, "every thread stages whole pieces");
  static_assert(kLds <= kBlockLdsBudget && kLds % 16 == 0 && kSplitFixedLds % 16 == 0, "the tile fits, images 16-byte aligned");
  static_assert(kMergeFloats * 4 <= segment_tile_bytes(F, TR, 0), "the partial states fit the tile area");
};

// dense_stage_load / _absmax / _store for kSplitThreads threads: TR rows x F features, global -> registers -> hi / lo image
template <int FR>
struct SplitStageRegs {
  float4 a[SplitCfg<FR>::PER], b[SplitCfg<FR>::PER];
  int row0, row_end;
};
template <int FR>
__device__ __forceinline__ void split_stage_load(SplitStageRegs<FR> &r, const float *__restrict__ src, unsigned hf, int row0,
                                                 int row_end) {
  using C = SplitCfg<FR>;
  constexpr int C8 = C::F / 8;
  const int tid = opaque_tid();
  r.row0 = row0;
  r.row_end = row_end;
#pragma unroll
  for (int k = 0; k < C::PER; ++k) {
    const int idx = tid + k * kSplitThreads;
    const int row = idx / C8, c8 = idx % C8;
    // (clamped to the last valid row; a piece past the real width reads the row's first piece: both are zeroed at the store)
    const unsigned off = (unsigned)min(row0 + row, row_end - 1) * hf + ((FR >= C::F || 8 * c8 < FR) ? 8u * c8 : 0u);
    r.a[k] = ld32_f4(src, off);
    r.b[k] = ld32_f4(src, off + 4);
  }
}
template <int FR>
__device__ __forceinline__ float split_stage_absmax(const SplitStageRegs<FR> &r) {
  float m = 0.f;
#pragma unroll
  for (int k = 0; k < SplitCfg<FR>::PER; ++k) m = fmaxf(m, absmax8(r.a[k], r.b[k]));
  return m;
}
template <int FR>
__device__ __forceinline__ void split_stage_store(const SplitStageRegs<FR> &r, h16 *hi, h16 *lo, float scale) {
  using C = SplitCfg<FR>;
  constexpr int C8 = C::F / 8;
  const int tid = opaque_tid();
#pragma unroll
  for (int k = 0; k < C::PER; ++k) {
    const int idx = tid + k * kSplitThreads;
    const int row = idx / C8, c8 = idx - row * C8;
    const bool valid = r.row0 + row < r.row_end && (FR >= C::F || 8 * c8 < FR);
    const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
    hx8 h, l;
    split_hx8(valid ? r.a[k] : z, valid ? r.b[k] : z, scale, h, l);
    *reinterpret_cast<hx8 *>(hi + row * C::RS + 8 * c8) = h;
    *reinterpret_cast<hx8 *>(lo + row * C::RS + 8 * c8) = l;
  }
  asm volatile("" ::: "memory");  // (as dense_stage_store: the next prefetch is not interleaved with these stores)
}
// wg_max_post / wg_max_read over kSplitWaves slots
__device__ __forceinline__ void split_max_post(float *slot, float v) {
  v = wave_max(v);
  if ((threadIdx.x & (kWave - 1)) == 0) slot[threadIdx.x / kWave] = v;
}
__device__ __forceinline__ float split_max_read(const float *slot) {
  static_assert(kSplitWaves == 4, "one 16-byte read");
  const float4 a = *reinterpret_cast<const float4 *>(slot);
  return fmaxf(fmaxf(a.x, a.y), fmaxf(a.z, a.w));
}

// seg_tile_loop for the split workgroup: rows [t0, t1) of A and B in tiles of kSplitTR rows, fn(t, images) with rows
// t .. t + TR - 1 resident (rows at or past t1 are zero).  Workgroup-uniform; fn may leave early per wave.
template <int FR, class Fn>
__device__ __forceinline__ void split_tile_loop(float *lds, const float *__restrict__ A, const float *__restrict__ B, unsigned hf,
                                                int t0, int t1, Fn &&fn) {
  using C = SplitCfg<FR>;
  constexpr int TR = C::TR;
  if (t0 >= t1) return;
  float *smax = lds;
  h16 *ahi = reinterpret_cast<h16 *>(lds + 2 * kSplitWaves), *alo = ahi + C::PLANE, *bhi = alo + C::PLANE, *blo = bhi + C::PLANE;
  SplitStageRegs<FR> sa, sb;
  split_stage_load<FR>(sa, A, hf, t0, t1);
  split_stage_load<FR>(sb, B, hf, t0, t1);
  for (int t = t0; t < t1; t += TR) {
    split_max_post(smax, split_stage_absmax<FR>(sa));
    split_max_post(smax + kSplitWaves, split_stage_absmax<FR>(sb));
    lds_barrier();  // every wave is done with the previous tile
    const Pow2Scale pa = pow2_scale(split_max_read(smax)), pb = pow2_scale(split_max_read(smax + kSplitWaves));
    split_stage_store<FR>(sa, ahi, alo, pa.s);
    split_stage_store<FR>(sb, bhi, blo, pb.s);
    if (t + TR < t1) {
      split_stage_load<FR>(sa, A, hf, t + TR, t1);
      split_stage_load<FR>(sb, B, hf, t + TR, t1);
    }
    lds_barrier();
    fn(t, SegImages{ahi, alo, bhi, blo, pa.inv, pb.inv, nullptr});
  }
}

// the strip of a split work item: the same 16 rows in every wave; its visible range is the whole walk [t0, t1)
__device__ __forceinline__ SegStrip split_strip(const int *__restrict__ qbounds, int m_q, int s0, int t0, int t1, const LaneIds &L) {
  SegStrip s;
  s.live = true;  // (the grid has no strip at or past m_q)
  s.row = s0 + L.mi;
  const int rc = min(s.row, m_q - 1);
  s.lo = s.row < m_q ? qbounds[2 * rc] : 0;
  s.hi = s.row < m_q ? qbounds[2 * rc + 1] : 0;
  s.vis_lo = t0;
  s.vis_hi = t1;
  return s;
}

// ---- the merge --------------------------------------------------------------------------------------------------------
// Every wave puts its accumulator tiles (and two per-row words x, y) into LDS; wave 0 reads them back in wave order.
// part(w): wave w's area, [2 + 4 FT][kWave] floats; lane-major inside a word so that every access is conflict-free.
template <int FT>
__device__ __forceinline__ void split_post(float *area, int wave, const f32x4 (&acc)[FT], float x, float y) {
  const int lane = threadIdx.x & (kWave - 1);
  float *p = area + wave * (2 + 4 * FT) * kWave + lane;
  p[0] = x;
  p[kWave] = y;
#pragma unroll
  for (int ft = 0; ft < FT; ++ft)
#pragma unroll
    for (int r = 0; r < 4; ++r) p[(2 + 4 * ft + r) * kWave] = acc[ft][r];
}
__device__ __forceinline__ const float *split_part(const float *area, int w, int FT) {
  return area + w * (2 + 4 * FT) * kWave + (threadIdx.x & (kWave - 1));
}

// ---- forward ----------------------------------------------------------------------------------------------------------
template <int FR>
__device__ __forceinline__ void segment_split_fwd_body(float *lds, int m_q, int h, float scale, const int *__restrict__ qbounds,
                                                       const float *__restrict__ Q, const float *__restrict__ K,
                                                       const float *__restrict__ V, float *__restrict__ out,
                                                       float *__restrict__ row_max, float *__restrict__ row_sum) {
  using C = SplitCfg<FR>;
  constexpr int F = C::F, FT = C::FT;
  const int head = blockIdx.y, s0 = blockIdx.x * 16;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const unsigned hf = (unsigned)h * FR, hoff = (unsigned)head * FR;
  const int t0 = qbounds[2 * s0], t1 = qbounds[2 * min(s0 + 15, m_q - 1) + 1];
  const LaneIds L = lane_ids();
  const SegStrip st = split_strip(qbounds, m_q, s0, t0, t1, L);
  SegRows<FR> q;
  seg_rows_load<FR>(q, Q + hoff, hf, st.row, m_q, L);
  float mrun = -INFINITY, lrun = 0.f;
  f32x4 o[FT];
#pragma unroll
  for (int ft = 0; ft < FT; ++ft) o[ft] = f32x4{0.f, 0.f, 0.f, 0.f};

  split_tile_loop<FR>(lds, K + hoff, V + hoff, hf, t0, t1, [&](int t, const SegImages &im) {
    const int b0 = t + 32 * wave;  // this wave's k-block of the tile
    if (!st.sees(b0, 32)) return;
    const LaneIds L = lane_ids();
    f32x4 S[2];
    const float c = im.ainv * q.inv * scale;
    float mx = -INFINITY;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const bool seen = st.sees(b0 + 16 * u, 16);
      S[u] = seen ? dense_rows_mma<F>(im.ahi, im.alo, 2 * wave + u, q.h, q.l, L) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = b0 + 16 * u + 4 * L.mq + r;
        const float x = (seen && j >= st.lo && j < st.hi) ? S[u][r] * c : -INFINITY;
        S[u][r] = x;
        mx = fmaxf(mx, x);
      }
    }
    const float mnew = fmaxf(mrun, xor16_32_max(mx));
    const float base = (mnew == -INFINITY) ? 0.f : mnew;
    const float alpha = fast_exp(mrun - base);
    float sum = 0.f;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = fast_exp(S[u][r] - base);  // exp(-inf) = 0 for the masked pairs
        S[u][r] = p;
        sum += p;
      }
    lrun = lrun * alpha + xor16_32_sum(sum);
    mrun = mnew;
    if (__builtin_amdgcn_ballot_w64(alpha != 1.f)) {
#pragma unroll
      for (int ft = 0; ft < FT; ++ft) o[ft] *= alpha;
    }
    f32x4 tile[FT];
#pragma unroll
    for (int ft = 0; ft < FT; ++ft) tile[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
    dense_cols_mma<F>(tile, im.bhi, im.blo, wave, S[0], S[1], kUnitScale, L);
    const float u = im.binv * kUnitScaleInv;
#pragma unroll
    for (int ft = 0; ft < FT; ++ft) o[ft] += tile[ft] * u;
  });

  // merge the waves' (m, l, O) in wave order
  float *area = lds + 2 * kSplitWaves;
  lds_barrier();  // the last tile is free
  split_post<FT>(area, wave, o, mrun, lrun);
  lds_barrier();
  if (wave != 0) return;
  float mw[kSplitWaves], mall = -INFINITY;
#pragma unroll
  for (int w = 0; w < kSplitWaves; ++w) {
    mw[w] = split_part(area, w, FT)[0];
    mall = fmaxf(mall, mw[w]);
  }
  const float base = (mall == -INFINITY) ? 0.f : mall;
  float lall = 0.f;
#pragma unroll
  for (int ft = 0; ft < FT; ++ft) o[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int w = 0; w < kSplitWaves; ++w) {
    const float *p = split_part(area, w, FT);
    const float a = fast_exp(mw[w] - base);  // 0 for a wave that saw nothing
    lall = fmaf(p[kWave], a, lall);
#pragma unroll
    for (int ft = 0; ft < FT; ++ft)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[ft][r] = fmaf(p[(2 + 4 * ft + r) * kWave], a, o[ft][r]);
  }
  seg_store<FR, FT>(o, lall > 0.f ? 1.f / lall : 0.f, out + hoff, hf, st, m_q, L);
  if (row_max && st.row < m_q && L.mq == 0) {
    row_max[(size_t)st.row * h + head] = (mall == -INFINITY) ? -1e38f : mall;
    row_sum[(size_t)st.row * h + head] = lall;
  }
}

// P and dP of this wave's k-block of the resident tile, from the rows' saved statistics; masked pairs are 0
template <int FR>
__device__ __forceinline__ void split_recompute_p(f32x4 (&S)[2], f32x4 (&dP)[2], const SegImages &im, int b0, int wave,
                                                  const SegStrip &st, const SegRows<FR> &q, const SegRows<FR> &g, float scale,
                                                  float mx, float il, const LaneIds &L) {
  constexpr int F = SplitCfg<FR>::F;
  const float c = im.ainv * q.inv * scale, cd = im.binv * g.inv;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const bool seen = st.sees(b0 + 16 * u, 16);
    S[u] = seen ? dense_rows_mma<F>(im.ahi, im.alo, 2 * wave + u, q.h, q.l, L) : f32x4{0.f, 0.f, 0.f, 0.f};
    dP[u] = seen ? dense_rows_mma<F>(im.bhi, im.blo, 2 * wave + u, g.h, g.l, L) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = b0 + 16 * u + 4 * L.mq + r;
      const float e = fast_exp(S[u][r] * c - mx) * il;
      S[u][r] = (seen && j >= st.lo && j < st.hi) ? e : 0.f;
      dP[u][r] *= cd;
    }
  }
}

// ---- dQ (and delta) ---------------------------------------------------------------------------------------------------
template <int FR>
__device__ __forceinline__ void segment_split_dq_body(float *lds, int m_q, int h, float scale, const int *__restrict__ qbounds,
                                                      const float *__restrict__ Q, const float *__restrict__ K,
                                                      const float *__restrict__ V, const float *__restrict__ row_max,
                                                      const float *__restrict__ row_sum, const float *__restrict__ dO,
                                                      float *__restrict__ dQ, float *__restrict__ delta) {
  using C = SplitCfg<FR>;
  constexpr int F = C::F, FT = C::FT;
  const int head = blockIdx.y, s0 = blockIdx.x * 16;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const unsigned hf = (unsigned)h * FR, hoff = (unsigned)head * FR;
  const int t0 = qbounds[2 * s0], t1 = qbounds[2 * min(s0 + 15, m_q - 1) + 1];
  const LaneIds L = lane_ids();
  const SegStrip st = split_strip(qbounds, m_q, s0, t0, t1, L);
  SegRows<FR> q, g;
  seg_rows_load<FR>(q, Q + hoff, hf, st.row, m_q, L);
  seg_rows_load<FR>(g, dO + hoff, hf, st.row, m_q, L);
  const size_t si = (size_t)min(st.row, m_q - 1) * h + head;
  const float mx = row_max[si], rs = row_sum[si], il = rs > 0.f ? 1.f / rs : 0.f;
  float *area = lds + 2 * kSplitWaves;

  float tsum = 0.f;  // pass 1: this wave's share of t_i = sum_j P_ij dP_ij
  split_tile_loop<FR>(lds, K + hoff, V + hoff, hf, t0, t1, [&](int t, const SegImages &im) {
    const int b0 = t + 32 * wave;
    if (!st.sees(b0, 32)) return;
    const LaneIds L = lane_ids();
    f32x4 S[2], dP[2];
    split_recompute_p<FR>(S, dP, im, b0, wave, st, q, g, scale, mx, il, L);
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) tsum = fmaf(S[u][r], dP[u][r], tsum);
  });
  // the waves' shares in wave order, read back by every wave (the same sum in all of them)
  lds_barrier();
  area[wave * kWave + (threadIdx.x & (kWave - 1))] = xor16_32_sum(tsum);
  lds_barrier();
  float dl = 0.f;
#pragma unroll
  for (int w = 0; w < kSplitWaves; ++w) dl += area[w * kWave + (threadIdx.x & (kWave - 1))];
  if (wave == 0 && st.row < m_q && L.mq == 0) delta[si] = dl;
  // (pass 2 writes the tile area only behind the first barrier of its loop: every wave has read its sum by then)

  f32x4 dq[FT];  // pass 2: dS = P (dP - t), this wave's share of dQ += dS K
#pragma unroll
  for (int ft = 0; ft < FT; ++ft) dq[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
  split_tile_loop<FR>(lds, K + hoff, V + hoff, hf, t0, t1, [&](int t, const SegImages &im) {
    const int b0 = t + 32 * wave;
    if (!st.sees(b0, 32)) return;
    const LaneIds L = lane_ids();
    f32x4 S[2], dP[2];
    split_recompute_p<FR>(S, dP, im, b0, wave, st, q, g, scale, mx, il, L);
    float am = 0.f;
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        S[u][r] *= dP[u][r] - dl;
        am = fmaxf(am, fabsf(S[u][r]));
      }
    const Pow2Scale ds = pow2_scale(wave_max(am));
    f32x4 tile[FT];
#pragma unroll
    for (int ft = 0; ft < FT; ++ft) tile[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
    dense_cols_mma<F>(tile, im.ahi, im.alo, wave, S[0], S[1], ds.s, L);
    const float u = im.ainv * ds.inv;
#pragma unroll
    for (int ft = 0; ft < FT; ++ft) dq[ft] += tile[ft] * u;
  });

  lds_barrier();
  split_post<FT>(area, wave, dq, 0.f, 0.f);
  lds_barrier();
  if (wave != 0) return;
#pragma unroll
  for (int ft = 0; ft < FT; ++ft) dq[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int w = 0; w < kSplitWaves; ++w) {
    const float *p = split_part(area, w, FT);
#pragma unroll
    for (int ft = 0; ft < FT; ++ft)
#pragma unroll
      for (int r = 0; r < 4; ++r) dq[ft][r] += p[(2 + 4 * ft + r) * kWave];
  }
  seg_store<FR, FT>(dq, scale, dQ + hoff, hf, st, m_q, L);
}

}  // namespace dfgnn
