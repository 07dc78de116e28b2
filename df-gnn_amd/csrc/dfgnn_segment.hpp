// dfgnn_segment.hpp -- kernel bodies of the segment multi-head attention pair (segment_mha.hip, include/dfgnn_segment.h):
// every node attends to all nodes of its own graph in a batch, the "global" half of a GraphGPS-style layer.
//
// Flash-style on the matrix cores, with the numerics and operand layouts of dfgnn_dense.hpp (power-of-two-scaled fp16
// hi / lo halves, three MFMAs per product, fp32 accumulation).  The three kernels are ONE shape:
//   * a work item is an aligned 128-row window of the node array and one head; wave w owns the 16-row strip w, whose rows
//     of one or two matrices stay in registers as hi / lo operands for the whole item (SegRows);
//   * the item walks the contiguous node range its rows can see -- lo of the first row to hi of the last -- in tiles of TR
//     rows of two other matrices, staged as hi / lo images while the next tile's loads are in flight (seg_tile_loop);
//   * per tile, D^T = Image . Rows^T leaves a row of the strip on 4 lanes (dense_rows_mma), the mask lo_i <= j < hi_i
//     comes from two registers per row, and the result is the B operand of the second product (dense_cols_mma).
//              strip rows   register rows   images      first products          second products
//   forward    queries      Q               K, V        S^T = K Q^T             O^T  += V^T P^T
//   dQ         queries      Q, dO           K, V        S^T, dP^T = V dO^T      dQ^T += K^T dS^T   (after a pass for t, below)
//   dK / dV    keys         K, V            Q, dO       S = Q K^T, dP = dO V^T  dV^T += dO^T P,  dK^T += Q^T dS
// The strip side and the tile side need not be one node array: a body takes the strip side's extent and bounds, and walks
// whatever range of the other side those bounds name (the forward and dQ: m_q and the key range of each query; dK / dV: m_k
// and the query range of each key, plus the queries' own bounds for the mask).  segment_cross.hip runs them that way.
// The dK / dV kernel is the forward turned round: with the KEYS on the register side the accumulators of S and dP are
// already the B operands of dO^T P and Q^T dS, so P and dS never leave the registers (no LDS tile, no third barrier) and
// every key row is summed by one wave in a fixed order: no atomics.  It takes the row statistics, delta and the bounds
// of a tile's query rows from LDS, staged with the images.
//
// Every image has its own power-of-two scale, and dS a per-wave one.  A second product therefore goes into a zeroed
// accumulator and is added to the running one in fp32 under the product of the inverse scales: one rounding per tile
// and element, an fp32 FMA chain.  (Rescaling the running accumulator to the new tile's units instead overflows when a
// tile of dO or dS is all zero and its scale the largest normal one.)
//
// delta_i = sum_j P_ij dP_ij is formed from P and dP themselves, never from the stored `out` row; a
// row's keys may straddle two tiles however small its graph is, so the dQ kernel walks the keys twice: the first pass
// accumulates t_i in registers, the second forms dS = P (dP - t) and dQ.  See DESIGN.md 3.3k.
//
// BIAS (include/dfgnn_segment_bias.h): s_ij = scale <Q_i, K_j> + bias[head, row_off_i + j - lo_i], fp32 planes of
// packed n x n blocks.  Every bias element meets exactly one accumulator register of one lane, once per pass, so it goes
// from global memory straight into registers (no LDS): the lane of a query strip owns 4 consecutive keys of its row per
// key tile (one 16-byte load wherever the row covers all four), the lane of a key strip owns one key of four queries, whose
// offsets are staged with the other per-row words.  A pair the mask removes is never read; dbias = dS is stored by the dQ
// kernel's second pass under the same mask.  The logit is fma(S, c, b) in all four places that form one.
//
// TYPED BIAS (include/dfgnn_segment_tbias.h): b = B[min(types[row_off_i + j - lo_i], T - 1), head], one byte per
// pair shared by all heads.  The head's column of B is staged once per workgroup into LDS behind the tile (seg_table_stage);
// a lane of a query strip reads the 4 types of its 4 keys as ONE dword from a byte-aligned address (byte loads at a row's
// ends), a lane of a key strip reads one byte per query; every lookup is one LDS read.  The same fma forms the logit, so
// everything but dB equals the plane pair's bits.  dB comes from the dS registers of the dQ kernel's second pass, without
// atomics: every wave owns a table tab[T][W] in LDS, lane l adds to slot t W + (l mod W) with a plain read, add and write
// (W = 64: a slot and a bank of its own; smaller W for larger T: the 64 / W lanes of a slot take turns, a wave's DS
// operations execute in issue order), the workgroup folds slots and waves in a fixed order into one partial [T] per work
// item, and segment_tbias_reduce_kernel sums the partials of a head in a fixed order.
//
// GATES AND A LOGIT OUTPUT (include/dfgnn_segment_gate.h; instantiated in segment_gate.hip): the plane pair with
// out_i = sum_j P_ij g_ij V_j, g = sigmoid(gate), and x itself as an output whose gradient re-enters: dS = P (g dP - t) + dlogits,
// t_i = sum_j P_ij g_ij dP_ij.  Four more optional planes in the bias' layout and lane ownership (gate, logits, dlogits, dgate);
// g is multiplied into the raw product dP before its scale, so g = 1 leaves every expression -- and every bit -- of the plane pair.
#pragma once
#include "dfgnn_dense.hpp"
#include "dfgnn_launch.hpp"

namespace dfgnn {

constexpr int kSegWindow = kDenseWaves * 16;  // rows of a work item: one 16-row strip per wave
constexpr int kSegFixedLds = 2 * kDenseWaves * 4;  // the two workgroup-maximum slots

// FR: the real width (16 runs zero-padded on the 32-wide layout, as in dfgnn_dense_fwd.hpp); ROW_WORDS: staged dwords
// per tile row (dK / dV: row_max, 1 / row_sum, delta, lo, hi, and with a bias the two halves of seg_bias_at); CAP: rows * f the registers allow (dfgnn_lds_layout.hpp);
// MAXR: rows at most (dK / dV: 64 -- with 128 the narrow heads' S, dP and staged row values spill)
template <int FR, int ROW_WORDS, int CAP, int MAXR = 128>
struct SegCfg {
  static constexpr int F = FR < 32 ? 32 : FR;
  static constexpr int RS = DenseCfg<F>::RS, KT = DenseCfg<F>::KT, FT = DenseCfg<F>::FT;
  static constexpr int TR0 = segment_tile_rows(F, ROW_WORDS, kSegFixedLds, kBlockLdsBudget, CAP), TR = TR0 < MAXR ? TR0 : MAXR;
  static constexpr int NT = TR / 16, PLANE = TR * RS;
  static constexpr int kLds = kSegFixedLds + segment_tile_bytes(F, TR, ROW_WORDS);
  static_assert(TR % 32 == 0 && kLds <= kBlockLdsBudget, "a tile is whole 32-row k-blocks inside the LDS budget");
};
// the bias of a logit: none, read from a plane, looked up by the pair's type; Gated: the plane pair with a sigmoid gate on the
// attention weights and the logits as an output (below)
enum class SegKind { None, Plane, Typed, Gated };
constexpr bool seg_plane(SegKind k) { return k == SegKind::Plane || k == SegKind::Gated; }  // a bias plane is read
constexpr int kSegCapFwd = 8192, kSegCapBwd = 4096;
template <int FR> using SegFwdCfg = SegCfg<FR, 0, kSegCapFwd>;
template <int FR> using SegDqCfg = SegCfg<FR, 0, kSegCapBwd>;
template <int FR, bool BIAS = false> using SegDkvCfg = SegCfg<FR, BIAS ? 7 : 5, kSegCapBwd, 64>;  // (+ a 64-bit bias offset)

struct SegImages {
  const h16 *ahi, *alo, *bhi, *blo;
  float ainv, binv;  // 1 / scale of the two resident images
  float *rows;       // the staged per-row values, ROW_WORDS arrays of TR
};

// 16 rows of a matrix as the register operand of dense_rows_mma: lane (mi, mq) holds row `row`, features 32 t + 8 mq ..
template <int FR>
struct SegRows {
  static constexpr int KT = (FR < 32 ? 32 : FR) / 32;
  hx8 h[KT], l[KT];
  float inv;
};
template <int FR>
__device__ __forceinline__ void seg_rows_load(SegRows<FR> &x, const float *__restrict__ base, unsigned hf, int row, int m,
                                              const LaneIds &L) {
  constexpr int F = FR < 32 ? 32 : FR, KT = F / 32;
  const unsigned off = (unsigned)min(row, m - 1) * hf;
  float4 a[KT], b[KT];
  float am = 0.f;
#pragma unroll
  for (int t = 0; t < KT; ++t) {
    const bool in = FR == F || 32 * t + 8 * L.mq < FR;
    const unsigned c = in ? 32u * t + 8u * L.mq : 0u;
    a[t] = ld32_f4(base, off + c);
    b[t] = ld32_f4(base, off + c + 4);
    if (row >= m || !in) a[t] = b[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    am = fmaxf(am, absmax8(a[t], b[t]));
  }
  const Pow2Scale s = pow2_scale(wave_max(am));
  x.inv = s.inv;
#pragma unroll
  for (int t = 0; t < KT; ++t) split_hx8(a[t], b[t], s.s, x.h[t], x.l[t]);
}

// Rows [t0, t1) of A and B (row 0 at the pointers, row stride hf) in tiles of TR rows: fn(t, images) runs with rows
// t .. t + TR - 1 resident (rows at or past t1 are zero).  xload(t) issues a tile's further loads, xstore(rows) puts them
// into LDS next to the images.  Everything here is workgroup-uniform; fn may leave early per wave.
template <class C, class XL, class XS, class Fn>
__device__ __forceinline__ void seg_tile_loop(float *lds, const float *__restrict__ A, const float *__restrict__ B,
                                              unsigned hf, int t0, int t1, int fr, XL &&xload, XS &&xstore, Fn &&fn) {
  constexpr int F = C::F, TR = C::TR;
  if (t0 >= t1) return;
  float *smax = lds;
  h16 *ahi = reinterpret_cast<h16 *>(lds + 2 * kDenseWaves), *alo = ahi + C::PLANE, *bhi = alo + C::PLANE, *blo = bhi + C::PLANE;
  float *rows = reinterpret_cast<float *>(blo + C::PLANE);
  DenseStageRegs<F, TR> sa, sb;
  dense_stage_load<F, TR>(sa, A, hf, t0, t1, fr);
  dense_stage_load<F, TR>(sb, B, hf, t0, t1, fr);
  xload(t0);
  for (int t = t0; t < t1; t += TR) {
    wg_max_post(smax, dense_stage_absmax<F, TR>(sa));
    wg_max_post(smax + kDenseWaves, dense_stage_absmax<F, TR>(sb));
    lds_barrier();  // every wave is done with the previous tile
    const Pow2Scale pa = pow2_scale(wg_max_read(smax)), pb = pow2_scale(wg_max_read(smax + kDenseWaves));
    dense_stage_store<F, TR>(sa, ahi, alo, pa.s, fr);
    dense_stage_store<F, TR>(sb, bhi, blo, pb.s, fr);
    xstore(rows);
    if (t + TR < t1) {
      dense_stage_load<F, TR>(sa, A, hf, t + TR, t1, fr);
      dense_stage_load<F, TR>(sb, B, hf, t + TR, t1, fr);
      xload(t + TR);
    }
    lds_barrier();
    fn(t, SegImages{ahi, alo, bhi, blo, pa.inv, pb.inv, rows});
  }
}

// What a strip knows of itself: its rows, their bounds, and the node range any of them can see (wave-uniform).
struct SegStrip {
  int row, lo, hi;       // this lane's row (absolute) and its bounds; a row at or past m sees nothing
  int vis_lo, vis_hi;    // lo of the strip's first row, hi of its last: uniform
  bool live;             // the strip has a row below m: uniform
  // rows [a, a + len) of a tile can be seen by some row of the strip
  __device__ __forceinline__ bool sees(int a, int len) const { return live && a < vis_hi && a + len > vis_lo; }
};
__device__ __forceinline__ SegStrip seg_strip(const int *__restrict__ bounds, int m, int w0, const LaneIds &L) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const int s0 = w0 + 16 * wave;
  SegStrip s;
  s.live = s0 < m;
  s.row = s0 + L.mi;
  const int rc = min(s.row, m - 1);
  s.lo = s.row < m ? bounds[2 * rc] : 0;
  s.hi = s.row < m ? bounds[2 * rc + 1] : 0;
  s.vis_lo = __builtin_amdgcn_readfirstlane(bounds[2 * min(s0, m - 1)]);
  s.vis_hi = __builtin_amdgcn_readfirstlane(bounds[2 * min(s0 + 15, m - 1) + 1]);
  return s;
}

// ---- the pair bias ----------------------------------------------------------------------------------------------------
struct SegBias {
  const long long *row_off;  // int64[m]: offset of pair (i, lo_i) in a head's plane
  long long n_pairs;         // length of a plane
  const float *bias;         // fp32[h, n_pairs]
  float *dbias;              // (dQ kernel) fp32[h, n_pairs] or null
};
constexpr long long kSegNoBias = -0x7fffffffffffffffll - 1;  // "this row has no place in the plane"
// `at` such that element at + j of the planes is pair (row, j) for lo <= j < hi: row_off is clamped into [0, n_pairs - n],
// so whatever row_off holds, at + j stays inside the head's plane; kSegNoBias when the plane cannot hold the row at all
__device__ __forceinline__ long long seg_bias_at(const SegBias &sb, int head, int row, int lo, int hi) {
  const long long room = sb.n_pairs - (long long)(hi - lo);
  if (room < 0) return kSegNoBias;
  return (long long)head * sb.n_pairs + min(max(sb.row_off[row], 0ll), room) - lo;
}
struct __attribute__((packed, aligned(4))) SegF4U {  // 4 floats at a 4-byte aligned address: a bias row starts anywhere
  float v[4];
};
// keys j0 .. j0 + 3 of this lane's row: one 16-byte access where the row covers all four, else only the pairs in [lo, hi)
__device__ __forceinline__ f32x4 seg_bias_load4(const float *__restrict__ bias, long long at, int j0, int lo, int hi) {
  f32x4 b = {0.f, 0.f, 0.f, 0.f};
  if (at == kSegNoBias) return b;
  if (j0 >= lo && j0 + 4 <= hi) {
    const SegF4U x = *reinterpret_cast<const SegF4U *>(bias + at + j0);
    b = f32x4{x.v[0], x.v[1], x.v[2], x.v[3]};
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (j0 + r >= lo && j0 + r < hi) b[r] = bias[at + j0 + r];
  }
  return b;
}
__device__ __forceinline__ void seg_bias_store4(float *__restrict__ dbias, long long at, int j0, int lo, int hi, const f32x4 &d) {
  if (at == kSegNoBias) return;
  if (j0 >= lo && j0 + 4 <= hi) {
    *reinterpret_cast<SegF4U *>(dbias + at + j0) = SegF4U{{d[0], d[1], d[2], d[3]}};
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (j0 + r >= lo && j0 + r < hi) dbias[at + j0 + r] = d[r];
  }
}

// ---- pair gates and the logit output (SegKind::Gated) ---------------------------------------------------------------------
// The bias planes plus four more in the same layout, each optional (null: wave-uniform tests inside the Gated instances).
struct SegGate : SegBias {
  const float *gate;     // fp32[h, n_pairs] or null: g = 1
  float *dgate;          // (dQ kernel) or null
  float *logits;         // (forward) or null
  const float *dlogits;  // (backward) or null: no second stream into dS
};
// 1 / (1 + e^-x): e^-x = inf gives 0, e^-x = 0 gives 1 -- finite x of any size stays in [0, 1]
__device__ __forceinline__ float seg_sigmoid(float x) { return __builtin_amdgcn_rcpf(1.f + fast_exp(-x)); }

// ---- the typed pair bias ----------------------------------------------------------------------------------------------
constexpr int kSegMaxTypes = 256;                    // a type is a byte
constexpr int kSegTabBytes = 4 * kSegMaxTypes;       // the head's staged column of B, behind the tile of every typed kernel
constexpr int kSegWaveTabFloats = 3072;              // floats of a wave's dB table at most: T W
// slots per type of a wave's dB table: the widest power of two that keeps T W inside kSegWaveTabFloats, by T alone
constexpr int seg_tbias_slots(int T) { return T <= 48 ? 64 : T <= 96 ? 32 : T <= 192 ? 16 : 8; }
static_assert(48 * seg_tbias_slots(48) <= kSegWaveTabFloats && 96 * seg_tbias_slots(96) <= kSegWaveTabFloats &&
                  192 * seg_tbias_slots(192) <= kSegWaveTabFloats && 256 * seg_tbias_slots(256) <= kSegWaveTabFloats,
              "a wave's dB table fits its share of LDS at every threshold");
struct SegTBias {
  const long long *row_off;    // int64[m]: offset of pair (i, lo_i) in types
  long long n_pairs;           // length of types
  const unsigned char *types;  // uint8[n_pairs], one plane for all heads
  const float *table;          // B, fp32[T, h]
  int T;
  float *ws;                   // (dQ kernel) the dB partials [windows, T, h], or null: the table is frozen
  int W, wshift;               // (dQ kernel) seg_tbias_slots(T) and its log2
};
// seg_bias_at without the head: element at + j of types is pair (row, j)
__device__ __forceinline__ long long seg_types_at(const SegTBias &tb, int row, int lo, int hi) {
  const long long room = tb.n_pairs - (long long)(hi - lo);
  if (room < 0) return kSegNoBias;
  return min(max(tb.row_off[row], 0ll), room) - lo;
}
struct __attribute__((packed)) SegB4U {  // 4 bytes at any address
  unsigned v;
};
// the types of keys j0 .. j0 + 3 of this lane's row, key j0 + r in byte r: one 4-byte access where the row covers all four,
// else only the pairs in [lo, hi) (the other bytes are 0)
__device__ __forceinline__ unsigned seg_types_load4(const unsigned char *__restrict__ types, long long at, int j0, int lo, int hi) {
  unsigned x = 0;
  if (at == kSegNoBias) return x;
  if (j0 >= lo && j0 + 4 <= hi) {
    x = reinterpret_cast<const SegB4U *>(types + at + j0)->v;
  } else {
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (j0 + r >= lo && j0 + r < hi) x |= (unsigned)types[at + j0 + r] << (8 * r);
  }
  return x;
}
// the head's column of B -> tab[0 .. T); visible after the next workgroup barrier (seg_tile_loop has two before its first fn)
__device__ __forceinline__ void seg_table_stage(float *tab, const SegTBias &tb, int head, int h) {
  const int tid = opaque_tid();
  if (tid < tb.T) tab[tid] = tb.table[(size_t)tid * h + head];
}
// bias of the pair whose type is byte r of x (clamped to T - 1: no address outside tab)
__device__ __forceinline__ float seg_table_at(const float *tab, unsigned x, int r, int T) {
  return tab[min((int)((x >> (8 * r)) & 255u), T - 1)];
}
// what seg_recompute_p needs for KIND == Typed, and the tile's packed types it hands back for the dB sums
struct SegTypedLane {
  const unsigned char *types;
  const float *tab;
  int T;
  long long at;  // seg_types_at of the lane's row
};

// dB of a tile: lane l adds dS of its 4 NT pairs to slot type W + (l mod W) of its wave's table, a plain read, add and write.
// The 64 / W lanes that share a slot take turns, round after round; within a round a lane's slots are its own, and a wave's
// DS operations execute in issue order, so a round sees what the rounds before it wrote (wave_sync keeps the compiler from
// moving them).  Masked pairs hold dS = 0 and type 0: they add nothing.
template <int NT>
__device__ __forceinline__ void seg_dtable_add(float *wtab, const SegTBias &tb, const f32x4 (&dS)[NT], const unsigned (&ty)[NT],
                                               const SegStrip &st, int t, bool nobias, const LaneIds &L) {
  const int lane = L.mi + 16 * L.mq, turn = lane >> tb.wshift;
  float *mine = wtab + (lane & (tb.W - 1));
  for (int round = 0; round < (kWave >> tb.wshift); ++round) {
    if (turn == round) {
#pragma unroll
      for (int jt = 0; jt < NT; ++jt)
        if (st.sees(t + 16 * jt, 16)) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            float *p = mine + (min((int)((ty[jt] >> (8 * r)) & 255u), tb.T - 1) << tb.wshift);
            *p += nobias ? 0.f : dS[jt][r];
          }
        }
    }
    wave_sync();
  }
}
// the work item's partial: every wave folds the W slots of its types (lane l the types l, l + 64, ..: each read of a round
// hits 64 banks, the start rotated by the type), then the first T threads add the 8 waves and store [T] with stride h
__device__ __forceinline__ void seg_dtable_fold(float *tabs, const SegTBias &tb, float *__restrict__ part, int h) {
  const int tid = opaque_tid(), lane = tid & (kWave - 1), per = tb.T << tb.wshift;
  float *wtab = tabs + (tid / kWave) * per;
  wave_sync();
  for (int ty = lane; ty < tb.T; ty += kWave) {
    float s = 0.f;
    for (int w = 0; w < tb.W; ++w) s += wtab[(ty << tb.wshift) + ((w + ty) & (tb.W - 1))];
    wtab[ty << tb.wshift] = s;
  }
  lds_barrier();
  if (tid < tb.T) {
    float s = 0.f;
#pragma unroll
    for (int wv = 0; wv < kDenseWaves; ++wv) s += tabs[wv * per + (tid << tb.wshift)];
    part[(size_t)tid * h] = s;
  }
}

// accumulator tiles of a strip -> its global rows (whole lines; the padded width tile by tile)
template <int FR, int FT>
__device__ __forceinline__ void seg_store(const f32x4 (&acc)[FT], float scale, float *__restrict__ base, unsigned hf,
                                          const SegStrip &s, int m, const LaneIds &L) {
  if (!s.live) return;
  if constexpr (FR >= 32) dense_store_rows<FT>(acc, scale, base, hf, s.row, m, L);
  else if (s.row < m) dense_store_acc<FT, true>(acc, scale, base, (unsigned)s.row * hf + 4u * L.mq, false, 4 * L.mq, FR);
}

// dense_cols_mma for the NFT feature tiles from tile ft0 on
template <int F, int NFT>
__device__ __forceinline__ void seg_cols_mma(f32x4 (&acc)[NFT], const h16 *ihi, const h16 *ilo, int jb, int ft0, const f32x4 &y0,
                                             const f32x4 &y1, float yscale, const LaneIds &L) {
  constexpr int RS = DenseCfg<F>::RS;
  hx8 yh, yl;
  dense_split8(y0, y1, yscale, yh, yl);
  dense_kblock_mma<16 * NFT>(acc, ihi, ilo, (32 * jb + 4 * L.mq + L.tq) * RS + 4 * L.tp + 16 * ft0, 16 * RS, yh, yl);
}

// ---- forward ----------------------------------------------------------------------------------------------------------
template <int FR, SegKind KIND = SegKind::None, class SB = SegBias>
__device__ __forceinline__ void segment_fwd_body(float *lds, int m, int h, float scale, const int *__restrict__ bounds,
                                                 const float *__restrict__ Q, const float *__restrict__ K,
                                                 const float *__restrict__ V, float *__restrict__ out,
                                                 float *__restrict__ row_max, float *__restrict__ row_sum,
                                                 const SB &sb = SB{}) {
  using C = SegFwdCfg<FR>;
  constexpr int F = C::F, FT = C::FT, NT = C::NT, TR = C::TR;
  const int head = blockIdx.y, w0 = blockIdx.x * kSegWindow;
  const unsigned hf = (unsigned)h * FR, hoff = (unsigned)head * FR;
  const int t0 = bounds[2 * w0], t1 = bounds[2 * min(w0 + kSegWindow - 1, m - 1) + 1];
  const LaneIds L = lane_ids();
  const SegStrip st = seg_strip(bounds, m, w0, L);
  SegRows<FR> q;
  seg_rows_load<FR>(q, Q + hoff, hf, st.row, m, L);
  float mrun = -INFINITY, lrun = 0.f;
  long long bat = kSegNoBias;
  if constexpr (seg_plane(KIND))
    if (st.row < m) bat = seg_bias_at(sb, head, st.row, st.lo, st.hi);
  [[maybe_unused]] float *tab = lds + C::kLds / 4;  // (Typed) the head's column of the table
  if constexpr (KIND == SegKind::Typed) {
    if (st.row < m) bat = seg_types_at(sb, st.row, st.lo, st.hi);
    seg_table_stage(tab, sb, head, h);
  }
  f32x4 o[FT];
#pragma unroll
  for (int ft = 0; ft < FT; ++ft) o[ft] = f32x4{0.f, 0.f, 0.f, 0.f};

  seg_tile_loop<C>(lds, K + hoff, V + hoff, hf, t0, t1, FR, [](int) {}, [](float *) {}, [&](int t, const SegImages &im) {
    if (!st.sees(t, TR)) return;  // (wave-uniform: staging and barriers stay with seg_tile_loop)
    const LaneIds L = lane_ids();
    f32x4 S[NT];
    const float c = im.ainv * q.inv * scale;
    float mx = -INFINITY;
    [[maybe_unused]] f32x4 B[seg_plane(KIND) ? NT : 1];  // the tile's bias: issued ahead of the products
    if constexpr (seg_plane(KIND)) {
#pragma unroll
      for (int jt = 0; jt < NT; ++jt)
        B[jt] = st.sees(t + 16 * jt, 16) ? seg_bias_load4(sb.bias, bat, t + 16 * jt + 4 * L.mq, st.lo, st.hi) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    [[maybe_unused]] f32x4 G[KIND == SegKind::Gated ? NT : 1];  // (Gated) the tile's gate values, loaded with the bias
    [[maybe_unused]] bool gated = false;
    if constexpr (KIND == SegKind::Gated) {
      gated = sb.gate != nullptr;
      if (gated) {
#pragma unroll
        for (int jt = 0; jt < NT; ++jt)
          G[jt] = st.sees(t + 16 * jt, 16) ? seg_bias_load4(sb.gate, bat, t + 16 * jt + 4 * L.mq, st.lo, st.hi) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    [[maybe_unused]] unsigned ty[KIND == SegKind::Typed ? NT : 1];  // the tile's types, likewise; looked up under the products
    if constexpr (KIND == SegKind::Typed) {
#pragma unroll
      for (int jt = 0; jt < NT; ++jt)
        ty[jt] = st.sees(t + 16 * jt, 16) ? seg_types_load4(sb.types, bat, t + 16 * jt + 4 * L.mq, st.lo, st.hi) : 0u;
    }
#pragma unroll
    for (int jt = 0; jt < NT; ++jt) {
      const bool seen = st.sees(t + 16 * jt, 16);
      S[jt] = seen ? dense_rows_mma<F>(im.ahi, im.alo, jt, q.h, q.l, L) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = t + 16 * jt + 4 * L.mq + r;
        float s;
        if constexpr (seg_plane(KIND)) s = fmaf(S[jt][r], c, B[jt][r]);
        else if constexpr (KIND == SegKind::Typed) s = fmaf(S[jt][r], c, bat == kSegNoBias ? 0.f : seg_table_at(tab, ty[jt], r, sb.T));
        else s = S[jt][r] * c;
        if constexpr (KIND == SegKind::Gated) B[jt][r] = s;  // the logit itself, before the mask
        const float x = (seen && j >= st.lo && j < st.hi) ? s : -INFINITY;
        S[jt][r] = x;
        mx = fmaxf(mx, x);
      }
      if constexpr (KIND == SegKind::Gated) {  // logits = x, one store per valid pair (the mask of the loads)
        if (sb.logits && seen) seg_bias_store4(sb.logits, bat, t + 16 * jt + 4 * L.mq, st.lo, st.hi, B[jt]);
      }
    }
    // online softmax: the running maximum and sum of the row, the accumulators rescaled only when the maximum moved
    const float mnew = fmaxf(mrun, xor16_32_max(mx));
    const float base = (mnew == -INFINITY) ? 0.f : mnew;
    const float alpha = fast_exp(mrun - base);
    float sum = 0.f;
#pragma unroll
    for (int jt = 0; jt < NT; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float p = fast_exp(S[jt][r] - base);  // exp(-inf) = 0 for the masked pairs
        S[jt][r] = p;
        sum += p;
        if constexpr (KIND == SegKind::Gated)  // the second product takes e^{x - m} g, the row sum stays ungated
          if (gated && bat != kSegNoBias) S[jt][r] = p * seg_sigmoid(G[jt][r]);
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
#pragma unroll
    for (int jb = 0; jb < TR / 32; ++jb)
      if (st.sees(t + 32 * jb, 32)) dense_cols_mma<F>(tile, im.bhi, im.blo, jb, S[2 * jb], S[2 * jb + 1], kUnitScale, L);
    const float u = im.binv * kUnitScaleInv;
#pragma unroll
    for (int ft = 0; ft < FT; ++ft) o[ft] += tile[ft] * u;
  });

  seg_store<FR, FT>(o, lrun > 0.f ? 1.f / lrun : 0.f, out + hoff, hf, st, m, L);
  if (row_max && st.row < m && L.mq == 0) {
    row_max[(size_t)st.row * h + head] = (mrun == -INFINITY) ? -1e38f : mrun;
    row_sum[(size_t)st.row * h + head] = lrun;
  }
}

// P of this strip against the resident K tile, from the rows' saved statistics; masked pairs are 0.  dP = <dO_i, V_j>.
// (Gated) G[NT]: g of the same pairs, 1 where there is no gate (gate null, or a row without a place in the planes), and dP
// comes back as g dP: the gate is folded into the raw product before its scale, so that g = 1 leaves the plane pair's bits
template <class C, int FR, SegKind KIND = SegKind::None>
__device__ __forceinline__ void seg_recompute_p(f32x4 (&S)[C::NT], f32x4 (&dP)[C::NT], const SegImages &im, int t,
                                                const SegStrip &st, const SegRows<FR> &q, const SegRows<FR> &g, float scale,
                                                float mx, float il, const LaneIds &L, const float *__restrict__ bias = nullptr,
                                                long long bat = kSegNoBias, const SegTypedLane *tl = nullptr,
                                                unsigned *ty = nullptr, const float *__restrict__ gate = nullptr,
                                                f32x4 *G = nullptr) {
  const float c = im.ainv * q.inv * scale, cd = im.binv * g.inv;
  [[maybe_unused]] f32x4 B[seg_plane(KIND) ? C::NT : 1];  // the tile's bias: issued ahead of the products
  if constexpr (seg_plane(KIND)) {
#pragma unroll
    for (int jt = 0; jt < C::NT; ++jt)
      B[jt] = st.sees(t + 16 * jt, 16) ? seg_bias_load4(bias, bat, t + 16 * jt + 4 * L.mq, st.lo, st.hi) : f32x4{0.f, 0.f, 0.f, 0.f};
  }
  [[maybe_unused]] const bool gated = gate != nullptr && bat != kSegNoBias;
  if constexpr (KIND == SegKind::Gated) {  // the gate values with the bias; turned into g under the products
    if (gate) {
#pragma unroll
      for (int jt = 0; jt < C::NT; ++jt)
        G[jt] = st.sees(t + 16 * jt, 16) ? seg_bias_load4(gate, bat, t + 16 * jt + 4 * L.mq, st.lo, st.hi) : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  }
  if constexpr (KIND == SegKind::Typed) {  // ty[NT]: the tile's types, the caller's to keep
#pragma unroll
    for (int jt = 0; jt < C::NT; ++jt)
      ty[jt] = st.sees(t + 16 * jt, 16) ? seg_types_load4(tl->types, tl->at, t + 16 * jt + 4 * L.mq, st.lo, st.hi) : 0u;
  }
#pragma unroll
  for (int jt = 0; jt < C::NT; ++jt) {
    const bool seen = st.sees(t + 16 * jt, 16);
    S[jt] = seen ? dense_rows_mma<C::F>(im.ahi, im.alo, jt, q.h, q.l, L) : f32x4{0.f, 0.f, 0.f, 0.f};
    dP[jt] = seen ? dense_rows_mma<C::F>(im.bhi, im.blo, jt, g.h, g.l, L) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = t + 16 * jt + 4 * L.mq + r;
      float e;
      if constexpr (seg_plane(KIND)) e = fast_exp(fmaf(S[jt][r], c, B[jt][r]) - mx) * il;
      else if constexpr (KIND == SegKind::Typed)
        e = fast_exp(fmaf(S[jt][r], c, tl->at == kSegNoBias ? 0.f : seg_table_at(tl->tab, ty[jt], r, tl->T)) - mx) * il;
      else e = fast_exp(S[jt][r] * c - mx) * il;
      S[jt][r] = (seen && j >= st.lo && j < st.hi) ? e : 0.f;
      if constexpr (KIND == SegKind::Gated) {
        G[jt][r] = gated ? seg_sigmoid(G[jt][r]) : 1.f;
        dP[jt][r] *= G[jt][r];
      }
      dP[jt][r] *= cd;
    }
  }
}

// ---- dQ (and delta) ---------------------------------------------------------------------------------------------------
template <int FR, SegKind KIND = SegKind::None, class SB = SegBias>
__device__ __forceinline__ void segment_dq_body(float *lds, int m, int h, float scale, const int *__restrict__ bounds,
                                                const float *__restrict__ Q, const float *__restrict__ K,
                                                const float *__restrict__ V, const float *__restrict__ row_max,
                                                const float *__restrict__ row_sum, const float *__restrict__ dO,
                                                float *__restrict__ dQ, float *__restrict__ delta,
                                                const SB &sb = SB{}) {
  using C = SegDqCfg<FR>;
  constexpr int F = C::F, FT = C::FT, NT = C::NT, TR = C::TR;
  const int head = blockIdx.y, w0 = blockIdx.x * kSegWindow;
  const unsigned hf = (unsigned)h * FR, hoff = (unsigned)head * FR;
  const int t0 = bounds[2 * w0], t1 = bounds[2 * min(w0 + kSegWindow - 1, m - 1) + 1];
  const LaneIds L = lane_ids();
  const SegStrip st = seg_strip(bounds, m, w0, L);
  SegRows<FR> q, g;
  seg_rows_load<FR>(q, Q + hoff, hf, st.row, m, L);
  seg_rows_load<FR>(g, dO + hoff, hf, st.row, m, L);
  const size_t si = (size_t)min(st.row, m - 1) * h + head;
  const float mx = row_max[si], rs = row_sum[si], il = rs > 0.f ? 1.f / rs : 0.f;
  long long bat = kSegNoBias;
  if constexpr (seg_plane(KIND))
    if (st.row < m) bat = seg_bias_at(sb, head, st.row, st.lo, st.hi);
  // (Typed) behind the tile: the head's column of the table, then one dB table per wave, zeroed by its wave
  [[maybe_unused]] float *tab = lds + C::kLds / 4, *tabs = tab + kSegMaxTypes;
  [[maybe_unused]] SegTypedLane tl{};
  [[maybe_unused]] float *wtab = nullptr;
  if constexpr (KIND == SegKind::Typed) {
    if (st.row < m) bat = seg_types_at(sb, st.row, st.lo, st.hi);
    tl = SegTypedLane{sb.types, tab, sb.T, bat};
    seg_table_stage(tab, sb, head, h);
    if (sb.ws) {
      const int tid = opaque_tid(), per = sb.T << sb.wshift;
      wtab = tabs + (tid / kWave) * per;
      for (int k = tid & (kWave - 1); k < per; k += kWave) wtab[k] = 0.f;
    }
  }

  float tsum = 0.f;  // pass 1: t_i = sum_j P_ij dP_ij (Gated: dP is g dP from here on)
  seg_tile_loop<C>(lds, K + hoff, V + hoff, hf, t0, t1, FR, [](int) {}, [](float *) {}, [&](int t, const SegImages &im) {
    if (!st.sees(t, TR)) return;
    const LaneIds L = lane_ids();
    f32x4 S[NT], dP[NT];
    if constexpr (KIND == SegKind::Typed) {
      unsigned ty[NT];
      seg_recompute_p<C, FR, KIND>(S, dP, im, t, st, q, g, scale, mx, il, L, nullptr, kSegNoBias, &tl, ty);
    } else if constexpr (KIND == SegKind::Gated) {
      f32x4 G[NT];
      seg_recompute_p<C, FR, KIND>(S, dP, im, t, st, q, g, scale, mx, il, L, sb.bias, bat, nullptr, nullptr, sb.gate, G);
    } else {
      seg_recompute_p<C, FR, KIND>(S, dP, im, t, st, q, g, scale, mx, il, L, sb.bias, bat);
    }
#pragma unroll
    for (int jt = 0; jt < NT; ++jt)
#pragma unroll
      for (int r = 0; r < 4; ++r) tsum = fmaf(S[jt][r], dP[jt][r], tsum);
  });
  const float dl = xor16_32_sum(tsum);
  if (st.row < m && L.mq == 0) delta[si] = dl;

  f32x4 dq[FT];  // pass 2: dS = P (dP - t), dQ += dS K (Gated: dS = P (g dP - t) + dlogits)
#pragma unroll
  for (int ft = 0; ft < FT; ++ft) dq[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
  seg_tile_loop<C>(lds, K + hoff, V + hoff, hf, t0, t1, FR, [](int) {}, [](float *) {}, [&](int t, const SegImages &im) {
    if (!st.sees(t, TR)) return;
    const LaneIds L = lane_ids();
    f32x4 S[NT], dP[NT];
    [[maybe_unused]] unsigned ty[KIND == SegKind::Typed ? NT : 1];
    [[maybe_unused]] f32x4 G[KIND == SegKind::Gated ? NT : 1], DL[KIND == SegKind::Gated ? NT : 1];
    if constexpr (KIND == SegKind::Gated) {  // the second stream into dS, issued ahead of the products like the bias
      if (sb.dlogits) {
#pragma unroll
        for (int jt = 0; jt < NT; ++jt)
          DL[jt] = st.sees(t + 16 * jt, 16) ? seg_bias_load4(sb.dlogits, bat, t + 16 * jt + 4 * L.mq, st.lo, st.hi) : f32x4{0.f, 0.f, 0.f, 0.f};
      }
    }
    if constexpr (KIND == SegKind::Typed) seg_recompute_p<C, FR, KIND>(S, dP, im, t, st, q, g, scale, mx, il, L, nullptr, kSegNoBias, &tl, ty);
    else if constexpr (KIND == SegKind::Gated) seg_recompute_p<C, FR, KIND>(S, dP, im, t, st, q, g, scale, mx, il, L, sb.bias, bat, nullptr, nullptr, sb.gate, G);
    else seg_recompute_p<C, FR, KIND>(S, dP, im, t, st, q, g, scale, mx, il, L, sb.bias, bat);
    float am = 0.f;
    if constexpr (KIND == SegKind::Gated) {
      // dgate = (g dP) P (1 - g) needs dP, P and g of the same pair: stored before dS takes P's registers
      if (sb.dgate) {
#pragma unroll
        for (int jt = 0; jt < NT; ++jt)
          if (st.sees(t + 16 * jt, 16)) {
            f32x4 dg;
#pragma unroll
            for (int r = 0; r < 4; ++r) dg[r] = dP[jt][r] * S[jt][r] * (1.f - G[jt][r]);
            seg_bias_store4(sb.dgate, bat, t + 16 * jt + 4 * L.mq, st.lo, st.hi, dg);
          }
      }
      const bool second = sb.dlogits != nullptr;
#pragma unroll
      for (int jt = 0; jt < NT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          S[jt][r] *= dP[jt][r] - dl;
          if (second) S[jt][r] += DL[jt][r];  // (a masked pair loaded 0)
          am = fmaxf(am, fabsf(S[jt][r]));    // the wave's dS scale is taken with dlogits in it
        }
    } else {
#pragma unroll
      for (int jt = 0; jt < NT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          S[jt][r] *= dP[jt][r] - dl;
          am = fmaxf(am, fabsf(S[jt][r]));
        }
    }
    if constexpr (KIND == SegKind::Typed) {  // dB += dS by type, in this wave's table
      if (sb.ws) seg_dtable_add<NT>(wtab, sb, S, ty, st, t, bat == kSegNoBias, L);
    }
    if constexpr (seg_plane(KIND)) {  // dbias = dS, one store per valid pair (the mask of the loads)
      if (sb.dbias) {
#pragma unroll
        for (int jt = 0; jt < NT; ++jt)
          if (st.sees(t + 16 * jt, 16)) seg_bias_store4(sb.dbias, bat, t + 16 * jt + 4 * L.mq, st.lo, st.hi, S[jt]);
      }
    }
    const Pow2Scale ds = pow2_scale(wave_max(am));
    f32x4 tile[FT];
#pragma unroll
    for (int ft = 0; ft < FT; ++ft) tile[ft] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jb = 0; jb < TR / 32; ++jb)
      if (st.sees(t + 32 * jb, 32)) dense_cols_mma<F>(tile, im.ahi, im.alo, jb, S[2 * jb], S[2 * jb + 1], ds.s, L);
    const float u = im.ainv * ds.inv;
#pragma unroll
    for (int ft = 0; ft < FT; ++ft) dq[ft] += tile[ft] * u;
  });
  seg_store<FR, FT>(dq, scale, dQ + hoff, hf, st, m, L);
  if constexpr (KIND == SegKind::Typed) {
    if (sb.ws) seg_dtable_fold(tabs, sb, sb.ws + ((size_t)blockIdx.x * sb.T) * h + head, h);
  }
}

// ---- dK, dV -----------------------------------------------------------------------------------------------------------
// m, bounds: the strip side (the keys and, per key, the query rows that see it); tbounds: the tile side (per query row its
// key range, the mask).  One node array has one bounds array for both; the cross pair (segment_cross.hip) has two.
template <int FR, SegKind KIND = SegKind::None, class SB = SegBias>
__device__ __forceinline__ void segment_dkv_body(float *lds, int m, int h, float scale, const int *__restrict__ bounds,
                                                 const int *__restrict__ tbounds, const float *__restrict__ Q, const float *__restrict__ K,
                                                 const float *__restrict__ V, const float *__restrict__ row_max,
                                                 const float *__restrict__ row_sum, const float *__restrict__ dO,
                                                 const float *__restrict__ delta, float *__restrict__ dK,
                                                 float *__restrict__ dV, const SB &sb = SB{}) {
  using C = SegDkvCfg<FR, KIND != SegKind::None>;
  constexpr int F = C::F, FT = C::FT, NT = C::NT, TR = C::TR;
  const int head = blockIdx.y, w0 = blockIdx.x * kSegWindow;
  const unsigned hf = (unsigned)h * FR, hoff = (unsigned)head * FR;
  // the queries that see this window's keys: the graphs of its first and last key (a node's bounds are its graph)
  const int t0 = bounds[2 * w0], t1 = bounds[2 * min(w0 + kSegWindow - 1, m - 1) + 1];
  const LaneIds L = lane_ids();
  const SegStrip st = seg_strip(bounds, m, w0, L);  // (strip rows are keys here)
  SegRows<FR> k, v;
  seg_rows_load<FR>(k, K + hoff, hf, st.row, m, L);
  seg_rows_load<FR>(v, V + hoff, hf, st.row, m, L);
  f32x4 dk[FT], dv[FT];
#pragma unroll
  for (int ft = 0; ft < FT; ++ft) dk[ft] = dv[ft] = f32x4{0.f, 0.f, 0.f, 0.f};

  float xm = 0.f, xs = 0.f, xd = 0.f;  // a tile row's statistics, delta and bounds on their way to LDS (threads < TR)
  int xlo = 0, xhi = 0;
  [[maybe_unused]] long long xat = kSegNoBias;  // (with a bias) seg_bias_at / seg_types_at of the tile row: two more words
  [[maybe_unused]] float *tab = lds + C::kLds / 4;  // (Typed) the head's column of the table
  if constexpr (KIND == SegKind::Typed) seg_table_stage(tab, sb, head, h);
  auto xload = [&](int t) {
    const int tid = opaque_tid();
    if (tid < TR) {
      const int i = min(t + tid, t1 - 1);
      const size_t si = (size_t)i * h + head;
      xm = row_max[si];
      xs = row_sum[si];
      xd = delta[si];
      xlo = t + tid < t1 ? tbounds[2 * i] : 0;  // a row past the range sees nothing
      xhi = t + tid < t1 ? tbounds[2 * i + 1] : 0;
      if constexpr (seg_plane(KIND)) xat = seg_bias_at(sb, head, i, xlo, xhi);
      if constexpr (KIND == SegKind::Typed) xat = seg_types_at(sb, i, xlo, xhi);
    }
  };
  auto xstore = [&](float *rows) {
    const int tid = opaque_tid();
    if (tid < TR) {
      rows[tid] = xm;
      rows[TR + tid] = xs > 0.f ? 1.f / xs : 0.f;
      rows[2 * TR + tid] = xd;
      reinterpret_cast<int *>(rows)[3 * TR + tid] = xlo;
      reinterpret_cast<int *>(rows)[4 * TR + tid] = xhi;
      if constexpr (KIND != SegKind::None) {
        reinterpret_cast<int *>(rows)[5 * TR + tid] = (int)(unsigned)(unsigned long long)xat;
        reinterpret_cast<int *>(rows)[6 * TR + tid] = (int)(xat >> 32);
      }
    }
  };
  seg_tile_loop<C>(lds, Q + hoff, dO + hoff, hf, t0, t1, FR, xload, xstore, [&](int t, const SegImages &im) {
    if (!st.sees(t, TR)) return;
    const LaneIds L = lane_ids();
    f32x4 S[NT], dP[NT];
    const float c = im.ainv * k.inv * scale, cd = im.binv * v.inv;
    const int j = st.row;  // this lane's key; its values of tile u belong to the queries t + 16 u + 4 mq + r
    float am = 0.f;
#pragma unroll
    for (int u = 0; u < NT; ++u) {
      const bool seen = st.sees(t + 16 * u, 16);
      const int at = 16 * u + 4 * L.mq;
      [[maybe_unused]] f32x4 B = {0.f, 0.f, 0.f, 0.f};  // bias of (query at + r, key j): issued ahead of the products
      // (Gated) g and dlogits of the same pairs, single dwords like the bias: 1 and 0 where there is none
      [[maybe_unused]] f32x4 Gq = {1.f, 1.f, 1.f, 1.f}, DLq = {0.f, 0.f, 0.f, 0.f};
      [[maybe_unused]] unsigned inm = 0;  // (Gated) bit r: key j lies in the range of query at + r -- lo and hi are not kept under the products
      if constexpr (seg_plane(KIND)) {
        if (seen) {
          const int4 al = *reinterpret_cast<const int4 *>(im.rows + 5 * TR + at), ah = *reinterpret_cast<const int4 *>(im.rows + 6 * TR + at);
          const int4 lo = *reinterpret_cast<const int4 *>(im.rows + 3 * TR + at), hi = *reinterpret_cast<const int4 *>(im.rows + 4 * TR + at);
          const int alr[4] = {al.x, al.y, al.z, al.w}, ahr[4] = {ah.x, ah.y, ah.z, ah.w};
          const int lor[4] = {lo.x, lo.y, lo.z, lo.w}, hir[4] = {hi.x, hi.y, hi.z, hi.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const long long a = (long long)(((unsigned long long)(unsigned)ahr[r] << 32) | (unsigned)alr[r]);
            if constexpr (KIND == SegKind::Gated) inm |= (j >= lor[r] && j < hir[r]) ? 1u << r : 0u;
            if (a != kSegNoBias && j >= lor[r] && j < hir[r]) {
              B[r] = sb.bias[a + j];
              if constexpr (KIND == SegKind::Gated) {
                if (sb.gate) Gq[r] = seg_sigmoid(sb.gate[a + j]);
                if (sb.dlogits) DLq[r] = sb.dlogits[a + j];
              }
            }
          }
        }
      }
      [[maybe_unused]] int tyq[4] = {-1, -1, -1, -1};  // (Typed) type of (query at + r, key j), -1 where there is none
      if constexpr (KIND == SegKind::Typed) {
        if (seen) {
          const int4 al = *reinterpret_cast<const int4 *>(im.rows + 5 * TR + at), ah = *reinterpret_cast<const int4 *>(im.rows + 6 * TR + at);
          const int4 lo = *reinterpret_cast<const int4 *>(im.rows + 3 * TR + at), hi = *reinterpret_cast<const int4 *>(im.rows + 4 * TR + at);
          const int alr[4] = {al.x, al.y, al.z, al.w}, ahr[4] = {ah.x, ah.y, ah.z, ah.w};
          const int lor[4] = {lo.x, lo.y, lo.z, lo.w}, hir[4] = {hi.x, hi.y, hi.z, hi.w};
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const long long a = (long long)(((unsigned long long)(unsigned)ahr[r] << 32) | (unsigned)alr[r]);
            if (a != kSegNoBias && j >= lor[r] && j < hir[r]) tyq[r] = sb.types[a + j];
          }
        }
      }
      S[u] = seen ? dense_rows_mma<F>(im.ahi, im.alo, u, k.h, k.l, L) : f32x4{0.f, 0.f, 0.f, 0.f};
      dP[u] = seen ? dense_rows_mma<F>(im.bhi, im.blo, u, v.h, v.l, L) : f32x4{0.f, 0.f, 0.f, 0.f};
      if constexpr (KIND == SegKind::Typed) {
#pragma unroll
        for (int r = 0; r < 4; ++r) B[r] = tyq[r] < 0 ? 0.f : tab[min(tyq[r], sb.T - 1)];
      }
      const float4 mx = *reinterpret_cast<const float4 *>(im.rows + at), il = *reinterpret_cast<const float4 *>(im.rows + TR + at),
                   dl = *reinterpret_cast<const float4 *>(im.rows + 2 * TR + at);
      const int4 lo = *reinterpret_cast<const int4 *>(im.rows + 3 * TR + at), hi = *reinterpret_cast<const int4 *>(im.rows + 4 * TR + at);
      const float mxr[4] = {mx.x, mx.y, mx.z, mx.w}, ilr[4] = {il.x, il.y, il.z, il.w}, dlr[4] = {dl.x, dl.y, dl.z, dl.w};
      const int lor[4] = {lo.x, lo.y, lo.z, lo.w}, hir[4] = {hi.x, hi.y, hi.z, hi.w};
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float e;
        if constexpr (KIND != SegKind::None) e = fast_exp(fmaf(S[u][r], c, B[r]) - mxr[r]) * ilr[r];
        else e = fast_exp(S[u][r] * c - mxr[r]) * ilr[r];
        bool in;
        if constexpr (KIND == SegKind::Gated) in = (inm >> r) & 1u;  // (set only where seen)
        else in = seen && j >= lor[r] && j < hir[r];
        const float p = in ? e : 0.f;
        float ds;
        if constexpr (KIND == SegKind::Gated) {  // dV takes P g, dK the whole dS = P (g dP - t) + dlogits; g folded as in seg_recompute_p
          ds = p * ((dP[u][r] * Gq[r]) * cd - dlr[r]) + DLq[r];
          S[u][r] = p * Gq[r];
        } else {
          ds = p * (dP[u][r] * cd - dlr[r]);
          S[u][r] = p;
        }
        dP[u][r] = ds;
        am = fmaxf(am, fabsf(ds));
      }
    }
    const Pow2Scale dsc = pow2_scale(wave_max(am));
    const float uv = im.binv * kUnitScaleInv, uk = im.ainv * dsc.inv;
    // the widest head takes the feature tiles in two halves: dk, dv and a whole tile[] next to the K and V operands do not fit
    constexpr int PARTS = F == 128 ? 2 : 1, PT = FT / PARTS;
#pragma unroll
    for (int part = 0; part < PARTS; ++part) {
      f32x4 tile[PT];
#pragma unroll
      for (int k = 0; k < PT; ++k) tile[k] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ib = 0; ib < TR / 32; ++ib)
        if (st.sees(t + 32 * ib, 32)) seg_cols_mma<F, PT>(tile, im.bhi, im.blo, ib, part * PT, S[2 * ib], S[2 * ib + 1], kUnitScale, L);
#pragma unroll
      for (int k = 0; k < PT; ++k) {
        dv[part * PT + k] += tile[k] * uv;
        tile[k] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int ib = 0; ib < TR / 32; ++ib)
        if (st.sees(t + 32 * ib, 32)) seg_cols_mma<F, PT>(tile, im.ahi, im.alo, ib, part * PT, dP[2 * ib], dP[2 * ib + 1], dsc.s, L);
#pragma unroll
      for (int k = 0; k < PT; ++k) dk[part * PT + k] += tile[k] * uk;
    }
  });
  seg_store<FR, FT>(dv, 1.f, dV + hoff, hf, st, m, L);
  seg_store<FR, FT>(dk, scale, dK + hoff, hf, st, m, L);
}

}  // namespace dfgnn
