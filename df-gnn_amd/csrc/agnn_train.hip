// agnn_train.hip -- AGNN / dot-product attention with TIED keys and values for gfx950: fused inference and training pair (any
// graph, no plan, no degree limit).
//
// The logit of edge e = (i, j) is  s_e = beta r_i q_j <Xr_i, Xc_j>  with r, q the inverse L2 norms of the two rows (COS: AGNN,
// softmax_j(beta cos(h_i, h_j))) or 1 (dot-product attention, beta = f^-1/2), and the message is Xc_j itself.  Key and value
// of an edge are therefore ONE row up to a scalar: every pass gathers it once per edge, and the norm is taken from the
// registers that hold the row -- in the same cross-lane sweep as the dot product -- so nothing per node is precomputed,
// saved or gathered.  The structure is gatv2_train.hip's: a forward with online softmax that saves two floats per (row, head),
// a CSR pass and a CSC pass that recompute each edge, each in a wave-per-row and a lane-group-per-row form:
//   c_e  = r_i q_j <Xr_i, Xc_j>    s_e = beta c_e    P_e = exp(s_e - row_max_i) / row_sum_i    out_i = sum_e P_e Xc_j
//   dS_e = P_e (<dO_i, Xc_j> - delta_i)              g_i = sum_{e of i} dS_e c_e              g'_j = sum_{e into j} dS_e c_e
//   forward           CSR.  Xr_i and r_i in registers.  The lane-group form gathers Xc_j once per edge (dot, norm, message);
//                     the wave form works in 64-edge tiles (logits through LDS, then the weighted sum, whose gathers hit the
//                     lines the logits just brought in)
//   backward, CSR     Xr_i, dO_i in registers, Xc_j gathered once per edge: <Xr_i, Xc_j>, |Xc_j|^2 and <dO_i, Xc_j> in one
//                     sweep; dXr_i = beta r_i (sum_e dS_e q_j Xc_j - k g_i r_i Xr_i), dbeta_rows[i, h] = g_i   (k = COS)
//   backward, CSC     Xc_j, q_j in registers, Xr_i and dO_i gathered per entry plus the three row scalars, r_i from the
//                     gathered row: dXc_j = sum_e P_e dO_i + beta q_j (sum_e dS_e r_i Xr_i - k g'_j q_j Xc_j)
// dbeta[h] = sum_i g_i is the caller's column sum of dbeta_rows: no workspace, no persistent grid, no reduction kernel.
// Every output is written in full by plain stores; all sums are deterministic (no atomics).
#include "dfgnn_launch.hpp"
#include "dfgnn_rows.hpp"

namespace dfgnn {

// Everything the per-row routines need; at_head() offsets the feature pointers to the workgroup's head.
struct Agnn {
  int m, n_cols, nnz, h, f, head;          // m rows (queries, outputs) x n_cols columns (keys = values)
  size_t hf;
  float bh;                                // beta[head]
  const int *row_ptr, *col_ind;            // CSR
  const int *col_ptr, *row_ind;            // CSC (column pass)
  const float *beta;                       // [h]
  const float *Xrh, *Xch, *dOh, *Oh;       // features, output gradient, forward output (+ head * f)
  float *row_max, *row_sum, *delta;        // [m, h]: written by the forward / the CSR pass, read by the passes after
  float *dbeta_rows;                       // [m, h] or null
  float *outh, *dXrh, *dXch;               // (+ head * f)
  __device__ __forceinline__ size_t nh(int node) const { return (size_t)node * h + head; }
  __device__ __forceinline__ void at_head(int hd) {
    head = hd;
    bh = beta[hd];
    const size_t o = (size_t)hd * f;
    Xrh += o; Xch += o;
    if (dOh) dOh += o;
    if (Oh) Oh += o;
    if (outh) outh += o;
    if (dXrh) dXrh += o;
    if (dXch) dXch += o;
  }
};

// lanes_sum of N values at once: the N reductions go through ONE sweep of cross-lane steps, each step's N permutes
// independent of each other (dot product, squared norm and <dO, x> of an edge cost the latency of one reduction).
template <int W, int N>
__device__ __forceinline__ void lanes_sum_n(float (&v)[N]) {
#pragma unroll
  for (int i = 0; i < N; ++i)
    if constexpr (W >= 2) v[i] += dpp_perm<kDppXor1>(v[i]);
#pragma unroll
  for (int i = 0; i < N; ++i)
    if constexpr (W >= 4) v[i] += dpp_perm<kDppXor2>(v[i]);
#pragma unroll
  for (int i = 0; i < N; ++i)
    if constexpr (W >= 8) v[i] += dpp_perm<kDppHalfMirror>(v[i]);
#pragma unroll
  for (int i = 0; i < N; ++i)
    if constexpr (W >= 16) v[i] += dpp_perm<kDppMirror>(v[i]);
#pragma unroll
  for (int i = 0; i < N; ++i)
    if constexpr (W >= 32) v[i] += __shfl_xor(v[i], 16, kWave);
#pragma unroll
  for (int i = 0; i < N; ++i)
    if constexpr (W >= 64) v[i] += __shfl_xor(v[i], 32, kWave);
}

// 1 / max(sqrt(n2), 1e-12) (F.normalize's eps) = min(rsqrt(n2), 1e12): a row of zeros gives 1e12, not inf.
__device__ __forceinline__ float inv_norm(float n2) { return fminf(__builtin_amdgcn_rsqf(n2), 1e12f); }

// r of the row x held by one lane group (every lane gets it); 1 in dot mode, where nothing is computed.
template <class C, bool COS>
__device__ __forceinline__ float agnn_row_scale(const Frag<C> &x) {
  if constexpr (COS) return inv_norm(lanes_sum<C::G>(frag_dot<C>(x, x)));
  else return 1.f;
}

// c_e of the edge whose FIXED row is `own` (scale s_own, in registers) and whose GATHERED row is `oth`: the dot product and
// the gathered row's squared norm in one sweep.  Lanes past f hold zeros and add nothing.
template <class C, bool COS>
__device__ __forceinline__ float agnn_cos(const Frag<C> &own, float s_own, const Frag<C> &oth) {
  float v[COS ? 2 : 1];
  v[0] = frag_dot<C>(own, oth);
  if constexpr (COS) v[1] = frag_dot<C>(oth, oth);
  lanes_sum_n<C::G>(v);
  if constexpr (COS) return s_own * inv_norm(v[1]) * v[0];
  else return v[0];
}

// ... for the backward passes: also dp = <go, xc> (xc: the COLUMN row, fixed or gathered) and the gathered row's scale, all
// in the same sweep.  -> c_e
template <class C, bool COS>
__device__ __forceinline__ float agnn_cos_dp(const Frag<C> &own, float s_own, const Frag<C> &oth, const Frag<C> &go,
                                             const Frag<C> &xc, float &s_oth, float &dp) {
  float v[COS ? 3 : 2];
  v[0] = frag_dot<C>(own, oth);
  v[1] = frag_dot<C>(go, xc);
  if constexpr (COS) v[2] = frag_dot<C>(oth, oth);
  lanes_sum_n<C::G>(v);
  dp = v[1];
  if constexpr (COS) {
    s_oth = inv_norm(v[2]);
    return s_own * s_oth * v[0];
  } else {
    s_oth = 1.f;
    return v[0];
  }
}

// acc -= w x
template <class C>
__device__ __forceinline__ void frag_sub_scaled(Frag<C> &acc, float w, const Frag<C> &x) {
  frag_fma<C>(acc, -w, x);
}

// sum of a per-group scalar over the EPW groups of a wave; afterwards every group holds the total
template <class C>
__device__ __forceinline__ float groups_sum(float v) {
#pragma unroll
  for (int o = C::G; o < kWave; o <<= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// ======================================================================================================================
// forward, a wave per row: 64-edge tiles as gatv2_fwd_row_wave (sw / sc: the wave's 64-float / 64-int LDS scratch)
// ======================================================================================================================
template <class C, bool COS>
__device__ __forceinline__ void agnn_fwd_row_wave(const Agnn &a, int r, int lane, float *sw, int *sc) {
  const int gid = lane / C::G, gl = lane % C::G;
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  Frag<C> xr, acc;
  frag_load<C>(xr, a.Xrh + (size_t)r * a.hf, a.f, gl);
  frag_zero<C>(acc);
  const float ri = agnn_row_scale<C, COS>(xr);
  float m_run = -INFINITY, l_run = 0.f;
  for (int t0 = 0; t0 < deg; t0 += kWave) {
    const int nt = min(kWave, deg - t0);
    sc[lane] = (lane < nt) ? a.col_ind[lb + t0 + lane] : 0;
    wave_sync();
    int e = gid;  // the tile's logits -> sw, four gathers in flight per group (as tile_dots)
    for (; e + 3 * C::EPW < nt; e += 4 * C::EPW) {
      Frag<C> x0, x1, x2, x3;
      frag_load<C>(x0, a.Xch + (size_t)sc[e] * a.hf, a.f, gl);
      frag_load<C>(x1, a.Xch + (size_t)sc[e + C::EPW] * a.hf, a.f, gl);
      frag_load<C>(x2, a.Xch + (size_t)sc[e + 2 * C::EPW] * a.hf, a.f, gl);
      frag_load<C>(x3, a.Xch + (size_t)sc[e + 3 * C::EPW] * a.hf, a.f, gl);
      const float s0 = a.bh * agnn_cos<C, COS>(xr, ri, x0), s1 = a.bh * agnn_cos<C, COS>(xr, ri, x1);
      const float s2 = a.bh * agnn_cos<C, COS>(xr, ri, x2), s3 = a.bh * agnn_cos<C, COS>(xr, ri, x3);
      if (gl == 0) {
        sw[e] = s0;
        sw[e + C::EPW] = s1;
        sw[e + 2 * C::EPW] = s2;
        sw[e + 3 * C::EPW] = s3;
      }
    }
    for (; e < nt; e += C::EPW) {
      Frag<C> x0;
      frag_load<C>(x0, a.Xch + (size_t)sc[e] * a.hf, a.f, gl);
      const float s0 = a.bh * agnn_cos<C, COS>(xr, ri, x0);
      if (gl == 0) sw[e] = s0;
    }
    wave_sync();
    const float s = (lane < nt) ? sw[lane] : -INFINITY;
    online_step<C>(s, lane, sw, acc, m_run, l_run);
    wave_sync();
    spmm_accum<C>(acc, sw, sc, nt, a.Xch, a.hf, a.f, gid, gl);
    wave_sync();
  }
  const float inv = (l_run != 0.f) ? 1.f / l_run : 0.f;  // empty row -> 0
  frag_reduce_groups<C>(acc);
  if (gid == 0) frag_store_scaled<C>(acc, inv, a.outh + (size_t)r * a.hf, a.f, gl);
  if (lane == 0 && a.row_max) {
    a.row_max[a.nh(r)] = deg > 0 ? m_run : -1e38f;  // the sentinel of the statistics pairs (include/dfgnn.h)
    a.row_sum[a.nh(r)] = l_run;
  }
}

// ======================================================================================================================
// a group of G lanes (one feature row wide) per row / column, everything in registers, no LDS.  COOP: the row is taken by
// all EPW groups of the wave together (group gid: edges gid, gid + EPW, ...) and the partial results are merged across
// the groups -- the long rows of a low-degree graph, and EVERY row of the wave-per-row form of the two backward passes.
// ======================================================================================================================
template <class C, bool COS, bool COOP>
__device__ __forceinline__ void agnn_fwd_row_group(const Agnn &a, int r, int gid, int gl) {
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  Frag<C> xr, acc;
  frag_load<C>(xr, a.Xrh + (size_t)r * a.hf, a.f, gl);
  frag_zero<C>(acc);
  const float ri = agnn_row_scale<C, COS>(xr);
  float m_run = -INFINITY, l_run = 0.f;  // online softmax: one sweep, ONE gather per edge (key = value)
  for (int e = COOP ? gid : 0; e < deg; e += COOP ? C::EPW : 1) {
    Frag<C> xc;
    frag_load<C>(xc, a.Xch + (size_t)a.col_ind[lb + e] * a.hf, a.f, gl);
    const float s = a.bh * agnn_cos<C, COS>(xr, ri, xc);
    const float m_new = fmaxf(m_run, s);
    const float sc = (m_run == -INFINITY) ? 0.f : fast_exp(m_run - m_new);
    const float p = (s == -INFINITY) ? 0.f : fast_exp(s - m_new);
    l_run = l_run * sc + p;
    frag_scale<C>(acc, sc);
    frag_fma<C>(acc, p, xc);
    m_run = m_new;
  }
  if constexpr (COOP) {  // merge the groups' (max, sum, accumulator) states pairwise
#pragma unroll
    for (int o = C::G; o < kWave; o <<= 1) {
      const float m_o = __shfl_xor(m_run, o, kWave), l_o = __shfl_xor(l_run, o, kWave);
      const float m_new = fmaxf(m_run, m_o);
      const float sa = (m_run == -INFINITY) ? 0.f : fast_exp(m_run - m_new);
      const float sb = (m_o == -INFINITY) ? 0.f : fast_exp(m_o - m_new);
      l_run = l_run * sa + l_o * sb;
#pragma unroll
      for (int ch = 0; ch < C::NCH; ++ch)
#pragma unroll
        for (int k = 0; k < C::VEC; ++k)
          acc.v[ch][k] = acc.v[ch][k] * sa + __shfl_xor(acc.v[ch][k], o, kWave) * sb;
      m_run = m_new;
    }
  }
  if (!COOP || gid == 0) {
    frag_store_scaled<C>(acc, l_run != 0.f ? 1.f / l_run : 0.f, a.outh + (size_t)r * a.hf, a.f, gl);
    if (gl == 0 && a.row_max) {
      a.row_max[a.nh(r)] = deg > 0 ? m_run : -1e38f;
      a.row_sum[a.nh(r)] = l_run;
    }
  }
}

// CSR pass, row r: delta_r = <dO_r, out_r> -> delta; sum_e dS_e q_j Xc_j and g_r in one sweep, up to four gathers in flight
// per group; the epilogue applies beta r_r (... - k g_r r_r Xr_r).  Every lane of a group holds the edge's reductions
// (lanes_sum_n is an all-reduce), so dS_e needs no exchange.  An empty row writes zeros.
template <class C, bool COS, bool COOP>
__device__ __forceinline__ void agnn_bwd_row_group(const Agnn &a, int r, int gid, int gl) {
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  const int es = COOP ? C::EPW : 1;
  Frag<C> acc;
  frag_zero<C>(acc);
  float dl = 0.f, g = 0.f, scale = 1.f;  // empty row: dXr = 0, delta = 0, dbeta_rows = 0
  if (deg > 0) {
    Frag<C> xr, go;
    frag_load<C>(xr, a.Xrh + (size_t)r * a.hf, a.f, gl);
    frag_load<C>(go, a.dOh + (size_t)r * a.hf, a.f, gl);
    {
      Frag<C> o;
      frag_load<C>(o, a.Oh + (size_t)r * a.hf, a.f, gl);
      dl = lanes_sum<C::G>(frag_dot<C>(go, o));
    }
    const float ri = agnn_row_scale<C, COS>(xr);
    const float mx = a.row_max[a.nh(r)], inv = 1.f / a.row_sum[a.nh(r)];
    auto edge = [&](const Frag<C> &xc) {
      float qj, dp;
      const float c = agnn_cos_dp<C, COS>(xr, ri, xc, go, xc, qj, dp);
      const float ds = fast_exp(a.bh * c - mx) * inv * (dp - dl);
      frag_fma<C>(acc, COS ? ds * qj : ds, xc);
      g = fmaf(ds, c, g);
    };
    int e = COOP ? gid : 0;
    for (; e + 3 * es < deg; e += 4 * es) {  // one gather per edge: four edges in flight cost what two cost gt_bwd_row_group
      Frag<C> x0, x1, x2, x3;
      frag_load<C>(x0, a.Xch + (size_t)a.col_ind[lb + e] * a.hf, a.f, gl);
      frag_load<C>(x1, a.Xch + (size_t)a.col_ind[lb + e + es] * a.hf, a.f, gl);
      frag_load<C>(x2, a.Xch + (size_t)a.col_ind[lb + e + 2 * es] * a.hf, a.f, gl);
      frag_load<C>(x3, a.Xch + (size_t)a.col_ind[lb + e + 3 * es] * a.hf, a.f, gl);
      edge(x0);
      edge(x1);
      edge(x2);
      edge(x3);
    }
    for (; e + es < deg; e += 2 * es) {
      Frag<C> x0, x1;
      frag_load<C>(x0, a.Xch + (size_t)a.col_ind[lb + e] * a.hf, a.f, gl);
      frag_load<C>(x1, a.Xch + (size_t)a.col_ind[lb + e + es] * a.hf, a.f, gl);
      edge(x0);
      edge(x1);
    }
    for (; e < deg; e += es) {
      Frag<C> x0;
      frag_load<C>(x0, a.Xch + (size_t)a.col_ind[lb + e] * a.hf, a.f, gl);
      edge(x0);
    }
    if constexpr (COOP) {
      frag_reduce_groups<C>(acc);
      g = groups_sum<C>(g);
    }
    if constexpr (COS) frag_sub_scaled<C>(acc, g * ri, xr);
    scale = a.bh * ri;
  }
  if (!COOP || gid == 0) {
    frag_store_scaled<C>(acc, scale, a.dXrh + (size_t)r * a.hf, a.f, gl);
    if (gl == 0) {
      a.delta[a.nh(r)] = dl;
      if (a.dbeta_rows) a.dbeta_rows[a.nh(r)] = g;
    }
  }
}

// CSC pass, column j: dXc_j = sum P_e dO_i + beta q_j (sum dS_e r_i Xr_i - k g'_j q_j Xc_j) over the column's entries, two
// entries (four gathers + their row scalars) in flight per group; r_i comes from the gathered Xr_i.  An empty column
// writes zeros.
template <class C, bool COS, bool COOP>
__device__ __forceinline__ void agnn_bwd_col_group(const Agnn &a, int j, int gid, int gl) {
  const int lb = a.col_ptr[j], n = a.col_ptr[j + 1] - lb;
  const int es = COOP ? C::EPW : 1;
  Frag<C> acc;
  frag_zero<C>(acc);
  if (n > 0) {
    Frag<C> xc;
    frag_load<C>(xc, a.Xch + (size_t)j * a.hf, a.f, gl);
    const float qj = agnn_row_scale<C, COS>(xc);
    const float w = a.bh * qj;
    float g = 0.f;
    struct Entry {
      int i;
      float mx, sum, dl;
    };
    auto entry = [&](int t) {
      Entry x;
      x.i = a.row_ind[lb + t];
      const size_t s = a.nh(x.i);
      x.mx = a.row_max[s];
      x.sum = a.row_sum[s];
      x.dl = a.delta[s];
      return x;
    };
    auto accum = [&](const Entry &x, const Frag<C> &xr, const Frag<C> &gi) {
      float ri, dp;
      const float c = agnn_cos_dp<C, COS>(xc, qj, xr, gi, xc, ri, dp);
      const float p = fast_exp(a.bh * c - x.mx) * __builtin_amdgcn_rcpf(x.sum);
      const float ds = p * (dp - x.dl);
      frag_fma<C>(acc, p, gi);
      frag_fma<C>(acc, COS ? w * ds * ri : w * ds, xr);
      g = fmaf(ds, c, g);
    };
    int t = COOP ? gid : 0;
    for (; t + es < n; t += 2 * es) {
      const Entry x0 = entry(t), x1 = entry(t + es);
      Frag<C> r0, g0, r1, g1;
      frag_load<C>(r0, a.Xrh + (size_t)x0.i * a.hf, a.f, gl);
      frag_load<C>(g0, a.dOh + (size_t)x0.i * a.hf, a.f, gl);
      frag_load<C>(r1, a.Xrh + (size_t)x1.i * a.hf, a.f, gl);
      frag_load<C>(g1, a.dOh + (size_t)x1.i * a.hf, a.f, gl);
      accum(x0, r0, g0);
      accum(x1, r1, g1);
    }
    for (; t < n; t += es) {
      const Entry x0 = entry(t);
      Frag<C> r0, g0;
      frag_load<C>(r0, a.Xrh + (size_t)x0.i * a.hf, a.f, gl);
      frag_load<C>(g0, a.dOh + (size_t)x0.i * a.hf, a.f, gl);
      accum(x0, r0, g0);
    }
    if constexpr (COOP) {
      frag_reduce_groups<C>(acc);
      if constexpr (COS) g = groups_sum<C>(g);
    }
    if constexpr (COS) frag_sub_scaled<C>(acc, w * qj * g, xc);
  }
  if (!COOP || gid == 0) frag_store_scaled<C>(acc, 1.f, a.dXch + (size_t)j * a.hf, a.f, gl);
}

// ======================================================================================================================
// kernels.  PASS: 0 forward, 1 backward CSR pass, 2 backward CSC pass.
// ======================================================================================================================
template <class C, bool COS, int PASS, bool COOP>
__device__ __forceinline__ void agnn_group_pass(const Agnn &a, int r, int gid, int gl) {
  if constexpr (PASS == 0) agnn_fwd_row_group<C, COS, COOP>(a, r, gid, gl);
  else if constexpr (PASS == 1) agnn_bwd_row_group<C, COS, COOP>(a, r, gid, gl);
  else agnn_bwd_col_group<C, COS, COOP>(a, r, gid, gl);
}

// general: a wave per row / column, grid-strided over the whole graph.  The forward works in 64-edge tiles through the
// wave's LDS scratch; the backward passes are the COOP form of the group routines.
template <class C, bool COS, int PASS>
__global__ __launch_bounds__(kBlock) void agnn_wave_kernel(Agnn a) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int gid = lane / C::G, gl = lane % C::G;
  a.at_head(blockIdx.y);
  const int n = PASS == 2 ? a.n_cols : a.m;  // the extent this pass walks: rows, or (CSC pass) columns
  const int beg = blockIdx.x * kWavesPerBlock + wave, step = gridDim.x * kWavesPerBlock;
  if constexpr (PASS == 0) {
    __shared__ __attribute__((aligned(16))) float lds[kWavesPerBlock * kScratchFloatsPerWave];
    float *sw = lds + wave * kScratchFloatsPerWave;
    int *sc = reinterpret_cast<int *>(sw + kWave);
    for (int r = beg; r < n; r += step) agnn_fwd_row_wave<C, COS>(a, r, lane, sw, sc);
  } else {
    for (int r = beg; r < n; r += step) agnn_group_pass<C, COS, PASS, true>(a, r, gid, gl);
  }
}

// low-degree graphs: a workgroup takes blocks of kBlock / G consecutive rows, one lane group per row -- unless a wave's
// EPW rows include one of more than kAgnnGroupMaxDegree entries, which a single lane group would walk serially while the
// rest of the wave waits: that wave takes its rows one after the other with all its groups on each (COOP).  The choice is
// wave-uniform (ballot).  As gatv2_group_kernel.
constexpr int kAgnnGroupMaxDegree = 24;
template <class C, bool COS, int PASS>
__global__ __launch_bounds__(kBlock) void agnn_group_kernel(Agnn a) {
  constexpr int G = C::G, R = kBlock / G;  // rows per block
  const int gid = (threadIdx.x & (kWave - 1)) / G, gl = threadIdx.x % G, wave = threadIdx.x / kWave;
  a.at_head(blockIdx.y);
  const int *ptr = PASS == 2 ? a.col_ptr : a.row_ptr;
  const int n = PASS == 2 ? a.n_cols : a.m;  // the extent this pass walks: rows, or (CSC pass) columns
  for (int b0 = blockIdx.x * R; b0 < n; b0 += gridDim.x * R) {
    const int r = b0 + threadIdx.x / G;
    const int deg = r < n ? ptr[r + 1] - ptr[r] : 0;
    if (__any(deg > kAgnnGroupMaxDegree)) {
      for (int rr = b0 + wave * C::EPW; rr < min(n, b0 + (wave + 1) * C::EPW); ++rr)
        agnn_group_pass<C, COS, PASS, true>(a, rr, gid, gl);
    } else if (r < n) {
      agnn_group_pass<C, COS, PASS, false>(a, r, gid, gl);
    }
  }
}

static dim3 agnn_group_grid(int n, int h, int G) {
  const long per = kBlock / G;
  long blocks = ((long)n + per - 1) / per;
  if (blocks > 16384) blocks = 16384;
  return dim3((unsigned)(blocks < 1 ? 1 : blocks), h);
}
static dim3 agnn_wave_grid(int n, int h) {
  const long want = ((long)n + kWavesPerBlock - 1) / kWavesPerBlock;
  return dim3((unsigned)(want > (1 << 20) ? (1 << 20) : want), h);
}

template <int PASS>
static int launch_agnn_pass(const Agnn &a, bool cosine, bool v4, hipStream_t s) {
  const int n = PASS == 2 ? a.n_cols : a.m;  // the form is chosen per pass, by the average degree of what it walks
  if (n == 0) return 0;  // nothing to walk and nothing to write (a rectangular graph without rows / without columns)
  const bool groups = low_degree(n, a.nnz);
  return dispatch_cfg(a.f, v4, [&](auto cfg) {
    using C = decltype(cfg);
    auto go = [&](auto cos) {
      constexpr bool COS = decltype(cos)::value;
      if (groups) agnn_group_kernel<C, COS, PASS><<<agnn_group_grid(n, a.h, C::G), kBlock, 0, s>>>(a);
      else agnn_wave_kernel<C, COS, PASS><<<agnn_wave_grid(n, a.h), kBlock, 0, s>>>(a);
    };
    if (cosine) go(std::true_type{});
    else go(std::false_type{});
    return launch_status();
  });
}

static Agnn agnn_args(const Csr &g, const AgnnGraph &v, const float *X_row, const float *X_col) {
  Agnn a{};
  a.m = g.m; a.n_cols = g.n_cols; a.nnz = g.nnz; a.h = g.h; a.f = g.f; a.hf = (size_t)g.h * g.f;
  a.row_ptr = g.row_ptr; a.col_ind = g.col_ind; a.col_ptr = v.col_ptr; a.row_ind = v.row_ind;
  a.beta = v.beta; a.Xrh = X_row; a.Xch = X_col;
  return a;
}

int launch_agnn_fwd(const Csr &g, const AgnnGraph &v, const float *X_row, const float *X_col, float *row_max,
                    float *row_sum, float *out, hipStream_t s) {
  Agnn a = agnn_args(g, v, X_row, X_col);
  a.outh = out; a.row_max = row_max; a.row_sum = row_sum;
  const bool v4 = (g.f % 4 == 0) && aligned16(X_row) && aligned16(X_col) && aligned16(out);
  return launch_agnn_pass<0>(a, v.cosine, v4, s);
}

int launch_agnn_bwd(const Csr &g, const AgnnGraph &v, const float *X_row, const float *X_col, const float *out,
                    const float *row_max, const float *row_sum, const float *grad_out, float *delta, float *dX_row,
                    float *dX_col, float *dbeta_rows, hipStream_t s) {
  Agnn a = agnn_args(g, v, X_row, X_col);
  a.Oh = out; a.dOh = grad_out; a.delta = delta; a.dXrh = dX_row; a.dXch = dX_col; a.dbeta_rows = dbeta_rows;
  a.row_max = const_cast<float *>(row_max); a.row_sum = const_cast<float *>(row_sum);
  const bool v4 = (g.f % 4 == 0) && aligned16(X_row) && aligned16(X_col) && aligned16(out) && aligned16(grad_out) &&
                  aligned16(dX_row) && aligned16(dX_col);
  if (int rc = launch_agnn_pass<1>(a, v.cosine, v4, s)) return rc;
  return launch_agnn_pass<2>(a, v.cosine, v4, s);
}

}  // namespace dfgnn
