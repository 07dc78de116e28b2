// gt_bias_train.hip -- GT conv with a per-edge, per-head ADDITIVE attention bias for gfx950: fused inference and training
// pair, general kernels (any graph, no plan, no degree limit).  The logit of every other GT operator here is
// val_e <Q_i, K_j>; this one adds a scalar per (head, edge) before the softmax -- Graphormer's spatial / edge encodings,
// GraphGPS / GRIT-style attention, any relative positional or edge-type bias, and (bias = -inf) an attention mask:
//   s_e    = val_e <Q_i, K_j> + bias[h, e]
//   P_e    = exp(s_e - row_max_i) / row_sum_i
//   out_i  = sum_e P_e V_j
//   delta_i = <dO_i, out_i>
//   dP_e   = <dO_i, V_j>
//   dS_e   = P_e (dP_e - delta_i)
//   dQ_i   = sum_e dS_e val_e K_j
//   dK_j   = sum_e dS_e val_e Q_i
//   dV_j   = sum_e P_e dO_i
//   dbias[h, e] = dS_e
// bias, dbias: fp32[h, nnz] in CSR edge order (the layout of attn_edge: the wave-per-row forward reads a 64-edge tile of
// one head as one coalesced load), indexed with size_t (h nnz exceeds 2^31 on large graphs at 8 heads).
//
// The structure is gt_train.hip's, pass for pass -- forward, CSR backward pass, CSC backward pass; each as a wave per row /
// column and, for low-degree graphs (nnz < 8 m), as a group of G lanes per row / column with the cooperative switch for long
// rows; two floats saved per (row, head); no atomics -- and the code is a copy with the bias worked in, so that the
// existing pair's code objects stay as they are and this operator is one file:
//   forward           adds the bias after the val multiply and before the running maximum
//   backward, CSR     every lane of a group holds its edge's dS_e (lanes_sum is an all-reduce); lane 0 of the group stores
//                     it to dbias when the caller wants it.  Every slot of dbias is written, plainly (no pre-zeroing)
//   backward, CSC     gathers bias[val_idx[t]] next to val and recomputes P_e and dS_e; val_idx is therefore always read
// Masks.  An edge with bias = -inf has P_e = 0 and dbias_e = 0 and adds nothing to any sum.  A (row, head) whose edges are
// all masked behaves like an empty row: out = 0, row_max = -1e38, row_sum = 0, dQ = 0 -- the forward tests the running
// maximum, not the degree, and both backward passes take 1 / row_sum of such a row as 0, so nothing is NaN or inf.
// +inf and NaN in bias are the caller's error.
#include "dfgnn_launch.hpp"
#include "dfgnn_rows.hpp"

namespace dfgnn {

// Everything the per-row routines need; at_head() offsets the feature pointers and bias / dbias to the workgroup's head.
struct GtBias {
  int m, n_cols, nnz, h, f, head;             // m rows (queries, outputs) x n_cols columns (keys, values)
  size_t hf;
  const int *row_ptr, *col_ind;                // CSR
  const float *val;                            // CSR order, NULL = unit values
  const float *bias;                           // [h, nnz] CSR order (+ head * nnz)
  float *dbias;                                // [h, nnz] (+ head * nnz), NULL = not wanted
  const int *col_ptr, *row_ind, *val_idx;      // CSC (column pass)
  const float *Qh, *Kh, *Vh, *dOh, *Oh;        // features, output gradient, forward output (+ head * f)
  float *row_max, *row_sum, *delta;            // [m, h]: written by the forward / the CSR pass, read by the passes after
  float *outh, *dQh, *dKh, *dVh;               // (+ head * f)
  __device__ __forceinline__ size_t nh(int node) const { return (size_t)node * h + head; }
  __device__ __forceinline__ void at_head(int hd) {
    head = hd;
    const size_t o = (size_t)hd * f, eo = (size_t)hd * (size_t)nnz;
    Qh += o; Kh += o; Vh += o;
    if (bias) bias += eo;
    if (dbias) dbias += eo;
    if (dOh) dOh += o;
    if (Oh) Oh += o;
    if (outh) outh += o;
    if (dQh) dQh += o;
    if (dKh) dKh += o;
    if (dVh) dVh += o;
  }
};

// the saved maximum of a row: a row without an unmasked edge gets the sentinel of the statistics pairs (include/dfgnn.h)
__device__ __forceinline__ float gtb_saved_max(float m_run) { return m_run == -INFINITY ? -1e38f : m_run; }
// 1 / row_sum; a row without an unmasked edge (row_sum = 0) has P = 0 everywhere
__device__ __forceinline__ float gtb_inv_sum(float sum) { return sum != 0.f ? 1.f / sum : 0.f; }

// ======================================================================================================================
// forward, a wave per row: 64-edge tiles (sw / sc: the wave's 64-float / 64-int LDS scratch)
// ======================================================================================================================
template <class C>
__device__ __forceinline__ void gtb_fwd_row_wave(const GtBias &a, int r, int lane, float *sw, int *sc) {
  const int gid = lane / C::G, gl = lane % C::G;
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  Frag<C> q, acc;
  frag_load<C>(q, a.Qh + (size_t)r * a.hf, a.f, gl);
  frag_zero<C>(acc);
  float m_run = -INFINITY, l_run = 0.f;
  for (int t0 = 0; t0 < deg; t0 += kWave) {
    const int nt = min(kWave, deg - t0);
    sc[lane] = (lane < nt) ? a.col_ind[lb + t0 + lane] : 0;
    const float b = (lane < nt) ? a.bias[(size_t)lb + t0 + lane] : 0.f;  // one coalesced load per tile
    wave_sync();
    tile_dots<C>(q, sc, nt, a.Kh, a.hf, a.f, gid, gl, sw);
    wave_sync();
    float s = -INFINITY;
    if (lane < nt) s = (a.val ? sw[lane] * a.val[lb + t0 + lane] : sw[lane]) + b;  // the maximum is taken AFTER the bias
    online_step<C>(s, lane, sw, acc, m_run, l_run);
    wave_sync();
    spmm_accum<C>(acc, sw, sc, nt, a.Vh, a.hf, a.f, gid, gl);
    wave_sync();
  }
  const float inv = gtb_inv_sum(l_run);  // empty or fully masked row -> 0
  frag_reduce_groups<C>(acc);
  if (gid == 0) frag_store_scaled<C>(acc, inv, a.outh + (size_t)r * a.hf, a.f, gl);
  if (lane == 0 && a.row_max) {
    a.row_max[a.nh(r)] = gtb_saved_max(m_run);
    a.row_sum[a.nh(r)] = l_run;
  }
}

// ======================================================================================================================
// a group of G lanes (one feature row wide) per row / column, everything in registers, no LDS.  COOP: the row is taken by
// all EPW groups of the wave together (group gid: edges gid, gid + EPW, ...) and the partial results are merged across
// the groups -- the long rows of a low-degree graph, and EVERY row of the wave-per-row form of the two backward passes.
// ======================================================================================================================
template <class C, bool COOP>
__device__ __forceinline__ void gtb_fwd_row_group(const GtBias &a, int r, int gid, int gl) {
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  Frag<C> q, acc;
  frag_load<C>(q, a.Qh + (size_t)r * a.hf, a.f, gl);
  frag_zero<C>(acc);
  float m_run = -INFINITY, l_run = 0.f;  // online softmax: one sweep, one dependent gather chain per edge
  for (int e = COOP ? gid : 0; e < deg; e += COOP ? C::EPW : 1) {
    const int c = a.col_ind[lb + e];
    const float b = a.bias[(size_t)lb + e];
    Frag<C> k, v;
    frag_load<C>(k, a.Kh + (size_t)c * a.hf, a.f, gl);
    frag_load<C>(v, a.Vh + (size_t)c * a.hf, a.f, gl);
    float s = lanes_sum<C::G>(frag_dot<C>(q, k));
    if (a.val) s *= a.val[lb + e];
    s += b;
    const float m_new = fmaxf(m_run, s);
    const float sc = (m_run == -INFINITY) ? 0.f : fast_exp(m_run - m_new);
    const float p = (s == -INFINITY) ? 0.f : fast_exp(s - m_new);
    l_run = l_run * sc + p;
    frag_scale<C>(acc, sc);
    frag_fma<C>(acc, p, v);
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
    frag_store_scaled<C>(acc, gtb_inv_sum(l_run), a.outh + (size_t)r * a.hf, a.f, gl);
    if (gl == 0 && a.row_max) {
      a.row_max[a.nh(r)] = gtb_saved_max(m_run);
      a.row_sum[a.nh(r)] = l_run;
    }
  }
}

// CSR pass, row r: delta_r = <dO_r, out_r> -> delta; dQ_r = sum_e dS_e val_e K_c and dbias_e = dS_e in one sweep, two
// edges (four gathers) in flight per group.  Every lane of a group holds the two dot products of its edge (lanes_sum is
// an all-reduce), so the edge's dS needs no exchange: lane 0 of the group stores it.
template <class C, bool COOP>
__device__ __forceinline__ void gtb_bwd_row_group(const GtBias &a, int r, int gid, int gl) {
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  const int es = COOP ? C::EPW : 1;
  Frag<C> acc;
  frag_zero<C>(acc);
  float dl = 0.f;  // empty row: dQ = 0, delta = 0
  if (deg > 0) {
    Frag<C> q, go, o;
    frag_load<C>(q, a.Qh + (size_t)r * a.hf, a.f, gl);
    frag_load<C>(go, a.dOh + (size_t)r * a.hf, a.f, gl);
    frag_load<C>(o, a.Oh + (size_t)r * a.hf, a.f, gl);
    dl = lanes_sum<C::G>(frag_dot<C>(go, o));
    const float mx = a.row_max[a.nh(r)], inv = gtb_inv_sum(a.row_sum[a.nh(r)]);
    auto weight = [&](int e, float b, const Frag<C> &k, const Frag<C> &v) {  // dS_e -> dbias; returns dS_e val_e
      const float vl = a.val ? a.val[lb + e] : 1.f;
      const float s = vl * lanes_sum<C::G>(frag_dot<C>(q, k)) + b;
      const float dp = lanes_sum<C::G>(frag_dot<C>(go, v));
      const float ds = fast_exp(s - mx) * inv * (dp - dl);  // a masked edge: exp(-inf) = 0
      if (a.dbias && gl == 0) a.dbias[(size_t)lb + e] = ds;
      return ds * vl;
    };
    int e = COOP ? gid : 0;
    for (; e + es < deg; e += 2 * es) {
      const int c0 = a.col_ind[lb + e], c1 = a.col_ind[lb + e + es];
      const float b0 = a.bias[(size_t)lb + e], b1 = a.bias[(size_t)lb + e + es];
      Frag<C> k0, v0, k1, v1;
      frag_load<C>(k0, a.Kh + (size_t)c0 * a.hf, a.f, gl);
      frag_load<C>(v0, a.Vh + (size_t)c0 * a.hf, a.f, gl);
      frag_load<C>(k1, a.Kh + (size_t)c1 * a.hf, a.f, gl);
      frag_load<C>(v1, a.Vh + (size_t)c1 * a.hf, a.f, gl);
      frag_fma<C>(acc, weight(e, b0, k0, v0), k0);
      frag_fma<C>(acc, weight(e + es, b1, k1, v1), k1);
    }
    for (; e < deg; e += es) {
      const int c0 = a.col_ind[lb + e];
      const float b0 = a.bias[(size_t)lb + e];
      Frag<C> k0, v0;
      frag_load<C>(k0, a.Kh + (size_t)c0 * a.hf, a.f, gl);
      frag_load<C>(v0, a.Vh + (size_t)c0 * a.hf, a.f, gl);
      frag_fma<C>(acc, weight(e, b0, k0, v0), k0);
    }
  }
  if constexpr (COOP) frag_reduce_groups<C>(acc);
  if (!COOP || gid == 0) {
    frag_store_scaled<C>(acc, 1.f, a.dQh + (size_t)r * a.hf, a.f, gl);
    if (gl == 0) a.delta[a.nh(r)] = dl;
  }
}

// CSC pass, column j: dV_j = sum P_e dO_i, dK_j = sum P_e (dP_e - delta_i) val_e Q_i over the column's entries, two
// entries (four gathers + their row scalars, edge value and bias) in flight per group.  An empty column writes zeros.
template <class C, bool COOP>
__device__ __forceinline__ void gtb_bwd_col_group(const GtBias &a, int j, int gid, int gl) {
  const int lb = a.col_ptr[j], n = a.col_ptr[j + 1] - lb;
  const int es = COOP ? C::EPW : 1;
  Frag<C> aK, aV;
  frag_zero<C>(aK);
  frag_zero<C>(aV);
  if (n > 0) {
    Frag<C> k, v;
    frag_load<C>(k, a.Kh + (size_t)j * a.hf, a.f, gl);
    frag_load<C>(v, a.Vh + (size_t)j * a.hf, a.f, gl);
    struct Entry {
      int i;
      float vl, b, mx, sum, dl;
    };
    auto entry = [&](int t) {
      Entry x;
      x.i = a.row_ind[lb + t];
      const int e = a.val_idx[lb + t];  // val and bias are in CSR order
      x.vl = a.val ? a.val[e] : 1.f;
      x.b = a.bias[(size_t)e];
      const size_t s = a.nh(x.i);
      x.mx = a.row_max[s];
      x.sum = a.row_sum[s];
      x.dl = a.delta[s];
      return x;
    };
    auto accum = [&](const Entry &x, const Frag<C> &qi, const Frag<C> &gi) {
      const float s = x.vl * lanes_sum<C::G>(frag_dot<C>(qi, k)) + x.b;
      const float dp = lanes_sum<C::G>(frag_dot<C>(gi, v));
      // (a fully masked row has row_sum = 0: its P is 0, not 0 * inf)
      const float p = fast_exp(s - x.mx) * (x.sum != 0.f ? __builtin_amdgcn_rcpf(x.sum) : 0.f);
      frag_fma<C>(aV, p, gi);
      frag_fma<C>(aK, p * (dp - x.dl) * x.vl, qi);
    };
    int t = COOP ? gid : 0;
    for (; t + es < n; t += 2 * es) {
      const Entry x0 = entry(t), x1 = entry(t + es);
      Frag<C> q0, g0, q1, g1;
      frag_load<C>(q0, a.Qh + (size_t)x0.i * a.hf, a.f, gl);
      frag_load<C>(g0, a.dOh + (size_t)x0.i * a.hf, a.f, gl);
      frag_load<C>(q1, a.Qh + (size_t)x1.i * a.hf, a.f, gl);
      frag_load<C>(g1, a.dOh + (size_t)x1.i * a.hf, a.f, gl);
      accum(x0, q0, g0);
      accum(x1, q1, g1);
    }
    for (; t < n; t += es) {
      const Entry x0 = entry(t);
      Frag<C> q0, g0;
      frag_load<C>(q0, a.Qh + (size_t)x0.i * a.hf, a.f, gl);
      frag_load<C>(g0, a.dOh + (size_t)x0.i * a.hf, a.f, gl);
      accum(x0, q0, g0);
    }
  }
  if constexpr (COOP) {
    frag_reduce_groups<C>(aK);
    frag_reduce_groups<C>(aV);
  }
  if (!COOP || gid == 0) {
    frag_store_scaled<C>(aK, 1.f, a.dKh + (size_t)j * a.hf, a.f, gl);
    frag_store_scaled<C>(aV, 1.f, a.dVh + (size_t)j * a.hf, a.f, gl);
  }
}

// ======================================================================================================================
// kernels.  PASS: 0 forward, 1 backward CSR pass, 2 backward CSC pass.
// ======================================================================================================================
template <class C, int PASS, bool COOP>
__device__ __forceinline__ void gtb_group_pass(const GtBias &a, int r, int gid, int gl) {
  if constexpr (PASS == 0) gtb_fwd_row_group<C, COOP>(a, r, gid, gl);
  else if constexpr (PASS == 1) gtb_bwd_row_group<C, COOP>(a, r, gid, gl);
  else gtb_bwd_col_group<C, COOP>(a, r, gid, gl);
}

// general: a wave per row / column, grid-strided over the whole graph.  The forward works in 64-edge tiles through the
// wave's LDS scratch; the backward passes are the COOP form of the group routines (no LDS).
template <class C, int PASS>
__global__ __launch_bounds__(kBlock) void gt_bias_wave_kernel(GtBias a) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  a.at_head(blockIdx.y);
  const int n = PASS == 2 ? a.n_cols : a.m;  // the extent this pass walks: rows, or (CSC pass) columns
  const int beg = blockIdx.x * kWavesPerBlock + wave, step = gridDim.x * kWavesPerBlock;
  if constexpr (PASS == 0) {
    __shared__ __attribute__((aligned(16))) float lds[kWavesPerBlock * kScratchFloatsPerWave];
    float *sw = lds + wave * kScratchFloatsPerWave;
    int *sc = reinterpret_cast<int *>(sw + kWave);
    for (int r = beg; r < n; r += step) gtb_fwd_row_wave<C>(a, r, lane, sw, sc);
  } else {
    for (int r = beg; r < n; r += step) gtb_group_pass<C, PASS, true>(a, r, lane / C::G, lane % C::G);
  }
}

// low-degree graphs: a workgroup takes blocks of kBlock / G consecutive rows, one lane group per row -- unless a wave's
// EPW rows include one of more than kGtBiasGroupMaxDegree entries, which a single lane group would walk serially while the
// rest of the wave waits: that wave takes its rows one after the other with all its groups on each (COOP).  The choice is
// wave-uniform (ballot): no barrier, no LDS.  As gt_train_group_kernel of gt_train.hip, with the same threshold.
constexpr int kGtBiasGroupMaxDegree = 24;
template <class C, int PASS>
__global__ __launch_bounds__(kBlock) void gt_bias_group_kernel(GtBias a) {
  constexpr int G = C::G, R = kBlock / G;  // rows per block
  const int gid = (threadIdx.x & (kWave - 1)) / G, gl = threadIdx.x % G, wave = threadIdx.x / kWave;
  a.at_head(blockIdx.y);
  const int *ptr = PASS == 2 ? a.col_ptr : a.row_ptr;
  const int n = PASS == 2 ? a.n_cols : a.m;  // the extent this pass walks: rows, or (CSC pass) columns
  for (int b0 = blockIdx.x * R; b0 < n; b0 += gridDim.x * R) {
    const int r = b0 + threadIdx.x / G;
    const int deg = r < n ? ptr[r + 1] - ptr[r] : 0;
    if (__any(deg > kGtBiasGroupMaxDegree)) {
      for (int rr = b0 + wave * C::EPW; rr < min(n, b0 + (wave + 1) * C::EPW); ++rr)
        gtb_group_pass<C, PASS, true>(a, rr, gid, gl);
    } else if (r < n) {
      gtb_group_pass<C, PASS, false>(a, r, gid, gl);
    }
  }
}

static dim3 gtb_group_grid(int m, int h, int G) {
  const long per = kBlock / G;
  long blocks = ((long)m + per - 1) / per;
  if (blocks > 16384) blocks = 16384;
  return dim3((unsigned)(blocks < 1 ? 1 : blocks), h);
}
static dim3 gtb_wave_grid(int m, int h) {
  const long want = ((long)m + kWavesPerBlock - 1) / kWavesPerBlock;
  return dim3((unsigned)(want > (1 << 20) ? (1 << 20) : want), h);
}

template <int PASS>
static int launch_gt_bias_pass(const GtBias &a, bool v4, hipStream_t s) {
  const int n = PASS == 2 ? a.n_cols : a.m;  // the form is chosen per pass, by the average degree of what it walks
  if (n == 0) return 0;  // nothing to walk and nothing to write (a rectangular graph without rows / without columns)
  const bool groups = low_degree(n, a.nnz);
  return dispatch_cfg(a.f, v4, [&](auto cfg) {
    using C = decltype(cfg);
    if (groups) gt_bias_group_kernel<C, PASS><<<gtb_group_grid(n, a.h, C::G), kBlock, 0, s>>>(a);
    else gt_bias_wave_kernel<C, PASS><<<gtb_wave_grid(n, a.h), kBlock, 0, s>>>(a);
    return launch_status();
  });
}

static GtBias gt_bias_args(const Csr &g, const float *bias, const float *Q, const float *K, const float *V) {
  GtBias a{};
  a.m = g.m; a.n_cols = g.n_cols; a.nnz = g.nnz; a.h = g.h; a.f = g.f; a.hf = (size_t)g.h * g.f;
  a.row_ptr = g.row_ptr; a.col_ind = g.col_ind; a.val = g.val; a.bias = bias;
  a.Qh = Q; a.Kh = K; a.Vh = V;
  return a;
}

int launch_gt_bias_fwd(const Csr &g, const float *bias, const float *Q, const float *K, const float *V, float *row_max,
                       float *row_sum, float *out, hipStream_t s) {
  GtBias a = gt_bias_args(g, bias, Q, K, V);
  a.outh = out; a.row_max = row_max; a.row_sum = row_sum;
  return launch_gt_bias_pass<0>(a, (g.f % 4 == 0) && aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(out), s);
}

int launch_gt_bias_bwd_rows(const Csr &g, const float *bias, const float *Q, const float *K, const float *V,
                            const float *out, const float *row_max, const float *row_sum, const float *grad_out,
                            float *delta, float *dQ, float *dbias, hipStream_t s) {
  GtBias a = gt_bias_args(g, bias, Q, K, V);
  a.Oh = out; a.dOh = grad_out; a.delta = delta; a.dQh = dQ; a.dbias = dbias;
  a.row_max = const_cast<float *>(row_max); a.row_sum = const_cast<float *>(row_sum);
  const bool v4 = (g.f % 4 == 0) && aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(out) &&
                  aligned16(grad_out) && aligned16(dQ);
  return launch_gt_bias_pass<1>(a, v4, s);
}

int launch_gt_bias_bwd_cols(const Csr &g, const float *bias, const int *col_ptr, const int *row_ind, const int *val_idx,
                            const float *Q, const float *K, const float *V, const float *row_max, const float *row_sum,
                            const float *delta, const float *grad_out, float *dK, float *dV, hipStream_t s) {
  GtBias a = gt_bias_args(g, bias, Q, K, V);
  a.col_ptr = col_ptr; a.row_ind = row_ind; a.val_idx = val_idx;
  a.dOh = grad_out; a.dKh = dK; a.dVh = dV;
  a.row_max = const_cast<float *>(row_max); a.row_sum = const_cast<float *>(row_sum);
  a.delta = const_cast<float *>(delta);
  const bool v4 = (g.f % 4 == 0) && aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(grad_out) &&
                  aligned16(dK) && aligned16(dV);
  return launch_gt_bias_pass<2>(a, v4, s);
}

}  // namespace dfgnn
