// gat_edge_train.hip -- GAT (v1) with an optional per-edge, per-head attention term for gfx950: fused inference and training
// pair, general kernels (any graph -- square or m x n_cols --, no plan, no degree limit).  Per head, edge e = (row i,
// column j); rows are the outputs, columns the sources:
//   pre_e  = (attn_row[i] + attn_col[j]) + score[h, e]          score NULL: + 0.f, the same instruction sequence
//   s_e    = LeakyReLU(pre_e)
//   P_e    = exp(s_e - edge_max_i) / edge_sum_i                  statistics over ALL edges of the row, dropped or not
//   k_e    = mask ? (mask[e, h] > attn_drop) / (1 - attn_drop) : 1
//   out_i  = sum_e k_e P_e X_j
//   delta_i = <dO_i, out_i> = sum_e k_e P_e <dO_i, X_j>
//   dS_e   = P_e (k_e <dO_i, X_j> - delta_i)
//   G_e    = dS_e (pre_e > 0 ? 1 : slope)
//   grad_attn_row[i] = sum_{e of i} G_e    grad_attn_col[j] = sum_{e into j} G_e    grad_score[h, e] = G_e
//   grad_feat[j]     = sum_{e into j} k_e P_e dO_i
// score, grad_score: fp32[h, nnz] in CSR edge order (the layout of bias / dbias in gt_bias_train.hip), indexed with size_t.
// mask: fp32[nnz, h], edge-major uniform randoms, the layout and the comparison of gat_train.hip, so one set of randoms
// serves both GAT pairs.
//
// The structure is gt_bias_train.hip's, pass for pass -- forward, CSR backward pass, CSC backward pass; each as a wave per
// row / column and, for low-degree sides (nnz < 8 n), as a group of G lanes per row / column with the cooperative switch
// for long rows; two floats saved per (row, head); no atomics -- with GAT's rank-one logit in place of the dot product:
//   forward           a lane per edge forms the logit of a 64-edge tile (wave form); no key gather exists
//   backward, CSR     gathers X_j once per edge for <dO_i, X_j> and sums delta_i over the edges (the forward's `out` is
//                     not read); grad_attn_row from three running sums; grad_score, when the caller wants it, parked and
//                     finished in place.  Every slot of grad_score is written, plainly (no pre-zeroing)
//   backward, CSC     holds the column's X_j in registers, gathers dO_i per entry (needed for grad_feat anyway), forms
//                     <dO_i, X_j> itself and recomputes P_e and G_e from the row scalars: nothing of size nnz passes from
//                     the CSR pass to this one, only delta [m, h].  score and mask are found through val_idx, which is read
//                     only when one of the two is given
// Masks.  An edge with score = -inf has s_e = -inf, P_e = 0 and G_e = 0 and adds nothing to any sum.  A (row, head) whose
// edges are all masked behaves like an empty row: out = 0, edge_max = -1e38, edge_sum = 0, grad_attn_row = 0 -- the forward
// tests the running maximum, not the degree, and both backward passes take 1 / edge_sum of such a row as 0, so nothing is
// NaN or inf.  +inf and NaN in score are the caller's error.  A row whose edges are all DROPPED keeps its statistics (they
// cover every edge) and has out = 0, delta = 0.  Saved between forward and backward: edge_max and edge_sum (and the caller's
// randoms); the backward needs neither `out` nor anything of size nnz.
#include "dfgnn_launch.hpp"
#include "dfgnn_rows.hpp"

namespace dfgnn {

// Everything the per-row routines need; at_head() offsets the feature pointers and score / grad_score to the workgroup's
// head.  The [nodes, h] arrays stay whole and are indexed with nh().
struct GatEdge {
  int m, n_cols, nnz, h, f, head;              // m rows (outputs) x n_cols columns (sources)
  size_t hf;
  float slope, drop, keep_scale;               // keep_scale = 1 / (1 - drop), 1 without a mask
  const int *row_ptr, *col_ind;                // CSR
  const int *col_ptr, *row_ind, *val_idx;      // CSC (column pass)
  const float *attn_row, *attn_col;            // [m, h] / [n_cols, h]
  const float *score;                          // [h, nnz] CSR order (+ head * nnz), NULL = no edge term
  float *grad_score;                           // [h, nnz] (+ head * nnz), NULL = not wanted
  const float *mask;                           // [nnz, h] uniform randoms, NULL = keep everything
  const float *Xh, *dOh;                       // sources, output gradient (+ head * f)
  float *edge_max, *edge_sum, *delta;          // [m, h]: written by the forward / the CSR pass, read by the passes after
  float *outh, *grad_feath;                    // (+ head * f)
  float *grad_attn_row, *grad_attn_col;        // [m, h] / [n_cols, h]
  __device__ __forceinline__ size_t nh(int node) const { return (size_t)node * h + head; }
  __device__ __forceinline__ void at_head(int hd) {
    head = hd;
    const size_t o = (size_t)hd * f, eo = (size_t)hd * (size_t)nnz;
    if (Xh) Xh += o;
    if (score) score += eo;
    if (grad_score) grad_score += eo;
    if (dOh) dOh += o;
    if (outh) outh += o;
    if (grad_feath) grad_feath += o;
  }
  // the edge term of CSR position e; without one the same add runs with 0.f, so score = zeros gives the same bits
  __device__ __forceinline__ float term(size_t e) const { return score ? score[e] : 0.f; }
  // k_e of CSR position e
  __device__ __forceinline__ float keep(size_t e) const {
    return mask ? (mask[e * (size_t)h + head] > drop ? keep_scale : 0.f) : 1.f;
  }
  // the logit from the two node scores and the edge term; a masked edge (-inf) stays -inf for every slope
  __device__ __forceinline__ float pre(float ar, float ac, float sc) const { return (ar + ac) + sc; }
  __device__ __forceinline__ float logit(float p) const { return p == -INFINITY ? -INFINITY : leaky_relu(p, slope); }
  __device__ __forceinline__ float dlrelu(float p) const { return p > 0.f ? 1.f : slope; }
};

// the saved maximum of a row: a row without an unmasked edge gets the sentinel of the statistics pairs (include/dfgnn.h)
__device__ __forceinline__ float gte_saved_max(float m_run) { return m_run == -INFINITY ? -1e38f : m_run; }
// 1 / edge_sum; a row without an unmasked edge (edge_sum = 0) has P = 0 everywhere
__device__ __forceinline__ float gte_inv_sum(float sum) { return sum != 0.f ? 1.f / sum : 0.f; }

// ======================================================================================================================
// forward, a wave per row: 64-edge tiles, a lane per edge for the logit (sw / sc: the wave's 64-float / 64-int LDS scratch)
// ======================================================================================================================
template <class C>
__device__ __forceinline__ void gte_fwd_row_wave(const GatEdge &a, int r, int lane, float *sw, int *sc) {
  const int gid = lane / C::G, gl = lane % C::G;
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  const float ar = a.attn_row[a.nh(r)];
  Frag<C> acc;
  frag_zero<C>(acc);
  float m_run = -INFINITY, l_run = 0.f;
  for (int t0 = 0; t0 < deg; t0 += kWave) {
    const int nt = min(kWave, deg - t0);
    float s = -INFINITY, k = 0.f;
    int c = 0;
    if (lane < nt) {
      const size_t e = (size_t)lb + t0 + lane;
      c = a.col_ind[e];
      s = a.logit(a.pre(ar, a.attn_col[a.nh(c)], a.term(e)));
      k = a.keep(e);
    }
    sc[lane] = c;
    online_step<C>(s, lane, sw, acc, m_run, l_run);  // the statistics take every edge
    sw[lane] *= k;                                   // ... the message only the kept ones (same lane wrote it)
    wave_sync();
    spmm_accum<C>(acc, sw, sc, nt, a.Xh, a.hf, a.f, gid, gl);
    wave_sync();
  }
  const float inv = gte_inv_sum(l_run);  // empty or fully masked row -> 0
  frag_reduce_groups<C>(acc);
  if (gid == 0) frag_store_scaled<C>(acc, inv, a.outh + (size_t)r * a.hf, a.f, gl);
  if (lane == 0 && a.edge_max) {
    a.edge_max[a.nh(r)] = gte_saved_max(m_run);
    a.edge_sum[a.nh(r)] = l_run;
  }
}

// ======================================================================================================================
// a group of G lanes (one feature row wide) per row / column, everything in registers, no LDS.  COOP: the row is taken by
// all EPW groups of the wave together (group gid: edges gid, gid + EPW, ...) and the partial results are merged across
// the groups -- the long rows of a low-degree graph, and EVERY row of the wave-per-row form of the two backward passes.
// ======================================================================================================================
template <class C, bool COOP>
__device__ __forceinline__ void gte_fwd_row_group(const GatEdge &a, int r, int gid, int gl) {
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  const float ar = a.attn_row[a.nh(r)];
  Frag<C> acc;
  frag_zero<C>(acc);
  float m_run = -INFINITY, l_run = 0.f;  // online softmax: one sweep, one gather per edge
  for (int e = COOP ? gid : 0; e < deg; e += COOP ? C::EPW : 1) {
    const size_t ee = (size_t)lb + e;
    const int c = a.col_ind[ee];
    Frag<C> x;
    frag_load<C>(x, a.Xh + (size_t)c * a.hf, a.f, gl);
    const float s = a.logit(a.pre(ar, a.attn_col[a.nh(c)], a.term(ee)));
    const float k = a.keep(ee);
    const float m_new = fmaxf(m_run, s);
    const float sc = (m_run == -INFINITY) ? 0.f : fast_exp(m_run - m_new);
    const float p = (s == -INFINITY) ? 0.f : fast_exp(s - m_new);
    l_run = l_run * sc + p;
    frag_scale<C>(acc, sc);
    frag_fma<C>(acc, p * k, x);
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
    frag_store_scaled<C>(acc, gte_inv_sum(l_run), a.outh + (size_t)r * a.hf, a.f, gl);
    if (gl == 0 && a.edge_max) {
      a.edge_max[a.nh(r)] = gte_saved_max(m_run);
      a.edge_sum[a.nh(r)] = l_run;
    }
  }
}

// CSR pass, row r, one sweep over the row's sources, two edges (two gathers) in flight per group.  With t_e = k_e <dO_r,
// X_j> and l_e the LeakyReLU derivative it accumulates delta_r = sum P_e t_e (= <dO_r, out_r>, summed over the edges: `out`
// is not read, and delta carries the rounding of the dot products alone, not that of a stored output row -- which is what
// keeps rows of three edges inside the fp32-level bound), B = sum P_e l_e t_e and C = sum P_e l_e; then grad_attn_row_r = sum
// P_e (t_e - delta_r) l_e = B - delta_r C.  grad_score, when wanted: lane 0 of the group parks t_e in the edge's slot during
// the sweep and, once delta_r is known, turns its own slots into G_e = P_e (t_e - delta_r) l_e from the row scalars alone (no
// gather; the same thread wrote the slot).  grad_attn_row is formed the same way with and without grad_score: the same bits.
template <class C, bool COOP>
__device__ __forceinline__ void gte_bwd_row_group(const GatEdge &a, int r, int gid, int gl) {
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  const int es = COOP ? C::EPW : 1;
  float dl = 0.f, ga = 0.f;  // empty row: delta = 0, grad_attn_row = 0
  if (deg > 0) {
    Frag<C> go;
    frag_load<C>(go, a.dOh + (size_t)r * a.hf, a.f, gl);
    const float ar = a.attn_row[a.nh(r)];
    const float mx = a.edge_max[a.nh(r)], inv = gte_inv_sum(a.edge_sum[a.nh(r)]);
    float B = 0.f, Cs = 0.f;
    auto prob = [&](float pr) { return fast_exp(a.logit(pr) - mx) * inv; };  // a masked edge: exp(-inf) = 0
    auto grad = [&](size_t e, int c, const Frag<C> &x) {
      const float pr = a.pre(ar, a.attn_col[a.nh(c)], a.term(e));
      const float t = a.keep(e) * lanes_sum<C::G>(frag_dot<C>(go, x));
      const float p = prob(pr), pl = p * a.dlrelu(pr);
      dl = fmaf(p, t, dl);
      B = fmaf(pl, t, B);
      Cs += pl;
      if (a.grad_score && gl == 0) a.grad_score[e] = t;  // parked until delta is known
    };
    int e = COOP ? gid : 0;
    for (; e + es < deg; e += 2 * es) {
      const size_t e0 = (size_t)lb + e, e1 = e0 + es;
      const int c0 = a.col_ind[e0], c1 = a.col_ind[e1];
      Frag<C> x0, x1;
      frag_load<C>(x0, a.Xh + (size_t)c0 * a.hf, a.f, gl);
      frag_load<C>(x1, a.Xh + (size_t)c1 * a.hf, a.f, gl);
      grad(e0, c0, x0);
      grad(e1, c1, x1);
    }
    for (; e < deg; e += es) {
      const size_t e0 = (size_t)lb + e;
      const int c0 = a.col_ind[e0];
      Frag<C> x0;
      frag_load<C>(x0, a.Xh + (size_t)c0 * a.hf, a.f, gl);
      grad(e0, c0, x0);
    }
    if constexpr (COOP) {
#pragma unroll
      for (int o = C::G; o < kWave; o <<= 1) {
        dl += __shfl_xor(dl, o, kWave);
        B += __shfl_xor(B, o, kWave);
        Cs += __shfl_xor(Cs, o, kWave);
      }
    }
    ga = fmaf(-dl, Cs, B);
    if (a.grad_score && gl == 0) {
      for (e = COOP ? gid : 0; e < deg; e += es) {
        const size_t e0 = (size_t)lb + e;
        const float pr = a.pre(ar, a.attn_col[a.nh(a.col_ind[e0])], a.term(e0));
        a.grad_score[e0] = prob(pr) * (a.grad_score[e0] - dl) * a.dlrelu(pr);
      }
    }
  }
  if ((!COOP || gid == 0) && gl == 0) {
    a.delta[a.nh(r)] = dl;
    a.grad_attn_row[a.nh(r)] = ga;
  }
}

// CSC pass, column j: grad_feat_j = sum k_e P_e dO_i, grad_attn_col_j = sum G_e over the column's entries, two entries (two
// gathers + their row scalars, edge term and random) in flight per group.  An empty column writes zeros.
template <class C, bool COOP>
__device__ __forceinline__ void gte_bwd_col_group(const GatEdge &a, int j, int gid, int gl) {
  const int lb = a.col_ptr[j], n = a.col_ptr[j + 1] - lb;
  const int es = COOP ? C::EPW : 1;
  Frag<C> aF;
  frag_zero<C>(aF);
  float gc = 0.f;
  if (n > 0) {
    Frag<C> x;
    frag_load<C>(x, a.Xh + (size_t)j * a.hf, a.f, gl);
    const float ac = a.attn_col[a.nh(j)];
    const bool per_edge = a.score || a.mask;  // (uniform over the launch)
    struct Entry {
      int i;
      float pr, k, mx, sum, dl;
    };
    auto entry = [&](int t) {
      Entry y;
      y.i = a.row_ind[lb + t];
      const size_t e = per_edge ? (size_t)a.val_idx[lb + t] : 0;  // score and mask are in CSR order
      const size_t s = a.nh(y.i);
      y.pr = a.pre(a.attn_row[s], ac, a.term(e));
      y.k = a.keep(e);
      y.mx = a.edge_max[s];
      y.sum = a.edge_sum[s];
      y.dl = a.delta[s];
      return y;
    };
    auto accum = [&](const Entry &y, const Frag<C> &gi) {
      const float dp = lanes_sum<C::G>(frag_dot<C>(gi, x));
      // (a fully masked row has edge_sum = 0: its P is 0, not 0 * inf)
      const float p = fast_exp(a.logit(y.pr) - y.mx) * gte_inv_sum(y.sum);
      frag_fma<C>(aF, p * y.k, gi);
      gc += p * (y.k * dp - y.dl) * a.dlrelu(y.pr);
    };
    int t = COOP ? gid : 0;
    for (; t + es < n; t += 2 * es) {
      const Entry y0 = entry(t), y1 = entry(t + es);
      Frag<C> g0, g1;
      frag_load<C>(g0, a.dOh + (size_t)y0.i * a.hf, a.f, gl);
      frag_load<C>(g1, a.dOh + (size_t)y1.i * a.hf, a.f, gl);
      accum(y0, g0);
      accum(y1, g1);
    }
    for (; t < n; t += es) {
      const Entry y0 = entry(t);
      Frag<C> g0;
      frag_load<C>(g0, a.dOh + (size_t)y0.i * a.hf, a.f, gl);
      accum(y0, g0);
    }
  }
  if constexpr (COOP) {
    frag_reduce_groups<C>(aF);
#pragma unroll
    for (int o = C::G; o < kWave; o <<= 1) gc += __shfl_xor(gc, o, kWave);
  }
  if (!COOP || gid == 0) {
    frag_store_scaled<C>(aF, 1.f, a.grad_feath + (size_t)j * a.hf, a.f, gl);
    if (gl == 0) a.grad_attn_col[a.nh(j)] = gc;
  }
}

// ======================================================================================================================
// kernels.  PASS: 0 forward, 1 backward CSR pass, 2 backward CSC pass.
// ======================================================================================================================
template <class C, int PASS, bool COOP>
__device__ __forceinline__ void gte_group_pass(const GatEdge &a, int r, int gid, int gl) {
  if constexpr (PASS == 0) gte_fwd_row_group<C, COOP>(a, r, gid, gl);
  else if constexpr (PASS == 1) gte_bwd_row_group<C, COOP>(a, r, gid, gl);
  else gte_bwd_col_group<C, COOP>(a, r, gid, gl);
}

// general: a wave per row / column, grid-strided over the whole graph.  The forward works in 64-edge tiles through the
// wave's LDS scratch; the backward passes are the COOP form of the group routines (no LDS).
template <class C, int PASS>
__global__ __launch_bounds__(kBlock) void gat_edge_wave_kernel(GatEdge a) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  a.at_head(blockIdx.y);
  const int n = PASS == 2 ? a.n_cols : a.m;  // the extent this pass walks: rows, or (CSC pass) columns
  const int beg = blockIdx.x * kWavesPerBlock + wave, step = gridDim.x * kWavesPerBlock;
  if constexpr (PASS == 0) {
    __shared__ __attribute__((aligned(16))) float lds[kWavesPerBlock * kScratchFloatsPerWave];
    float *sw = lds + wave * kScratchFloatsPerWave;
    int *sc = reinterpret_cast<int *>(sw + kWave);
    for (int r = beg; r < n; r += step) gte_fwd_row_wave<C>(a, r, lane, sw, sc);
  } else {
    for (int r = beg; r < n; r += step) gte_group_pass<C, PASS, true>(a, r, lane / C::G, lane % C::G);
  }
}

// low-degree sides: a workgroup takes blocks of kBlock / G consecutive rows, one lane group per row -- unless a wave's
// EPW rows include one of more than kGatEdgeGroupMaxDegree entries, which a single lane group would walk serially while the
// rest of the wave waits: that wave takes its rows one after the other with all its groups on each (COOP).  The choice is
// wave-uniform (ballot): no barrier, no LDS.  As gt_bias_group_kernel of gt_bias_train.hip, with the same threshold.
constexpr int kGatEdgeGroupMaxDegree = 24;
template <class C, int PASS>
__global__ __launch_bounds__(kBlock) void gat_edge_group_kernel(GatEdge a) {
  constexpr int G = C::G, R = kBlock / G;  // rows per block
  const int gid = (threadIdx.x & (kWave - 1)) / G, gl = threadIdx.x % G, wave = threadIdx.x / kWave;
  a.at_head(blockIdx.y);
  const int *ptr = PASS == 2 ? a.col_ptr : a.row_ptr;
  const int n = PASS == 2 ? a.n_cols : a.m;  // the extent this pass walks: rows, or (CSC pass) columns
  for (int b0 = blockIdx.x * R; b0 < n; b0 += gridDim.x * R) {
    const int r = b0 + threadIdx.x / G;
    const int deg = r < n ? ptr[r + 1] - ptr[r] : 0;
    if (__any(deg > kGatEdgeGroupMaxDegree)) {
      for (int rr = b0 + wave * C::EPW; rr < min(n, b0 + (wave + 1) * C::EPW); ++rr)
        gte_group_pass<C, PASS, true>(a, rr, gid, gl);
    } else if (r < n) {
      gte_group_pass<C, PASS, false>(a, r, gid, gl);
    }
  }
}

static dim3 gte_group_grid(int m, int h, int G) {
  const long per = kBlock / G;
  long blocks = ((long)m + per - 1) / per;
  if (blocks > 16384) blocks = 16384;
  return dim3((unsigned)(blocks < 1 ? 1 : blocks), h);
}
static dim3 gte_wave_grid(int m, int h) {
  const long want = ((long)m + kWavesPerBlock - 1) / kWavesPerBlock;
  return dim3((unsigned)(want > (1 << 20) ? (1 << 20) : want), h);
}

template <int PASS>
static int launch_gat_edge_pass(const GatEdge &a, bool v4, hipStream_t s) {
  const int n = PASS == 2 ? a.n_cols : a.m;  // the form is chosen per pass, by the average degree of what it walks
  if (n == 0) return 0;  // nothing to walk and nothing to write (a rectangular graph without rows / without columns)
  const bool groups = low_degree(n, a.nnz);
  return dispatch_cfg(a.f, v4, [&](auto cfg) {
    using C = decltype(cfg);
    if (groups) gat_edge_group_kernel<C, PASS><<<gte_group_grid(n, a.h, C::G), kBlock, 0, s>>>(a);
    else gat_edge_wave_kernel<C, PASS><<<gte_wave_grid(n, a.h), kBlock, 0, s>>>(a);
    return launch_status();
  });
}

static GatEdge gat_edge_args(const Csr &g, const GatEdgeTerms &t, const float *X) {
  GatEdge a{};
  a.m = g.m; a.n_cols = g.n_cols; a.nnz = g.nnz; a.h = g.h; a.f = g.f; a.hf = (size_t)g.h * g.f;
  a.row_ptr = g.row_ptr; a.col_ind = g.col_ind;
  a.attn_row = t.attn_row; a.attn_col = t.attn_col; a.slope = t.slope; a.score = t.score;
  a.mask = t.mask; a.drop = t.attn_drop; a.keep_scale = t.mask ? 1.f / (1.f - t.attn_drop) : 1.f;
  a.Xh = X;
  return a;
}

int launch_gat_edge_fwd(const Csr &g, const GatEdgeTerms &t, const float *X, float *edge_max, float *edge_sum, float *out,
                        hipStream_t s) {
  GatEdge a = gat_edge_args(g, t, X);
  a.outh = out; a.edge_max = edge_max; a.edge_sum = edge_sum;
  return launch_gat_edge_pass<0>(a, (g.f % 4 == 0) && aligned16(X) && aligned16(out), s);
}

int launch_gat_edge_bwd(const Csr &g, const GatEdgeTerms &t, const int *col_ptr, const int *row_ind, const int *val_idx,
                        const float *X, const float *edge_max, const float *edge_sum, const float *grad_out, float *delta, float *grad_feat, float *grad_attn_row, float *grad_attn_col,
                        float *grad_score, hipStream_t s) {
  GatEdge a = gat_edge_args(g, t, X);
  a.col_ptr = col_ptr; a.row_ind = row_ind; a.val_idx = val_idx;
  a.dOh = grad_out; a.delta = delta;
  a.edge_max = const_cast<float *>(edge_max); a.edge_sum = const_cast<float *>(edge_sum);
  a.grad_feath = grad_feat; a.grad_attn_row = grad_attn_row; a.grad_attn_col = grad_attn_col; a.grad_score = grad_score;
  // one layout for both passes, so that <dO_i, X_j> is summed in the same order on either side
  const bool v4 = (g.f % 4 == 0) && aligned16(X) && aligned16(grad_out) && aligned16(grad_feat);
  if (int rc = launch_gat_edge_pass<1>(a, v4, s)) return rc;
  return launch_gat_edge_pass<2>(a, v4, s);
}

}  // namespace dfgnn
