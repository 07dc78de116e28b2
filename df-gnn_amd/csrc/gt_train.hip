// gt_train.hip -- GT training pair for gfx950 without per-edge saved state: general kernels (any graph, no plan, no
// degree limit).
//
// The forward saves two floats per (row, head) -- logit maximum and sum of exponentials -- instead of attn_edge[h, nnz];
// the backward rebuilds every edge's dS from rows that each pass gathers anyway.  With delta_i = <dO_i, out_i>
// (= sum_e P_e dP_e, the row term of the softmax derivative):
//   s_e  = val_e <Q_i, K_j>          P_e  = exp(s_e - row_max_i) / row_sum_i
//   dP_e = <dO_i, V_j>               dS_e = P_e (dP_e - delta_i)
//   dQ_i = sum_e dS_e val_e K_j      dK_j = sum_e dS_e val_e Q_i      dV_j = sum_e P_e dO_i
// Three passes, each in two forms -- a wave per row / column (any degree) and, for low-degree graphs (nnz < 8 m, as on
// the attn_edge path), a group of G lanes per row / column:
//   forward           CSR, online softmax; writes out, row_max, row_sum.  replaces gt_hyper_forward
//                     (DFGNN/src/fused_gtconv/fused_gtconv_hyper.cu:31-163, 727-760) without its attn_edge
//   backward, CSR     Q_i, dO_i, out_i in registers, K_j and V_j gathered once per edge: delta_i, dQ_i in ONE sweep (the
//                     attn_edge form needs two, with dP parked in grad_edge for long rows).  replaces
//                     fused_backward_kernel (fused_gtconv_backward.cu:73-191)
//   backward, CSC     K_j, V_j in registers, Q_i and dO_i gathered per entry plus the three row scalars row_max_i,
//                     row_sum_i, delta_i: dK_j, dV_j.  No attn_edge, no grad_edge, and val_idx is read only when there
//                     are edge values.  replaces spmm_backward_kernel (fused_gtconv_backward.cu:40-70)
// Every output is written in full by plain stores; the column sums are deterministic (no atomics).
// The graph is m x n_cols (rows: queries and outputs; columns: keys and values; a square adjacency has n_cols == m).  Rows
// appear only in the forward and the CSR pass, columns only in the CSC pass, each side gathering the other by index: the
// CSC pass takes its loop bounds, its grid and its form (low_degree(n_cols, nnz)) from the column extent, the other two
// from m.  A neighbour-sampled block (96 seeds x 257 sampled nodes, fanout 10) runs a wave per row and a lane group per
// column.
// This file holds the per-row routines and the launch functions; the kernels that call the former, their grids and the
// choice between the two forms are the shared shell of dfgnn_pair_shell.hpp, which GtTrainOp below plugs into.
#include "dfgnn_launch.hpp"
#include "dfgnn_pair_shell.hpp"
#include "dfgnn_rows.hpp"

namespace dfgnn {

// Everything the per-row routines need; at_head() offsets the feature pointers to the workgroup's head.
struct GtTrain {
  int m, n_cols, nnz, h, f, head;             // m rows (queries, outputs) x n_cols columns (keys, values)
  size_t hf;
  const int *row_ptr, *col_ind;                // CSR
  const float *val;                            // CSR order, NULL = unit values
  const int *col_ptr, *row_ind, *val_idx;      // CSC (column pass)
  const float *Qh, *Kh, *Vh, *dOh, *Oh;        // features, output gradient, forward output (+ head * f)
  float *row_max, *row_sum, *delta;            // [m, h]: written by the forward / the CSR pass, read by the passes after
  float *outh, *dQh, *dKh, *dVh;               // (+ head * f)
  __device__ __forceinline__ size_t nh(int node) const { return (size_t)node * h + head; }
  __device__ __forceinline__ void at_head(int hd) {
    head = hd;
    const size_t o = (size_t)hd * f;
    Qh += o; Kh += o; Vh += o;
    if (dOh) dOh += o;
    if (Oh) Oh += o;
    if (outh) outh += o;
    if (dQh) dQh += o;
    if (dKh) dKh += o;
    if (dVh) dVh += o;
  }
};

// ======================================================================================================================
// forward, a wave per row: 64-edge tiles as gt_row_online (sw / sc: the wave's 64-float / 64-int LDS scratch)
// ======================================================================================================================
template <class C>
__device__ __forceinline__ void gt_fwd_row_wave(const GtTrain &a, int r, int lane, float *sw, int *sc) {
  const int gid = lane / C::G, gl = lane % C::G;
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  Frag<C> q, acc;
  frag_load<C>(q, a.Qh + (size_t)r * a.hf, a.f, gl);
  frag_zero<C>(acc);
  float m_run = -INFINITY, l_run = 0.f;
  for (int t0 = 0; t0 < deg; t0 += kWave) {
    const int nt = min(kWave, deg - t0);
    sc[lane] = (lane < nt) ? a.col_ind[lb + t0 + lane] : 0;
    wave_sync();
    tile_dots<C>(q, sc, nt, a.Kh, a.hf, a.f, gid, gl, sw);
    wave_sync();
    float s = -INFINITY;
    if (lane < nt) s = a.val ? sw[lane] * a.val[lb + t0 + lane] : sw[lane];
    online_step<C>(s, lane, sw, acc, m_run, l_run);
    wave_sync();
    spmm_accum<C>(acc, sw, sc, nt, a.Vh, a.hf, a.f, gid, gl);
    wave_sync();
  }
  const float inv = (l_run != 0.f) ? 1.f / l_run : 0.f;  // empty row -> 0 (fused_gtconv_hyper.cu:143)
  frag_reduce_groups<C>(acc);
  if (gid == 0) frag_store_scaled<C>(acc, inv, a.outh + (size_t)r * a.hf, a.f, gl);
  if (lane == 0 && a.row_max) {
    a.row_max[a.nh(r)] = deg > 0 ? m_run : -1e38f;  // the sentinel of the dense statistics pair (include/dfgnn.h)
    a.row_sum[a.nh(r)] = l_run;
  }
}

// ======================================================================================================================
// a group of G lanes (one feature row wide) per row / column, everything in registers, no LDS.  COOP: the row is taken by
// all EPW groups of the wave together (group gid: edges gid, gid + EPW, ...) and the partial results are merged across
// the groups -- the long rows of a low-degree graph, and EVERY row of the wave-per-row form of the two backward passes.
// ======================================================================================================================
template <class C, bool COOP>
__device__ __forceinline__ void gt_fwd_row_group(const GtTrain &a, int r, int gid, int gl) {
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  Frag<C> q, acc;
  frag_load<C>(q, a.Qh + (size_t)r * a.hf, a.f, gl);
  frag_zero<C>(acc);
  float m_run = -INFINITY, l_run = 0.f;  // online softmax: one sweep, one dependent gather chain per edge
  for (int e = COOP ? gid : 0; e < deg; e += COOP ? C::EPW : 1) {
    const int c = a.col_ind[lb + e];
    Frag<C> k, v;
    frag_load<C>(k, a.Kh + (size_t)c * a.hf, a.f, gl);
    frag_load<C>(v, a.Vh + (size_t)c * a.hf, a.f, gl);
    float s = lanes_sum<C::G>(frag_dot<C>(q, k));
    if (a.val) s *= a.val[lb + e];
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
    frag_store_scaled<C>(acc, l_run != 0.f ? 1.f / l_run : 0.f, a.outh + (size_t)r * a.hf, a.f, gl);
    if (gl == 0 && a.row_max) {
      a.row_max[a.nh(r)] = deg > 0 ? m_run : -1e38f;
      a.row_sum[a.nh(r)] = l_run;
    }
  }
}

// CSR pass, row r: delta_r = <dO_r, out_r> -> delta; dQ_r = sum_e P_e (dP_e - delta_r) val_e K_c in one sweep, two
// edges (four gathers) in flight per group.  Every lane of a group holds the two dot products of its edge (lanes_sum is
// an all-reduce), so the edge's weight needs no exchange.
template <class C, bool COOP>
__device__ __forceinline__ void gt_bwd_row_group(const GtTrain &a, int r, int gid, int gl) {
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
    const float mx = a.row_max[a.nh(r)], inv = 1.f / a.row_sum[a.nh(r)];
    auto weight = [&](int e, const Frag<C> &k, const Frag<C> &v) {  // dS_e val_e
      const float vl = a.val ? a.val[lb + e] : 1.f;
      const float s = vl * lanes_sum<C::G>(frag_dot<C>(q, k));
      const float dp = lanes_sum<C::G>(frag_dot<C>(go, v));
      return fast_exp(s - mx) * inv * (dp - dl) * vl;
    };
    int e = COOP ? gid : 0;
    for (; e + es < deg; e += 2 * es) {
      const int c0 = a.col_ind[lb + e], c1 = a.col_ind[lb + e + es];
      Frag<C> k0, v0, k1, v1;
      frag_load<C>(k0, a.Kh + (size_t)c0 * a.hf, a.f, gl);
      frag_load<C>(v0, a.Vh + (size_t)c0 * a.hf, a.f, gl);
      frag_load<C>(k1, a.Kh + (size_t)c1 * a.hf, a.f, gl);
      frag_load<C>(v1, a.Vh + (size_t)c1 * a.hf, a.f, gl);
      frag_fma<C>(acc, weight(e, k0, v0), k0);
      frag_fma<C>(acc, weight(e + es, k1, v1), k1);
    }
    for (; e < deg; e += es) {
      const int c0 = a.col_ind[lb + e];
      Frag<C> k0, v0;
      frag_load<C>(k0, a.Kh + (size_t)c0 * a.hf, a.f, gl);
      frag_load<C>(v0, a.Vh + (size_t)c0 * a.hf, a.f, gl);
      frag_fma<C>(acc, weight(e, k0, v0), k0);
    }
  }
  if constexpr (COOP) frag_reduce_groups<C>(acc);
  if (!COOP || gid == 0) {
    frag_store_scaled<C>(acc, 1.f, a.dQh + (size_t)r * a.hf, a.f, gl);
    if (gl == 0) a.delta[a.nh(r)] = dl;
  }
}

// CSC pass, column j: dV_j = sum P_e dO_i, dK_j = sum P_e (dP_e - delta_i) val_e Q_i over the column's entries, two
// entries (four gathers + their row scalars) in flight per group.  An empty column writes zeros.
template <class C, bool COOP>
__device__ __forceinline__ void gt_bwd_col_group(const GtTrain &a, int j, int gid, int gl) {
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
      float vl, mx, sum, dl;
    };
    auto entry = [&](int t) {
      Entry x;
      x.i = a.row_ind[lb + t];
      x.vl = a.val ? a.val[a.val_idx[lb + t]] : 1.f;  // val is in CSR order; unit values never touch val_idx
      const size_t s = a.nh(x.i);
      x.mx = a.row_max[s];
      x.sum = a.row_sum[s];
      x.dl = a.delta[s];
      return x;
    };
    auto accum = [&](const Entry &x, const Frag<C> &qi, const Frag<C> &gi) {
      const float s = x.vl * lanes_sum<C::G>(frag_dot<C>(qi, k));
      const float dp = lanes_sum<C::G>(frag_dot<C>(gi, v));
      const float p = fast_exp(s - x.mx) * __builtin_amdgcn_rcpf(x.sum);
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
// the operator as dfgnn_pair_shell.hpp sees it: the kernels, their grids and the launch are there.
// ======================================================================================================================
constexpr int kGtGroupMaxDegree = 24;  // a lane-group wave with a longer row takes its rows cooperatively
struct GtTrainOp {
  using Args = GtTrain;
  static constexpr int kGroupMaxDegree = kGtGroupMaxDegree;
  static constexpr bool kFwdTiles = true;
  template <class C>
  static __device__ __forceinline__ void fwd_row_wave(const Args &a, int r, int lane, float *sw, int *sc) {
    gt_fwd_row_wave<C>(a, r, lane, sw, sc);
  }
  template <class C, int PASS, bool COOP>
  static __device__ __forceinline__ void group_pass(const Args &a, int r, int gid, int gl) {
    if constexpr (PASS == 0) gt_fwd_row_group<C, COOP>(a, r, gid, gl);
    else if constexpr (PASS == 1) gt_bwd_row_group<C, COOP>(a, r, gid, gl);
    else gt_bwd_col_group<C, COOP>(a, r, gid, gl);
  }
};

static GtTrain gt_train_args(const Csr &g, const float *Q, const float *K, const float *V) {
  GtTrain a{};
  a.m = g.m; a.n_cols = g.n_cols; a.nnz = g.nnz; a.h = g.h; a.f = g.f; a.hf = (size_t)g.h * g.f;
  a.row_ptr = g.row_ptr; a.col_ind = g.col_ind; a.val = g.val;
  a.Qh = Q; a.Kh = K; a.Vh = V;
  return a;
}

int launch_gt_train_fwd(const Csr &g, const float *Q, const float *K, const float *V, float *row_max, float *row_sum,
                        float *out, hipStream_t s) {
  GtTrain a = gt_train_args(g, Q, K, V);
  a.outh = out; a.row_max = row_max; a.row_sum = row_sum;
  const bool v4 = (g.f % 4 == 0) && aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(out);
  return launch_pair_pass<GtTrainOp, 0>(a, v4, s);
}

int launch_gt_train_bwd_rows(const Csr &g, const float *Q, const float *K, const float *V, const float *out,
                             const float *row_max, const float *row_sum, const float *grad_out, float *delta, float *dQ,
                             hipStream_t s) {
  GtTrain a = gt_train_args(g, Q, K, V);
  a.Oh = out; a.dOh = grad_out; a.delta = delta; a.dQh = dQ;
  a.row_max = const_cast<float *>(row_max); a.row_sum = const_cast<float *>(row_sum);
  const bool v4 = (g.f % 4 == 0) && aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(out) &&
                  aligned16(grad_out) && aligned16(dQ);
  return launch_pair_pass<GtTrainOp, 1>(a, v4, s);
}

int launch_gt_train_bwd_cols(const Csr &g, const int *col_ptr, const int *row_ind, const int *val_idx, const float *Q,
                             const float *K, const float *V, const float *row_max, const float *row_sum,
                             const float *delta, const float *grad_out, float *dK, float *dV, hipStream_t s) {
  GtTrain a = gt_train_args(g, Q, K, V);
  a.col_ptr = col_ptr; a.row_ind = row_ind; a.val_idx = val_idx;
  a.dOh = grad_out; a.dKh = dK; a.dVh = dV;
  a.row_max = const_cast<float *>(row_max); a.row_sum = const_cast<float *>(row_sum);
  a.delta = const_cast<float *>(delta);
  const bool v4 = (g.f % 4 == 0) && aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(grad_out) &&
                  aligned16(dK) && aligned16(dV);
  return launch_pair_pass<GtTrainOp, 2>(a, v4, s);
}

}  // namespace dfgnn
