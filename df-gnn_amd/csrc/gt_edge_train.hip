// gt_edge_train.hip -- GT conv with a per-edge FEATURE VECTOR added to keys and values for gfx950: fused inference and
// training pair, general kernels (any graph, no plan, no degree limit).  PyG's TransformerConv(edge_dim=...), Shaw-style
// relative position vectors, the edge channel of GPS / GRIT-type models: edge e = (i, j) carries E_e in R^f per head, and
//   k~_e   = K_j + E_e                  v~_e = V_j + E_e                  (one E serves key and value)
//   s_e    = val_e <Q_i, k~_e>
//   P_e    = exp(s_e - row_max_i) / row_sum_i
//   out_i  = sum_e P_e v~_e
//   delta_i = <dO_i, out_i>
//   dP_e   = <dO_i, v~_e>
//   dS_e   = P_e (dP_e - delta_i)
//   dQ_i   = sum_e dS_e val_e k~_e
//   dK_j   = sum_e dS_e val_e Q_i
//   dV_j   = sum_e P_e dO_i
//   dE_e   = dS_e val_e Q_i + P_e dO_i
// E, dE: fp32[nnz, h, f] in CSR edge order -- the feature layout with the edge in place of the node, so the row of (edge
// e, head) starts at (e h + head) f and a row's edges are one contiguous block; offsets are size_t (nnz h f exceeds 2^31).
// E cannot be folded into Q, K, V or val: <Q_i, E_e> is a per-edge scalar of the trainable Q, and P_e E_e enters out.
//
// The structure is gt_bias_train.hip's, pass for pass -- forward, CSR backward pass, CSC backward pass; each as a wave per
// row / column and, for low-degree graphs (nnz < 8 m), as a group of G lanes per row / column with the cooperative switch
// for long rows; two floats saved per (row, head); no atomics, fixed summation order.  The kernels, their grids and the
// choice between the two forms are the shared shell of dfgnn_pair_shell.hpp (GtEdgeOp below plugs into it); the per-row
// routines are this file's own, a copy with E worked in, so that the existing pairs' code objects stay as they are:
//   forward           one more fragment load per edge, of E_e at the edge's own slot (no index), added to the K_j and V_j
//                     fragments before the dot product and the accumulate.  The wave form's 64-edge tiles go through
//                     gte_tile_dots / gte_spmm_accum below, the tile routines of dfgnn_rows.hpp with that load
//   backward, CSR     owns edge e: after k += E_e, v += E_e it holds dS_e, P_e, Q_i, dO_i in registers and the lanes of
//                     the group store their slices of dE_e -- one contiguous f-float row per edge, plain stores that cover
//                     every slot (no pre-zeroing).  dE == NULL: nothing of size nnz h f is written
//   backward, CSC     gathers the row E[val_idx[t]] next to Q_i, dO_i and the three row scalars and recomputes P_e and dS_e;
//                     val_idx is therefore always read
// The sum k + E is formed first and the dot product taken of it, in all three passes alike, so the logit a backward pass
// recomputes is the forward's to the bit; with E = 0 every output equals gt_train.hip's.
// An empty row: out = 0, row_max = -1e38, row_sum = 0, dQ = 0.
#include "dfgnn_launch.hpp"
#include "dfgnn_pair_shell.hpp"
#include "dfgnn_rows.hpp"

namespace dfgnn {

// Everything the per-row routines need; at_head() offsets the feature pointers, E and dE to the workgroup's head.
struct GtEdge {
  int m, n_cols, nnz, h, f, head;             // m rows (queries, outputs) x n_cols columns (keys, values)
  size_t hf;
  const int *row_ptr, *col_ind;                // CSR
  const float *val;                            // CSR order, NULL = unit values
  const float *Eh;                             // [nnz, h, f] CSR order (+ head * f): edge e's row starts at e * hf
  float *dEh;                                  // [nnz, h, f] (+ head * f), NULL = not wanted
  const int *col_ptr, *row_ind, *val_idx;      // CSC (column pass)
  const float *Qh, *Kh, *Vh, *dOh, *Oh;        // features, output gradient, forward output (+ head * f)
  float *row_max, *row_sum, *delta;            // [m, h]: written by the forward / the CSR pass, read by the passes after
  float *outh, *dQh, *dKh, *dVh;               // (+ head * f)
  __device__ __forceinline__ size_t nh(int node) const { return (size_t)node * h + head; }
  __device__ __forceinline__ void at_head(int hd) {
    head = hd;
    const size_t o = (size_t)hd * f;
    Qh += o; Kh += o; Vh += o;
    if (Eh) Eh += o;
    if (dEh) dEh += o;
    if (dOh) dOh += o;
    if (Oh) Oh += o;
    if (outh) outh += o;
    if (dQh) dQh += o;
    if (dKh) dKh += o;
    if (dVh) dVh += o;
  }
};

// 1 / row_sum; an empty row (row_sum = 0) has no edges, the value is never multiplied with anything but zeros
__device__ __forceinline__ float gte_inv_sum(float sum) { return sum != 0.f ? 1.f / sum : 0.f; }

template <class C>
__device__ __forceinline__ void frag_add(Frag<C> &a, const Frag<C> &b) {
#pragma unroll
  for (int ch = 0; ch < C::NCH; ++ch)
#pragma unroll
    for (int k = 0; k < C::VEC; ++k) a.v[ch][k] += b.v[ch][k];
}

// <a, b + c>, the sum formed first: the bits of frag_add followed by frag_dot, without a fragment for the sum
template <class C>
__device__ __forceinline__ float frag_dot_sum(const Frag<C> &a, const Frag<C> &b, const Frag<C> &c) {
  float d = 0.f;
#pragma unroll
  for (int ch = 0; ch < C::NCH; ++ch)
#pragma unroll
    for (int k = 0; k < C::VEC; ++k) d = fmaf(a.v[ch][k], b.v[ch][k] + c.v[ch][k], d);
  return d;
}

// ======================================================================================================================
// the tile routines of the wave-per-row forward: tile_dots / spmm_accum (dfgnn_rows.hpp, dfgnn_device.hpp) with the tile's
// E rows, which are contiguous from Et = E + (lb + t0) hf.  Two edges (four loads) in flight per group.
// ======================================================================================================================
// d_e = <a, X[cols[e]] + Et[e]> for the nt (<= 64) edges of a tile; lane 0 of each group writes sw[e]
template <class C>
__device__ __forceinline__ void gte_tile_dots(const Frag<C> &a, const int *cols, int nt, const float *__restrict__ X,
                                              const float *__restrict__ Et, size_t hf, int f, int gid, int gl,
                                              float *sw) {
  int e = gid;
  for (; e + C::EPW < nt; e += 2 * C::EPW) {
    Frag<C> x0, x1, e0, e1;
    frag_load<C>(x0, X + (size_t)cols[e] * hf, f, gl);
    frag_load<C>(e0, Et + (size_t)e * hf, f, gl);
    frag_load<C>(x1, X + (size_t)cols[e + C::EPW] * hf, f, gl);
    frag_load<C>(e1, Et + (size_t)(e + C::EPW) * hf, f, gl);
    frag_add<C>(x0, e0);
    frag_add<C>(x1, e1);
    const float d0 = lanes_sum<C::G>(frag_dot<C>(a, x0)), d1 = lanes_sum<C::G>(frag_dot<C>(a, x1));
    if (gl == 0) {
      sw[e] = d0;
      sw[e + C::EPW] = d1;
    }
  }
  for (; e < nt; e += C::EPW) {
    Frag<C> x0, e0;
    frag_load<C>(x0, X + (size_t)cols[e] * hf, f, gl);
    frag_load<C>(e0, Et + (size_t)e * hf, f, gl);
    frag_add<C>(x0, e0);
    const float d0 = lanes_sum<C::G>(frag_dot<C>(a, x0));
    if (gl == 0) sw[e] = d0;
  }
}

// acc += sum_{e<n} w[e] (X[cols[e]] + Et[e]); the wave's EPW groups stride over the n edges, each in increasing order
template <class C>
__device__ __forceinline__ void gte_spmm_accum(Frag<C> &acc, const float *w, const int *cols, int n,
                                               const float *__restrict__ X, const float *__restrict__ Et, size_t hf,
                                               int f, int gid, int gl) {
  int e = gid;
  for (; e + C::EPW < n; e += 2 * C::EPW) {
    const int c0 = cols[e], c1 = cols[e + C::EPW];
    const float w0 = w[e], w1 = w[e + C::EPW];
    Frag<C> x0, x1, e0, e1;
    frag_load<C>(x0, X + (size_t)c0 * hf, f, gl);
    frag_load<C>(e0, Et + (size_t)e * hf, f, gl);
    frag_load<C>(x1, X + (size_t)c1 * hf, f, gl);
    frag_load<C>(e1, Et + (size_t)(e + C::EPW) * hf, f, gl);
    frag_add<C>(x0, e0);
    frag_add<C>(x1, e1);
    frag_fma<C>(acc, w0, x0);
    frag_fma<C>(acc, w1, x1);
  }
  for (; e < n; e += C::EPW) {
    Frag<C> x0, e0;
    frag_load<C>(x0, X + (size_t)cols[e] * hf, f, gl);
    frag_load<C>(e0, Et + (size_t)e * hf, f, gl);
    frag_add<C>(x0, e0);
    frag_fma<C>(acc, w[e], x0);
  }
}

// ======================================================================================================================
// forward, a wave per row: 64-edge tiles (sw / sc: the wave's 64-float / 64-int LDS scratch)
// ======================================================================================================================
template <class C>
__device__ __forceinline__ void gte_fwd_row_wave(const GtEdge &a, int r, int lane, float *sw, int *sc) {
  const int gid = lane / C::G, gl = lane % C::G;
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  Frag<C> q, acc;
  frag_load<C>(q, a.Qh + (size_t)r * a.hf, a.f, gl);
  frag_zero<C>(acc);
  float m_run = -INFINITY, l_run = 0.f;
  for (int t0 = 0; t0 < deg; t0 += kWave) {
    const int nt = min(kWave, deg - t0);
    const float *Et = a.Eh + ((size_t)lb + t0) * a.hf;
    sc[lane] = (lane < nt) ? a.col_ind[lb + t0 + lane] : 0;
    wave_sync();
    gte_tile_dots<C>(q, sc, nt, a.Kh, Et, a.hf, a.f, gid, gl, sw);
    wave_sync();
    float s = -INFINITY;
    if (lane < nt) s = a.val ? sw[lane] * a.val[lb + t0 + lane] : sw[lane];
    online_step<C>(s, lane, sw, acc, m_run, l_run);
    wave_sync();
    gte_spmm_accum<C>(acc, sw, sc, nt, a.Vh, Et, a.hf, a.f, gid, gl);
    wave_sync();
  }
  const float inv = gte_inv_sum(l_run);  // empty row -> 0
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
template <class C, bool COOP>
__device__ __forceinline__ void gte_fwd_row_group(const GtEdge &a, int r, int gid, int gl) {
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  Frag<C> q, acc;
  frag_load<C>(q, a.Qh + (size_t)r * a.hf, a.f, gl);
  frag_zero<C>(acc);
  float m_run = -INFINITY, l_run = 0.f;  // online softmax: one sweep, one dependent gather chain per edge
  for (int e = COOP ? gid : 0; e < deg; e += COOP ? C::EPW : 1) {
    const int c = a.col_ind[lb + e];
    Frag<C> k, v, x;
    frag_load<C>(k, a.Kh + (size_t)c * a.hf, a.f, gl);
    frag_load<C>(v, a.Vh + (size_t)c * a.hf, a.f, gl);
    frag_load<C>(x, a.Eh + ((size_t)lb + e) * a.hf, a.f, gl);  // the edge's own slot: no index
    frag_add<C>(k, x);
    frag_add<C>(v, x);
    float s = lanes_sum<C::G>(frag_dot<C>(q, k));
    if (a.val) s *= a.val[lb + e];
    const float m_new = fmaxf(m_run, s);
    const float sc = (m_run == -INFINITY) ? 0.f : fast_exp(m_run - m_new);
    const float p = fast_exp(s - m_new);
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
    frag_store_scaled<C>(acc, gte_inv_sum(l_run), a.outh + (size_t)r * a.hf, a.f, gl);
    if (gl == 0 && a.row_max) {
      a.row_max[a.nh(r)] = deg > 0 ? m_run : -1e38f;
      a.row_sum[a.nh(r)] = l_run;
    }
  }
}

// CSR pass, row r: delta_r = <dO_r, out_r> -> delta; dQ_r = sum_e dS_e val_e (K_c + E_e) and the row dE_e in one sweep,
// two edges (six loads) in flight per group.  Every lane of a group holds the two dot products of its edge (lanes_sum is
// an all-reduce), so the edge's dS and P need no exchange: each lane stores its slice of dE_e = dS_e val_e Q_r + P_e dO_r.
template <class C, bool COOP>
__device__ __forceinline__ void gte_bwd_row_group(const GtEdge &a, int r, int gid, int gl) {
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
    // k, v: K_c + E_e, V_c + E_e.  Stores dE_e when it is wanted; returns dS_e val_e
    auto weight = [&](int e, const Frag<C> &k, const Frag<C> &v) {
      const float vl = a.val ? a.val[lb + e] : 1.f;
      const float s = vl * lanes_sum<C::G>(frag_dot<C>(q, k));
      const float dp = lanes_sum<C::G>(frag_dot<C>(go, v));
      const float p = fast_exp(s - mx) * inv;
      const float w = p * (dp - dl) * vl;
      if (a.dEh) {
        Frag<C> de;
        frag_zero<C>(de);
        frag_fma<C>(de, p, go);
        frag_fma<C>(de, w, q);
        frag_store_scaled<C>(de, 1.f, a.dEh + ((size_t)lb + e) * a.hf, a.f, gl);
      }
      return w;
    };
    int e = COOP ? gid : 0;
    for (; e + es < deg; e += 2 * es) {
      const int c0 = a.col_ind[lb + e], c1 = a.col_ind[lb + e + es];
      Frag<C> k0, v0, x0, k1, v1, x1;
      frag_load<C>(k0, a.Kh + (size_t)c0 * a.hf, a.f, gl);
      frag_load<C>(v0, a.Vh + (size_t)c0 * a.hf, a.f, gl);
      frag_load<C>(x0, a.Eh + ((size_t)lb + e) * a.hf, a.f, gl);
      frag_load<C>(k1, a.Kh + (size_t)c1 * a.hf, a.f, gl);
      frag_load<C>(v1, a.Vh + (size_t)c1 * a.hf, a.f, gl);
      frag_load<C>(x1, a.Eh + ((size_t)lb + e + es) * a.hf, a.f, gl);
      frag_add<C>(k0, x0);
      frag_add<C>(v0, x0);
      frag_add<C>(k1, x1);
      frag_add<C>(v1, x1);
      frag_fma<C>(acc, weight(e, k0, v0), k0);
      frag_fma<C>(acc, weight(e + es, k1, v1), k1);
    }
    for (; e < deg; e += es) {
      const int c0 = a.col_ind[lb + e];
      Frag<C> k0, v0, x0;
      frag_load<C>(k0, a.Kh + (size_t)c0 * a.hf, a.f, gl);
      frag_load<C>(v0, a.Vh + (size_t)c0 * a.hf, a.f, gl);
      frag_load<C>(x0, a.Eh + ((size_t)lb + e) * a.hf, a.f, gl);
      frag_add<C>(k0, x0);
      frag_add<C>(v0, x0);
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
// entries (six gathers + their row scalars and edge value) in flight per group.  An empty column writes zeros.
template <class C, bool COOP>
__device__ __forceinline__ void gte_bwd_col_group(const GtEdge &a, int j, int gid, int gl) {
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
      int i, e;
      float vl, mx, sum, dl;
    };
    auto entry = [&](int t) {
      Entry x;
      x.i = a.row_ind[lb + t];
      x.e = a.val_idx[lb + t];  // val and E are in CSR order
      x.vl = a.val ? a.val[x.e] : 1.f;
      const size_t s = a.nh(x.i);
      x.mx = a.row_max[s];
      x.sum = a.row_sum[s];
      x.dl = a.delta[s];
      return x;
    };
    auto accum = [&](const Entry &x, const Frag<C> &qi, const Frag<C> &gi, const Frag<C> &xe) {
      const float s = x.vl * lanes_sum<C::G>(frag_dot_sum<C>(qi, k, xe));
      const float dp = lanes_sum<C::G>(frag_dot_sum<C>(gi, v, xe));
      const float p = fast_exp(s - x.mx) * __builtin_amdgcn_rcpf(x.sum);
      frag_fma<C>(aV, p, gi);
      frag_fma<C>(aK, p * (dp - x.dl) * x.vl, qi);
    };
    int t = COOP ? gid : 0;
    for (; t + es < n; t += 2 * es) {
      const Entry x0 = entry(t), x1 = entry(t + es);
      Frag<C> q0, g0, e0, q1, g1, e1;
      frag_load<C>(q0, a.Qh + (size_t)x0.i * a.hf, a.f, gl);
      frag_load<C>(g0, a.dOh + (size_t)x0.i * a.hf, a.f, gl);
      frag_load<C>(e0, a.Eh + (size_t)x0.e * a.hf, a.f, gl);
      frag_load<C>(q1, a.Qh + (size_t)x1.i * a.hf, a.f, gl);
      frag_load<C>(g1, a.dOh + (size_t)x1.i * a.hf, a.f, gl);
      frag_load<C>(e1, a.Eh + (size_t)x1.e * a.hf, a.f, gl);
      accum(x0, q0, g0, e0);
      accum(x1, q1, g1, e1);
    }
    for (; t < n; t += es) {
      const Entry x0 = entry(t);
      Frag<C> q0, g0, e0;
      frag_load<C>(q0, a.Qh + (size_t)x0.i * a.hf, a.f, gl);
      frag_load<C>(g0, a.dOh + (size_t)x0.i * a.hf, a.f, gl);
      frag_load<C>(e0, a.Eh + (size_t)x0.e * a.hf, a.f, gl);
      accum(x0, q0, g0, e0);
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
constexpr int kGtEdgeGroupMaxDegree = 24;  // a lane-group wave with a longer row takes its rows cooperatively
struct GtEdgeOp {
  using Args = GtEdge;
  static constexpr int kGroupMaxDegree = kGtEdgeGroupMaxDegree;
  static constexpr bool kFwdTiles = true;
  template <class C>
  static __device__ __forceinline__ void fwd_row_wave(const Args &a, int r, int lane, float *sw, int *sc) {
    gte_fwd_row_wave<C>(a, r, lane, sw, sc);
  }
  template <class C, int PASS, bool COOP>
  static __device__ __forceinline__ void group_pass(const Args &a, int r, int gid, int gl) {
    if constexpr (PASS == 0) gte_fwd_row_group<C, COOP>(a, r, gid, gl);
    else if constexpr (PASS == 1) gte_bwd_row_group<C, COOP>(a, r, gid, gl);
    else gte_bwd_col_group<C, COOP>(a, r, gid, gl);
  }
};

static GtEdge gt_edge_args(const Csr &g, const float *E, const float *Q, const float *K, const float *V) {
  GtEdge a{};
  a.m = g.m; a.n_cols = g.n_cols; a.nnz = g.nnz; a.h = g.h; a.f = g.f; a.hf = (size_t)g.h * g.f;
  a.row_ptr = g.row_ptr; a.col_ind = g.col_ind; a.val = g.val; a.Eh = E;
  a.Qh = Q; a.Kh = K; a.Vh = V;
  return a;
}

int launch_gt_edge_fwd(const Csr &g, const float *E, const float *Q, const float *K, const float *V, float *row_max,
                       float *row_sum, float *out, hipStream_t s) {
  GtEdge a = gt_edge_args(g, E, Q, K, V);
  a.outh = out; a.row_max = row_max; a.row_sum = row_sum;
  const bool v4 = (g.f % 4 == 0) && aligned16(E) && aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(out);
  return launch_pair_pass<GtEdgeOp, 0>(a, v4, s);
}

int launch_gt_edge_bwd_rows(const Csr &g, const float *E, const float *Q, const float *K, const float *V,
                            const float *out, const float *row_max, const float *row_sum, const float *grad_out,
                            float *delta, float *dQ, float *dE, hipStream_t s) {
  GtEdge a = gt_edge_args(g, E, Q, K, V);
  a.Oh = out; a.dOh = grad_out; a.delta = delta; a.dQh = dQ; a.dEh = dE;
  a.row_max = const_cast<float *>(row_max); a.row_sum = const_cast<float *>(row_sum);
  const bool v4 = (g.f % 4 == 0) && aligned16(E) && aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(out) &&
                  aligned16(grad_out) && aligned16(dQ) && aligned16(dE);
  return launch_pair_pass<GtEdgeOp, 1>(a, v4, s);
}

int launch_gt_edge_bwd_cols(const Csr &g, const float *E, const int *col_ptr, const int *row_ind, const int *val_idx,
                            const float *Q, const float *K, const float *V, const float *row_max, const float *row_sum,
                            const float *delta, const float *grad_out, float *dK, float *dV, hipStream_t s) {
  GtEdge a = gt_edge_args(g, E, Q, K, V);
  a.col_ptr = col_ptr; a.row_ind = row_ind; a.val_idx = val_idx;
  a.dOh = grad_out; a.dKh = dK; a.dVh = dV;
  a.row_max = const_cast<float *>(row_max); a.row_sum = const_cast<float *>(row_sum);
  a.delta = const_cast<float *>(delta);
  const bool v4 = (g.f % 4 == 0) && aligned16(E) && aligned16(Q) && aligned16(K) && aligned16(V) &&
                  aligned16(grad_out) && aligned16(dK) && aligned16(dV);
  return launch_pair_pass<GtEdgeOp, 2>(a, v4, s);
}

}  // namespace dfgnn
