// gt_typed_train.hip -- GT conv with TYPED edges for gfx950: the vector added to keys and values is looked up from a small
// table by the edge's type.  Fused inference and training pair, general kernels (any graph, no plan, no degree limit).
// Shaw-style relative positions, RGAT / HGT-style relation vectors, bucketed distances, bond types: edge e = (i, j) has
// a type t = etype[e] in [0, T), the table is R[T, h, f], and per head
//   k~_e   = K_j + R_t                  v~_e = V_j + R_t                  (one table serves key and value)
//   s_e    = val_e <Q_i, k~_e>
//   P_e    = exp(s_e - row_max_i) / row_sum_i
//   out_i  = sum_e P_e v~_e
//   delta_i = <dO_i, out_i>
//   dP_e   = <dO_i, v~_e>
//   dS_e   = P_e (dP_e - delta_i)
//   dQ_i   = sum_e dS_e val_e k~_e
//   dK_j   = sum_e dS_e val_e Q_i
//   dV_j   = sum_e P_e dO_i
//   dR_t   = sum_{e : etype[e] = t} (dS_e val_e Q_i + P_e dO_i)
// which is gt_edge_train.hip with E_e = R[etype[e]] and dR = index_add(dE, etype) -- without anything of size nnz h f:
// an edge costs 4 bytes of type instead of 4 h f bytes of E, and dE is never written.
//
// The structure is gt_edge_train.hip's, pass for pass, and the code is a copy with the lookup worked in, so that the
// existing pairs' code objects stay as they are and this operator is one file:
//   forward           the load of E_e becomes a load of the type and of the row R[(t h + head) f ..]; the wave form
//                     reads a tile's 64 types as one coalesced load next to the column ids
//   backward, CSC     takes its types from etype_csc[nnz], the types in CSC entry order (made once per graph by the
//                     caller): a stream, not a gather through val_idx, which is read only for edge values
//   backward, CSR     dR == NULL: the edge pair's pass, nothing more.  dR != NULL: a bounded number of persistent
//                     workgroups per head (kGtTypedParts at most); every wave owns a table [T, f] in LDS and adds each
//                     edge's dE_e -- formed exactly as gt_edge_train.hip forms it -- to the row of its type, the lane
//                     groups of a wave one after the other (two groups may hold the same type; gtt_table_add); at the
//                     end the workgroup adds its waves' tables in wave order and stores one full partial [T, f] per
//                     head (zeros included) to ws; gt_typed_reduce_kernel then sums the partials in a fixed order.
//                     No atomics, neither global nor LDS: two calls give the same bits
// The table itself is NOT staged in LDS: per head it is at most 32 KB at the supported limit, every workgroup of a head
// reads the same rows, so it lives in L2 (and the hot rows in the vector L1); staging would cost each workgroup a copy of
// T f floats before its first row and the forward its occupancy.
// The sum k + R_t is formed first and the dot product taken of it, in all three passes alike (the frag_add / frag_dot
// sequence of gt_edge_train.hip), so out, the statistics, dQ, dK and dV equal the edge pair's on E = R[etype] to the bit.
// An empty row: out = 0, row_max = -1e38, row_sum = 0, dQ = 0.  col_ind < n_cols, row_ind < m and 0 <= etype < T are the
// caller's contract: the kernels index by them unchecked.
#include "dfgnn_launch.hpp"
#include "dfgnn_rows.hpp"

namespace dfgnn {

// Everything the per-row routines need; at_head() offsets the feature pointers and R to the workgroup's head.
struct GtTyped {
  int m, n_cols, nnz, h, f, head, T;          // m rows (queries, outputs) x n_cols columns (keys, values); T types
  size_t hf;
  const int *row_ptr, *col_ind;                // CSR
  const float *val;                            // CSR order, NULL = unit values
  const int *etype, *etype_csc;                // [nnz] types in CSR order / in CSC entry order
  const float *Rh;                             // [T, h, f] (+ head * f): type t's row starts at t * hf
  float *parts;                                // [workgroups of the CSR pass, T, h, f] partial sums of dR, NULL = not wanted
  const int *col_ptr, *row_ind, *val_idx;      // CSC (column pass)
  const float *Qh, *Kh, *Vh, *dOh, *Oh;        // features, output gradient, forward output (+ head * f)
  float *row_max, *row_sum, *delta;            // [m, h]: written by the forward / the CSR pass, read by the passes after
  float *outh, *dQh, *dKh, *dVh;               // (+ head * f)
  __device__ __forceinline__ size_t nh(int node) const { return (size_t)node * h + head; }
  __device__ __forceinline__ void at_head(int hd) {
    head = hd;
    const size_t o = (size_t)hd * f;
    Qh += o; Kh += o; Vh += o;
    if (Rh) Rh += o;
    if (dOh) dOh += o;
    if (Oh) Oh += o;
    if (outh) outh += o;
    if (dQh) dQh += o;
    if (dKh) dKh += o;
    if (dVh) dVh += o;
  }
};

// 1 / row_sum; an empty row (row_sum = 0) has no edges, the value is never multiplied with anything but zeros
__device__ __forceinline__ float gtt_inv_sum(float sum) { return sum != 0.f ? 1.f / sum : 0.f; }

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
// the tile routines of the wave-per-row forward: gte_tile_dots / gte_spmm_accum of gt_edge_train.hip with the tile's
// types (LDS, next to the column ids) in place of its E rows.  Two edges (four loads) in flight per group.
// ======================================================================================================================
// d_e = <a, X[cols[e]] + R[types[e]]> for the nt (<= 64) edges of a tile; lane 0 of each group writes sw[e]
template <class C>
__device__ __forceinline__ void gtt_tile_dots(const Frag<C> &a, const int *cols, const int *types, int nt,
                                              const float *__restrict__ X, const float *__restrict__ R, size_t hf, int f,
                                              int gid, int gl, float *sw) {
  int e = gid;
  for (; e + C::EPW < nt; e += 2 * C::EPW) {
    Frag<C> x0, x1, e0, e1;
    frag_load<C>(x0, X + (size_t)cols[e] * hf, f, gl);
    frag_load<C>(e0, R + (size_t)types[e] * hf, f, gl);
    frag_load<C>(x1, X + (size_t)cols[e + C::EPW] * hf, f, gl);
    frag_load<C>(e1, R + (size_t)types[e + C::EPW] * hf, f, gl);
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
    frag_load<C>(e0, R + (size_t)types[e] * hf, f, gl);
    frag_add<C>(x0, e0);
    const float d0 = lanes_sum<C::G>(frag_dot<C>(a, x0));
    if (gl == 0) sw[e] = d0;
  }
}

// acc += sum_{e<n} w[e] (X[cols[e]] + R[types[e]]); the wave's EPW groups stride over the n edges, each in increasing order
template <class C>
__device__ __forceinline__ void gtt_spmm_accum(Frag<C> &acc, const float *w, const int *cols, const int *types, int n,
                                               const float *__restrict__ X, const float *__restrict__ R, size_t hf,
                                               int f, int gid, int gl) {
  int e = gid;
  for (; e + C::EPW < n; e += 2 * C::EPW) {
    const int c0 = cols[e], c1 = cols[e + C::EPW];
    const int t0 = types[e], t1 = types[e + C::EPW];
    const float w0 = w[e], w1 = w[e + C::EPW];
    Frag<C> x0, x1, e0, e1;
    frag_load<C>(x0, X + (size_t)c0 * hf, f, gl);
    frag_load<C>(e0, R + (size_t)t0 * hf, f, gl);
    frag_load<C>(x1, X + (size_t)c1 * hf, f, gl);
    frag_load<C>(e1, R + (size_t)t1 * hf, f, gl);
    frag_add<C>(x0, e0);
    frag_add<C>(x1, e1);
    frag_fma<C>(acc, w0, x0);
    frag_fma<C>(acc, w1, x1);
  }
  for (; e < n; e += C::EPW) {
    Frag<C> x0, e0;
    frag_load<C>(x0, X + (size_t)cols[e] * hf, f, gl);
    frag_load<C>(e0, R + (size_t)types[e] * hf, f, gl);
    frag_add<C>(x0, e0);
    frag_fma<C>(acc, w[e], x0);
  }
}

// ======================================================================================================================
// forward, a wave per row: 64-edge tiles (sw / sc / st: the wave's 64-float / 64-int / 64-int LDS scratch)
// ======================================================================================================================
constexpr int kGtTypedScratchPerWave = 3 * kWave;  // weights, column ids, types
template <class C>
__device__ __forceinline__ void gtt_fwd_row_wave(const GtTyped &a, int r, int lane, float *sw, int *sc, int *st) {
  const int gid = lane / C::G, gl = lane % C::G;
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  Frag<C> q, acc;
  frag_load<C>(q, a.Qh + (size_t)r * a.hf, a.f, gl);
  frag_zero<C>(acc);
  float m_run = -INFINITY, l_run = 0.f;
  for (int t0 = 0; t0 < deg; t0 += kWave) {
    const int nt = min(kWave, deg - t0);
    sc[lane] = (lane < nt) ? a.col_ind[lb + t0 + lane] : 0;
    st[lane] = (lane < nt) ? a.etype[lb + t0 + lane] : 0;
    wave_sync();
    gtt_tile_dots<C>(q, sc, st, nt, a.Kh, a.Rh, a.hf, a.f, gid, gl, sw);
    wave_sync();
    float s = -INFINITY;
    if (lane < nt) s = a.val ? sw[lane] * a.val[lb + t0 + lane] : sw[lane];
    online_step<C>(s, lane, sw, acc, m_run, l_run);
    wave_sync();
    gtt_spmm_accum<C>(acc, sw, sc, st, nt, a.Vh, a.Rh, a.hf, a.f, gid, gl);
    wave_sync();
  }
  const float inv = gtt_inv_sum(l_run);  // empty row -> 0
  frag_reduce_groups<C>(acc);
  if (gid == 0) frag_store_scaled<C>(acc, inv, a.outh + (size_t)r * a.hf, a.f, gl);
  if (lane == 0 && a.row_max) {
    a.row_max[a.nh(r)] = deg > 0 ? m_run : -1e38f;  // the sentinel of the statistics pairs (include/dfgnn.h)
    a.row_sum[a.nh(r)] = l_run;
  }
}

// ======================================================================================================================
// a group of G lanes (one feature row wide) per row / column, everything in registers.  COOP: the row is taken by all
// EPW groups of the wave together (group gid: edges gid, gid + EPW, ...) and the partial results are merged across
// the groups -- the long rows of a low-degree graph, and EVERY row of the wave-per-row form of the two backward passes.
// ======================================================================================================================
template <class C, bool COOP>
__device__ __forceinline__ void gtt_fwd_row_group(const GtTyped &a, int r, int gid, int gl) {
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  Frag<C> q, acc;
  frag_load<C>(q, a.Qh + (size_t)r * a.hf, a.f, gl);
  frag_zero<C>(acc);
  float m_run = -INFINITY, l_run = 0.f;  // online softmax: one sweep, one dependent gather chain per edge
  for (int e = COOP ? gid : 0; e < deg; e += COOP ? C::EPW : 1) {
    const int c = a.col_ind[lb + e], t = a.etype[lb + e];
    Frag<C> k, v, x;
    frag_load<C>(k, a.Kh + (size_t)c * a.hf, a.f, gl);
    frag_load<C>(v, a.Vh + (size_t)c * a.hf, a.f, gl);
    frag_load<C>(x, a.Rh + (size_t)t * a.hf, a.f, gl);
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
    frag_store_scaled<C>(acc, gtt_inv_sum(l_run), a.outh + (size_t)r * a.hf, a.f, gl);
    if (gl == 0 && a.row_max) {
      a.row_max[a.nh(r)] = deg > 0 ? m_run : -1e38f;
      a.row_sum[a.nh(r)] = l_run;
    }
  }
}

// tab[t, :] += de for the edges the wave's lane groups hold right now, one group after the other: two groups may hold
// the same type, and a fixed order is what makes the sum reproducible.  Plain LDS loads and stores, a wave's DS
// operations execute in issue order; wave_sync() keeps the compiler from merging or reordering the steps.  The order is
// group order among the groups that reach this call together.  The callers' loops have trip counts that differ per group
// (the two-edge loop against its tail; rows of different degree in the lane-group form), so after the wave has diverged
// the groups of one path add before those of the other, in the order the compiled code serialises the paths: fixed for
// one binary and one input -- two calls give the same bits -- but not a property of the source.
template <class C>
__device__ __forceinline__ void gtt_table_add(float *tab, int t, int f, const Frag<C> &de, int gid, int gl) {
  float *row = tab + (size_t)t * f;
#pragma unroll 1
  for (int g = 0; g < C::EPW; ++g) {
    if (gid == g) {
#pragma unroll
      for (int ch = 0; ch < C::NCH; ++ch) {
        const int c = (ch * C::G + gl) * C::VEC;
        if (c < f) {
#pragma unroll
          for (int k = 0; k < C::VEC; ++k) row[c + k] += de.v[ch][k];
        }
      }
    }
    wave_sync();
  }
}

// CSR pass, row r: delta_r = <dO_r, out_r> -> delta; dQ_r = sum_e dS_e val_e (K_c + R_t) in one sweep, two edges (six
// loads) in flight per group.  Every lane of a group holds the two dot products of its edge (lanes_sum is an all-reduce),
// so the edge's dS and P need no exchange.  TAB: each lane forms its slice of dE_e = dS_e val_e Q_r + P_e dO_r as
// gt_edge_train.hip does and adds it to row t of the wave's LDS table `tab`.
template <class C, bool COOP, bool TAB>
__device__ __forceinline__ void gtt_bwd_row_group(const GtTyped &a, int r, int gid, int gl, float *tab) {
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
    // k, v: K_c + R_t, V_c + R_t.  Adds dE_e to the table when dR is wanted; returns dS_e val_e
    auto weight = [&](int e, int t, const Frag<C> &k, const Frag<C> &v) {
      const float vl = a.val ? a.val[lb + e] : 1.f;
      const float s = vl * lanes_sum<C::G>(frag_dot<C>(q, k));
      const float dp = lanes_sum<C::G>(frag_dot<C>(go, v));
      const float p = fast_exp(s - mx) * inv;
      const float w = p * (dp - dl) * vl;
      if constexpr (TAB) {
        Frag<C> de;
        frag_zero<C>(de);
        frag_fma<C>(de, p, go);
        frag_fma<C>(de, w, q);
        gtt_table_add<C>(tab, t, a.f, de, gid, gl);
      }
      return w;
    };
    int e = COOP ? gid : 0;
    for (; e + es < deg; e += 2 * es) {
      const int c0 = a.col_ind[lb + e], c1 = a.col_ind[lb + e + es];
      const int t0 = a.etype[lb + e], t1 = a.etype[lb + e + es];
      Frag<C> k0, v0, x0, k1, v1, x1;
      frag_load<C>(k0, a.Kh + (size_t)c0 * a.hf, a.f, gl);
      frag_load<C>(v0, a.Vh + (size_t)c0 * a.hf, a.f, gl);
      frag_load<C>(x0, a.Rh + (size_t)t0 * a.hf, a.f, gl);
      frag_load<C>(k1, a.Kh + (size_t)c1 * a.hf, a.f, gl);
      frag_load<C>(v1, a.Vh + (size_t)c1 * a.hf, a.f, gl);
      frag_load<C>(x1, a.Rh + (size_t)t1 * a.hf, a.f, gl);
      frag_add<C>(k0, x0);
      frag_add<C>(v0, x0);
      frag_add<C>(k1, x1);
      frag_add<C>(v1, x1);
      frag_fma<C>(acc, weight(e, t0, k0, v0), k0);
      frag_fma<C>(acc, weight(e + es, t1, k1, v1), k1);
    }
    for (; e < deg; e += es) {
      const int c0 = a.col_ind[lb + e], t0 = a.etype[lb + e];
      Frag<C> k0, v0, x0;
      frag_load<C>(k0, a.Kh + (size_t)c0 * a.hf, a.f, gl);
      frag_load<C>(v0, a.Vh + (size_t)c0 * a.hf, a.f, gl);
      frag_load<C>(x0, a.Rh + (size_t)t0 * a.hf, a.f, gl);
      frag_add<C>(k0, x0);
      frag_add<C>(v0, x0);
      frag_fma<C>(acc, weight(e, t0, k0, v0), k0);
    }
  }
  if constexpr (COOP) frag_reduce_groups<C>(acc);
  if (!COOP || gid == 0) {
    frag_store_scaled<C>(acc, 1.f, a.dQh + (size_t)r * a.hf, a.f, gl);
    if (gl == 0) a.delta[a.nh(r)] = dl;
  }
}

// CSC pass, column j: dV_j = sum P_e dO_i, dK_j = sum P_e (dP_e - delta_i) val_e Q_i over the column's entries, two
// entries (six gathers + their row scalars, type and edge value) in flight per group.  An empty column writes zeros.
template <class C, bool COOP>
__device__ __forceinline__ void gtt_bwd_col_group(const GtTyped &a, int j, int gid, int gl) {
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
      int i, t;
      float vl, mx, sum, dl;
    };
    auto entry = [&](int t) {
      Entry x;
      x.i = a.row_ind[lb + t];
      x.t = a.etype_csc[lb + t];                       // streamed in entry order
      x.vl = a.val ? a.val[a.val_idx[lb + t]] : 1.f;  // val is in CSR order
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
      frag_load<C>(e0, a.Rh + (size_t)x0.t * a.hf, a.f, gl);
      frag_load<C>(q1, a.Qh + (size_t)x1.i * a.hf, a.f, gl);
      frag_load<C>(g1, a.dOh + (size_t)x1.i * a.hf, a.f, gl);
      frag_load<C>(e1, a.Rh + (size_t)x1.t * a.hf, a.f, gl);
      accum(x0, q0, g0, e0);
      accum(x1, q1, g1, e1);
    }
    for (; t < n; t += es) {
      const Entry x0 = entry(t);
      Frag<C> q0, g0, e0;
      frag_load<C>(q0, a.Qh + (size_t)x0.i * a.hf, a.f, gl);
      frag_load<C>(g0, a.dOh + (size_t)x0.i * a.hf, a.f, gl);
      frag_load<C>(e0, a.Rh + (size_t)x0.t * a.hf, a.f, gl);
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
// kernels.  PASS: 0 forward, 1 backward CSR pass, 2 backward CSC pass.  TAB (PASS 1 only): dR is wanted.
// ======================================================================================================================
template <class C, int PASS, bool COOP, bool TAB>
__device__ __forceinline__ void gtt_group_pass(const GtTyped &a, int r, int gid, int gl, float *tab) {
  if constexpr (PASS == 0) gtt_fwd_row_group<C, COOP>(a, r, gid, gl);
  else if constexpr (PASS == 1) gtt_bwd_row_group<C, COOP, TAB>(a, r, gid, gl, tab);
  else gtt_bwd_col_group<C, COOP>(a, r, gid, gl);
}

// The waves' tables of a TAB workgroup: kWavesPerBlock x [T, f] floats of dynamic LDS.
extern __shared__ __attribute__((aligned(16))) float gtt_tables[];

// Start of a TAB kernel: every wave zeroes its own table (no workgroup barrier needed before it adds to it).
__device__ __forceinline__ float *gtt_table_init(const GtTyped &a, int wave, int lane) {
  const int tf = a.T * a.f;
  float *tab = gtt_tables + (size_t)wave * tf;
  for (int i = lane; i < tf; i += kWave) tab[i] = 0.f;
  wave_sync();
  return tab;
}

// End of a TAB kernel: the workgroup's partial [T, f] of this head = its waves' tables added in wave order ->
// parts[blockIdx.x, :, head, :], every slot, the zeros of types it never met included.  Called by every thread.
__device__ __forceinline__ void gtt_table_store(const GtTyped &a) {
  __syncthreads();
  const int tf = a.T * a.f;
  float *dst = a.parts + (size_t)blockIdx.x * a.T * a.hf + (size_t)a.head * a.f;
  for (int i = threadIdx.x; i < tf; i += kBlock) {
    float s = gtt_tables[i];
#pragma unroll
    for (int w = 1; w < kWavesPerBlock; ++w) s += gtt_tables[(size_t)w * tf + i];
    const int t = i / a.f, c = i - t * a.f;
    dst[(size_t)t * a.hf + c] = s;
  }
}

// general: a wave per row / column, grid-strided over the whole graph.  The forward works in 64-edge tiles through the
// wave's LDS scratch; the backward passes are the COOP form of the group routines.
template <class C, int PASS, bool TAB>
__global__ __launch_bounds__(kBlock) void gt_typed_wave_kernel(GtTyped a) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  a.at_head(blockIdx.y);
  const int n = PASS == 2 ? a.n_cols : a.m;  // the extent this pass walks: rows, or (CSC pass) columns
  const int beg = blockIdx.x * kWavesPerBlock + wave, step = gridDim.x * kWavesPerBlock;
  if constexpr (PASS == 0) {
    __shared__ __attribute__((aligned(16))) float lds[kWavesPerBlock * kGtTypedScratchPerWave];
    float *sw = lds + wave * kGtTypedScratchPerWave;
    int *sc = reinterpret_cast<int *>(sw + kWave);
    for (int r = beg; r < n; r += step) gtt_fwd_row_wave<C>(a, r, lane, sw, sc, sc + kWave);
  } else {
    float *tab = nullptr;
    if constexpr (TAB) tab = gtt_table_init(a, wave, lane);
    for (int r = beg; r < n; r += step) gtt_group_pass<C, PASS, true, TAB>(a, r, lane / C::G, lane % C::G, tab);
    if constexpr (TAB) gtt_table_store(a);
  }
}

// low-degree graphs: a workgroup takes blocks of kBlock / G consecutive rows, one lane group per row -- unless a wave's
// EPW rows include one of more than kGtTypedGroupMaxDegree entries, which a single lane group would walk serially while
// the rest of the wave waits: that wave takes its rows one after the other with all its groups on each (COOP).  The choice
// is wave-uniform (ballot): no barrier.  As gt_edge_group_kernel of gt_edge_train.hip, with the same threshold.
constexpr int kGtTypedGroupMaxDegree = 24;
template <class C, int PASS, bool TAB>
__global__ __launch_bounds__(kBlock) void gt_typed_group_kernel(GtTyped a) {
  constexpr int G = C::G, R = kBlock / G;  // rows per block
  const int gid = (threadIdx.x & (kWave - 1)) / G, gl = threadIdx.x % G, wave = threadIdx.x / kWave;
  a.at_head(blockIdx.y);
  const int *ptr = PASS == 2 ? a.col_ptr : a.row_ptr;
  const int n = PASS == 2 ? a.n_cols : a.m;  // the extent this pass walks: rows, or (CSC pass) columns
  float *tab = nullptr;
  if constexpr (TAB) tab = gtt_table_init(a, wave, threadIdx.x & (kWave - 1));
  for (int b0 = blockIdx.x * R; b0 < n; b0 += gridDim.x * R) {
    const int r = b0 + threadIdx.x / G;
    const int deg = r < n ? ptr[r + 1] - ptr[r] : 0;
    if (__any(deg > kGtTypedGroupMaxDegree)) {
      for (int rr = b0 + wave * C::EPW; rr < min(n, b0 + (wave + 1) * C::EPW); ++rr)
        gtt_group_pass<C, PASS, true, TAB>(a, rr, gid, gl, tab);
    } else if (r < n) {
      gtt_group_pass<C, PASS, false, TAB>(a, r, gid, gl, tab);
    }
  }
  if constexpr (TAB) gtt_table_store(a);
}

// dR[c] = sum_p parts[p, c] over the nparts partials of the CSR pass (c over T * h * f): 64 entries per workgroup, wave w
// takes partials w, w + 16, ... in increasing order; the 16 wave sums are added in wave order.  nparts = 0: dR = 0.
constexpr int kGtTypedReduceBlock = 1024, kGtTypedReduceWaves = kGtTypedReduceBlock / kWave;
__global__ __launch_bounds__(kGtTypedReduceBlock) void gt_typed_reduce_kernel(const float *__restrict__ parts, int nparts,
                                                                              int thf, float *__restrict__ dR) {
  __shared__ float red[kGtTypedReduceWaves][kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int c = blockIdx.x * kWave + lane;
  float s = 0.f;
  if (c < thf)
    for (int p = wave; p < nparts; p += kGtTypedReduceWaves) s += parts[(size_t)p * thf + c];
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && c < thf) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < kGtTypedReduceWaves; ++w) t += red[w][lane];
    dR[c] = t;
  }
}

// grids.  Forward, CSC pass and the CSR pass without dR: the edge pair's.  The CSR pass with dR is capped: at
// kGtTypedParts workgroups per head (one partial each), and so that a workgroup's waves walk about T edges each at
// least -- zeroing, merging and storing a table is work of the order of T f, an edge's of the order of f.
static dim3 gtt_group_grid(int m, int h, int G, long cap) {
  const long per = kBlock / G;
  long blocks = ((long)m + per - 1) / per;
  if (blocks > cap) blocks = cap;
  return dim3((unsigned)(blocks < 1 ? 1 : blocks), h);
}
static dim3 gtt_wave_grid(int m, int h, long cap) {
  long want = ((long)m + kWavesPerBlock - 1) / kWavesPerBlock;
  if (want > cap) want = cap;
  return dim3((unsigned)(want < 1 ? 1 : want), h);
}
static long gtt_table_cap(int nnz, int T) {
  long cap = (long)nnz / ((long)kWavesPerBlock * T);
  if (cap > kGtTypedParts) cap = kGtTypedParts;
  return cap < 1 ? 1 : cap;
}

// -> the launch status; *nparts (TAB): the number of partials the pass writes
template <int PASS, bool TAB>
static int launch_gt_typed_pass(const GtTyped &a, bool v4, hipStream_t s, int *nparts = nullptr) {
  const int n = PASS == 2 ? a.n_cols : a.m;  // the form is chosen per pass, by the average degree of what it walks
  if (n == 0) return 0;  // nothing to walk and nothing to write (a rectangular graph without rows / without columns)
  const bool groups = low_degree(n, a.nnz);
  return dispatch_cfg(a.f, v4, [&](auto cfg) {
    using C = decltype(cfg);
    const dim3 grid = groups ? gtt_group_grid(n, a.h, C::G, TAB ? gtt_table_cap(a.nnz, a.T) : 16384)
                             : gtt_wave_grid(n, a.h, TAB ? gtt_table_cap(a.nnz, a.T) : (1 << 20));
    size_t lds = 0;
    if constexpr (TAB) {
      lds = (size_t)kWavesPerBlock * a.T * a.f * sizeof(float);
      if (lds > 64 * 1024) {  // (above the default limit of dynamic LDS)
        const void *fn = groups ? reinterpret_cast<const void *>(&gt_typed_group_kernel<C, PASS, TAB>)
                                : reinterpret_cast<const void *>(&gt_typed_wave_kernel<C, PASS, TAB>);
        if (int rc = set_max_lds_cached_ptr(fn)) return rc;
      }
      *nparts = (int)grid.x;
    }
    if (groups) gt_typed_group_kernel<C, PASS, TAB><<<grid, kBlock, lds, s>>>(a);
    else gt_typed_wave_kernel<C, PASS, TAB><<<grid, kBlock, lds, s>>>(a);
    return launch_status();
  });
}

static GtTyped gt_typed_args(const Csr &g, const GtTypedTable &t, const float *Q, const float *K, const float *V) {
  GtTyped a{};
  a.m = g.m; a.n_cols = g.n_cols; a.nnz = g.nnz; a.h = g.h; a.f = g.f; a.hf = (size_t)g.h * g.f;
  a.row_ptr = g.row_ptr; a.col_ind = g.col_ind; a.val = g.val;
  a.T = t.T; a.etype = t.etype; a.etype_csc = t.etype_csc; a.Rh = t.R;
  a.Qh = Q; a.Kh = K; a.Vh = V;
  return a;
}

bool gt_typed_table_fits(int T, int f) { return (long)T * f <= kGtTypedMaxTableFloats; }

int launch_gt_typed_fwd(const Csr &g, const GtTypedTable &t, const float *Q, const float *K, const float *V,
                        float *row_max, float *row_sum, float *out, hipStream_t s) {
  GtTyped a = gt_typed_args(g, t, Q, K, V);
  a.outh = out; a.row_max = row_max; a.row_sum = row_sum;
  const bool v4 = (g.f % 4 == 0) && aligned16(t.R) && aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(out);
  return launch_gt_typed_pass<0, false>(a, v4, s);
}

int launch_gt_typed_bwd_rows(const Csr &g, const GtTypedTable &t, const float *Q, const float *K, const float *V,
                             const float *out, const float *row_max, const float *row_sum, const float *grad_out,
                             float *delta, float *dQ, float *ws, float *dR, hipStream_t s) {
  GtTyped a = gt_typed_args(g, t, Q, K, V);
  a.Oh = out; a.dOh = grad_out; a.delta = delta; a.dQh = dQ; a.parts = ws;
  a.row_max = const_cast<float *>(row_max); a.row_sum = const_cast<float *>(row_sum);
  const bool v4 = (g.f % 4 == 0) && aligned16(t.R) && aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(out) &&
                  aligned16(grad_out) && aligned16(dQ);
  if (!dR) return launch_gt_typed_pass<1, false>(a, v4, s);
  if (!gt_typed_table_fits(t.T, g.f)) return kErrUnsupported;
  int nparts = 0;  // without rows or edges no workgroup has a table to fill: dR = 0 from the reduction alone
  if (g.nnz == 0) {
    if (int rc = launch_gt_typed_pass<1, false>(a, v4, s)) return rc;
  } else {
    if (int rc = launch_gt_typed_pass<1, true>(a, v4, s, &nparts)) return rc;
  }
  const long thf = (long)t.T * g.h * g.f;
  if (thf == 0) return 0;
  gt_typed_reduce_kernel<<<(unsigned)((thf + kWave - 1) / kWave), kGtTypedReduceBlock, 0, s>>>(ws, nparts, (int)thf, dR);
  return launch_status();
}

int launch_gt_typed_bwd_cols(const Csr &g, const GtTypedTable &t, const int *col_ptr, const int *row_ind,
                             const int *val_idx, const float *Q, const float *K, const float *V, const float *row_max,
                             const float *row_sum, const float *delta, const float *grad_out, float *dK, float *dV,
                             hipStream_t s) {
  GtTyped a = gt_typed_args(g, t, Q, K, V);
  a.col_ptr = col_ptr; a.row_ind = row_ind; a.val_idx = val_idx;
  a.dOh = grad_out; a.dKh = dK; a.dVh = dV;
  a.row_max = const_cast<float *>(row_max); a.row_sum = const_cast<float *>(row_sum);
  a.delta = const_cast<float *>(delta);
  const bool v4 = (g.f % 4 == 0) && aligned16(t.R) && aligned16(Q) && aligned16(K) && aligned16(V) &&
                  aligned16(grad_out) && aligned16(dK) && aligned16(dV);
  return launch_gt_typed_pass<2, false>(a, v4, s);
}

}  // namespace dfgnn
