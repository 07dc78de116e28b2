// gt_gate_train.hip -- GT conv with a per-edge MULTIPLICATIVE gate on the keys and an edge-output channel for gfx950: fused
// inference and training pair, general kernels (any graph, no plan, no degree limit).  The Graph Transformer layer with edge
// features of Dwivedi & Bresson, SAN, the GT variants inside GraphGPS-type stacks: edge e = (i, j) carries E_e in R^f per
// head, which scales the key dimension by dimension, and the per-dimension products are the next layer's edge features:
//   ke_e    = K_j (.) E_e                 formed first, in all three passes alike
//   s_e     = val_e <Q_i, ke_e>
//   W_e[d]  = val_e Q_i[d] ke_e[d]        the edge output (optional); s_e = sum_d W_e[d] up to rounding
//   P_e     = exp(s_e - row_max_i) / row_sum_i
//   out_i   = sum_e P_e V_j
//   delta_i = <dO_i, out_i>
//   dS_e    = P_e (<dO_i, V_j> - delta_i)
//   g_e[d]  = dS_e + G_e[d]               G = d loss / d W, the second gradient stream (optional: NULL = zero)
//   dQ_i[d] = sum_e val_e g_e[d] ke_e[d]
//   dK_j[d] = sum_e val_e g_e[d] Q_i[d] E_e[d]
//   dV_j    = sum_e P_e dO_i
//   dE_e[d] = val_e g_e[d] Q_i[d] K_j[d]  (optional)
// E, W, G, dE: fp32[nnz, h, f] in CSR edge order -- the feature layout with the edge in place of the node, so the row of
// (edge e, head) starts at (e h + head) f and a row's edges are one contiguous block; offsets are size_t (nnz h f exceeds
// 2^31).  E cannot be folded into Q, K or val: it is per edge AND per dimension.  There is no clamp on the logit.
//
// The structure is gt_edge_train.hip's, pass for pass -- forward, CSR backward pass, CSC backward pass; each as a wave per
// row / column and, for low-degree graphs (nnz < 8 m), as a group of G lanes per row / column with the cooperative switch
// for long rows; two floats saved per (row, head); no atomics, fixed summation order -- and the code is a copy with the gate
// worked in, so that the existing pairs' code objects stay as they are and this operator is one file:
//   forward           one more fragment load per edge, of E_e at the edge's own slot (no index), multiplied into the K_j
//                     fragment before the dot product; with W wanted the lanes that hold the slices store q (.) ke val_e,
//                     one contiguous f-float row per edge.  V is not gated, so the wave form's 64-edge tiles load E ONCE, in
//                     gtg_tile_dots below, and the accumulation is spmm_accum of dfgnn_device.hpp unchanged
//   backward, CSR     owns edge e: it holds Q_i, dO_i, K_j, V_j, E_e and (when given) G_e in registers, accumulates dQ and
//                     stores the lanes' slices of dE_e -- plain stores that cover every slot (no pre-zeroing)
//   backward, CSC     gathers the rows E[val_idx[t]] and (when given) G[val_idx[t]] next to Q_i, dO_i and the three row
//                     scalars and recomputes P_e and dS_e; val_idx is therefore always read
// W, G and dE absent are uniform branches on a kernel argument: the absent case issues no load or store of that array, and
// without G the per-dimension weight val_e g_e[d] is the scalar val_e dS_e of the row-statistics pair.  E, G, W and dE are
// streams that a pass touches once: non-temporal loads and stores.
// ke = K (.) E is formed first and the dot product taken of it with the routine of the row-statistics pair, in all three
// passes alike, so the logit a backward pass recomputes is the forward's to the bit; with E = 1 and neither W nor G every
// output equals gt_train.hip's to the bit (x 1 is exact).
// An empty row: out = 0, row_max = -1e38, row_sum = 0, dQ = 0.
#include "dfgnn_launch.hpp"
#include "dfgnn_rows.hpp"

namespace dfgnn {

// Everything the per-row routines need; at_head() offsets the feature pointers and the four per-edge arrays to the
// workgroup's head.
struct GtGate {
  int m, n_cols, nnz, h, f, head;             // m rows (queries, outputs) x n_cols columns (keys, values)
  size_t hf;
  const int *row_ptr, *col_ind;                // CSR
  const float *val;                            // CSR order, NULL = unit values
  const float *Eh;                             // [nnz, h, f] CSR order (+ head * f): edge e's row starts at e * hf
  const float *Gh;                             // [nnz, h, f] (+ head * f): d loss / d W, NULL = zero
  float *Wh;                                   // [nnz, h, f] (+ head * f), NULL = not wanted
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
    if (Gh) Gh += o;
    if (Wh) Wh += o;
    if (dEh) dEh += o;
    if (dOh) dOh += o;
    if (Oh) Oh += o;
    if (outh) outh += o;
    if (dQh) dQh += o;
    if (dKh) dKh += o;
    if (dVh) dVh += o;
  }
};

typedef float gtg_f4 __attribute__((ext_vector_type(4)));

// frag_load / frag_store_scaled (s = 1) of dfgnn_device.hpp with the non-temporal hint: the once-read streams E and G, the
// once-written W and dE
template <class C>
__device__ __forceinline__ void frag_load_nt(Frag<C> &a, const float *__restrict__ base, int f, int gl) {
#pragma unroll
  for (int ch = 0; ch < C::NCH; ++ch) {
    const int c = (ch * C::G + gl) * C::VEC;
    if constexpr (C::VEC == 4) {
      if (c < f) {
        const gtg_f4 t = __builtin_nontemporal_load(reinterpret_cast<const gtg_f4 *>(base + c));
        a.v[ch][0] = t.x; a.v[ch][1] = t.y; a.v[ch][2] = t.z; a.v[ch][3] = t.w;
      } else {
        a.v[ch][0] = a.v[ch][1] = a.v[ch][2] = a.v[ch][3] = 0.f;
      }
    } else {
      a.v[ch][0] = (c < f) ? __builtin_nontemporal_load(base + c) : 0.f;
    }
  }
}

template <class C>
__device__ __forceinline__ void frag_store_nt(const Frag<C> &a, float *__restrict__ base, int f, int gl) {
#pragma unroll
  for (int ch = 0; ch < C::NCH; ++ch) {
    const int c = (ch * C::G + gl) * C::VEC;
    if constexpr (C::VEC == 4) {
      if (c < f) {
        const gtg_f4 t = {a.v[ch][0], a.v[ch][1], a.v[ch][2], a.v[ch][3]};
        __builtin_nontemporal_store(t, reinterpret_cast<gtg_f4 *>(base + c));
      }
    } else {
      if (c < f) __builtin_nontemporal_store(a.v[ch][0], base + c);
    }
  }
}

// a (.)= b
template <class C>
__device__ __forceinline__ void frag_mul(Frag<C> &a, const Frag<C> &b) {
#pragma unroll
  for (int ch = 0; ch < C::NCH; ++ch)
#pragma unroll
    for (int k = 0; k < C::VEC; ++k) a.v[ch][k] *= b.v[ch][k];
}

// W_e = (q (.) ke) vl, this lane's slice, to the edge's row at `base`
template <class C>
__device__ __forceinline__ void gtg_store_w(const Frag<C> &q, const Frag<C> &ke, float vl, float *__restrict__ base, int f,
                                            int gl) {
  Frag<C> w;
#pragma unroll
  for (int ch = 0; ch < C::NCH; ++ch)
#pragma unroll
    for (int k = 0; k < C::VEC; ++k) w.v[ch][k] = q.v[ch][k] * ke.v[ch][k] * vl;
  frag_store_nt<C>(w, base, f, gl);
}

// The per-dimension weight val_e g_e[d] of an edge: (ds + G_e[d]) vl, or without G the scalar ds vl in every slot -- the
// bits of the G = 0 case, and the row-statistics pair's weight.
template <class C>
__device__ __forceinline__ void gtg_weight(Frag<C> &w, float ds, float vl, const float *__restrict__ Grow, int f, int gl) {
  if (Grow) {
    frag_load_nt<C>(w, Grow, f, gl);
#pragma unroll
    for (int ch = 0; ch < C::NCH; ++ch)
#pragma unroll
      for (int k = 0; k < C::VEC; ++k) w.v[ch][k] = (ds + w.v[ch][k]) * vl;
  } else {
    const float s = ds * vl;
#pragma unroll
    for (int ch = 0; ch < C::NCH; ++ch)
#pragma unroll
      for (int k = 0; k < C::VEC; ++k) w.v[ch][k] = s;
  }
}

// acc[d] += w[d] x[d]
template <class C>
__device__ __forceinline__ void frag_fma_vec(Frag<C> &acc, const Frag<C> &w, const Frag<C> &x) {
#pragma unroll
  for (int ch = 0; ch < C::NCH; ++ch)
#pragma unroll
    for (int k = 0; k < C::VEC; ++k) acc.v[ch][k] = fmaf(w.v[ch][k], x.v[ch][k], acc.v[ch][k]);
}

// ======================================================================================================================
// the dot-product tile routine of the wave-per-row forward: tile_dots (dfgnn_rows.hpp) with the tile's E rows, which are
// contiguous from Et = E + (lb + t0) hf, and the W rows at Wt likewise (NULL: not wanted; vt: the tile's edge values or
// NULL).  Two edges (four loads) in flight per group.  E is loaded here and nowhere else in the wave form.
// ======================================================================================================================
template <class C>
__device__ __forceinline__ void gtg_tile_dots(const Frag<C> &a, const int *cols, int nt, const float *__restrict__ X,
                                              const float *__restrict__ Et, float *__restrict__ Wt,
                                              const float *__restrict__ vt, size_t hf, int f, int gid, int gl,
                                              float *sw) {
  int e = gid;
  for (; e + C::EPW < nt; e += 2 * C::EPW) {
    Frag<C> x0, x1, e0, e1;
    frag_load<C>(x0, X + (size_t)cols[e] * hf, f, gl);
    frag_load_nt<C>(e0, Et + (size_t)e * hf, f, gl);
    frag_load<C>(x1, X + (size_t)cols[e + C::EPW] * hf, f, gl);
    frag_load_nt<C>(e1, Et + (size_t)(e + C::EPW) * hf, f, gl);
    frag_mul<C>(x0, e0);
    frag_mul<C>(x1, e1);
    const float d0 = lanes_sum<C::G>(frag_dot<C>(a, x0)), d1 = lanes_sum<C::G>(frag_dot<C>(a, x1));
    if (gl == 0) {
      sw[e] = d0;
      sw[e + C::EPW] = d1;
    }
    if (Wt) {
      gtg_store_w<C>(a, x0, vt ? vt[e] : 1.f, Wt + (size_t)e * hf, f, gl);
      gtg_store_w<C>(a, x1, vt ? vt[e + C::EPW] : 1.f, Wt + (size_t)(e + C::EPW) * hf, f, gl);
    }
  }
  for (; e < nt; e += C::EPW) {
    Frag<C> x0, e0;
    frag_load<C>(x0, X + (size_t)cols[e] * hf, f, gl);
    frag_load_nt<C>(e0, Et + (size_t)e * hf, f, gl);
    frag_mul<C>(x0, e0);
    const float d0 = lanes_sum<C::G>(frag_dot<C>(a, x0));
    if (gl == 0) sw[e] = d0;
    if (Wt) gtg_store_w<C>(a, x0, vt ? vt[e] : 1.f, Wt + (size_t)e * hf, f, gl);
  }
}

// ======================================================================================================================
// forward, a wave per row: 64-edge tiles (sw / sc: the wave's 64-float / 64-int LDS scratch)
// ======================================================================================================================
template <class C>
__device__ __forceinline__ void gtg_fwd_row_wave(const GtGate &a, int r, int lane, float *sw, int *sc) {
  const int gid = lane / C::G, gl = lane % C::G;
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  Frag<C> q, acc;
  frag_load<C>(q, a.Qh + (size_t)r * a.hf, a.f, gl);
  frag_zero<C>(acc);
  float m_run = -INFINITY, l_run = 0.f;
  for (int t0 = 0; t0 < deg; t0 += kWave) {
    const int nt = min(kWave, deg - t0);
    const size_t eo = ((size_t)lb + t0) * a.hf;
    sc[lane] = (lane < nt) ? a.col_ind[lb + t0 + lane] : 0;
    wave_sync();
    gtg_tile_dots<C>(q, sc, nt, a.Kh, a.Eh + eo, a.Wh ? a.Wh + eo : nullptr, a.val ? a.val + lb + t0 : nullptr, a.hf, a.f,
                     gid, gl, sw);
    wave_sync();
    float s = -INFINITY;
    if (lane < nt) s = a.val ? sw[lane] * a.val[lb + t0 + lane] : sw[lane];
    online_step<C>(s, lane, sw, acc, m_run, l_run);
    wave_sync();
    spmm_accum<C>(acc, sw, sc, nt, a.Vh, a.hf, a.f, gid, gl);
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
template <class C, bool COOP>
__device__ __forceinline__ void gtg_fwd_row_group(const GtGate &a, int r, int gid, int gl) {
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
    frag_load_nt<C>(x, a.Eh + ((size_t)lb + e) * a.hf, a.f, gl);  // the edge's own slot: no index
    frag_mul<C>(k, x);
    const float vl = a.val ? a.val[lb + e] : 1.f;
    float s = lanes_sum<C::G>(frag_dot<C>(q, k));
    if (a.val) s *= vl;
    if (a.Wh) gtg_store_w<C>(q, k, vl, a.Wh + ((size_t)lb + e) * a.hf, a.f, gl);
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

// CSR pass, row r: delta_r = <dO_r, out_r> -> delta; dQ_r[d] = sum_e val_e g_e[d] ke_e[d] and the row dE_e in one sweep, two
// edges (six loads, eight with G) in flight per group.  Every lane of a group holds the two dot products of its edge
// (lanes_sum is an all-reduce), so the edge's dS needs no exchange: each lane forms its slice of the weight val_e g_e and
// stores its slice of dE_e = val_e g_e (.) Q_r (.) K_c.
template <class C, bool COOP>
__device__ __forceinline__ void gtg_bwd_row_group(const GtGate &a, int r, int gid, int gl) {
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  const int es = COOP ? C::EPW : 1;
  Frag<C> acc;
  frag_zero<C>(acc);
  float dl = 0.f;  // empty row: dQ = 0, delta = 0
  if (deg > 0) {
    Frag<C> q, go;
    frag_load<C>(q, a.Qh + (size_t)r * a.hf, a.f, gl);
    frag_load<C>(go, a.dOh + (size_t)r * a.hf, a.f, gl);
    {
      Frag<C> o;
      frag_load<C>(o, a.Oh + (size_t)r * a.hf, a.f, gl);
      dl = lanes_sum<C::G>(frag_dot<C>(go, o));
    }
    const float mx = a.row_max[a.nh(r)], inv = 1.f / a.row_sum[a.nh(r)];
    // k: K_c, x: E_e, v: V_c.  Adds the edge's term to acc and stores dE_e when it is wanted
    auto edge = [&](int e, Frag<C> &k, const Frag<C> &x, const Frag<C> &v) {
      const size_t eo = ((size_t)lb + e) * a.hf;
      Frag<C> ke = k, w;
      frag_mul<C>(ke, x);
      const float vl = a.val ? a.val[lb + e] : 1.f;
      const float s = vl * lanes_sum<C::G>(frag_dot<C>(q, ke));
      const float dp = lanes_sum<C::G>(frag_dot<C>(go, v));
      const float ds = fast_exp(s - mx) * inv * (dp - dl);
      gtg_weight<C>(w, ds, vl, a.Gh ? a.Gh + eo : nullptr, a.f, gl);
      frag_fma_vec<C>(acc, w, ke);
      if (a.dEh) {
#pragma unroll
        for (int ch = 0; ch < C::NCH; ++ch)
#pragma unroll
          for (int i = 0; i < C::VEC; ++i) k.v[ch][i] = w.v[ch][i] * q.v[ch][i] * k.v[ch][i];
        frag_store_nt<C>(k, a.dEh + eo, a.f, gl);
      }
    };
    int e = COOP ? gid : 0;
    for (; e + es < deg; e += 2 * es) {
      const int c0 = a.col_ind[lb + e], c1 = a.col_ind[lb + e + es];
      Frag<C> k0, v0, x0, k1, v1, x1;
      frag_load<C>(k0, a.Kh + (size_t)c0 * a.hf, a.f, gl);
      frag_load<C>(v0, a.Vh + (size_t)c0 * a.hf, a.f, gl);
      frag_load_nt<C>(x0, a.Eh + ((size_t)lb + e) * a.hf, a.f, gl);
      frag_load<C>(k1, a.Kh + (size_t)c1 * a.hf, a.f, gl);
      frag_load<C>(v1, a.Vh + (size_t)c1 * a.hf, a.f, gl);
      frag_load_nt<C>(x1, a.Eh + ((size_t)lb + e + es) * a.hf, a.f, gl);
      edge(e, k0, x0, v0);
      edge(e + es, k1, x1, v1);
    }
    for (; e < deg; e += es) {
      const int c0 = a.col_ind[lb + e];
      Frag<C> k0, v0, x0;
      frag_load<C>(k0, a.Kh + (size_t)c0 * a.hf, a.f, gl);
      frag_load<C>(v0, a.Vh + (size_t)c0 * a.hf, a.f, gl);
      frag_load_nt<C>(x0, a.Eh + ((size_t)lb + e) * a.hf, a.f, gl);
      edge(e, k0, x0, v0);
    }
  }
  if constexpr (COOP) frag_reduce_groups<C>(acc);
  if (!COOP || gid == 0) {
    frag_store_scaled<C>(acc, 1.f, a.dQh + (size_t)r * a.hf, a.f, gl);
    if (gl == 0) a.delta[a.nh(r)] = dl;
  }
}

// CSC pass, column j: dV_j = sum P_e dO_i, dK_j[d] = sum val_e g_e[d] Q_i[d] E_e[d] over the column's entries, two entries
// (six gathers, eight with G, + their row scalars and edge value) in flight per group.  An empty column writes zeros.
template <class C, bool COOP>
__device__ __forceinline__ void gtg_bwd_col_group(const GtGate &a, int j, int gid, int gl) {
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
      x.e = a.val_idx[lb + t];  // val, E and G are in CSR order
      x.vl = a.val ? a.val[x.e] : 1.f;
      const size_t s = a.nh(x.i);
      x.mx = a.row_max[s];
      x.sum = a.row_sum[s];
      x.dl = a.delta[s];
      return x;
    };
    // qi: Q_i, gi: dO_i, xe: E_e (turned into Q_i (.) E_e)
    auto accum = [&](const Entry &x, const Frag<C> &qi, const Frag<C> &gi, Frag<C> &xe) {
      Frag<C> ke = k, w;
      frag_mul<C>(ke, xe);
      const float s = x.vl * lanes_sum<C::G>(frag_dot<C>(qi, ke));
      const float dp = lanes_sum<C::G>(frag_dot<C>(gi, v));
      const float p = fast_exp(s - x.mx) * __builtin_amdgcn_rcpf(x.sum);
      frag_fma<C>(aV, p, gi);
      gtg_weight<C>(w, p * (dp - x.dl), x.vl, a.Gh ? a.Gh + (size_t)x.e * a.hf : nullptr, a.f, gl);
      frag_mul<C>(xe, qi);
      frag_fma_vec<C>(aK, w, xe);
    };
    int t = COOP ? gid : 0;
    for (; t + es < n; t += 2 * es) {
      const Entry x0 = entry(t), x1 = entry(t + es);
      Frag<C> q0, g0, e0, q1, g1, e1;
      frag_load<C>(q0, a.Qh + (size_t)x0.i * a.hf, a.f, gl);
      frag_load<C>(g0, a.dOh + (size_t)x0.i * a.hf, a.f, gl);
      frag_load_nt<C>(e0, a.Eh + (size_t)x0.e * a.hf, a.f, gl);
      frag_load<C>(q1, a.Qh + (size_t)x1.i * a.hf, a.f, gl);
      frag_load<C>(g1, a.dOh + (size_t)x1.i * a.hf, a.f, gl);
      frag_load_nt<C>(e1, a.Eh + (size_t)x1.e * a.hf, a.f, gl);
      accum(x0, q0, g0, e0);
      accum(x1, q1, g1, e1);
    }
    for (; t < n; t += es) {
      const Entry x0 = entry(t);
      Frag<C> q0, g0, e0;
      frag_load<C>(q0, a.Qh + (size_t)x0.i * a.hf, a.f, gl);
      frag_load<C>(g0, a.dOh + (size_t)x0.i * a.hf, a.f, gl);
      frag_load_nt<C>(e0, a.Eh + (size_t)x0.e * a.hf, a.f, gl);
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
// kernels.  PASS: 0 forward, 1 backward CSR pass, 2 backward CSC pass.
// ======================================================================================================================
template <class C, int PASS, bool COOP>
__device__ __forceinline__ void gtg_group_pass(const GtGate &a, int r, int gid, int gl) {
  if constexpr (PASS == 0) gtg_fwd_row_group<C, COOP>(a, r, gid, gl);
  else if constexpr (PASS == 1) gtg_bwd_row_group<C, COOP>(a, r, gid, gl);
  else gtg_bwd_col_group<C, COOP>(a, r, gid, gl);
}

// general: a wave per row / column, grid-strided over the whole graph.  The forward works in 64-edge tiles through the
// wave's LDS scratch; the backward passes are the COOP form of the group routines (no LDS).
template <class C, int PASS>
__global__ __launch_bounds__(kBlock) void gt_gate_wave_kernel(GtGate a) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  a.at_head(blockIdx.y);
  const int n = PASS == 2 ? a.n_cols : a.m;  // the extent this pass walks: rows, or (CSC pass) columns
  const int beg = blockIdx.x * kWavesPerBlock + wave, step = gridDim.x * kWavesPerBlock;
  if constexpr (PASS == 0) {
    __shared__ __attribute__((aligned(16))) float lds[kWavesPerBlock * kScratchFloatsPerWave];
    float *sw = lds + wave * kScratchFloatsPerWave;
    int *sc = reinterpret_cast<int *>(sw + kWave);
    for (int r = beg; r < n; r += step) gtg_fwd_row_wave<C>(a, r, lane, sw, sc);
  } else {
    for (int r = beg; r < n; r += step) gtg_group_pass<C, PASS, true>(a, r, lane / C::G, lane % C::G);
  }
}

// low-degree graphs: a workgroup takes blocks of kBlock / G consecutive rows, one lane group per row -- unless a wave's
// EPW rows include one of more than kGtGateGroupMaxDegree entries, which a single lane group would walk serially while the
// rest of the wave waits: that wave takes its rows one after the other with all its groups on each (COOP).  The choice is
// wave-uniform (ballot): no barrier, no LDS.  As gt_edge_group_kernel of gt_edge_train.hip, with the same threshold.
constexpr int kGtGateGroupMaxDegree = 24;
template <class C, int PASS>
__global__ __launch_bounds__(kBlock) void gt_gate_group_kernel(GtGate a) {
  constexpr int G = C::G, R = kBlock / G;  // rows per block
  const int gid = (threadIdx.x & (kWave - 1)) / G, gl = threadIdx.x % G, wave = threadIdx.x / kWave;
  a.at_head(blockIdx.y);
  const int *ptr = PASS == 2 ? a.col_ptr : a.row_ptr;
  const int n = PASS == 2 ? a.n_cols : a.m;  // the extent this pass walks: rows, or (CSC pass) columns
  for (int b0 = blockIdx.x * R; b0 < n; b0 += gridDim.x * R) {
    const int r = b0 + threadIdx.x / G;
    const int deg = r < n ? ptr[r + 1] - ptr[r] : 0;
    if (__any(deg > kGtGateGroupMaxDegree)) {
      for (int rr = b0 + wave * C::EPW; rr < min(n, b0 + (wave + 1) * C::EPW); ++rr)
        gtg_group_pass<C, PASS, true>(a, rr, gid, gl);
    } else if (r < n) {
      gtg_group_pass<C, PASS, false>(a, r, gid, gl);
    }
  }
}

static dim3 gtg_group_grid(int m, int h, int G) {
  const long per = kBlock / G;
  long blocks = ((long)m + per - 1) / per;
  if (blocks > 16384) blocks = 16384;
  return dim3((unsigned)(blocks < 1 ? 1 : blocks), h);
}
static dim3 gtg_wave_grid(int m, int h) {
  const long want = ((long)m + kWavesPerBlock - 1) / kWavesPerBlock;
  return dim3((unsigned)(want > (1 << 20) ? (1 << 20) : want), h);
}

template <int PASS>
static int launch_gt_gate_pass(const GtGate &a, bool v4, hipStream_t s) {
  const int n = PASS == 2 ? a.n_cols : a.m;  // the form is chosen per pass, by the average degree of what it walks
  if (n == 0) return 0;  // nothing to walk and nothing to write (a rectangular graph without rows / without columns)
  const bool groups = low_degree(n, a.nnz);
  return dispatch_cfg(a.f, v4, [&](auto cfg) {
    using C = decltype(cfg);
    if (groups) gt_gate_group_kernel<C, PASS><<<gtg_group_grid(n, a.h, C::G), kBlock, 0, s>>>(a);
    else gt_gate_wave_kernel<C, PASS><<<gtg_wave_grid(n, a.h), kBlock, 0, s>>>(a);
    return launch_status();
  });
}

static GtGate gt_gate_args(const Csr &g, const float *E, const float *Q, const float *K, const float *V) {
  GtGate a{};
  a.m = g.m; a.n_cols = g.n_cols; a.nnz = g.nnz; a.h = g.h; a.f = g.f; a.hf = (size_t)g.h * g.f;
  a.row_ptr = g.row_ptr; a.col_ind = g.col_ind; a.val = g.val; a.Eh = E;
  a.Qh = Q; a.Kh = K; a.Vh = V;
  return a;
}

int launch_gt_gate_fwd(const Csr &g, const float *E, const float *Q, const float *K, const float *V, float *row_max,
                       float *row_sum, float *out, float *W, hipStream_t s) {
  GtGate a = gt_gate_args(g, E, Q, K, V);
  a.outh = out; a.row_max = row_max; a.row_sum = row_sum; a.Wh = W;
  const bool v4 = (g.f % 4 == 0) && aligned16(E) && aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(out) &&
                  aligned16(W);
  return launch_gt_gate_pass<0>(a, v4, s);
}

int launch_gt_gate_bwd_rows(const Csr &g, const float *E, const float *Q, const float *K, const float *V,
                            const float *out, const float *row_max, const float *row_sum, const float *grad_out,
                            const float *G, float *delta, float *dQ, float *dE, hipStream_t s) {
  GtGate a = gt_gate_args(g, E, Q, K, V);
  a.Oh = out; a.dOh = grad_out; a.Gh = G; a.delta = delta; a.dQh = dQ; a.dEh = dE;
  a.row_max = const_cast<float *>(row_max); a.row_sum = const_cast<float *>(row_sum);
  const bool v4 = (g.f % 4 == 0) && aligned16(E) && aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(out) &&
                  aligned16(grad_out) && aligned16(G) && aligned16(dQ) && aligned16(dE);
  return launch_gt_gate_pass<1>(a, v4, s);
}

int launch_gt_gate_bwd_cols(const Csr &g, const float *E, const int *col_ptr, const int *row_ind, const int *val_idx,
                            const float *Q, const float *K, const float *V, const float *row_max, const float *row_sum,
                            const float *delta, const float *grad_out, const float *G, float *dK, float *dV,
                            hipStream_t s) {
  GtGate a = gt_gate_args(g, E, Q, K, V);
  a.col_ptr = col_ptr; a.row_ind = row_ind; a.val_idx = val_idx;
  a.dOh = grad_out; a.Gh = G; a.dKh = dK; a.dVh = dV;
  a.row_max = const_cast<float *>(row_max); a.row_sum = const_cast<float *>(row_sum);
  a.delta = const_cast<float *>(delta);
  const bool v4 = (g.f % 4 == 0) && aligned16(E) && aligned16(Q) && aligned16(K) && aligned16(V) &&
                  aligned16(grad_out) && aligned16(G) && aligned16(dK) && aligned16(dV);
  return launch_gt_gate_pass<2>(a, v4, s);
}

}  // namespace dfgnn
