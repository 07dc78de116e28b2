// gatv2_edge_train.hip -- GATv2 convolution with a per-edge FEATURE VECTOR inside the LeakyReLU for gfx950: fused inference
// and training pair (any graph, no plan, no degree limit).  PyG's GATv2Conv(edge_dim=...): edge e = (i, j) carries E_e in
// R^f per head (E = lin_edge(edge_attr) viewed [nnz, h, f]), and
//   z_e  = Xr_i + Xc_j + E_e            s_e = sum_d a[d] lrelu(z_e[d])
//   P_e  = exp(s_e - row_max_i) / row_sum_i            out_i = sum_e P_e Xc_j       (E is NOT in the message)
//   dP_e = <dO_i, Xc_j>    dS_e = P_e (dP_e - delta_i)    g_e[d] = dS_e a[d] (z_e[d] > 0 ? 1 : slope)
//   dXr_i = sum_e g_e      dXc_j = sum_e (P_e dO_i + g_e)      dattn[d] = sum_{all e} dS_e lrelu(z_e[d])      dE_e = g_e
// E, dE: fp32[nnz, h, f] in CSR edge order -- the feature layout with the edge in place of the node, so the row of (edge
// e, head) starts at (e h + head) f and a row's edges are one contiguous block; offsets are size_t (nnz h f exceeds 2^31).
// E sits inside the LeakyReLU, so it cannot be folded into Xr, Xc or a.
//
// The structure is gatv2_train.hip's, pass for pass -- forward, CSR backward pass with the persistent-workgroup partials
// of dattn, CSC backward pass, the fixed-order reduction; each pass as a wave per row / column and, for low-degree graphs,
// as a group of G lanes per row / column with the cooperative switch for long rows -- and the code is a copy with E worked
// in, so that the plain pair's code objects stay as they are and this operator is one file:
//   forward           one more fragment load per edge, of E_e at the edge's own slot (no index).  Xc_j is still gathered
//                     once and serves logit and message.  The wave form loads the tile's E rows, contiguous from
//                     E + (lb + t0) hf, in the logit loop only: the weighted sum has no E and does not touch it
//   backward, CSR     owns edge e: after forming z_e it holds dS_e, a and z_e in registers and the lanes of the group store
//                     their slices of dE_e = g_e -- one contiguous f-float row per edge, plain stores that cover every
//                     slot (no pre-zeroing).  dE == NULL: nothing of size nnz h f is written
//   backward, CSC     gathers the row E[val_idx[t]] next to Xr_i, dO_i and the three row scalars and recomputes P_e, dS_e,
//                     g_e; val_idx is therefore always read
// z_e is formed as (Xr_i + Xc_j) + E_e in all three passes alike, so the logit a backward pass recomputes is the forward's
// to the bit; with E = 0 every output equals gatv2_train.hip's.  The layouts of 16 floats per lane (f > 128 in the
// float4 form) keep ONE edge in flight in the two backward passes instead of two -- the summation order is the same either
// way -- which holds them at or below the plain pair's register count; no instance needs scratch.
// An empty row: out = 0, row_max = -1e38, row_sum = 0, dXr = 0; an empty column: dXc = 0.
#include "dfgnn_launch.hpp"
#include "dfgnn_rows.hpp"

namespace dfgnn {

// Everything the per-row routines need; at_head() offsets the feature pointers, E and dE to the workgroup's head.
struct Gatv2Edge {
  int m, n_cols, nnz, h, f, head;             // m rows (queries, outputs) x n_cols columns (keys, values)
  size_t hf;
  float slope;
  const int *row_ptr, *col_ind;            // CSR
  const int *col_ptr, *row_ind, *val_idx;  // CSC (column pass); val_idx: the entry's place in CSR order = its row of E
  const float *ah;                         // attention vector (+ head * f)
  const float *Eh;                         // [nnz, h, f] CSR order (+ head * f): edge e's row starts at e * hf
  float *dEh;                              // [nnz, h, f] (+ head * f), NULL = not wanted
  const float *Xrh, *Xch, *dOh, *Oh;       // features, output gradient, forward output (+ head * f)
  float *row_max, *row_sum, *delta;        // [m, h]: written by the forward / the CSR pass, read by the passes after
  float *outh, *dXrh, *dXch;               // (+ head * f)
  float *parts;                            // [gridDim.x of the CSR pass, h, f] partial sums of dattn
  __device__ __forceinline__ size_t nh(int node) const { return (size_t)node * h + head; }
  __device__ __forceinline__ void at_head(int hd) {
    head = hd;
    const size_t o = (size_t)hd * f;
    ah += o; Xrh += o; Xch += o;
    if (Eh) Eh += o;
    if (dEh) dEh += o;
    if (dOh) dOh += o;
    if (Oh) Oh += o;
    if (outh) outh += o;
    if (dXrh) dXrh += o;
    if (dXch) dXch += o;
  }
};

// two edges in flight per group in the backward passes where their E fragments fit next to everything else
template <class C>
constexpr bool kGatv2EdgeTwoInFlight = C::NCH * C::VEC <= 8;

// s_e for the rows xr, xc, xe held by one lane group (all-reduce: every lane of the group gets it).  Lanes past f hold
// zeros in all four fragments and add nothing.  z = (xr + xc) + xe: the one expression of all passes.
template <class C>
__device__ __forceinline__ float gatv2e_logit(const Frag<C> &av, const Frag<C> &xr, const Frag<C> &xc, const Frag<C> &xe,
                                              float slope) {
  float d = 0.f;
#pragma unroll
  for (int ch = 0; ch < C::NCH; ++ch)
#pragma unroll
    for (int k = 0; k < C::VEC; ++k)
      d = fmaf(av.v[ch][k], leaky_relu((xr.v[ch][k] + xc.v[ch][k]) + xe.v[ch][k], slope), d);
  return lanes_sum<C::G>(d);
}

// The edge's terms of the two feature-wide sums of the backward: g += dS a lrelu'(z), and (DATTN) da += dS lrelu(z).
template <class C, bool DATTN>
__device__ __forceinline__ void gatv2e_edge_grads(Frag<C> &g, Frag<C> &da, float ds, const Frag<C> &av, const Frag<C> &xr,
                                                  const Frag<C> &xc, const Frag<C> &xe, float slope) {
#pragma unroll
  for (int ch = 0; ch < C::NCH; ++ch)
#pragma unroll
    for (int k = 0; k < C::VEC; ++k) {
      const float z = (xr.v[ch][k] + xc.v[ch][k]) + xe.v[ch][k];
      const float w = ds * av.v[ch][k];
      g.v[ch][k] = fmaf(w, z > 0.f ? 1.f : slope, g.v[ch][k]);
      if constexpr (DATTN) da.v[ch][k] = fmaf(ds, leaky_relu(z, slope), da.v[ch][k]);
    }
}

// dE_e = g_e: the group's lanes store their slices of the edge's row (every slot below f)
template <class C>
__device__ __forceinline__ void gatv2e_store_dE(float ds, const Frag<C> &av, const Frag<C> &xr, const Frag<C> &xc,
                                                const Frag<C> &xe, float slope, float *__restrict__ row, int f, int gl) {
  Frag<C> de;
#pragma unroll
  for (int ch = 0; ch < C::NCH; ++ch)
#pragma unroll
    for (int k = 0; k < C::VEC; ++k) {
      const float z = (xr.v[ch][k] + xc.v[ch][k]) + xe.v[ch][k];
      de.v[ch][k] = ds * av.v[ch][k] * (z > 0.f ? 1.f : slope);
    }
  frag_store_scaled<C>(de, 1.f, row, f, gl);
}

// ======================================================================================================================
// forward, a wave per row: 64-edge tiles as gatv2_fwd_row_wave (sw / sc: the wave's 64-float / 64-int LDS scratch)
// ======================================================================================================================
template <class C>
__device__ __forceinline__ void gatv2e_fwd_row_wave(const Gatv2Edge &a, const Frag<C> &av, int r, int lane, float *sw,
                                                    int *sc) {
  const int gid = lane / C::G, gl = lane % C::G;
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  Frag<C> xr, acc;
  frag_load<C>(xr, a.Xrh + (size_t)r * a.hf, a.f, gl);
  frag_zero<C>(acc);
  float m_run = -INFINITY, l_run = 0.f;
  for (int t0 = 0; t0 < deg; t0 += kWave) {
    const int nt = min(kWave, deg - t0);
    const float *Et = a.Eh + ((size_t)lb + t0) * a.hf;  // the tile's E rows: contiguous, edge e of the tile at e * hf
    sc[lane] = (lane < nt) ? a.col_ind[lb + t0 + lane] : 0;
    wave_sync();
    int e = gid;  // the tile's logits -> sw, two edges (four loads) in flight per group
    for (; e + C::EPW < nt; e += 2 * C::EPW) {
      Frag<C> x0, x1, e0, e1;
      frag_load<C>(x0, a.Xch + (size_t)sc[e] * a.hf, a.f, gl);
      frag_load<C>(e0, Et + (size_t)e * a.hf, a.f, gl);
      frag_load<C>(x1, a.Xch + (size_t)sc[e + C::EPW] * a.hf, a.f, gl);
      frag_load<C>(e1, Et + (size_t)(e + C::EPW) * a.hf, a.f, gl);
      const float s0 = gatv2e_logit<C>(av, xr, x0, e0, a.slope), s1 = gatv2e_logit<C>(av, xr, x1, e1, a.slope);
      if (gl == 0) {
        sw[e] = s0;
        sw[e + C::EPW] = s1;
      }
    }
    for (; e < nt; e += C::EPW) {
      Frag<C> x0, e0;
      frag_load<C>(x0, a.Xch + (size_t)sc[e] * a.hf, a.f, gl);
      frag_load<C>(e0, Et + (size_t)e * a.hf, a.f, gl);
      const float s0 = gatv2e_logit<C>(av, xr, x0, e0, a.slope);
      if (gl == 0) sw[e] = s0;
    }
    wave_sync();
    const float s = (lane < nt) ? sw[lane] : -INFINITY;
    online_step<C>(s, lane, sw, acc, m_run, l_run);
    wave_sync();
    spmm_accum<C>(acc, sw, sc, nt, a.Xch, a.hf, a.f, gid, gl);  // the message has no E
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
__device__ __forceinline__ void gatv2e_fwd_row_group(const Gatv2Edge &a, const Frag<C> &av, int r, int gid, int gl) {
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  Frag<C> xr, acc;
  frag_load<C>(xr, a.Xrh + (size_t)r * a.hf, a.f, gl);
  frag_zero<C>(acc);
  float m_run = -INFINITY, l_run = 0.f;  // online softmax: one sweep, ONE gather per edge (logit operand = message)
  for (int e = COOP ? gid : 0; e < deg; e += COOP ? C::EPW : 1) {
    Frag<C> xc, xe;
    frag_load<C>(xc, a.Xch + (size_t)a.col_ind[lb + e] * a.hf, a.f, gl);
    frag_load<C>(xe, a.Eh + ((size_t)lb + e) * a.hf, a.f, gl);
    const float s = gatv2e_logit<C>(av, xr, xc, xe, a.slope);
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

// CSR pass, row r: delta_r = <dO_r, out_r> -> delta; dXr_r = sum_e g_e and the rows dE_e = g_e in one sweep, two edges
// (four loads) in flight per group where they fit; the edges' terms of dattn go to `da`, which the caller keeps over all
// its rows.  Every lane of a group holds the edge's two reductions (lanes_sum is an all-reduce), so dS_e needs no exchange.
template <class C, bool COOP>
__device__ __forceinline__ void gatv2e_bwd_row_group(const Gatv2Edge &a, const Frag<C> &av, Frag<C> &da, int r, int gid,
                                                     int gl) {
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  const int es = COOP ? C::EPW : 1;
  Frag<C> acc;
  frag_zero<C>(acc);
  float dl = 0.f;  // empty row: dXr = 0, delta = 0
  if (deg > 0) {
    Frag<C> xr, go;
    frag_load<C>(xr, a.Xrh + (size_t)r * a.hf, a.f, gl);
    frag_load<C>(go, a.dOh + (size_t)r * a.hf, a.f, gl);
    {
      Frag<C> o;
      frag_load<C>(o, a.Oh + (size_t)r * a.hf, a.f, gl);
      dl = lanes_sum<C::G>(frag_dot<C>(go, o));
    }
    const float mx = a.row_max[a.nh(r)], inv = 1.f / a.row_sum[a.nh(r)];
    auto edge = [&](int e, const Frag<C> &xc, const Frag<C> &xe) {
      const float s = gatv2e_logit<C>(av, xr, xc, xe, a.slope);
      const float dp = lanes_sum<C::G>(frag_dot<C>(go, xc));
      const float ds = fast_exp(s - mx) * inv * (dp - dl);
      gatv2e_edge_grads<C, true>(acc, da, ds, av, xr, xc, xe, a.slope);
      if (a.dEh) gatv2e_store_dE<C>(ds, av, xr, xc, xe, a.slope, a.dEh + ((size_t)lb + e) * a.hf, a.f, gl);
    };
    int e = COOP ? gid : 0;
    if constexpr (kGatv2EdgeTwoInFlight<C>) {
      for (; e + es < deg; e += 2 * es) {
        Frag<C> x0, x1, e0, e1;
        frag_load<C>(x0, a.Xch + (size_t)a.col_ind[lb + e] * a.hf, a.f, gl);
        frag_load<C>(e0, a.Eh + ((size_t)lb + e) * a.hf, a.f, gl);
        frag_load<C>(x1, a.Xch + (size_t)a.col_ind[lb + e + es] * a.hf, a.f, gl);
        frag_load<C>(e1, a.Eh + ((size_t)lb + e + es) * a.hf, a.f, gl);
        edge(e, x0, e0);
        edge(e + es, x1, e1);
      }
    }
    for (; e < deg; e += es) {
      Frag<C> x0, e0;
      frag_load<C>(x0, a.Xch + (size_t)a.col_ind[lb + e] * a.hf, a.f, gl);
      frag_load<C>(e0, a.Eh + ((size_t)lb + e) * a.hf, a.f, gl);
      edge(e, x0, e0);
    }
  }
  if constexpr (COOP) frag_reduce_groups<C>(acc);
  if (!COOP || gid == 0) {
    frag_store_scaled<C>(acc, 1.f, a.dXrh + (size_t)r * a.hf, a.f, gl);
    if (gl == 0) a.delta[a.nh(r)] = dl;
  }
}

// CSC pass, column j: dXc_j = sum (P_e dO_i + g_e) over the column's entries, two entries (six gathers + their row
// scalars) in flight per group where they fit.  An empty column writes zeros.
template <class C, bool COOP>
__device__ __forceinline__ void gatv2e_bwd_col_group(const Gatv2Edge &a, const Frag<C> &av, int j, int gid, int gl) {
  const int lb = a.col_ptr[j], n = a.col_ptr[j + 1] - lb;
  const int es = COOP ? C::EPW : 1;
  Frag<C> acc;
  frag_zero<C>(acc);
  if (n > 0) {
    Frag<C> xc;
    frag_load<C>(xc, a.Xch + (size_t)j * a.hf, a.f, gl);
    struct Entry {
      int i, e;
      float mx, sum, dl;
    };
    auto entry = [&](int t) {
      Entry x;
      x.i = a.row_ind[lb + t];
      x.e = a.val_idx[lb + t];  // E is in CSR order
      const size_t s = a.nh(x.i);
      x.mx = a.row_max[s];
      x.sum = a.row_sum[s];
      x.dl = a.delta[s];
      return x;
    };
    auto accum = [&](const Entry &x, const Frag<C> &xr, const Frag<C> &gi, const Frag<C> &xe) {
      const float s = gatv2e_logit<C>(av, xr, xc, xe, a.slope);
      const float dp = lanes_sum<C::G>(frag_dot<C>(gi, xc));
      const float p = fast_exp(s - x.mx) * __builtin_amdgcn_rcpf(x.sum);
      frag_fma<C>(acc, p, gi);
      gatv2e_edge_grads<C, false>(acc, acc, p * (dp - x.dl), av, xr, xc, xe, a.slope);
    };
    int t = COOP ? gid : 0;
    if constexpr (kGatv2EdgeTwoInFlight<C>) {
      for (; t + es < n; t += 2 * es) {
        const Entry x0 = entry(t), x1 = entry(t + es);
        Frag<C> r0, g0, e0, r1, g1, e1;
        frag_load<C>(r0, a.Xrh + (size_t)x0.i * a.hf, a.f, gl);
        frag_load<C>(g0, a.dOh + (size_t)x0.i * a.hf, a.f, gl);
        frag_load<C>(e0, a.Eh + (size_t)x0.e * a.hf, a.f, gl);
        frag_load<C>(r1, a.Xrh + (size_t)x1.i * a.hf, a.f, gl);
        frag_load<C>(g1, a.dOh + (size_t)x1.i * a.hf, a.f, gl);
        frag_load<C>(e1, a.Eh + (size_t)x1.e * a.hf, a.f, gl);
        accum(x0, r0, g0, e0);
        accum(x1, r1, g1, e1);
      }
    }
    for (; t < n; t += es) {
      const Entry x0 = entry(t);
      Frag<C> r0, g0, e0;
      frag_load<C>(r0, a.Xrh + (size_t)x0.i * a.hf, a.f, gl);
      frag_load<C>(g0, a.dOh + (size_t)x0.i * a.hf, a.f, gl);
      frag_load<C>(e0, a.Eh + (size_t)x0.e * a.hf, a.f, gl);
      accum(x0, r0, g0, e0);
    }
  }
  if constexpr (COOP) frag_reduce_groups<C>(acc);
  if (!COOP || gid == 0) frag_store_scaled<C>(acc, 1.f, a.dXch + (size_t)j * a.hf, a.f, gl);
}

// ======================================================================================================================
// kernels.  PASS: 0 forward, 1 backward CSR pass, 2 backward CSC pass.
// ======================================================================================================================
template <class C, int PASS, bool COOP>
__device__ __forceinline__ void gatv2e_group_pass(const Gatv2Edge &a, const Frag<C> &av, Frag<C> &da, int r, int gid,
                                                  int gl) {
  if constexpr (PASS == 0) gatv2e_fwd_row_group<C, COOP>(a, av, r, gid, gl);
  else if constexpr (PASS == 1) gatv2e_bwd_row_group<C, COOP>(a, av, da, r, gid, gl);
  else gatv2e_bwd_col_group<C, COOP>(a, av, r, gid, gl);
}

// End of the CSR pass: the workgroup's share of dattn -> parts[blockIdx.x, head, :].  Each wave sums its groups, waves
// 1.. hand their sums to wave 0 through LDS, which adds them in wave order and stores.  Called by every thread.
template <class C>
__device__ __forceinline__ void gatv2e_store_part(const Gatv2Edge &a, Frag<C> &da, int wave, int gid, int gl) {
  constexpr int W = C::G * C::NCH * C::VEC;  // floats of a (padded) feature row
  __shared__ float red[(kWavesPerBlock - 1) * W];
  frag_reduce_groups<C>(da);
  if (wave > 0 && gid == 0) {
#pragma unroll
    for (int ch = 0; ch < C::NCH; ++ch)
#pragma unroll
      for (int k = 0; k < C::VEC; ++k) red[(wave - 1) * W + (ch * C::G + gl) * C::VEC + k] = da.v[ch][k];
  }
  __syncthreads();
  if (wave == 0 && gid == 0) {
    for (int w = 0; w < kWavesPerBlock - 1; ++w)
#pragma unroll
      for (int ch = 0; ch < C::NCH; ++ch)
#pragma unroll
        for (int k = 0; k < C::VEC; ++k) da.v[ch][k] += red[w * W + (ch * C::G + gl) * C::VEC + k];
    frag_store_scaled<C>(da, 1.f, a.parts + ((size_t)blockIdx.x * a.h + a.head) * a.f, a.f, gl);
  }
}

// general: a wave per row / column, grid-strided over the whole graph.  The forward works in 64-edge tiles through the
// wave's LDS scratch; the backward passes are the COOP form of the group routines.
template <class C, int PASS>
__global__ __launch_bounds__(kBlock) void gatv2_edge_wave_kernel(Gatv2Edge a) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int gid = lane / C::G, gl = lane % C::G;
  a.at_head(blockIdx.y);
  Frag<C> av, da;
  frag_load<C>(av, a.ah, a.f, gl);
  frag_zero<C>(da);
  const int n = PASS == 2 ? a.n_cols : a.m;  // the extent this pass walks: rows, or (CSC pass) columns
  const int beg = blockIdx.x * kWavesPerBlock + wave, step = gridDim.x * kWavesPerBlock;
  if constexpr (PASS == 0) {
    __shared__ __attribute__((aligned(16))) float lds[kWavesPerBlock * kScratchFloatsPerWave];
    float *sw = lds + wave * kScratchFloatsPerWave;
    int *sc = reinterpret_cast<int *>(sw + kWave);
    for (int r = beg; r < n; r += step) gatv2e_fwd_row_wave<C>(a, av, r, lane, sw, sc);
  } else {
    for (int r = beg; r < n; r += step) gatv2e_group_pass<C, PASS, true>(a, av, da, r, gid, gl);
  }
  if constexpr (PASS == 1) gatv2e_store_part<C>(a, da, wave, gid, gl);
}

// low-degree graphs: a workgroup takes blocks of kBlock / G consecutive rows, one lane group per row -- unless a wave's
// EPW rows include one of more than kGatv2EdgeGroupMaxDegree entries, which a single lane group would walk serially while
// the rest of the wave waits: that wave takes its rows one after the other with all its groups on each (COOP).  The choice
// is wave-uniform (ballot).  As gatv2_group_kernel, with the same threshold.
constexpr int kGatv2EdgeGroupMaxDegree = 24;
template <class C, int PASS>
__global__ __launch_bounds__(kBlock) void gatv2_edge_group_kernel(Gatv2Edge a) {
  constexpr int G = C::G, R = kBlock / G;  // rows per block
  const int gid = (threadIdx.x & (kWave - 1)) / G, gl = threadIdx.x % G, wave = threadIdx.x / kWave;
  a.at_head(blockIdx.y);
  Frag<C> av, da;
  frag_load<C>(av, a.ah, a.f, gl);
  frag_zero<C>(da);
  const int *ptr = PASS == 2 ? a.col_ptr : a.row_ptr;
  const int n = PASS == 2 ? a.n_cols : a.m;  // the extent this pass walks: rows, or (CSC pass) columns
  for (int b0 = blockIdx.x * R; b0 < n; b0 += gridDim.x * R) {
    const int r = b0 + threadIdx.x / G;
    const int deg = r < n ? ptr[r + 1] - ptr[r] : 0;
    if (__any(deg > kGatv2EdgeGroupMaxDegree)) {
      for (int rr = b0 + wave * C::EPW; rr < min(n, b0 + (wave + 1) * C::EPW); ++rr)
        gatv2e_group_pass<C, PASS, true>(a, av, da, rr, gid, gl);
    } else if (r < n) {
      gatv2e_group_pass<C, PASS, false>(a, av, da, r, gid, gl);
    }
  }
  if constexpr (PASS == 1) gatv2e_store_part<C>(a, da, wave, gid, gl);
}

// dattn[c] = sum_p parts[p, c] over the nparts partials of the CSR pass (c over h * f): 64 columns per workgroup, wave w
// takes partials w, w + 16, ...; the 16 wave sums are added in wave order.  As gatv2_dattn_reduce_kernel.
constexpr int kGatv2EdgeReduceBlock = 1024, kGatv2EdgeReduceWaves = kGatv2EdgeReduceBlock / kWave;
__global__ __launch_bounds__(kGatv2EdgeReduceBlock) void gatv2_edge_dattn_reduce_kernel(const float *__restrict__ parts,
                                                                                       int nparts, int hf,
                                                                                       float *__restrict__ dattn) {
  __shared__ float red[kGatv2EdgeReduceWaves][kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int c = blockIdx.x * kWave + lane;
  float s = 0.f;
  if (c < hf)
    for (int p = wave; p < nparts; p += kGatv2EdgeReduceWaves) s += parts[(size_t)p * hf + c];
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && c < hf) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < kGatv2EdgeReduceWaves; ++w) t += red[w][lane];
    dattn[c] = t;
  }
}

// grids.  The CSR pass of the backward (PASS 1) is capped at kGatv2Parts workgroups per head whatever m: one partial each.
static dim3 gatv2e_group_grid(int m, int h, int G, long cap) {
  const long per = kBlock / G;
  long blocks = ((long)m + per - 1) / per;
  if (blocks > cap) blocks = cap;
  return dim3((unsigned)(blocks < 1 ? 1 : blocks), h);
}
static dim3 gatv2e_wave_grid(int m, int h, long cap) {
  long want = ((long)m + kWavesPerBlock - 1) / kWavesPerBlock;
  if (want > cap) want = cap;
  return dim3((unsigned)(want < 1 ? 1 : want), h);
}

// -> the launch status; *nparts (PASS 1): the number of partials the pass writes
template <int PASS>
static int launch_gatv2_edge_pass(const Gatv2Edge &a, bool v4, hipStream_t s, int *nparts = nullptr) {
  const int n = PASS == 2 ? a.n_cols : a.m;  // the form is chosen per pass, by the average degree of what it walks
  if (n == 0) return 0;  // nothing to walk and nothing to write (a rectangular graph without rows / without columns)
  const bool groups = low_degree(n, a.nnz);
  return dispatch_cfg(a.f, v4, [&](auto cfg) {
    using C = decltype(cfg);
    const dim3 grid = groups ? gatv2e_group_grid(n, a.h, C::G, PASS == 1 ? kGatv2Parts : 16384)
                             : gatv2e_wave_grid(n, a.h, PASS == 1 ? kGatv2Parts : (1 << 20));
    if (nparts) *nparts = (int)grid.x;
    if (groups) gatv2_edge_group_kernel<C, PASS><<<grid, kBlock, 0, s>>>(a);
    else gatv2_edge_wave_kernel<C, PASS><<<grid, kBlock, 0, s>>>(a);
    return launch_status();
  });
}

static Gatv2Edge gatv2_edge_args(const Csr &g, const Gatv2Graph &v, const float *X_row, const float *X_col, const float *E) {
  Gatv2Edge a{};
  a.m = g.m; a.n_cols = g.n_cols; a.nnz = g.nnz; a.h = g.h; a.f = g.f; a.hf = (size_t)g.h * g.f;
  a.slope = v.slope;
  a.row_ptr = g.row_ptr; a.col_ind = g.col_ind; a.col_ptr = v.col_ptr; a.row_ind = v.row_ind;
  a.ah = v.attn; a.Xrh = X_row; a.Xch = X_col; a.Eh = E;
  return a;
}

int launch_gatv2_edge_fwd(const Csr &g, const Gatv2Graph &v, const float *X_row, const float *X_col, const float *E,
                          float *row_max, float *row_sum, float *out, hipStream_t s) {
  Gatv2Edge a = gatv2_edge_args(g, v, X_row, X_col, E);
  a.outh = out; a.row_max = row_max; a.row_sum = row_sum;
  const bool v4 = (g.f % 4 == 0) && aligned16(v.attn) && aligned16(X_row) && aligned16(X_col) && aligned16(E) && aligned16(out);
  return launch_gatv2_edge_pass<0>(a, v4, s);
}

int launch_gatv2_edge_bwd(const Csr &g, const Gatv2Graph &v, const int *val_idx, const float *X_row, const float *X_col,
                          const float *E, const float *out, const float *row_max, const float *row_sum,
                          const float *grad_out, float *delta, float *ws, float *dX_row, float *dX_col, float *dattn,
                          float *dE, hipStream_t s) {
  Gatv2Edge a = gatv2_edge_args(g, v, X_row, X_col, E);
  a.val_idx = val_idx;
  a.Oh = out; a.dOh = grad_out; a.delta = delta; a.dXrh = dX_row; a.dXch = dX_col; a.parts = ws; a.dEh = dE;
  a.row_max = const_cast<float *>(row_max); a.row_sum = const_cast<float *>(row_sum);
  const bool v4 = (g.f % 4 == 0) && aligned16(v.attn) && aligned16(X_row) && aligned16(X_col) && aligned16(E) &&
                  aligned16(out) && aligned16(grad_out) && aligned16(ws) && aligned16(dX_row) && aligned16(dX_col) &&
                  aligned16(dE);
  int nparts = 0;
  if (int rc = launch_gatv2_edge_pass<1>(a, v4, s, &nparts)) return rc;
  if (int rc = launch_gatv2_edge_pass<2>(a, v4, s)) return rc;
  const int hf = g.h * g.f;
  gatv2_edge_dattn_reduce_kernel<<<(hf + kWave - 1) / kWave, kGatv2EdgeReduceBlock, 0, s>>>(ws, nparts, hf, dattn);
  return launch_status();
}

}  // namespace dfgnn
