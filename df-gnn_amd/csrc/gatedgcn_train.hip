// gatedgcn_train.hip -- residual gated graph convolution (GatedGCN, Bresson & Laurent; the local layer of GraphGPS, PyG's
// ResGatedGraphConv) for gfx950: fused inference and training pair (any graph, no plan, no degree limit).  The attention is
// per DIMENSION -- a sigmoid gate where the other pairs have a softmax over a logit.  Edge e = (i, j), per head:
//   z_e    = (Xr_i + Xc_j) + E_e                  formed like this in all three passes
//   sg_e   = 1 / (1 + exp(-z_e))
//   den_i  = sum_e sg_e
//   out_i  = sum_e sg_e (.) V_j / (den_i + eps)   normalize; without it the plain sum
//   Z_e    = z_e                                  the edge output (optional)
//   s_i    = dO_i / (den_i + eps)                 (without normalize: dO_i)
//   dsg_e  = s_i (.) (V_j - out_i)                (without normalize: s_i (.) V_j)
//   g_e    = dsg_e (.) sg_e (.) (1 - sg_e) + G_e  G = d loss / d Z, the second gradient stream (optional: NULL = zero)
//   dXr_i  = sum_{row i} g_e     dXc_j = sum_{col j} g_e     dV_j = sum_{col j} sg_e (.) s_i     dE_e = g_e (optional)
// E, Z, G, dE: fp32[nnz, h, f] in CSR edge order -- the feature layout with the edge in place of the node, so the row of
// (edge e, head) starts at (e h + head) f and a row's edges are one contiguous block; offsets are size_t (nnz h f exceeds
// 2^31).  They are streams that a pass touches once: non-temporal loads and stores.
//
// The structure is gatv2_edge_train.hip's and gt_gate_train.hip's -- forward, CSR backward pass, CSC backward pass; each as
// a wave per row / column and, for low-degree graphs (nnz < 8 m on the side it walks), as a group of G lanes per row /
// column with the cooperative switch for long rows; no atomics, fixed summation order -- with these differences:
//   no row maximum, no dot product, no cross-lane sum: a lane's slice of an edge never meets another lane's.  The only
//       exchange is the sum over the wave's lane groups at the end of a cooperative row (frag_reduce_groups), so the
//       forward needs no 64-edge tiles either: its wave form is the cooperative group routine, and no kernel uses LDS
//   the saved state is row-sized: out and den [m, h, f].  Nothing per (row, head), nothing per edge
//   the CSC pass needs dO_i / (den_i + eps) of the ROW of each entry: the CSR pass, which forms it once per row, leaves it
//       in a row-sized scratch and the CSC pass gathers that instead of dO_i and den_i and divides nothing.  Without
//       normalize the scratch is not touched: s_i is dO_i itself, and out / den are not read (NULL is accepted)
// E, G, Z and dE absent are uniform branches on a kernel argument: the absent case issues no load or store of that array.
// An absent E or G is a fragment of zeros that goes through the same arithmetic, so E = NULL gives the bits of E = 0
// (z + 0 is exact) and G = NULL those of G = 0 (the last operation of g_e is fmaf(., ., G_e)); Z and dE are stores only.
// sigmoid: v_exp_f32 and v_rcp_f32.  exp(-z) overflows to +inf for z < -88.7 and 1 / (1 + inf) = 0: finite for any finite z.
// An empty row: out = 0, den = 0, dXr = 0; an empty column: dXc = dV = 0.
#include "dfgnn_launch.hpp"

namespace dfgnn {

// Everything the per-row routines need; at_head() offsets every feature-shaped pointer to the workgroup's head.
struct GatedGcn {
  int m, n_cols, nnz, h, f, head;          // m rows (outputs) x n_cols columns (messages)
  size_t hf;
  int normalize;
  float eps;
  const int *row_ptr, *col_ind;            // CSR
  const int *col_ptr, *row_ind, *val_idx;  // CSC (column pass); val_idx: the entry's place in CSR order = its row of E, G
  const float *Eh;                         // [nnz, h, f] CSR order (+ head * f), NULL = zero
  const float *Gh;                         // [nnz, h, f] (+ head * f): d loss / d Z, NULL = zero
  float *Zh;                               // [nnz, h, f] (+ head * f), NULL = not wanted
  float *dEh;                              // [nnz, h, f] (+ head * f), NULL = not wanted
  const float *Xrh, *Xch, *Vh;             // features (+ head * f)
  const float *dOh, *Oh, *Dh;              // output gradient, forward output, forward den (+ head * f); Oh, Dh: normalize only
  const float *Sh;                         // what the CSC pass gathers as s_i: the scratch (normalize) or dO
  float *outh, *denh;                      // forward outputs (+ head * f); denh NULL = not wanted
  float *wsh;                              // [m, h, f] scratch the CSR pass writes s_i to (normalize only)
  float *dXrh, *dXch, *dVh;                // (+ head * f)
  __device__ __forceinline__ void at_head(int hd) {
    head = hd;
    const size_t o = (size_t)hd * f;
    Xrh += o; Xch += o; Vh += o;
    if (Eh) Eh += o;
    if (Gh) Gh += o;
    if (Zh) Zh += o;
    if (dEh) dEh += o;
    if (dOh) dOh += o;
    if (Oh) Oh += o;
    if (Dh) Dh += o;
    if (Sh) Sh += o;
    if (outh) outh += o;
    if (denh) denh += o;
    if (wsh) wsh += o;
    if (dXrh) dXrh += o;
    if (dXch) dXch += o;
    if (dVh) dVh += o;
  }
};

typedef float ggc_f4 __attribute__((ext_vector_type(4)));

// frag_load / frag_store_scaled (s = 1) of dfgnn_device.hpp with the non-temporal hint: the once-read streams E and G, the
// once-written Z and dE.  (As in gt_gate_train.hip.)
template <class C>
__device__ __forceinline__ void ggc_load_nt(Frag<C> &a, const float *__restrict__ base, int f, int gl) {
#pragma unroll
  for (int ch = 0; ch < C::NCH; ++ch) {
    const int c = (ch * C::G + gl) * C::VEC;
    if constexpr (C::VEC == 4) {
      if (c < f) {
        const ggc_f4 t = __builtin_nontemporal_load(reinterpret_cast<const ggc_f4 *>(base + c));
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
__device__ __forceinline__ void ggc_store_nt(const Frag<C> &a, float *__restrict__ base, int f, int gl) {
#pragma unroll
  for (int ch = 0; ch < C::NCH; ++ch) {
    const int c = (ch * C::G + gl) * C::VEC;
    if constexpr (C::VEC == 4) {
      if (c < f) {
        const ggc_f4 t = {a.v[ch][0], a.v[ch][1], a.v[ch][2], a.v[ch][3]};
        __builtin_nontemporal_store(t, reinterpret_cast<ggc_f4 *>(base + c));
      }
    } else {
      if (c < f) __builtin_nontemporal_store(a.v[ch][0], base + c);
    }
  }
}

// an optional per-edge stream: the edge's row, or zeros without a load when the array is absent
template <class C>
__device__ __forceinline__ void ggc_load_opt(Frag<C> &a, const float *__restrict__ arr, size_t off, int f, int gl) {
  if (arr) ggc_load_nt<C>(a, arr + off, f, gl);
  else frag_zero<C>(a);
}

// z = (xr + xc) + xe and sg = sigmoid(z): the one expression of all three passes
template <class C>
__device__ __forceinline__ void ggc_gate(Frag<C> &z, Frag<C> &sg, const Frag<C> &xr, const Frag<C> &xc, const Frag<C> &xe) {
#pragma unroll
  for (int ch = 0; ch < C::NCH; ++ch)
#pragma unroll
    for (int k = 0; k < C::VEC; ++k) {
      const float t = (xr.v[ch][k] + xc.v[ch][k]) + xe.v[ch][k];
      z.v[ch][k] = t;
      sg.v[ch][k] = __builtin_amdgcn_rcpf(1.f + fast_exp(-t));
    }
}

// g = (s (.) (v - o)) (.) sg (.) (1 - sg) + gg: the one expression of both backward passes (o = 0 without normalize)
template <class C>
__device__ __forceinline__ void ggc_edge_grad(Frag<C> &g, const Frag<C> &s, const Frag<C> &v, const Frag<C> &o,
                                              const Frag<C> &sg, const Frag<C> &gg) {
#pragma unroll
  for (int ch = 0; ch < C::NCH; ++ch)
#pragma unroll
    for (int k = 0; k < C::VEC; ++k) {
      const float dsg = s.v[ch][k] * (v.v[ch][k] - o.v[ch][k]);
      g.v[ch][k] = fmaf(dsg * sg.v[ch][k], 1.f - sg.v[ch][k], gg.v[ch][k]);
    }
}

template <class C>
__device__ __forceinline__ void ggc_add(Frag<C> &acc, const Frag<C> &x) {
#pragma unroll
  for (int ch = 0; ch < C::NCH; ++ch)
#pragma unroll
    for (int k = 0; k < C::VEC; ++k) acc.v[ch][k] += x.v[ch][k];
}

// acc[d] += w[d] x[d]
template <class C>
__device__ __forceinline__ void ggc_fma_vec(Frag<C> &acc, const Frag<C> &w, const Frag<C> &x) {
#pragma unroll
  for (int ch = 0; ch < C::NCH; ++ch)
#pragma unroll
    for (int k = 0; k < C::VEC; ++k) acc.v[ch][k] = fmaf(w.v[ch][k], x.v[ch][k], acc.v[ch][k]);
}

// two edges in flight per group where their fragments fit next to everything else: the layouts of up to 8 floats per lane.
// The summation order is the same either way.
template <class C>
constexpr bool kGatedGcnTwoInFlight = C::NCH * C::VEC <= 8;

// ======================================================================================================================
// a group of G lanes (one feature row wide) per row / column, everything in registers, no LDS.  COOP: the row is taken by
// all EPW groups of the wave together (group gid: edges gid, gid + EPW, ...) and the partial sums are added across the
// groups -- the long rows of a low-degree graph, and EVERY row of the wave-per-row form.
// ======================================================================================================================
template <class C, bool COOP>
__device__ __forceinline__ void ggc_fwd_row_group(const GatedGcn &a, int r, int gid, int gl) {
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  const int es = COOP ? C::EPW : 1;
  Frag<C> num, den;
  frag_zero<C>(num);
  frag_zero<C>(den);
  if (deg > 0) {
    Frag<C> xr;
    frag_load<C>(xr, a.Xrh + (size_t)r * a.hf, a.f, gl);
    auto edge = [&](int e, const Frag<C> &xc, const Frag<C> &v, const Frag<C> &xe) {
      Frag<C> z, sg;
      ggc_gate<C>(z, sg, xr, xc, xe);
      if (a.Zh) ggc_store_nt<C>(z, a.Zh + ((size_t)lb + e) * a.hf, a.f, gl);
      ggc_add<C>(den, sg);
      ggc_fma_vec<C>(num, sg, v);
    };
    int e = COOP ? gid : 0;
    if constexpr (kGatedGcnTwoInFlight<C>) {
      for (; e + es < deg; e += 2 * es) {
        const int c0 = a.col_ind[lb + e], c1 = a.col_ind[lb + e + es];
        Frag<C> x0, v0, e0, x1, v1, e1;
        frag_load<C>(x0, a.Xch + (size_t)c0 * a.hf, a.f, gl);
        frag_load<C>(v0, a.Vh + (size_t)c0 * a.hf, a.f, gl);
        ggc_load_opt<C>(e0, a.Eh, ((size_t)lb + e) * a.hf, a.f, gl);
        frag_load<C>(x1, a.Xch + (size_t)c1 * a.hf, a.f, gl);
        frag_load<C>(v1, a.Vh + (size_t)c1 * a.hf, a.f, gl);
        ggc_load_opt<C>(e1, a.Eh, ((size_t)lb + e + es) * a.hf, a.f, gl);
        edge(e, x0, v0, e0);
        edge(e + es, x1, v1, e1);
      }
    }
    for (; e < deg; e += es) {
      const int c0 = a.col_ind[lb + e];
      Frag<C> x0, v0, e0;
      frag_load<C>(x0, a.Xch + (size_t)c0 * a.hf, a.f, gl);
      frag_load<C>(v0, a.Vh + (size_t)c0 * a.hf, a.f, gl);
      ggc_load_opt<C>(e0, a.Eh, ((size_t)lb + e) * a.hf, a.f, gl);
      edge(e, x0, v0, e0);
    }
  }
  if constexpr (COOP) {
    frag_reduce_groups<C>(num);
    frag_reduce_groups<C>(den);
  }
  if (!COOP || gid == 0) {
    if (a.denh) frag_store_scaled<C>(den, 1.f, a.denh + (size_t)r * a.hf, a.f, gl);
    if (a.normalize) {  // a division per row and dimension; an empty row: 0 / eps = 0
#pragma unroll
      for (int ch = 0; ch < C::NCH; ++ch)
#pragma unroll
        for (int k = 0; k < C::VEC; ++k) num.v[ch][k] = num.v[ch][k] / (den.v[ch][k] + a.eps);
    }
    frag_store_scaled<C>(num, 1.f, a.outh + (size_t)r * a.hf, a.f, gl);
  }
}

// CSR pass, row r: s_r = dO_r / (den_r + eps) -> the scratch (normalize); dXr_r = sum_e g_e and the rows dE_e = g_e in one
// sweep, two edges (six loads, eight with G) in flight per group where they fit.  An empty row writes zeros to dXr and
// nothing to the scratch, which no entry of the CSC pass will ask for.
template <class C, bool COOP>
__device__ __forceinline__ void ggc_bwd_row_group(const GatedGcn &a, int r, int gid, int gl) {
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  const int es = COOP ? C::EPW : 1;
  Frag<C> acc;
  frag_zero<C>(acc);
  if (deg > 0) {
    Frag<C> xr, s, o;
    frag_load<C>(xr, a.Xrh + (size_t)r * a.hf, a.f, gl);
    frag_load<C>(s, a.dOh + (size_t)r * a.hf, a.f, gl);
    if (a.normalize) {
      Frag<C> d;
      frag_load<C>(o, a.Oh + (size_t)r * a.hf, a.f, gl);
      frag_load<C>(d, a.Dh + (size_t)r * a.hf, a.f, gl);
#pragma unroll
      for (int ch = 0; ch < C::NCH; ++ch)
#pragma unroll
        for (int k = 0; k < C::VEC; ++k) s.v[ch][k] = s.v[ch][k] / (d.v[ch][k] + a.eps);
      if (!COOP || gid == 0) frag_store_scaled<C>(s, 1.f, a.wsh + (size_t)r * a.hf, a.f, gl);
    } else {
      frag_zero<C>(o);
    }
    auto edge = [&](int e, const Frag<C> &xc, const Frag<C> &v, const Frag<C> &xe, const Frag<C> &gg) {
      Frag<C> z, sg, g;
      ggc_gate<C>(z, sg, xr, xc, xe);
      ggc_edge_grad<C>(g, s, v, o, sg, gg);
      ggc_add<C>(acc, g);
      if (a.dEh) ggc_store_nt<C>(g, a.dEh + ((size_t)lb + e) * a.hf, a.f, gl);
    };
    int e = COOP ? gid : 0;
    if constexpr (kGatedGcnTwoInFlight<C>) {
      for (; e + es < deg; e += 2 * es) {
        const int c0 = a.col_ind[lb + e], c1 = a.col_ind[lb + e + es];
        const size_t o0 = ((size_t)lb + e) * a.hf, o1 = ((size_t)lb + e + es) * a.hf;
        Frag<C> x0, v0, e0, g0, x1, v1, e1, g1;
        frag_load<C>(x0, a.Xch + (size_t)c0 * a.hf, a.f, gl);
        frag_load<C>(v0, a.Vh + (size_t)c0 * a.hf, a.f, gl);
        ggc_load_opt<C>(e0, a.Eh, o0, a.f, gl);
        ggc_load_opt<C>(g0, a.Gh, o0, a.f, gl);
        frag_load<C>(x1, a.Xch + (size_t)c1 * a.hf, a.f, gl);
        frag_load<C>(v1, a.Vh + (size_t)c1 * a.hf, a.f, gl);
        ggc_load_opt<C>(e1, a.Eh, o1, a.f, gl);
        ggc_load_opt<C>(g1, a.Gh, o1, a.f, gl);
        edge(e, x0, v0, e0, g0);
        edge(e + es, x1, v1, e1, g1);
      }
    }
    for (; e < deg; e += es) {
      const int c0 = a.col_ind[lb + e];
      const size_t o0 = ((size_t)lb + e) * a.hf;
      Frag<C> x0, v0, e0, g0;
      frag_load<C>(x0, a.Xch + (size_t)c0 * a.hf, a.f, gl);
      frag_load<C>(v0, a.Vh + (size_t)c0 * a.hf, a.f, gl);
      ggc_load_opt<C>(e0, a.Eh, o0, a.f, gl);
      ggc_load_opt<C>(g0, a.Gh, o0, a.f, gl);
      edge(e, x0, v0, e0, g0);
    }
  }
  if constexpr (COOP) frag_reduce_groups<C>(acc);
  if (!COOP || gid == 0) frag_store_scaled<C>(acc, 1.f, a.dXrh + (size_t)r * a.hf, a.f, gl);
}

// CSC pass, column j: dXc_j = sum g_e, dV_j = sum sg_e (.) s_i over the column's entries; per entry the gathers Xr_i, s_i,
// (normalize) out_i and the rows E[val_idx], G[val_idx] when given, two entries in flight per group where they fit.  An
// empty column writes zeros.
template <class C, bool COOP>
__device__ __forceinline__ void ggc_bwd_col_group(const GatedGcn &a, int j, int gid, int gl) {
  const int lb = a.col_ptr[j], n = a.col_ptr[j + 1] - lb;
  const int es = COOP ? C::EPW : 1;
  Frag<C> aX, aV;
  frag_zero<C>(aX);
  frag_zero<C>(aV);
  if (n > 0) {
    Frag<C> xc, v;
    frag_load<C>(xc, a.Xch + (size_t)j * a.hf, a.f, gl);
    frag_load<C>(v, a.Vh + (size_t)j * a.hf, a.f, gl);
    struct Entry {
      Frag<C> xr, s, o, xe, gg;
    };
    auto load = [&](Entry &x, int t) {
      const size_t ro = (size_t)a.row_ind[lb + t] * a.hf;
      const size_t eo = (size_t)a.val_idx[lb + t] * a.hf;  // E and G are in CSR order
      frag_load<C>(x.xr, a.Xrh + ro, a.f, gl);
      frag_load<C>(x.s, a.Sh + ro, a.f, gl);
      if (a.normalize) frag_load<C>(x.o, a.Oh + ro, a.f, gl);
      else frag_zero<C>(x.o);
      ggc_load_opt<C>(x.xe, a.Eh, eo, a.f, gl);
      ggc_load_opt<C>(x.gg, a.Gh, eo, a.f, gl);
    };
    auto accum = [&](const Entry &x) {
      Frag<C> z, sg, g;
      ggc_gate<C>(z, sg, x.xr, xc, x.xe);
      ggc_fma_vec<C>(aV, sg, x.s);
      ggc_edge_grad<C>(g, x.s, v, x.o, sg, x.gg);
      ggc_add<C>(aX, g);
    };
    int t = COOP ? gid : 0;
    if constexpr (kGatedGcnTwoInFlight<C>) {
      for (; t + es < n; t += 2 * es) {
        Entry x0, x1;
        load(x0, t);
        load(x1, t + es);
        accum(x0);
        accum(x1);
      }
    }
    for (; t < n; t += es) {
      Entry x0;
      load(x0, t);
      accum(x0);
    }
  }
  if constexpr (COOP) {
    frag_reduce_groups<C>(aX);
    frag_reduce_groups<C>(aV);
  }
  if (!COOP || gid == 0) {
    frag_store_scaled<C>(aX, 1.f, a.dXch + (size_t)j * a.hf, a.f, gl);
    frag_store_scaled<C>(aV, 1.f, a.dVh + (size_t)j * a.hf, a.f, gl);
  }
}

// ======================================================================================================================
// kernels.  PASS: 0 forward, 1 backward CSR pass, 2 backward CSC pass.
// ======================================================================================================================
template <class C, int PASS, bool COOP>
__device__ __forceinline__ void ggc_group_pass(const GatedGcn &a, int r, int gid, int gl) {
  if constexpr (PASS == 0) ggc_fwd_row_group<C, COOP>(a, r, gid, gl);
  else if constexpr (PASS == 1) ggc_bwd_row_group<C, COOP>(a, r, gid, gl);
  else ggc_bwd_col_group<C, COOP>(a, r, gid, gl);
}

// general: a wave per row / column, grid-strided over the whole graph: the COOP form of the group routines (no LDS).
template <class C, int PASS>
__global__ __launch_bounds__(kBlock) void gatedgcn_wave_kernel(GatedGcn a) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  a.at_head(blockIdx.y);
  const int n = PASS == 2 ? a.n_cols : a.m;  // the extent this pass walks: rows, or (CSC pass) columns
  const int beg = blockIdx.x * kWavesPerBlock + wave, step = gridDim.x * kWavesPerBlock;
  for (int r = beg; r < n; r += step) ggc_group_pass<C, PASS, true>(a, r, lane / C::G, lane % C::G);
}

// low-degree graphs: a workgroup takes blocks of kBlock / G consecutive rows, one lane group per row -- unless a wave's
// EPW rows include one of more than kGatedGcnGroupMaxDegree entries, which a single lane group would walk serially while
// the rest of the wave waits: that wave takes its rows one after the other with all its groups on each (COOP).  The choice
// is wave-uniform (ballot): no barrier, no LDS.  As gt_gate_group_kernel, with the same threshold.
constexpr int kGatedGcnGroupMaxDegree = 24;
template <class C, int PASS>
__global__ __launch_bounds__(kBlock) void gatedgcn_group_kernel(GatedGcn a) {
  constexpr int G = C::G, R = kBlock / G;  // rows per block
  const int gid = (threadIdx.x & (kWave - 1)) / G, gl = threadIdx.x % G, wave = threadIdx.x / kWave;
  a.at_head(blockIdx.y);
  const int *ptr = PASS == 2 ? a.col_ptr : a.row_ptr;
  const int n = PASS == 2 ? a.n_cols : a.m;  // the extent this pass walks: rows, or (CSC pass) columns
  for (int b0 = blockIdx.x * R; b0 < n; b0 += gridDim.x * R) {
    const int r = b0 + threadIdx.x / G;
    const int deg = r < n ? ptr[r + 1] - ptr[r] : 0;
    if (__any(deg > kGatedGcnGroupMaxDegree)) {
      for (int rr = b0 + wave * C::EPW; rr < min(n, b0 + (wave + 1) * C::EPW); ++rr)
        ggc_group_pass<C, PASS, true>(a, rr, gid, gl);
    } else if (r < n) {
      ggc_group_pass<C, PASS, false>(a, r, gid, gl);
    }
  }
}

static dim3 ggc_group_grid(int m, int h, int G) {
  const long per = kBlock / G;
  long blocks = ((long)m + per - 1) / per;
  if (blocks > 16384) blocks = 16384;
  return dim3((unsigned)(blocks < 1 ? 1 : blocks), h);
}
static dim3 ggc_wave_grid(int m, int h) {
  const long want = ((long)m + kWavesPerBlock - 1) / kWavesPerBlock;
  return dim3((unsigned)(want > (1 << 20) ? (1 << 20) : want), h);
}

template <int PASS>
static int launch_gatedgcn_pass(const GatedGcn &a, bool v4, hipStream_t s) {
  const int n = PASS == 2 ? a.n_cols : a.m;  // the form is chosen per pass, by the average degree of what it walks
  if (n == 0) return 0;  // nothing to walk and nothing to write (a rectangular graph without rows / without columns)
  const bool groups = low_degree(n, a.nnz);
  return dispatch_cfg(a.f, v4, [&](auto cfg) {
    using C = decltype(cfg);
    if (groups) gatedgcn_group_kernel<C, PASS><<<ggc_group_grid(n, a.h, C::G), kBlock, 0, s>>>(a);
    else gatedgcn_wave_kernel<C, PASS><<<ggc_wave_grid(n, a.h), kBlock, 0, s>>>(a);
    return launch_status();
  });
}

static GatedGcn gatedgcn_args(const Csr &g, const GatedGcnGraph &v, const float *X_row, const float *X_col, const float *V,
                              const float *E) {
  GatedGcn a{};
  a.m = g.m; a.n_cols = g.n_cols; a.nnz = g.nnz; a.h = g.h; a.f = g.f; a.hf = (size_t)g.h * g.f;
  a.normalize = v.normalize ? 1 : 0; a.eps = v.eps;
  a.row_ptr = g.row_ptr; a.col_ind = g.col_ind; a.col_ptr = v.col_ptr; a.row_ind = v.row_ind; a.val_idx = v.val_idx;
  a.Xrh = X_row; a.Xch = X_col; a.Vh = V; a.Eh = E;
  return a;
}

int launch_gatedgcn_fwd(const Csr &g, const GatedGcnGraph &v, const float *X_row, const float *X_col, const float *V,
                        const float *E, float *den, float *out, float *Z, hipStream_t s) {
  GatedGcn a = gatedgcn_args(g, v, X_row, X_col, V, E);
  a.denh = den; a.outh = out; a.Zh = Z;
  const bool v4 = (g.f % 4 == 0) && aligned16(X_row) && aligned16(X_col) && aligned16(V) && aligned16(E) && aligned16(den) &&
                  aligned16(out) && aligned16(Z);
  return launch_gatedgcn_pass<0>(a, v4, s);
}

int launch_gatedgcn_bwd(const Csr &g, const GatedGcnGraph &v, const float *X_row, const float *X_col, const float *V,
                        const float *E, const float *out, const float *den, const float *grad_out, const float *G,
                        float *dX_row, float *dX_col, float *dV, float *dE, float *ws, hipStream_t s) {
  GatedGcn a = gatedgcn_args(g, v, X_row, X_col, V, E);
  a.dOh = grad_out; a.Gh = G; a.dXrh = dX_row; a.dXch = dX_col; a.dVh = dV; a.dEh = dE;
  if (v.normalize) {
    a.Oh = out; a.Dh = den; a.wsh = ws; a.Sh = ws;
  } else {  // out, den and the scratch are not touched: s_i is dO_i
    a.Sh = grad_out;
    out = nullptr; den = nullptr; ws = nullptr;  // (whatever was passed takes no part in the alignment rule)
  }
  const bool v4 = (g.f % 4 == 0) && aligned16(X_row) && aligned16(X_col) && aligned16(V) && aligned16(E) && aligned16(out) &&
                  aligned16(den) && aligned16(grad_out) && aligned16(G) && aligned16(dX_row) && aligned16(dX_col) &&
                  aligned16(dV) && aligned16(dE) && aligned16(ws);
  if (int rc = launch_gatedgcn_pass<1>(a, v4, s)) return rc;
  return launch_gatedgcn_pass<2>(a, v4, s);
}

}  // namespace dfgnn
