// gt_tbias_train.hip -- GT conv with a TYPED additive attention bias for gfx950: the scalar added to an edge's logit is looked
// up from a small table by the edge's type.  Fused inference and training pair, general kernels (any graph, no plan, no
// degree limit).  Graphormer's spatial encoding (nn.Embedding(num_spatial, num_heads) indexed by the shortest-path bucket),
// T5 / Swin-style relative-position bias, any bucketed-distance or edge-type bias: edge e = (i, j) has a type
// t = etype[e] in [0, T), the table is B[T, h], and per head hd
//   s_e    = val_e <Q_i, K_j> + B[t, hd]
//   P_e    = exp(s_e - row_max_i) / row_sum_i
//   out_i  = sum_e P_e V_j
//   delta_i = <dO_i, out_i>
//   dP_e   = <dO_i, V_j>
//   dS_e   = P_e (dP_e - delta_i)
//   dQ_i   = sum_e dS_e val_e K_j
//   dK_j   = sum_e dS_e val_e Q_i
//   dV_j   = sum_e P_e dO_i
//   dB[t, hd] = sum_{e : etype[e] = t} dS_e
// which is gt_bias_train.hip with bias[hd, e] = B[etype[e], hd] and dB = index_add(dbias.t(), etype) -- without anything of
// size h nnz: an edge costs 4 bytes of type per pass instead of 4 h bytes of bias, and dbias is never written.
//
// The structure is gt_bias_train.hip's, pass for pass, and the code is a copy with the lookup worked in, so that the
// existing pairs' code objects stay as they are and this operator is one file:
//   forward           the load of bias[lb + e] becomes a load of the type and of B[t h + hd]; the wave form reads a tile's
//                     64 types as one coalesced load next to the column ids.  A lane needs only its own edge's bias (the
//                     logits of a tile are finished one per lane), so type and bias stay in registers: the typed pair's
//                     third LDS array, which hands a type to whichever lane group gathers the edge's table row, has
//                     nothing to do here
//   backward, CSC     takes its types from etype_csc[nnz], the types in CSC entry order (made once per graph by the
//                     caller): a stream, not a gather through val_idx, which is read only for edge values
//   backward, CSR     dB == NULL: the bias pair's pass without the store of dbias, nothing more.  dB != NULL: a bounded
//                     number of persistent workgroups per head; every wave owns a table of T floats in LDS, which it
//                     zeroes itself, and lane 0 of a lane group adds its edge's dS_e to the slot of its type, the groups
//                     of a wave one after the other (two groups may hold the same type; gtz_table_add); at the end the
//                     workgroup adds its waves' tables in wave order and stores one full partial [T] per head (zeros
//                     included) to ws; gt_tbias_reduce_kernel then sums the partials in a fixed order.  No atomics,
//                     neither global nor LDS: two calls give the same bits
// The table itself is NOT staged in LDS: per head it is T floats with stride h, at most 16 KB of lines at the supported
// limit and usually a few lines, every workgroup of a head reads the same ones, so it lives in L2 and the hot lines in the
// vector L1 -- the typed pair's choice, kept here; staging would cost each workgroup a strided copy of T floats before its
// first row.
// The bias is added after the val multiply and before the running maximum, with the expressions of gt_bias_train.hip, so
// out, the statistics, dQ, dK and dV equal the bias pair's on the materialised bias to the bit.
// Masks.  B[t, hd] = -inf masks every edge of type t for that head: P_e = 0, nothing is added to any sum, dB[t, hd] = 0.
// A (row, head) whose edges are all masked behaves like an empty row: out = 0, row_max = -1e38, row_sum = 0, dQ = 0 -- the
// forward tests the running maximum, not the degree, and both backward passes take 1 / row_sum of such a row as 0, so
// nothing is NaN or inf.  +inf and NaN in B are the caller's error.  col_ind < n_cols, row_ind < m and 0 <= etype < T are
// the caller's contract: the kernels index by them unchecked.
#include "dfgnn_launch.hpp"
#include "dfgnn_rows.hpp"

namespace dfgnn {

// Everything the per-row routines need; at_head() offsets the feature pointers and B to the workgroup's head.
struct GtTBias {
  int m, n_cols, nnz, h, f, head, T;          // m rows (queries, outputs) x n_cols columns (keys, values); T types
  size_t hf;
  const int *row_ptr, *col_ind;                // CSR
  const float *val;                            // CSR order, NULL = unit values
  const int *etype, *etype_csc;                // [nnz] types in CSR order / in CSC entry order
  const float *Bh;                             // [T, h] (+ head): type t's bias is Bh[t * h]
  float *parts;                                // [workgroups of the CSR pass, T, h] partial sums of dB, NULL = not wanted
  const int *col_ptr, *row_ind, *val_idx;      // CSC (column pass)
  const float *Qh, *Kh, *Vh, *dOh, *Oh;        // features, output gradient, forward output (+ head * f)
  float *row_max, *row_sum, *delta;            // [m, h]: written by the forward / the CSR pass, read by the passes after
  float *outh, *dQh, *dKh, *dVh;               // (+ head * f)
  __device__ __forceinline__ size_t nh(int node) const { return (size_t)node * h + head; }
  __device__ __forceinline__ float bias_of(int t) const { return Bh[(size_t)t * h]; }
  __device__ __forceinline__ void at_head(int hd) {
    head = hd;
    const size_t o = (size_t)hd * f;
    Qh += o; Kh += o; Vh += o;
    if (Bh) Bh += hd;
    if (dOh) dOh += o;
    if (Oh) Oh += o;
    if (outh) outh += o;
    if (dQh) dQh += o;
    if (dKh) dKh += o;
    if (dVh) dVh += o;
  }
};

// the saved maximum of a row: a row without an unmasked edge gets the sentinel of the statistics pairs (include/dfgnn.h)
__device__ __forceinline__ float gtz_saved_max(float m_run) { return m_run == -INFINITY ? -1e38f : m_run; }
// 1 / row_sum; a row without an unmasked edge (row_sum = 0) has P = 0 everywhere
__device__ __forceinline__ float gtz_inv_sum(float sum) { return sum != 0.f ? 1.f / sum : 0.f; }

// ======================================================================================================================
// forward, a wave per row: 64-edge tiles (sw / sc: the wave's 64-float / 64-int LDS scratch)
// ======================================================================================================================
template <class C>
__device__ __forceinline__ void gtz_fwd_row_wave(const GtTBias &a, int r, int lane, float *sw, int *sc) {
  const int gid = lane / C::G, gl = lane % C::G;
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  Frag<C> q, acc;
  frag_load<C>(q, a.Qh + (size_t)r * a.hf, a.f, gl);
  frag_zero<C>(acc);
  float m_run = -INFINITY, l_run = 0.f;
  for (int t0 = 0; t0 < deg; t0 += kWave) {
    const int nt = min(kWave, deg - t0);
    sc[lane] = (lane < nt) ? a.col_ind[lb + t0 + lane] : 0;
    const float b = (lane < nt) ? a.bias_of(a.etype[lb + t0 + lane]) : 0.f;  // one coalesced load of the tile's types
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
  const float inv = gtz_inv_sum(l_run);  // empty or fully masked row -> 0
  frag_reduce_groups<C>(acc);
  if (gid == 0) frag_store_scaled<C>(acc, inv, a.outh + (size_t)r * a.hf, a.f, gl);
  if (lane == 0 && a.row_max) {
    a.row_max[a.nh(r)] = gtz_saved_max(m_run);
    a.row_sum[a.nh(r)] = l_run;
  }
}

// ======================================================================================================================
// a group of G lanes (one feature row wide) per row / column, everything in registers.  COOP: the row is taken by all
// EPW groups of the wave together (group gid: edges gid, gid + EPW, ...) and the partial results are merged across
// the groups -- the long rows of a low-degree graph, and EVERY row of the wave-per-row form of the two backward passes.
// ======================================================================================================================
template <class C, bool COOP>
__device__ __forceinline__ void gtz_fwd_row_group(const GtTBias &a, int r, int gid, int gl) {
  const int lb = a.row_ptr[r], deg = a.row_ptr[r + 1] - lb;
  Frag<C> q, acc;
  frag_load<C>(q, a.Qh + (size_t)r * a.hf, a.f, gl);
  frag_zero<C>(acc);
  float m_run = -INFINITY, l_run = 0.f;  // online softmax: one sweep, one dependent gather chain per edge
  for (int e = COOP ? gid : 0; e < deg; e += COOP ? C::EPW : 1) {
    const int c = a.col_ind[lb + e];
    const float b = a.bias_of(a.etype[lb + e]);
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
    frag_store_scaled<C>(acc, gtz_inv_sum(l_run), a.outh + (size_t)r * a.hf, a.f, gl);
    if (gl == 0 && a.row_max) {
      a.row_max[a.nh(r)] = gtz_saved_max(m_run);
      a.row_sum[a.nh(r)] = l_run;
    }
  }
}

// tab[t] += ds for the edges the wave's lane groups hold right now, one group after the other: two groups may hold the
// same type, and a fixed order is what makes the sum reproducible.  Lane 0 of a group does a plain LDS load and store; a
// wave's DS operations execute in issue order, and wave_sync() keeps the compiler from merging or reordering the steps.
// The order is group order among the groups that reach this call together.  The callers' loops have trip counts that
// differ per group (the two-edge loop against its tail; rows of different degree in the lane-group form), so after the
// wave has diverged the groups of one path add before those of the other, in the order the compiled code serialises the
// paths: fixed for one binary and one input -- two calls give the same bits -- but not a property of the source
// (gtt_table_add of gt_typed_train.hip, a scalar wide).
template <class C>
__device__ __forceinline__ void gtz_table_add(float *tab, int t, float ds, int gid, int gl) {
#pragma unroll 1
  for (int g = 0; g < C::EPW; ++g) {
    if (gid == g && gl == 0) tab[t] += ds;
    wave_sync();
  }
}

// CSR pass, row r: delta_r = <dO_r, out_r> -> delta; dQ_r = sum_e dS_e val_e K_c in one sweep, two edges (four gathers)
// in flight per group.  Every lane of a group holds the two dot products of its edge (lanes_sum is an all-reduce), so the
// edge's dS needs no exchange.  TAB: lane 0 of the group adds it to slot t of the wave's LDS table `tab`.
template <class C, bool COOP, bool TAB>
__device__ __forceinline__ void gtz_bwd_row_group(const GtTBias &a, int r, int gid, int gl, float *tab) {
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
    const float mx = a.row_max[a.nh(r)], inv = gtz_inv_sum(a.row_sum[a.nh(r)]);
    auto weight = [&](int e, int t, float b, const Frag<C> &k, const Frag<C> &v) {  // dS_e -> the table; returns dS_e val_e
      const float vl = a.val ? a.val[lb + e] : 1.f;
      const float s = vl * lanes_sum<C::G>(frag_dot<C>(q, k)) + b;
      const float dp = lanes_sum<C::G>(frag_dot<C>(go, v));
      const float ds = fast_exp(s - mx) * inv * (dp - dl);  // a masked edge: exp(-inf) = 0
      if constexpr (TAB) gtz_table_add<C>(tab, t, ds, gid, gl);
      return ds * vl;
    };
    int e = COOP ? gid : 0;
    for (; e + es < deg; e += 2 * es) {
      const int c0 = a.col_ind[lb + e], c1 = a.col_ind[lb + e + es];
      const int t0 = a.etype[lb + e], t1 = a.etype[lb + e + es];
      const float b0 = a.bias_of(t0), b1 = a.bias_of(t1);
      Frag<C> k0, v0, k1, v1;
      frag_load<C>(k0, a.Kh + (size_t)c0 * a.hf, a.f, gl);
      frag_load<C>(v0, a.Vh + (size_t)c0 * a.hf, a.f, gl);
      frag_load<C>(k1, a.Kh + (size_t)c1 * a.hf, a.f, gl);
      frag_load<C>(v1, a.Vh + (size_t)c1 * a.hf, a.f, gl);
      frag_fma<C>(acc, weight(e, t0, b0, k0, v0), k0);
      frag_fma<C>(acc, weight(e + es, t1, b1, k1, v1), k1);
    }
    for (; e < deg; e += es) {
      const int c0 = a.col_ind[lb + e], t0 = a.etype[lb + e];
      const float b0 = a.bias_of(t0);
      Frag<C> k0, v0;
      frag_load<C>(k0, a.Kh + (size_t)c0 * a.hf, a.f, gl);
      frag_load<C>(v0, a.Vh + (size_t)c0 * a.hf, a.f, gl);
      frag_fma<C>(acc, weight(e, t0, b0, k0, v0), k0);
    }
  }
  if constexpr (COOP) frag_reduce_groups<C>(acc);
  if (!COOP || gid == 0) {
    frag_store_scaled<C>(acc, 1.f, a.dQh + (size_t)r * a.hf, a.f, gl);
    if (gl == 0) a.delta[a.nh(r)] = dl;
  }
}

// CSC pass, column j: dV_j = sum P_e dO_i, dK_j = sum P_e (dP_e - delta_i) val_e Q_i over the column's entries, two
// entries (four gathers + their row scalars, type, bias and edge value) in flight per group.  An empty column writes zeros.
template <class C, bool COOP>
__device__ __forceinline__ void gtz_bwd_col_group(const GtTBias &a, int j, int gid, int gl) {
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
      x.b = a.bias_of(a.etype_csc[lb + t]);            // the types are streamed in entry order
      x.vl = a.val ? a.val[a.val_idx[lb + t]] : 1.f;  // val is in CSR order
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
// kernels.  PASS: 0 forward, 1 backward CSR pass, 2 backward CSC pass.  TAB (PASS 1 only): dB is wanted.
// ======================================================================================================================
template <class C, int PASS, bool COOP, bool TAB>
__device__ __forceinline__ void gtz_group_pass(const GtTBias &a, int r, int gid, int gl, float *tab) {
  if constexpr (PASS == 0) gtz_fwd_row_group<C, COOP>(a, r, gid, gl);
  else if constexpr (PASS == 1) gtz_bwd_row_group<C, COOP, TAB>(a, r, gid, gl, tab);
  else gtz_bwd_col_group<C, COOP>(a, r, gid, gl);
}

// The waves' tables of a TAB workgroup: kWavesPerBlock x T floats of dynamic LDS (at most 64 KB: no attribute call).
extern __shared__ __attribute__((aligned(16))) float gtz_tables[];

// Start of a TAB kernel: every wave zeroes its own table (no workgroup barrier needed before it adds to it).
__device__ __forceinline__ float *gtz_table_init(const GtTBias &a, int wave, int lane) {
  float *tab = gtz_tables + (size_t)wave * a.T;
  for (int i = lane; i < a.T; i += kWave) tab[i] = 0.f;
  wave_sync();
  return tab;
}

// End of a TAB kernel: the workgroup's partial [T] of this head = its waves' tables added in wave order ->
// parts[blockIdx.x, :, head], every slot, the zeros of types it never met included.  Called by every thread.
__device__ __forceinline__ void gtz_table_store(const GtTBias &a) {
  __syncthreads();
  float *dst = a.parts + (size_t)blockIdx.x * a.T * a.h + a.head;
  for (int i = threadIdx.x; i < a.T; i += kBlock) {
    float s = gtz_tables[i];
#pragma unroll
    for (int w = 1; w < kWavesPerBlock; ++w) s += gtz_tables[(size_t)w * a.T + i];
    dst[(size_t)i * a.h] = s;
  }
}

// general: a wave per row / column, grid-strided over the whole graph.  The forward works in 64-edge tiles through the
// wave's LDS scratch; the backward passes are the COOP form of the group routines.
template <class C, int PASS, bool TAB>
__global__ __launch_bounds__(kBlock) void gt_tbias_wave_kernel(GtTBias a) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  a.at_head(blockIdx.y);
  const int n = PASS == 2 ? a.n_cols : a.m;  // the extent this pass walks: rows, or (CSC pass) columns
  const int beg = blockIdx.x * kWavesPerBlock + wave, step = gridDim.x * kWavesPerBlock;
  if constexpr (PASS == 0) {
    __shared__ __attribute__((aligned(16))) float lds[kWavesPerBlock * kScratchFloatsPerWave];
    float *sw = lds + wave * kScratchFloatsPerWave;
    int *sc = reinterpret_cast<int *>(sw + kWave);
    for (int r = beg; r < n; r += step) gtz_fwd_row_wave<C>(a, r, lane, sw, sc);
  } else {
    float *tab = nullptr;
    if constexpr (TAB) tab = gtz_table_init(a, wave, lane);
    for (int r = beg; r < n; r += step) gtz_group_pass<C, PASS, true, TAB>(a, r, lane / C::G, lane % C::G, tab);
    if constexpr (TAB) gtz_table_store(a);
  }
}

// low-degree graphs: a workgroup takes blocks of kBlock / G consecutive rows, one lane group per row -- unless a wave's
// EPW rows include one of more than kGtTBiasGroupMaxDegree entries, which a single lane group would walk serially while
// the rest of the wave waits: that wave takes its rows one after the other with all its groups on each (COOP).  The choice
// is wave-uniform (ballot): no barrier.  As gt_bias_group_kernel of gt_bias_train.hip, with the same threshold.
constexpr int kGtTBiasGroupMaxDegree = 24;
template <class C, int PASS, bool TAB>
__global__ __launch_bounds__(kBlock) void gt_tbias_group_kernel(GtTBias a) {
  constexpr int G = C::G, R = kBlock / G;  // rows per block
  const int gid = (threadIdx.x & (kWave - 1)) / G, gl = threadIdx.x % G, wave = threadIdx.x / kWave;
  a.at_head(blockIdx.y);
  const int *ptr = PASS == 2 ? a.col_ptr : a.row_ptr;
  const int n = PASS == 2 ? a.n_cols : a.m;  // the extent this pass walks: rows, or (CSC pass) columns
  float *tab = nullptr;
  if constexpr (TAB) tab = gtz_table_init(a, wave, threadIdx.x & (kWave - 1));
  for (int b0 = blockIdx.x * R; b0 < n; b0 += gridDim.x * R) {
    const int r = b0 + threadIdx.x / G;
    const int deg = r < n ? ptr[r + 1] - ptr[r] : 0;
    if (__any(deg > kGtTBiasGroupMaxDegree)) {
      for (int rr = b0 + wave * C::EPW; rr < min(n, b0 + (wave + 1) * C::EPW); ++rr)
        gtz_group_pass<C, PASS, true, TAB>(a, rr, gid, gl, tab);
    } else if (r < n) {
      gtz_group_pass<C, PASS, false, TAB>(a, r, gid, gl, tab);
    }
  }
  if constexpr (TAB) gtz_table_store(a);
}

// dB[c] = sum_p parts[p, c] over the nparts partials of the CSR pass (c over T * h): 64 entries per workgroup, wave w
// takes partials w, w + 16, ... in increasing order; the 16 wave sums are added in wave order.  nparts = 0: dB = 0.
constexpr int kGtTBiasReduceBlock = 1024, kGtTBiasReduceWaves = kGtTBiasReduceBlock / kWave;
__global__ __launch_bounds__(kGtTBiasReduceBlock) void gt_tbias_reduce_kernel(const float *__restrict__ parts, int nparts,
                                                                              int th, float *__restrict__ dB) {
  __shared__ float red[kGtTBiasReduceWaves][kWave];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int c = blockIdx.x * kWave + lane;
  float s = 0.f;
  if (c < th)
    for (int p = wave; p < nparts; p += kGtTBiasReduceWaves) s += parts[(size_t)p * th + c];
  red[wave][lane] = s;
  __syncthreads();
  if (wave == 0 && c < th) {
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < kGtTBiasReduceWaves; ++w) t += red[w][lane];
    dB[c] = t;
  }
}

// grids.  Forward, CSC pass and the CSR pass without dB: the bias pair's.  The CSR pass with dB is capped twice.  By
// gt_tbias_parts(T), which sizes ws: no more partials per head than workgroups that one head can keep resident (a
// persistent workgroup beyond that only adds a partial), at most 1024.  And by the work: zeroing four tables, merging them
// and storing and reducing the partial is about 10 T LDS / memory operations per workgroup, an edge about 50 / EPW wave
// instructions, so a wave that walks T / 8 edges at least (and never fewer than 8) spends about a tenth on its table.
int gt_tbias_parts(int T) {
  const long fit = (160L * 1024) / ((long)kWavesPerBlock * T * (long)sizeof(float));  // workgroups per CU by LDS
  const long parts = 256 * (fit < 1 ? 1 : fit);                                        // 256 CUs
  return (int)(parts > kGtTBiasParts ? kGtTBiasParts : parts);
}
static dim3 gtz_group_grid(int m, int h, int G, long cap) {
  const long per = kBlock / G;
  long blocks = ((long)m + per - 1) / per;
  if (blocks > cap) blocks = cap;
  return dim3((unsigned)(blocks < 1 ? 1 : blocks), h);
}
static dim3 gtz_wave_grid(int m, int h, long cap) {
  long want = ((long)m + kWavesPerBlock - 1) / kWavesPerBlock;
  if (want > cap) want = cap;
  return dim3((unsigned)(want < 1 ? 1 : want), h);
}
static long gtz_table_cap(int nnz, int T) {
  const long per_wave = T / 8 > 8 ? T / 8 : 8;
  long cap = (long)nnz / ((long)kWavesPerBlock * per_wave);
  const long parts = gt_tbias_parts(T);
  if (cap > parts) cap = parts;
  return cap < 1 ? 1 : cap;
}

// -> the launch status; *nparts (TAB): the number of partials the pass writes
template <int PASS, bool TAB>
static int launch_gt_tbias_pass(const GtTBias &a, bool v4, hipStream_t s, int *nparts = nullptr) {
  const int n = PASS == 2 ? a.n_cols : a.m;  // the form is chosen per pass, by the average degree of what it walks
  if (n == 0) return 0;  // nothing to walk and nothing to write (a rectangular graph without rows / without columns)
  const bool groups = low_degree(n, a.nnz);
  return dispatch_cfg(a.f, v4, [&](auto cfg) {
    using C = decltype(cfg);
    const dim3 grid = groups ? gtz_group_grid(n, a.h, C::G, TAB ? gtz_table_cap(a.nnz, a.T) : 16384)
                             : gtz_wave_grid(n, a.h, TAB ? gtz_table_cap(a.nnz, a.T) : (1 << 20));
    size_t lds = 0;
    if constexpr (TAB) {
      lds = (size_t)kWavesPerBlock * a.T * sizeof(float);  // <= 64 KB by kGtTBiasMaxTypes: the default limit of dynamic LDS
      *nparts = (int)grid.x;
    }
    if (groups) gt_tbias_group_kernel<C, PASS, TAB><<<grid, kBlock, lds, s>>>(a);
    else gt_tbias_wave_kernel<C, PASS, TAB><<<grid, kBlock, lds, s>>>(a);
    return launch_status();
  });
}

static GtTBias gt_tbias_args(const Csr &g, const GtTBiasTable &t, const float *Q, const float *K, const float *V) {
  GtTBias a{};
  a.m = g.m; a.n_cols = g.n_cols; a.nnz = g.nnz; a.h = g.h; a.f = g.f; a.hf = (size_t)g.h * g.f;
  a.row_ptr = g.row_ptr; a.col_ind = g.col_ind; a.val = g.val;
  a.T = t.T; a.etype = t.etype; a.etype_csc = t.etype_csc; a.Bh = t.B;
  a.Qh = Q; a.Kh = K; a.Vh = V;
  return a;
}

int launch_gt_tbias_fwd(const Csr &g, const GtTBiasTable &t, const float *Q, const float *K, const float *V,
                        float *row_max, float *row_sum, float *out, hipStream_t s) {
  GtTBias a = gt_tbias_args(g, t, Q, K, V);
  a.outh = out; a.row_max = row_max; a.row_sum = row_sum;
  return launch_gt_tbias_pass<0, false>(a, (g.f % 4 == 0) && aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(out), s);
}

int launch_gt_tbias_bwd_rows(const Csr &g, const GtTBiasTable &t, const float *Q, const float *K, const float *V,
                             const float *out, const float *row_max, const float *row_sum, const float *grad_out,
                             float *delta, float *dQ, float *ws, float *dB, hipStream_t s) {
  GtTBias a = gt_tbias_args(g, t, Q, K, V);
  a.Oh = out; a.dOh = grad_out; a.delta = delta; a.dQh = dQ; a.parts = ws;
  a.row_max = const_cast<float *>(row_max); a.row_sum = const_cast<float *>(row_sum);
  const bool v4 = (g.f % 4 == 0) && aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(out) &&
                  aligned16(grad_out) && aligned16(dQ);
  if (!dB) return launch_gt_tbias_pass<1, false>(a, v4, s);
  if (t.T > kGtTBiasMaxTypes) return kErrUnsupported;
  int nparts = 0;  // without rows or edges no workgroup has a table to fill: dB = 0 from the reduction alone
  if (g.nnz == 0) {
    if (int rc = launch_gt_tbias_pass<1, false>(a, v4, s)) return rc;
  } else {
    if (int rc = launch_gt_tbias_pass<1, true>(a, v4, s, &nparts)) return rc;
  }
  const long th = (long)t.T * g.h;
  if (th == 0) return 0;
  gt_tbias_reduce_kernel<<<(unsigned)((th + kWave - 1) / kWave), kGtTBiasReduceBlock, 0, s>>>(ws, nparts, (int)th, dB);
  return launch_status();
}

int launch_gt_tbias_bwd_cols(const Csr &g, const GtTBiasTable &t, const int *col_ptr, const int *row_ind,
                             const int *val_idx, const float *Q, const float *K, const float *V, const float *row_max,
                             const float *row_sum, const float *delta, const float *grad_out, float *dK, float *dV,
                             hipStream_t s) {
  GtTBias a = gt_tbias_args(g, t, Q, K, V);
  a.col_ptr = col_ptr; a.row_ind = row_ind; a.val_idx = val_idx;
  a.dOh = grad_out; a.dKh = dK; a.dVh = dV;
  a.row_max = const_cast<float *>(row_max); a.row_sum = const_cast<float *>(row_sum);
  a.delta = const_cast<float *>(delta);
  const bool v4 = (g.f % 4 == 0) && aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(grad_out) &&
                  aligned16(dK) && aligned16(dV);
  return launch_gt_tbias_pass<2, false>(a, v4, s);
}

}  // namespace dfgnn
