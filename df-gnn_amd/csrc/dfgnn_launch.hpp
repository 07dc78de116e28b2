// dfgnn_launch.hpp -- host-side plumbing shared by the launcher translation units.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "dfgnn_device.hpp"

namespace dfgnn {

struct Csr {
  int m, nnz, h, f;  // m rows; the columns: n_cols below
  const int *row_ptr;
  const int *col_ind;
  const int *rows;   // sorted COO row ids (hyper / softmax formats), may be null for CSR-only ops
  const float *val;  // may be null (all ones)
  // matrix-core kernels only (set by their launchers from the plan): uint16 per edge, (row << 8 | column) within the
  // edge's dense range -- read instead of rows / col_ind
  const unsigned short *coords = nullptr;
  // edge bitmaps of the dense ranges (plan.hip: masks), 8 words per node: bit c of mask[8 i ..] = node i has an edge to
  // the node c places after the first node of its range; maskT likewise for the edges INTO node i.  Read by the
  // statistics-saving training pair (gt_dense_stats.hip), which needs to know where the edges are but not their order.
  const unsigned *mask = nullptr, *maskT = nullptr;
  // edge VALUES of the dense ranges in dense form (plan.hip: plan_dense_weights), kPlanWeightStride floats per node:
  // wdense[256 i + c] = val of the edge from node i to the node c places after the first node of its range.  Read by the
  // WEIGHTED instances of the statistics-saving pair (gt_dense_stats_w.hip) wherever the edge bitmap has a bit; null = unit values
  const float *wdense = nullptr;
  // columns (keys / values; col_ind < n_cols, col_ptr has n_cols + 1 entries) of the pairs that take a rectangular graph:
  // gt_train / gt_bias_train / gt_edge_train / gatv2_train.hip, whose C entries set it (the square ones to m).  Nothing
  // else reads it: every other kernel takes m for both sides
  int n_cols = 0;
};
constexpr int kPlanWeightStride = 256;

constexpr int kErrBadArg = -1;
constexpr int kErrUnsupported = -2;

// Rows handled by one workgroup of the hyper-format kernels, and the LDS budget (floats) for the
// workgroup's edge logits.  A workgroup whose rows hold more edges than kHyperCap does not use the
// LDS path: its waves run the online (tiled) row routine instead, so there is no degree limit
// (the reference hard-codes 128 neighbours/row and overflows).
constexpr int kHyperRows = 16;
constexpr int kHyperCap = 4096;
// per-wave scratch for the online routine: 64 weights + 64 column ids
constexpr int kScratchFloatsPerWave = 2 * kWave;

// ---- block plan (plan.hip) ---------------------------------------------------------------------
// One workgroup of kBlockThreads keeps a closed node range's feature rows resident in LDS.
constexpr int kBlockThreads = 1024;                      // 16 waves, 4 per SIMD
constexpr int kBlockWaves = kBlockThreads / kWave;
constexpr int kBlockScratchBytes = kBlockWaves * kWave * 8;  // per-wave (col, weight) staging, 512 B each
constexpr int kLdsBytes = 160 * 1024;
constexpr int kBlockLdsBudget = kLdsBytes - kBlockScratchBytes - 256;  // resident rows + edge values + 1/sum
constexpr int kBlockMinAvgDegree = 8;                    // below this average degree the general kernels win
constexpr int kBlockMergeNodes = 256;                    // small graphs are merged up to this many nodes

constexpr int kPlanHeader = 12;                          // int32 header words of a plan buffer
constexpr int kPlanEdgeGlobal = 1 << 30;                 // flag on a fit range's n1: per-edge array in global scratch
constexpr int kPlanDense = 1 << 29;                      // flag on a fit range's n1: qualifies for the matrix-core kernels
constexpr int kPlanRangeMask = ~(kPlanEdgeGlobal | kPlanDense);

constexpr int kPlanMaskWords = 8;                        // 32-bit words of a node's edge bitmap (dense ranges: < 256 nodes)
// int32 offset of the edge bitmaps in a plan buffer whose packed coordinates start at coords_off
inline size_t plan_mask_off(size_t coords_off, int nnz) { return (coords_off + ((size_t)nnz + 1) / 2 + 4 + 3) & ~(size_t)3; }
// int32 offset of the dense ranges' descriptors: right behind the fit and spill lists, 16-byte aligned (kPlanHeader is a
// multiple of 4) -- over the scratch of the build (pairs, bounds, count, rocPRIM storage: plan.hip), which is dead once
// plan_cut_kernel has sorted the fit list.  The buffer keeps its size and every other offset.
inline size_t plan_desc_off(int m) { return kPlanHeader + 4 * (size_t)m; }
// Descriptors that fit between there and the packed coordinates (>= (3 m + 68) / 4).  The merge of plan_cut_kernel never
// leaves two neighbouring groups that would still merge: two dense ranges in a row were kept apart by the 128-node limit
// or by the LDS budget (duplicate-free, so edges <= nodes^2) and hold dozens of nodes together, every other pair of
// neighbours has at most one dense range on two nodes or more -- num_dense <= (m + 1) / 2, i.e. 2 m + 2 words.
// dfgnn_plan_build checks it all the same (kErrUnsupported), and plan_coords_kernel writes no descriptor past it.
inline size_t plan_desc_capacity(int m, size_t coords_off) { return (coords_off - plan_desc_off(m)) / 4; }
// What a matrix-core kernel needs to know of its range before its first vector load, in one 16-byte scalar load: the
// fit entry (n0, n1 | flags) and e0 = row_ptr[n0], ne = row_ptr[n1] - e0.  Read through fit and row_ptr these are three
// dependent scalar round trips (kernel arguments, fit pair, two row_ptr words on lines nothing else in the launch touches);
// the plan knows all four when it is built.  desc[k] describes fit range k, k < num_dense.
struct alignas(16) PlanDesc {
  int n0, n1f, e0, ne;
};
struct Plan {              // host view of a built plan (see plan.hip for the device layout)
  const int *dev;          // device buffer, may be null (= no plan: general kernels only)
  int num_fit, num_spill, max_fit_nodes, max_fit_edges, m, nnz, f, num_edge_global;
  int num_dense;           // the first num_dense fit ranges carry kPlanDense (gt_dense.hip)
  int num_dense_wide = 0;  // ... and the first num_dense_wide of those have more than 128 nodes
  int coords_off = 0;      // int32 offset of the packed edge coordinates of the dense ranges (plan.hip)
  const unsigned short *coords() const { return reinterpret_cast<const unsigned short *>(dev + coords_off); }
  // the edge bitmaps behind the coordinates: mask[8 m], maskT[8 m] (see Csr)
  size_t mask_off() const { return plan_mask_off((size_t)coords_off, nnz); }
  const unsigned *mask() const { return reinterpret_cast<const unsigned *>(dev + mask_off()); }
  const unsigned *maskT() const { return mask() + 8 * (size_t)m; }
  // ... and behind the bitmaps the coordinates once more, in RANK order: position row_ptr[i] + k holds (row, column) of the
  // k-th edge of row i by increasing column -- the order the bitmap-driven forward writes attention values in
  // (gt_dense_fwd_ranked_kernel) and its backward therefore reads them in
  size_t ranked_off() const { return mask_off() + 2 * (size_t)kPlanMaskWords * (size_t)m; }
  const unsigned short *coords_ranked() const { return reinterpret_cast<const unsigned short *>(dev + ranked_off()); }
  // one descriptor per dense range, in the order of the fit list, behind the spill list: what the matrix-core kernels read
  // where the edge-walking kernels read fit()
  size_t desc_off() const { return plan_desc_off(m); }
  const PlanDesc *desc() const { return reinterpret_cast<const PlanDesc *>(dev + desc_off()); }
  const int *fit() const { return dev + kPlanHeader; }
  const int *spill() const { return dev + kPlanHeader + 2 * (size_t)m; }
};

inline bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Pick the lane layout for feature width f.  vec4 requires f % 4 == 0 and 16-byte aligned bases.
// fn is a generic lambda taking a FeatCfg value; returns its int result, or kErrUnsupported.
template <class F>
int dispatch_vec4(int f, F &&fn) {
  // Up to f = 256 a row is held by at most 16 lanes (one DPP row): the SDDMM reduction stays in
  // VALU-rate DPP ops and a wave touches >= 4 rows per gather instruction.
  if (f <= 16) return fn(FeatCfg<4, 4, 1>{});
  if (f <= 32) return fn(FeatCfg<8, 4, 1>{});
  if (f <= 64) return fn(FeatCfg<16, 4, 1>{});
  if (f <= 128) return fn(FeatCfg<16, 4, 2>{});
  if (f <= 256) return fn(FeatCfg<16, 4, 4>{});
  if (f <= 512) return fn(FeatCfg<32, 4, 4>{});
  if (f <= 1024) return fn(FeatCfg<64, 4, 4>{});
  return kErrUnsupported;
}

template <class F>
int dispatch_cfg(int f, bool vec4, F &&fn) {
  if (vec4) return dispatch_vec4(f, fn);
  if (f <= 8) return fn(FeatCfg<8, 1, 1>{});
  if (f <= 16) return fn(FeatCfg<16, 1, 1>{});
  if (f <= 32) return fn(FeatCfg<32, 1, 1>{});
  if (f <= 64) return fn(FeatCfg<64, 1, 1>{});
  if (f <= 128) return fn(FeatCfg<64, 1, 2>{});
  if (f <= 256) return fn(FeatCfg<64, 1, 4>{});
  return kErrUnsupported;
}

// The feature widths the matrix-core kernels are instantiated for.  fn is a generic lambda taking the width as a
// std::integral_constant; returns its int result, or kErrUnsupported.
template <class Fn>
int dispatch_dense(int f, Fn &&fn) {
  if (f == 8) return fn(std::integral_constant<int, 8>{});    // f = 8 / 16: zero-padded onto the 32-wide layout
  if (f == 16) return fn(std::integral_constant<int, 16>{});
  if (f == 32) return fn(std::integral_constant<int, 32>{});
  if (f == 64) return fn(std::integral_constant<int, 64>{});
  if (f == 128) return fn(std::integral_constant<int, 128>{});
  return kErrUnsupported;
}

inline int launch_status() { return static_cast<int>(hipGetLastError()); }
// hipFuncSetAttribute(fn, MaxDynamicSharedMemorySize, 160 KB), issued once per (device, kernel) and remembered (capi.hip)
int set_max_lds_cached_ptr(const void *fn);

// ---- launchers implemented in the kernel translation units -----------------------------------
int launch_gt_hyper_fwd(const Csr &g, const float *Q, const float *K, const float *V, float *attn_edge,
                        float *out, const int *chunks, int nchunks, hipStream_t s);
bool block_width_ok(int f);
int launch_gt_block_fwd(const Csr &g, const Plan &p, const float *Q, const float *K, const float *V,
                        float *attn_edge, float *edge_ws, float *out, hipStream_t s);
// matrix-core kernels over the first p.num_dense fit ranges (GT: unit edge values only); DFGNN_DENSE=0 in the
// environment (diagnostic switch, read once) keeps every range on the edge-walking kernels
bool dense_enabled();
// this batch takes the 256-thread forward, two workgroups per CU (dfgnn_dense_lean.hpp): one head of 64 or 128 features and
// no range of more than 128 nodes; DFGNN_LEAN=0 in the environment (diagnostic switch, read once) keeps every dense range
// on the 512-thread forward
bool dense_lean_batch(const Csr &g, const Plan &p);
int launch_gt_dense_fwd(const Csr &g, const Plan &p, const float *Q, const float *K, const float *V,
                        float *attn_edge, float *out, hipStream_t s);
int launch_gt_dense_bwd(const Csr &g, const Plan &p, const float *Q, const float *K, const float *V,
                        const float *attn_edge, const float *grad_out, float *dQ, float *dK, float *dV,
                        hipStream_t s, bool ranked = false);
// ranges a backward keeps in plan position (the largest); it takes the others in reverse plan order (gt_dense.hip says why)
int bwd_reverse_keep(int num_dense);
// the statistics-saving training pair (gt_dense_stats.hip): no attn_edge, row statistics [m, h] instead
int launch_gt_dense_fwd_stats(const Csr &g, const Plan &p, const float *Q, const float *K, const float *V, float *out,
                              float *stat_max, float *stat_sum, hipStream_t s);
int launch_gt_dense_bwd_stats(const Csr &g, const Plan &p, const float *Q, const float *K, const float *V,
                              const float *stat_max, const float *stat_sum, const float *grad_out, float *dQ, float *dK,
                              float *dV, hipStream_t s);
// ... with edge values (gt_dense_stats_w.hip): g.wdense = the plan's dense weights (dfgnn_plan_dense_weights); the two
// launchers above hand over to these when g.wdense is set.  stat_max / stat_sum of the forward may be null (inference).
int launch_gt_dense_fwd_stats_w(const Csr &g, const Plan &p, const float *Q, const float *K, const float *V, float *out,
                                float *stat_max, float *stat_sum, hipStream_t s);
int launch_gt_dense_bwd_stats_w(const Csr &g, const Plan &p, const float *Q, const float *K, const float *V,
                                const float *stat_max, const float *stat_sum, const float *grad_out, float *dQ, float *dK,
                                float *dV, hipStream_t s);
// the attn_edge pair with the values in RANK order (gt_dense_stats_w.hip; one head): the forward is bitmap-driven, the
// backward is launch_gt_dense_bwd with ranked = true (the plan's rank-ordered coordinates)
int launch_gt_dense_fwd_ranked(const Csr &g, const Plan &p, const float *Q, const float *K, const float *V,
                               float *attn_ranked, float *out, hipStream_t s);
// edge_max / edge_sum (nullable): row statistics for the GAT training pair
int launch_gat_dense_fwd(const Csr &g, const Plan &p, const float *attn_row, const float *attn_col, float slope,
                         const float *X, float *out, hipStream_t s, float *edge_max = nullptr,
                         float *edge_sum = nullptr, const float *edge_mask = nullptr, float attn_drop = 0.f);
int launch_gat_dense_bwd(const Csr &g, const Plan &p, const float *attn_row, const float *attn_col, float slope,
                         const float *X, const float *edge_max, const float *edge_sum, const float *grad_out,
                         float *grad_feat, float *grad_row, float *grad_col, hipStream_t s,
                         const float *edge_mask = nullptr, float attn_drop = 0.f);
int launch_gt_tiling_fwd(const Csr &g, const float *Q, const float *K, const float *V, float *out,
                         hipStream_t s);
int launch_gt_sddmm(const Csr &g, const float *Q, const float *K, float *logits, hipStream_t s);
// node-parallel CSR baselines (csr_fwd.hip): 'csr' (row logits in LDS) / 'csr_gm' (in global memory), GAT 'hyper_recompute'
int launch_gt_csr_fwd(const Csr &g, const float *Q, const float *K, const float *V, float *logits, float *out,
                      bool use_lds, hipStream_t s);
int launch_gat_recompute_fwd(const Csr &g, const float *attn_row, const float *attn_col, float slope, const float *X,
                             float *out, hipStream_t s);
int launch_softmax_spmm(const Csr &g, const float *logits, const float *X, float *out, bool use_lds,
                        hipStream_t s);
int launch_gt_bwd_rows(const Csr &g, const float *K, const float *V, const float *attn_edge,
                       const float *grad_out, float *grad_edge, float *dQ, const int *chunks, int nchunks,
                       hipStream_t s);
int launch_gt_bwd_cols(const Csr &g, const int *col_ptr, const int *row_ind, const int *val_idx, const float *Q,
                       const float *attn_edge, const float *grad_edge, const float *grad_out, float *dK,
                       float *dV, const int *chunks, int nchunks, hipStream_t s);
int launch_gt_block_bwd(const Csr &g, const Plan &p, const int *col_ptr, const int *row_ind, const int *val_idx,
                        const float *Q, const float *K, const float *V, const float *attn_edge,
                        const float *grad_out, float *edge_ws, float *dQ, float *dK, float *dV, hipStream_t s);
int launch_gt_lowdeg_fwd(const Csr &g, const float *Q, const float *K, const float *V, float *attn_edge, float *out,
                         hipStream_t s);
int launch_gt_lowdeg_bwd(const Csr &g, const int *col_ptr, const int *row_ind, const int *val_idx, const float *Q,
                         const float *K, const float *V, const float *attn_edge, const float *grad_out,
                         float *grad_edge, float *dQ, float *dK, float *dV, hipStream_t s);
// GT training pair without per-edge saved state (gt_train.hip): any graph, no plan.  The forward saves row_max / row_sum
// [m, h] (both nullable: inference); the backward is the CSR pass (delta [m, h] = <dO_i, out_i>, dQ) then the CSC pass
// (dK, dV), each recomputing the attention of the edges it walks.
int launch_gt_train_fwd(const Csr &g, const float *Q, const float *K, const float *V, float *row_max, float *row_sum,
                        float *out, hipStream_t s);
int launch_gt_train_bwd_rows(const Csr &g, const float *Q, const float *K, const float *V, const float *out,
                             const float *row_max, const float *row_sum, const float *grad_out, float *delta, float *dQ,
                             hipStream_t s);
int launch_gt_train_bwd_cols(const Csr &g, const int *col_ptr, const int *row_ind, const int *val_idx, const float *Q,
                             const float *K, const float *V, const float *row_max, const float *row_sum,
                             const float *delta, const float *grad_out, float *dK, float *dV, hipStream_t s);
// GT pair with a per-edge additive attention bias (gt_bias_train.hip): launch_gt_train_* with bias [h, nnz] (CSR order) added
// to every logit; -inf masks an edge.  The CSR pass also writes dbias [h, nnz] = dS in full when it is not null; the CSC
// pass gathers the bias through val_idx, which it therefore always reads.
int launch_gt_bias_fwd(const Csr &g, const float *bias, const float *Q, const float *K, const float *V, float *row_max,
                       float *row_sum, float *out, hipStream_t s);
int launch_gt_bias_bwd_rows(const Csr &g, const float *bias, const float *Q, const float *K, const float *V,
                            const float *out, const float *row_max, const float *row_sum, const float *grad_out,
                            float *delta, float *dQ, float *dbias, hipStream_t s);
int launch_gt_bias_bwd_cols(const Csr &g, const float *bias, const int *col_ptr, const int *row_ind, const int *val_idx,
                            const float *Q, const float *K, const float *V, const float *row_max, const float *row_sum,
                            const float *delta, const float *grad_out, float *dK, float *dV, hipStream_t s);
// GT pair with a per-edge feature vector added to keys and values (gt_edge_train.hip): launch_gt_train_* with E [nnz, h, f]
// (CSR order), k~_e = K_j + E_e, v~_e = V_j + E_e.  The CSR pass also writes dE [nnz, h, f] in full when it is not null; the
// CSC pass gathers E rows through val_idx, which it therefore always reads.
int launch_gt_edge_fwd(const Csr &g, const float *E, const float *Q, const float *K, const float *V, float *row_max,
                       float *row_sum, float *out, hipStream_t s);
int launch_gt_edge_bwd_rows(const Csr &g, const float *E, const float *Q, const float *K, const float *V,
                            const float *out, const float *row_max, const float *row_sum, const float *grad_out,
                            float *delta, float *dQ, float *dE, hipStream_t s);
int launch_gt_edge_bwd_cols(const Csr &g, const float *E, const int *col_ptr, const int *row_ind, const int *val_idx,
                            const float *Q, const float *K, const float *V, const float *row_max, const float *row_sum,
                            const float *delta, const float *grad_out, float *dK, float *dV, hipStream_t s);
// GT pair with a per-edge multiplicative gate on the keys and an edge-output channel (gt_gate_train.hip): launch_gt_train_*
// with E [nnz, h, f] (CSR order), ke_e = K_j (.) E_e, s_e = val_e <Q_i, ke_e>.  The forward also writes W [nnz, h, f] =
// val_e Q_i (.) ke_e when it is not null; both backward passes add G [nnz, h, f] = d loss / d W to dS per dimension when it
// is not null (the CSC pass through val_idx, which it always reads); the CSR pass writes dE in full when it is not null.
int launch_gt_gate_fwd(const Csr &g, const float *E, const float *Q, const float *K, const float *V, float *row_max,
                       float *row_sum, float *out, float *W, hipStream_t s);
int launch_gt_gate_bwd_rows(const Csr &g, const float *E, const float *Q, const float *K, const float *V,
                            const float *out, const float *row_max, const float *row_sum, const float *grad_out,
                            const float *G, float *delta, float *dQ, float *dE, hipStream_t s);
int launch_gt_gate_bwd_cols(const Csr &g, const float *E, const int *col_ptr, const int *row_ind, const int *val_idx,
                            const float *Q, const float *K, const float *V, const float *row_max, const float *row_sum,
                            const float *delta, const float *grad_out, const float *G, float *dK, float *dV,
                            hipStream_t s);
// GT pair with typed edges (gt_typed_train.hip): launch_gt_edge_* with E_e = R[etype[e]], R [T, h, f], and never anything of
// size nnz h f.  The CSC pass streams etype_csc (the types in CSC entry order) and reads val_idx only for edge values.  The
// CSR pass with dR != NULL runs at most kGtTypedParts persistent workgroups per head, each storing one partial [T, h-slice,
// f] to ws, and then reduces them into dR in a fixed order; it needs T f <= kGtTypedMaxTableFloats (a table per wave in
// LDS) and answers kErrUnsupported beyond.  dR == NULL: the plain pass, any T, ws unused.
constexpr int kGtTypedParts = 1024;            // per head (the grid is (parts, h)): 4 workgroups per CU on 256 CUs; LDS admits 5 at T f = 2048
constexpr int kGtTypedMaxTableFloats = 8192;   // 4 waves x 32 KB = 128 KB of the CU's 160 KB
struct GtTypedTable {
  int T;
  const int *etype, *etype_csc;  // [nnz] CSR order / CSC entry order
  const float *R;                // [T, h, f]
};
bool gt_typed_table_fits(int T, int f);
int launch_gt_typed_fwd(const Csr &g, const GtTypedTable &t, const float *Q, const float *K, const float *V,
                        float *row_max, float *row_sum, float *out, hipStream_t s);
int launch_gt_typed_bwd_rows(const Csr &g, const GtTypedTable &t, const float *Q, const float *K, const float *V,
                             const float *out, const float *row_max, const float *row_sum, const float *grad_out,
                             float *delta, float *dQ, float *ws, float *dR, hipStream_t s);
int launch_gt_typed_bwd_cols(const Csr &g, const GtTypedTable &t, const int *col_ptr, const int *row_ind,
                             const int *val_idx, const float *Q, const float *K, const float *V, const float *row_max,
                             const float *row_sum, const float *delta, const float *grad_out, float *dK, float *dV,
                             hipStream_t s);
// GT pair with a typed attention bias (gt_tbias_train.hip): launch_gt_bias_* with bias[hd, e] = B[etype[e], hd], B [T, h],
// and never anything of size h nnz.  The CSC pass streams etype_csc (the types in CSC entry order) and reads val_idx only
// for edge values.  The CSR pass with dB != NULL runs at most gt_tbias_parts(T) persistent workgroups per head, each
// storing one partial [T, h-slice] to ws, and then reduces them into dB in a fixed order; it needs T <= kGtTBiasMaxTypes
// (a table per wave in LDS) and answers kErrUnsupported beyond.  dB == NULL: the plain pass, any T, ws unused.
constexpr int kGtTBiasParts = 1024;      // per head (the grid is (parts, h)): 4 workgroups per CU on 256 CUs
constexpr int kGtTBiasMaxTypes = 4096;   // 4 waves x 16 KB = 64 KB, the default limit of dynamic LDS: no attribute call
struct GtTBiasTable {
  int T;
  const int *etype, *etype_csc;  // [nnz] CSR order / CSC entry order
  const float *B;                // [T, h]
};
int gt_tbias_parts(int T);  // partials per head that ws holds: min(kGtTBiasParts, 256 x the workgroups a CU's LDS admits)
int launch_gt_tbias_fwd(const Csr &g, const GtTBiasTable &t, const float *Q, const float *K, const float *V,
                        float *row_max, float *row_sum, float *out, hipStream_t s);
int launch_gt_tbias_bwd_rows(const Csr &g, const GtTBiasTable &t, const float *Q, const float *K, const float *V,
                             const float *out, const float *row_max, const float *row_sum, const float *grad_out,
                             float *delta, float *dQ, float *ws, float *dB, hipStream_t s);
int launch_gt_tbias_bwd_cols(const Csr &g, const GtTBiasTable &t, const int *col_ptr, const int *row_ind,
                             const int *val_idx, const float *Q, const float *K, const float *V, const float *row_max,
                             const float *row_sum, const float *delta, const float *grad_out, float *dK, float *dV,
                             hipStream_t s);
// GATv2 pair (gatv2_train.hip): any graph, no plan.  The forward saves row_max / row_sum [m, h] (both nullable: inference);
// the backward is the CSR pass (delta, dX_row and at most kGatv2Parts partial sums [h, f] of dattn -> ws), the CSC pass
// (dX_col) and the reduction of the partials into dattn, on one stream.
constexpr int kGatv2Parts = 2048;  // persistent workgroups of the CSR pass per head = partial sums of dattn
struct Gatv2Graph {
  const int *col_ptr, *row_ind;  // CSC (backward only)
  const float *attn;             // [h, f]
  float slope;
};
int launch_gatv2_fwd(const Csr &g, const Gatv2Graph &v, const float *X_row, const float *X_col, float *row_max,
                     float *row_sum, float *out, hipStream_t s);
int launch_gatv2_bwd(const Csr &g, const Gatv2Graph &v, const float *X_row, const float *X_col, const float *out,
                     const float *row_max, const float *row_sum, const float *grad_out, float *delta, float *ws,
                     float *dX_row, float *dX_col, float *dattn, hipStream_t s);
// GATv2 pair with a per-edge feature vector inside the LeakyReLU (gatv2_edge_train.hip): launch_gatv2_* with E [nnz, h, f]
// (CSR order), z_e = X_row_i + X_col_j + E_e.  The CSR pass also writes dE [nnz, h, f] in full when it is not null; the CSC
// pass gathers E rows through val_idx, which it therefore always reads.  `ws` as for launch_gatv2_bwd.
int launch_gatv2_edge_fwd(const Csr &g, const Gatv2Graph &v, const float *X_row, const float *X_col, const float *E,
                          float *row_max, float *row_sum, float *out, hipStream_t s);
int launch_gatv2_edge_bwd(const Csr &g, const Gatv2Graph &v, const int *val_idx, const float *X_row, const float *X_col,
                          const float *E, const float *out, const float *row_max, const float *row_sum,
                          const float *grad_out, float *delta, float *ws, float *dX_row, float *dX_col, float *dattn,
                          float *dE, hipStream_t s);
// AGNN / dot-product pair with tied keys and values (agnn_train.hip): any graph, no plan.  s_e = beta[h] r_i q_j <X_row_i,
// X_col_j> with r, q the inverse row norms (cosine) or 1; X_col_j is key and value, gathered once per edge.  The forward
// saves row_max / row_sum [m, h] (both nullable: inference); the backward is the CSR pass (delta, dX_row and, when it is not
// null, dbeta_rows [m, h]) then the CSC pass (dX_col), on one stream.  No workspace.
struct AgnnGraph {
  const int *col_ptr, *row_ind;  // CSC (backward only)
  const float *beta;             // [h]
  bool cosine;
};
int launch_agnn_fwd(const Csr &g, const AgnnGraph &v, const float *X_row, const float *X_col, float *row_max,
                    float *row_sum, float *out, hipStream_t s);
int launch_agnn_bwd(const Csr &g, const AgnnGraph &v, const float *X_row, const float *X_col, const float *out,
                    const float *row_max, const float *row_sum, const float *grad_out, float *delta, float *dX_row,
                    float *dX_col, float *dbeta_rows, hipStream_t s);
// GatedGCN pair (gatedgcn_train.hip): any graph, no plan.  z_e = (X_row_i + X_col_j) + E_e, sg_e = sigmoid(z_e) per
// dimension, out_i = sum sg_e (.) V_j [/ (den_i + eps)].  The forward writes den [m, h, f] (nullable: inference) and Z =
// z [nnz, h, f] (nullable); the backward is the CSR pass (dX_row, dE, and with normalize s_i = dO_i / (den_i + eps) -> ws
// [m, h, f]) then the CSC pass (dX_col, dV), on one stream.  E, G, Z, dE nullable; out, den, ws unused without normalize.
struct GatedGcnGraph {
  const int *col_ptr, *row_ind, *val_idx;  // CSC (backward only)
  bool normalize;
  float eps;
};
int launch_gatedgcn_fwd(const Csr &g, const GatedGcnGraph &v, const float *X_row, const float *X_col, const float *V,
                        const float *E, float *den, float *out, float *Z, hipStream_t s);
int launch_gatedgcn_bwd(const Csr &g, const GatedGcnGraph &v, const float *X_row, const float *X_col, const float *V,
                        const float *E, const float *out, const float *den, const float *grad_out, const float *G,
                        float *dX_row, float *dX_col, float *dV, float *dE, float *ws, hipStream_t s);
// GAT pair for any graph with an optional per-edge attention term (gat_edge_train.hip): no plan.  pre_e = (attn_row_i +
// attn_col_j) + score[h, e], score [h, nnz] in CSR order (nullable: + 0.f); mask [nnz, h] uniform randoms (nullable: no
// dropout).  The forward saves edge_max / edge_sum [m, h] (both nullable: inference); the backward is the CSR pass (delta
// [m, h] summed over the edges -- the forward's out is not read --, grad_attn_row and, when it is not null, grad_score [h, nnz] in full) then the CSC pass (grad_feat, grad_attn_col),
// on one stream.  The CSC pass reads val_idx only when score or mask is given.  Nothing of size nnz is handed over.
struct GatEdgeTerms {
  const float *attn_row, *attn_col;  // [m, h] / [n_cols, h]
  float slope;
  const float *score;                // [h, nnz]
  const float *mask;                 // [nnz, h]
  float attn_drop;
};
int launch_gat_edge_fwd(const Csr &g, const GatEdgeTerms &t, const float *X, float *edge_max, float *edge_sum, float *out,
                        hipStream_t s);
int launch_gat_edge_bwd(const Csr &g, const GatEdgeTerms &t, const int *col_ptr, const int *row_ind, const int *val_idx,
                        const float *X, const float *edge_max, const float *edge_sum, const float *grad_out, float *delta,
                        float *grad_feat, float *grad_attn_row, float *grad_attn_col,
                        float *grad_score, hipStream_t s);
// graphs with fewer than kBlockMinAvgDegree edges per row on average take the row-per-lane-group kernels.  The pairs that
// take an m x n_cols graph ask per pass: (m, nnz) for the forward and the CSR pass, (n_cols, nnz) for the CSC pass
inline bool low_degree(int m, int nnz) { return (long)nnz < (long)kBlockMinAvgDegree * m; }
int launch_gat_hyper_fwd(const Csr &g, const float *attn_row, const float *attn_col, float slope,
                         const float *X, float *out, const int *chunks, int nchunks, hipStream_t s);
int launch_gat_block_fwd(const Csr &g, const Plan &p, const float *attn_row, const float *attn_col, float slope,
                         const float *X, float *edge_ws, float *out, hipStream_t s);
int launch_gat_tiling_fwd(const Csr &g, const float *attn_row, const float *attn_col, float slope,
                          const float *X, float *out, hipStream_t s);
int launch_gat_sddmm(const Csr &g, const float *attn_row, const float *attn_col, float slope, float *logits,
                     hipStream_t s);

// the CSC half of the preprocessing on its own (preprocess.hip), for a caller that already holds the CSR list (sample.hip):
// col_ptr [n_cols + 1], row_ind, val_idx [nnz] = a stable sort of the CSR list by column.  temp: rocPRIM storage of
// csc_sort_temp_bytes(n_cols, nnz) bytes or more; sorted_cols: int[nnz] of scratch.  nnz > 0
int csc_sort_temp_bytes(int n_cols, int nnz, size_t &bytes);
int launch_csc_of_csr(int n_cols, int nnz, const int *col_ind, const int *rows, int *col_ptr, int *row_ind, int *val_idx,
                      void *temp, size_t temp_bytes, int *sorted_cols, hipStream_t s);

int launch_gat_attn_scores(int m, int h, int f, const float *a_l, const float *a_r, const float *X, float *attn_row,
                           float *attn_col, hipStream_t s);
// GAT training pair (gat_train.hip).  rest != NULL: only the ranges of that plan which the matrix-core kernels do not
// serve (its non-dense fit ranges and its spill chunks); NULL: the whole graph.
int launch_gat_train_fwd(const Csr &g, const float *attn_row, const float *attn_col, float slope, const float *X,
                         const float *edge_mask, float attn_drop, float *edge_max, float *edge_sum, float *out,
                         hipStream_t s, const Plan *rest = nullptr);
int launch_gat_bwd_rows(const Csr &g, const float *attn_row, const float *attn_col, float slope, const float *X,
                        const float *edge_max, const float *edge_sum, const float *edge_mask, float attn_drop,
                        const float *grad_out, float *grad_edge, float *grad_row, hipStream_t s,
                        const Plan *rest = nullptr);
int launch_gat_bwd_cols(const Csr &g, const int *col_ptr, const int *row_ind, const int *permute,
                        const float *attn_row, const float *attn_col, float slope, const float *edge_max,
                        const float *edge_sum, const float *edge_mask, float attn_drop, const float *grad_edge,
                        const float *grad_out, float *grad_feat, float *grad_col, hipStream_t s,
                        const Plan *rest = nullptr);

}  // namespace dfgnn
