// capi.hip -- the extern "C" boundary of libdfgnn.so (declared in include/dfgnn.h).
// Argument validation + dispatch only; no allocation, no synchronisation.
#include "../../include/dfgnn.h"
#include "dfgnn_launch.hpp"
#include "dfgnn_errstr.h"

#include <mutex>
#include <set>
#include <utility>

using namespace dfgnn;

namespace dfgnn {
int set_max_lds_cached_ptr(const void *fn) {
  static std::mutex mu;
  static std::set<std::pair<int, const void *>> done;
  int dev = 0;
  if (hipError_t rc = hipGetDevice(&dev)) return (int)rc;
  std::lock_guard<std::mutex> lock(mu);
  if (done.count({dev, fn})) return 0;
  if (hipError_t rc = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsBytes)) return (int)rc;
  done.insert({dev, fn});
  return 0;
}
}  // namespace dfgnn

namespace {
inline hipStream_t as_stream(dfgnn_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// A plan is used only if it was built for exactly this (m, nnz, f) and LDS budget; otherwise the call
// silently takes the general kernels (same results, no LDS residency).
// The plan kernels (LDS-resident and matrix-core) address a feature row with 32-bit byte offsets; the general kernels
// use size_t throughout.  Feature matrices of 4 GiB or more therefore take the general kernels.
inline bool plan_offsets_fit(int m, int h, int f) { return (size_t)m * (size_t)h * (size_t)f * 4u < (1ull << 32); }

inline bool make_plan(Plan &p, const int *plan_dev, const int *meta, int m, int nnz, int h, int f) {
  p = Plan{nullptr, 0, 0, 0, 0, m, nnz, f, 0, 0};
  if (!plan_dev || !meta) return false;
  if (!plan_offsets_fit(m, h, f)) return false;
  if (meta[4] != m || meta[5] != nnz || meta[6] != f || meta[7] != kBlockLdsBudget) return false;
  if (meta[0] <= 0) return false;
  // Low-degree batches (e.g. molecule / peptide graphs, ~2 edges per row) are bound by the node features, not
  // by the per-edge gathers: a 1024-thread workgroup per range only adds fixed cost there (measured on the
  // Peptides-like config: 279 us resident vs 180 us general for fwd+bwd), so such graphs keep the general kernels.
  if ((long)nnz < (long)kBlockMinAvgDegree * m) return false;
  p = Plan{plan_dev, meta[0], meta[1], meta[2], meta[3], m, nnz, f, meta[8], meta[9], meta[10], meta[11]};
  if (p.num_dense > 0 && p.coords_off <= 0) return false;  // (a plan of an older layout)
  return true;
}

// A built plan is usable for width f when the LDS-resident kernels have an exact lane layout for f, or -- f = 8, which
// has none -- when every fit range goes to the matrix-core kernels anyway (unit edge values, COO rows, not disabled).
inline bool plan_usable(const Plan &p, int f, bool unit_val, const int *rows) {
  if (block_width_ok(f)) return true;
  return f == 8 && unit_val && rows && dense_enabled() && p.num_dense == p.num_fit;
}

// Returns <0 on a bad argument, 1 when there is nothing to do, 0 to proceed.
inline int check_common(int m, int nnz, int h, int f, const void *row_ptr, const void *col_ind) {
  if (m < 0 || nnz < 0 || h < 0 || f < 0) return kErrBadArg;
  if (m == 0 || h == 0 || f == 0) return 1;
  if (!row_ptr) return kErrBadArg;
  if (nnz > 0 && !col_ind) return kErrBadArg;
  if (h > 65535) return kErrUnsupported;
  return 0;
}

// check_common for an m x n_cols graph.  Nothing to do at all: no heads, no features, or neither rows nor columns.
inline int check_rect(int m, int n_cols, int nnz, int h, int f, const void *row_ptr, const void *col_ind) {
  if (m < 0 || n_cols < 0 || nnz < 0 || h < 0 || f < 0) return kErrBadArg;
  if ((m == 0 && n_cols == 0) || h == 0 || f == 0) return 1;
  if (nnz > 0 && (m == 0 || n_cols == 0)) return kErrBadArg;  // (an edge needs a row and a column)
  if (m > 0 && !row_ptr) return kErrBadArg;
  if (nnz > 0 && !col_ind) return kErrBadArg;
  if (h > 65535) return kErrUnsupported;
  return 0;
}
inline Csr rect_csr(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val) {
  Csr g{m, nnz, h, f, row_ptr, col_ind, nullptr, val};
  g.n_cols = n_cols;
  return g;
}
}  // namespace

extern "C" {

int dfgnn_abi_version(void) { return DFGNN_ABI_VERSION; }

int dfgnn_plan_applies(int m, int nnz, int h, int f, const int *plan_meta) {
  Plan p;
  static const int token = 0;  // (make_plan only stores the device pointer)
  return make_plan(p, &token, plan_meta, m, nnz, h, f) ? 1 : 0;
}

#ifndef DFGNN_SRC_HASH
#define DFGNN_SRC_HASH "unknown"
#endif
const char *dfgnn_build_id(void) { return DFGNN_SRC_HASH; }

const char *dfgnn_error_string(int code) {
  if (const char *text = dfgnn_static_error_string(code)) return text;
  return hipGetErrorString(static_cast<hipError_t>(code));
}

int dfgnn_gt_hyper_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const int *rows,
                       const float *val, const float *Q, const float *K, const float *V, float *attn_edge,
                       float *edge_ws, float *out, const int *plan, const int *plan_meta,
                       dfgnn_stream_t stream) {
  if (int c = check_common(m, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (!Q || !K || !V || !out || (nnz > 0 && !rows)) return kErrBadArg;
  const Csr g{m, nnz, h, f, row_ptr, col_ind, rows, val};
  Plan p;
  const bool v4 = (f % 4 == 0) && aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(out);
  if (v4 && make_plan(p, plan, plan_meta, m, nnz, h, f) && plan_usable(p, f, !val, rows)) {
    if (int rc = launch_gt_block_fwd(g, p, Q, K, V, attn_edge, edge_ws, out, as_stream(stream))) return rc;
    return launch_gt_hyper_fwd(g, Q, K, V, attn_edge, out, p.spill(), p.num_spill, as_stream(stream));
  }
  if (low_degree(m, nnz)) return launch_gt_lowdeg_fwd(g, Q, K, V, attn_edge, out, as_stream(stream));
  return launch_gt_hyper_fwd(g, Q, K, V, attn_edge, out, nullptr, 0, as_stream(stream));
}

int dfgnn_gt_bwd_rows(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const int *rows,
                      const float *val, const float *K, const float *V, const float *attn_edge,
                      const float *grad_out, float *grad_edge, float *dQ, dfgnn_stream_t stream) {
  if (int c = check_common(m, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (!K || !V || !grad_out || !dQ) return kErrBadArg;
  if (nnz > 0 && (!rows || !attn_edge || !grad_edge)) return kErrBadArg;
  const Csr g{m, nnz, h, f, row_ptr, col_ind, rows, val};
  return launch_gt_bwd_rows(g, K, V, attn_edge, grad_out, grad_edge, dQ, nullptr, 0, as_stream(stream));
}

int dfgnn_gt_bwd_cols(int m, int nnz, int h, int f, const float *val, const int *col_ptr, const int *row_ind,
                      const int *val_idx, const float *Q, const float *attn_edge, const float *grad_edge,
                      const float *grad_out, float *dK, float *dV, dfgnn_stream_t stream) {
  if (m < 0 || nnz < 0 || h < 0 || f < 0) return kErrBadArg;
  if (m == 0 || h == 0 || f == 0) return 0;
  if (h > 65535) return kErrUnsupported;
  if (!col_ptr || !Q || !grad_out || !dK || !dV) return kErrBadArg;
  if (nnz > 0 && (!row_ind || !val_idx || !attn_edge || !grad_edge)) return kErrBadArg;
  const Csr g{m, nnz, h, f, nullptr, nullptr, nullptr, val};
  return launch_gt_bwd_cols(g, col_ptr, row_ind, val_idx, Q, attn_edge, grad_edge, grad_out, dK, dV, nullptr, 0,
                            as_stream(stream));
}

int dfgnn_gt_bwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const int *rows,
                 const float *val, const int *col_ptr, const int *row_ind, const int *val_idx, const float *Q,
                 const float *K, const float *V, const float *attn_edge, const float *grad_out,
                 float *grad_edge, float *dQ, float *dK, float *dV, const int *plan, const int *plan_meta,
                 dfgnn_stream_t stream) {
  if (int c = check_common(m, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (!Q || !K || !V || !grad_out || !dQ || !dK || !dV || !col_ptr) return kErrBadArg;
  if (nnz > 0 && (!rows || !row_ind || !val_idx || !attn_edge || !grad_edge)) return kErrBadArg;
  const Csr g{m, nnz, h, f, row_ptr, col_ind, rows, val};
  Plan p;
  const bool v4 = (f % 4 == 0) && aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(grad_out) &&
                  aligned16(dQ) && aligned16(dK) && aligned16(dV);
  const int *chunks = nullptr;
  int nchunks = 0;
  if (v4 && make_plan(p, plan, plan_meta, m, nnz, h, f) && plan_usable(p, f, !val, rows)) {
    if (int rc = launch_gt_block_bwd(g, p, col_ptr, row_ind, val_idx, Q, K, V, attn_edge, grad_out, grad_edge, dQ,
                                     dK, dV, as_stream(stream)))
      return rc;
    if (p.num_spill == 0) return 0;
    chunks = p.spill();
    nchunks = p.num_spill;
  }
  if (!chunks && low_degree(m, nnz))
    return launch_gt_lowdeg_bwd(g, col_ptr, row_ind, val_idx, Q, K, V, attn_edge, grad_out, grad_edge, dQ, dK, dV,
                                as_stream(stream));
  if (int rc = launch_gt_bwd_rows(g, K, V, attn_edge, grad_out, grad_edge, dQ, chunks, nchunks, as_stream(stream)))
    return rc;
  return launch_gt_bwd_cols(g, col_ptr, row_ind, val_idx, Q, attn_edge, grad_edge, grad_out, dK, dV, chunks,
                            nchunks, as_stream(stream));
}

// ---- the statistics-saving training pair (gt_dense_stats.hip) -----------------------------------------------------------
// usable when every range of the plan is served by the matrix-core kernels (unit edge values are the caller's promise)
static bool gt_stats_plan(Plan &p, const int *plan, const int *plan_meta, int m, int nnz, int h, int f) {
  if (!dense_enabled()) return false;
  if (f != 8 && f != 16 && f != 32 && f != 64 && f != 128) return false;
  if (!make_plan(p, plan, plan_meta, m, nnz, h, f)) return false;
  return p.num_dense > 0 && p.num_dense == p.num_fit && p.num_spill == 0;
}

int dfgnn_gt_stats_applies(int m, int nnz, int h, int f, const int *plan_meta) {
  Plan p;
  static const int token = 0;
  return gt_stats_plan(p, &token, plan_meta, m, nnz, h, f) ? 1 : 0;
}

int dfgnn_gt_hyper_fwd_stats(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *weights,
                             const float *Q, const float *K, const float *V, float *row_max, float *row_sum, float *out,
                             const int *plan, const int *plan_meta, dfgnn_stream_t stream) {
  if (int c = check_common(m, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (!Q || !K || !V || !out || (!row_max != !row_sum)) return kErrBadArg;  // (both statistics or neither: inference)
  Plan p;
  if (!(aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(out)) || !gt_stats_plan(p, plan, plan_meta, m, nnz, h, f))
    return kErrUnsupported;
  if (weights && !aligned16(weights)) return kErrUnsupported;
  Csr g{m, nnz, h, f, row_ptr, col_ind, nullptr, nullptr};
  g.wdense = weights;
  return launch_gt_dense_fwd_stats(g, p, Q, K, V, out, row_max, row_sum, as_stream(stream));
}

int dfgnn_gt_bwd_stats(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *weights,
                       const float *Q, const float *K, const float *V, const float *row_max, const float *row_sum,
                       const float *grad_out, float *dQ, float *dK, float *dV, const int *plan, const int *plan_meta,
                       dfgnn_stream_t stream) {
  if (int c = check_common(m, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (!Q || !K || !V || !row_max || !row_sum || !grad_out || !dQ || !dK || !dV) return kErrBadArg;
  Plan p;
  if (!(aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(grad_out) && aligned16(dQ) && aligned16(dK) && aligned16(dV)) ||
      !gt_stats_plan(p, plan, plan_meta, m, nnz, h, f))
    return kErrUnsupported;
  if (weights && !aligned16(weights)) return kErrUnsupported;
  Csr g{m, nnz, h, f, row_ptr, col_ind, nullptr, nullptr};
  g.wdense = weights;
  return launch_gt_dense_bwd_stats(g, p, Q, K, V, row_max, row_sum, grad_out, dQ, dK, dV, as_stream(stream));
}

// the attn_edge pair in rank order (all-dense plan, unit edge values)
int dfgnn_gt_hyper_fwd_ranked(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *Q,
                              const float *K, const float *V, float *attn_ranked, float *out, const int *plan,
                              const int *plan_meta, dfgnn_stream_t stream) {
  if (int c = check_common(m, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (!Q || !K || !V || !out || !attn_ranked) return kErrBadArg;
  Plan p;
  if (!(aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(out)) || !gt_stats_plan(p, plan, plan_meta, m, nnz, h, f))
    return kErrUnsupported;
  const Csr g{m, nnz, h, f, row_ptr, col_ind, nullptr, nullptr};
  return launch_gt_dense_fwd_ranked(g, p, Q, K, V, attn_ranked, out, as_stream(stream));
}

int dfgnn_gt_bwd_ranked(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *Q,
                        const float *K, const float *V, const float *attn_ranked, const float *grad_out, float *dQ,
                        float *dK, float *dV, const int *plan, const int *plan_meta, dfgnn_stream_t stream) {
  if (int c = check_common(m, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (!Q || !K || !V || !attn_ranked || !grad_out || !dQ || !dK || !dV) return kErrBadArg;
  Plan p;
  if (!(aligned16(Q) && aligned16(K) && aligned16(V) && aligned16(grad_out) && aligned16(dQ) && aligned16(dK) && aligned16(dV)) ||
      !gt_stats_plan(p, plan, plan_meta, m, nnz, h, f))
    return kErrUnsupported;
  const Csr g{m, nnz, h, f, row_ptr, col_ind, nullptr, nullptr};
  return launch_gt_dense_bwd(g, p, Q, K, V, attn_ranked, grad_out, dQ, dK, dV, as_stream(stream), true);
}

// ---- the four pairs that take an m x n_cols graph (rows: queries / outputs, columns: keys / values) -----------------------
// Each has a *_rect entry with both extents; the entry of the square adjacency is that one with n_cols = m.  A pass whose
// extent is 0 launches nothing (dfgnn_launch.hpp), so: without rows the backward still zeroes dK / dV in full (every column
// is empty), without columns the forward writes out = 0 and the sentinels and the backward dQ = 0.  An array of an empty
// side may be NULL.

// ---- the general statistics pair (gt_train.hip): any graph, no plan, nothing of size nnz saved or parked ----------------
int dfgnn_gt_fwd_rowstats_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                               const float *val, const float *Q, const float *K, const float *V, float *row_max,
                               float *row_sum, float *out, dfgnn_stream_t stream) {
  if (int c = check_rect(m, n_cols, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (m == 0) return 0;  // (no row: nothing to write)
  if (!Q || !out || (n_cols > 0 && (!K || !V)) || (!row_max != !row_sum)) return kErrBadArg;  // (both statistics or neither: inference)
  const Csr g = rect_csr(m, n_cols, nnz, h, f, row_ptr, col_ind, val);
  return launch_gt_train_fwd(g, Q, K, V, row_max, row_sum, out, as_stream(stream));
}

int dfgnn_gt_fwd_rowstats(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                          const float *Q, const float *K, const float *V, float *row_max, float *row_sum, float *out,
                          dfgnn_stream_t stream) {
  return dfgnn_gt_fwd_rowstats_rect(m, m, nnz, h, f, row_ptr, col_ind, val, Q, K, V, row_max, row_sum, out, stream);
}

int dfgnn_gt_bwd_rowstats_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                               const float *val, const int *col_ptr, const int *row_ind, const int *val_idx, const float *Q,
                               const float *K, const float *V, const float *out, const float *row_max, const float *row_sum,
                               const float *grad_out, float *delta, float *dQ, float *dK, float *dV, dfgnn_stream_t stream) {
  if (int c = check_rect(m, n_cols, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (m > 0 && (!Q || !out || !row_max || !row_sum || !grad_out || !delta || !dQ)) return kErrBadArg;
  if (n_cols > 0 && (!K || !V || !dK || !dV || !col_ptr)) return kErrBadArg;
  if (nnz > 0 && (!row_ind || (val && !val_idx))) return kErrBadArg;  // (unit values never read val_idx)
  const Csr g = rect_csr(m, n_cols, nnz, h, f, row_ptr, col_ind, val);
  if (int rc = launch_gt_train_bwd_rows(g, Q, K, V, out, row_max, row_sum, grad_out, delta, dQ, as_stream(stream)))
    return rc;
  return launch_gt_train_bwd_cols(g, col_ptr, row_ind, val_idx, Q, K, V, row_max, row_sum, delta, grad_out, dK, dV,
                                  as_stream(stream));
}

int dfgnn_gt_bwd_rowstats(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                          const int *col_ptr, const int *row_ind, const int *val_idx, const float *Q, const float *K,
                          const float *V, const float *out, const float *row_max, const float *row_sum,
                          const float *grad_out, float *delta, float *dQ, float *dK, float *dV, dfgnn_stream_t stream) {
  return dfgnn_gt_bwd_rowstats_rect(m, m, nnz, h, f, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, Q, K, V, out, row_max,
                                    row_sum, grad_out, delta, dQ, dK, dV, stream);
}

// ---- the general statistics pair with a per-edge additive attention bias (gt_bias_train.hip) ------------------------------
int dfgnn_gt_fwd_bias_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                           const float *bias, const float *Q, const float *K, const float *V, float *row_max,
                           float *row_sum, float *out, dfgnn_stream_t stream) {
  if (int c = check_rect(m, n_cols, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (m == 0) return 0;  // (no row: nothing to write)
  if (!Q || !out || (n_cols > 0 && (!K || !V)) || (!row_max != !row_sum)) return kErrBadArg;  // (both statistics or neither: inference)
  if (nnz > 0 && !bias) return kErrBadArg;
  const Csr g = rect_csr(m, n_cols, nnz, h, f, row_ptr, col_ind, val);
  return launch_gt_bias_fwd(g, bias, Q, K, V, row_max, row_sum, out, as_stream(stream));
}

int dfgnn_gt_fwd_bias(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                      const float *bias, const float *Q, const float *K, const float *V, float *row_max, float *row_sum,
                      float *out, dfgnn_stream_t stream) {
  return dfgnn_gt_fwd_bias_rect(m, m, nnz, h, f, row_ptr, col_ind, val, bias, Q, K, V, row_max, row_sum, out, stream);
}

int dfgnn_gt_bwd_bias_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                           const float *bias, const int *col_ptr, const int *row_ind, const int *val_idx, const float *Q,
                           const float *K, const float *V, const float *out, const float *row_max, const float *row_sum,
                           const float *grad_out, float *delta, float *dQ, float *dK, float *dV, float *dbias,
                           dfgnn_stream_t stream) {
  if (int c = check_rect(m, n_cols, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (m > 0 && (!Q || !out || !row_max || !row_sum || !grad_out || !delta || !dQ)) return kErrBadArg;
  if (n_cols > 0 && (!K || !V || !dK || !dV || !col_ptr)) return kErrBadArg;
  if (nnz > 0 && (!bias || !row_ind || !val_idx)) return kErrBadArg;  // (the CSC pass finds an entry's bias through val_idx)
  const Csr g = rect_csr(m, n_cols, nnz, h, f, row_ptr, col_ind, val);
  if (int rc = launch_gt_bias_bwd_rows(g, bias, Q, K, V, out, row_max, row_sum, grad_out, delta, dQ, dbias,
                                       as_stream(stream)))
    return rc;
  return launch_gt_bias_bwd_cols(g, bias, col_ptr, row_ind, val_idx, Q, K, V, row_max, row_sum, delta, grad_out, dK, dV,
                                 as_stream(stream));
}

int dfgnn_gt_bwd_bias(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                      const float *bias, const int *col_ptr, const int *row_ind, const int *val_idx, const float *Q,
                      const float *K, const float *V, const float *out, const float *row_max, const float *row_sum,
                      const float *grad_out, float *delta, float *dQ, float *dK, float *dV, float *dbias,
                      dfgnn_stream_t stream) {
  return dfgnn_gt_bwd_bias_rect(m, m, nnz, h, f, row_ptr, col_ind, val, bias, col_ptr, row_ind, val_idx, Q, K, V, out, row_max,
                                row_sum, grad_out, delta, dQ, dK, dV, dbias, stream);
}

// ---- the general statistics pair with a per-edge feature vector in keys and values (gt_edge_train.hip) --------------------
int dfgnn_gt_fwd_edge_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                           const float *E, const float *Q, const float *K, const float *V, float *row_max, float *row_sum,
                           float *out, dfgnn_stream_t stream) {
  if (int c = check_rect(m, n_cols, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (m == 0) return 0;  // (no row: nothing to write)
  if (!Q || !out || (n_cols > 0 && (!K || !V)) || (!row_max != !row_sum)) return kErrBadArg;  // (both statistics or neither: inference)
  if (nnz > 0 && !E) return kErrBadArg;
  const Csr g = rect_csr(m, n_cols, nnz, h, f, row_ptr, col_ind, val);
  return launch_gt_edge_fwd(g, E, Q, K, V, row_max, row_sum, out, as_stream(stream));
}

int dfgnn_gt_fwd_edge(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                      const float *E, const float *Q, const float *K, const float *V, float *row_max, float *row_sum,
                      float *out, dfgnn_stream_t stream) {
  return dfgnn_gt_fwd_edge_rect(m, m, nnz, h, f, row_ptr, col_ind, val, E, Q, K, V, row_max, row_sum, out, stream);
}

int dfgnn_gt_bwd_edge_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                           const float *E, const int *col_ptr, const int *row_ind, const int *val_idx, const float *Q,
                           const float *K, const float *V, const float *out, const float *row_max, const float *row_sum,
                           const float *grad_out, float *delta, float *dQ, float *dK, float *dV, float *dE,
                           dfgnn_stream_t stream) {
  if (int c = check_rect(m, n_cols, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (m > 0 && (!Q || !out || !row_max || !row_sum || !grad_out || !delta || !dQ)) return kErrBadArg;
  if (n_cols > 0 && (!K || !V || !dK || !dV || !col_ptr)) return kErrBadArg;
  if (nnz > 0 && (!E || !row_ind || !val_idx)) return kErrBadArg;  // (the CSC pass finds an entry's E row through val_idx)
  const Csr g = rect_csr(m, n_cols, nnz, h, f, row_ptr, col_ind, val);
  if (int rc = launch_gt_edge_bwd_rows(g, E, Q, K, V, out, row_max, row_sum, grad_out, delta, dQ, dE, as_stream(stream)))
    return rc;
  return launch_gt_edge_bwd_cols(g, E, col_ptr, row_ind, val_idx, Q, K, V, row_max, row_sum, delta, grad_out, dK, dV,
                                 as_stream(stream));
}

int dfgnn_gt_bwd_edge(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                      const float *E, const int *col_ptr, const int *row_ind, const int *val_idx, const float *Q,
                      const float *K, const float *V, const float *out, const float *row_max, const float *row_sum,
                      const float *grad_out, float *delta, float *dQ, float *dK, float *dV, float *dE,
                      dfgnn_stream_t stream) {
  return dfgnn_gt_bwd_edge_rect(m, m, nnz, h, f, row_ptr, col_ind, val, E, col_ptr, row_ind, val_idx, Q, K, V, out, row_max,
                                row_sum, grad_out, delta, dQ, dK, dV, dE, stream);
}

// ---- the general statistics pair with a per-edge multiplicative gate and an edge-output channel (gt_gate_train.hip) -------
int dfgnn_gt_fwd_gate_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                           const float *E, const float *Q, const float *K, const float *V, float *row_max, float *row_sum,
                           float *out, float *W, dfgnn_stream_t stream) {
  if (int c = check_rect(m, n_cols, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (m == 0) return 0;  // (no row: nothing to write)
  if (!Q || !out || (n_cols > 0 && (!K || !V)) || (!row_max != !row_sum)) return kErrBadArg;  // (both statistics or neither: inference)
  if (nnz > 0 && !E) return kErrBadArg;
  const Csr g = rect_csr(m, n_cols, nnz, h, f, row_ptr, col_ind, val);
  return launch_gt_gate_fwd(g, E, Q, K, V, row_max, row_sum, out, W, as_stream(stream));
}

int dfgnn_gt_fwd_gate(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                      const float *E, const float *Q, const float *K, const float *V, float *row_max, float *row_sum,
                      float *out, float *W, dfgnn_stream_t stream) {
  return dfgnn_gt_fwd_gate_rect(m, m, nnz, h, f, row_ptr, col_ind, val, E, Q, K, V, row_max, row_sum, out, W, stream);
}

int dfgnn_gt_bwd_gate_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                           const float *E, const int *col_ptr, const int *row_ind, const int *val_idx, const float *Q,
                           const float *K, const float *V, const float *out, const float *row_max, const float *row_sum,
                           const float *grad_out, const float *G, float *delta, float *dQ, float *dK, float *dV, float *dE,
                           dfgnn_stream_t stream) {
  if (int c = check_rect(m, n_cols, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (m > 0 && (!Q || !out || !row_max || !row_sum || !grad_out || !delta || !dQ)) return kErrBadArg;
  if (n_cols > 0 && (!K || !V || !dK || !dV || !col_ptr)) return kErrBadArg;
  if (nnz > 0 && (!E || !row_ind || !val_idx)) return kErrBadArg;  // (the CSC pass finds an entry's E and G rows through val_idx)
  const Csr g = rect_csr(m, n_cols, nnz, h, f, row_ptr, col_ind, val);
  if (int rc = launch_gt_gate_bwd_rows(g, E, Q, K, V, out, row_max, row_sum, grad_out, G, delta, dQ, dE, as_stream(stream)))
    return rc;
  return launch_gt_gate_bwd_cols(g, E, col_ptr, row_ind, val_idx, Q, K, V, row_max, row_sum, delta, grad_out, G, dK, dV,
                                 as_stream(stream));
}

int dfgnn_gt_bwd_gate(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                      const float *E, const int *col_ptr, const int *row_ind, const int *val_idx, const float *Q,
                      const float *K, const float *V, const float *out, const float *row_max, const float *row_sum,
                      const float *grad_out, const float *G, float *delta, float *dQ, float *dK, float *dV, float *dE,
                      dfgnn_stream_t stream) {
  return dfgnn_gt_bwd_gate_rect(m, m, nnz, h, f, row_ptr, col_ind, val, E, col_ptr, row_ind, val_idx, Q, K, V, out, row_max,
                                row_sum, grad_out, G, delta, dQ, dK, dV, dE, stream);
}

// ---- the general statistics pair with typed edges: key / value vectors looked up from a table (gt_typed_train.hip) --------
int dfgnn_gt_typed_bwd_ws_floats(int T, int h, int f) {
  if (T < 1 || h < 0 || f < 0) return kErrBadArg;
  if (h > 65535 || !gt_typed_table_fits(T, f)) return kErrUnsupported;
  const long long n = (long long)kGtTypedParts * T * (h > 0 ? h : 1) * (f > 0 ? f : 1);
  return n > 0x7fffffffLL ? kErrUnsupported : (int)n;
}

int dfgnn_gt_fwd_typed_rect(int m, int n_cols, int nnz, int h, int f, int T, const int *row_ptr, const int *col_ind,
                            const float *val, const int *etype, const float *R, const float *Q, const float *K,
                            const float *V, float *row_max, float *row_sum, float *out, dfgnn_stream_t stream) {
  if (T < 1) return kErrBadArg;
  if (int c = check_rect(m, n_cols, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (m == 0) return 0;  // (no row: nothing to write)
  if (!Q || !out || (n_cols > 0 && (!K || !V)) || (!row_max != !row_sum)) return kErrBadArg;  // (both statistics or neither: inference)
  if (nnz > 0 && (!etype || !R)) return kErrBadArg;
  const Csr g = rect_csr(m, n_cols, nnz, h, f, row_ptr, col_ind, val);
  return launch_gt_typed_fwd(g, GtTypedTable{T, etype, nullptr, R}, Q, K, V, row_max, row_sum, out, as_stream(stream));
}

int dfgnn_gt_fwd_typed(int m, int nnz, int h, int f, int T, const int *row_ptr, const int *col_ind, const float *val,
                       const int *etype, const float *R, const float *Q, const float *K, const float *V, float *row_max,
                       float *row_sum, float *out, dfgnn_stream_t stream) {
  return dfgnn_gt_fwd_typed_rect(m, m, nnz, h, f, T, row_ptr, col_ind, val, etype, R, Q, K, V, row_max, row_sum, out, stream);
}

int dfgnn_gt_bwd_typed_rect(int m, int n_cols, int nnz, int h, int f, int T, const int *row_ptr, const int *col_ind,
                            const float *val, const int *etype, const int *col_ptr, const int *row_ind, const int *val_idx,
                            const int *etype_csc, const float *R, const float *Q, const float *K, const float *V,
                            const float *out, const float *row_max, const float *row_sum, const float *grad_out,
                            float *delta, float *ws, float *dQ, float *dK, float *dV, float *dR, dfgnn_stream_t stream) {
  if (T < 1) return kErrBadArg;
  const int c = check_rect(m, n_cols, nnz, h, f, row_ptr, col_ind);
  if (c < 0) return c;
  if (dR) {  // (the partials of dR are the only use of ws)
    if (!ws) return kErrBadArg;
    if (int n = dfgnn_gt_typed_bwd_ws_floats(T, h, f); n < 0) return n;
  }
  if (c > 0 && (!dR || h == 0 || f == 0)) return 0;  // (neither rows nor columns: dR = 0 is still written, below)
  if (m > 0 && (!Q || !out || !row_max || !row_sum || !grad_out || !delta || !dQ)) return kErrBadArg;
  if (n_cols > 0 && (!K || !V || !dK || !dV || !col_ptr)) return kErrBadArg;
  if (c == 0 && nnz > 0 && (!etype || !etype_csc || !R || !row_ind || (val && !val_idx))) return kErrBadArg;  // (unit values never read val_idx)
  const Csr g = rect_csr(m, n_cols, nnz, h, f, row_ptr, col_ind, val);
  const GtTypedTable t{T, etype, etype_csc, R};
  if (int rc = launch_gt_typed_bwd_rows(g, t, Q, K, V, out, row_max, row_sum, grad_out, delta, dQ, ws, dR, as_stream(stream)))
    return rc;
  return launch_gt_typed_bwd_cols(g, t, col_ptr, row_ind, val_idx, Q, K, V, row_max, row_sum, delta, grad_out, dK, dV,
                                  as_stream(stream));
}

int dfgnn_gt_bwd_typed(int m, int nnz, int h, int f, int T, const int *row_ptr, const int *col_ind, const float *val,
                       const int *etype, const int *col_ptr, const int *row_ind, const int *val_idx, const int *etype_csc,
                       const float *R, const float *Q, const float *K, const float *V, const float *out,
                       const float *row_max, const float *row_sum, const float *grad_out, float *delta, float *ws, float *dQ,
                       float *dK, float *dV, float *dR, dfgnn_stream_t stream) {
  return dfgnn_gt_bwd_typed_rect(m, m, nnz, h, f, T, row_ptr, col_ind, val, etype, col_ptr, row_ind, val_idx, etype_csc, R, Q,
                                 K, V, out, row_max, row_sum, grad_out, delta, ws, dQ, dK, dV, dR, stream);
}

// ---- the general statistics pair with a typed attention bias: scalars looked up from a table (gt_tbias_train.hip) --------
int dfgnn_gt_tbias_bwd_ws_floats(int T, int h) {
  if (T < 1 || h < 0) return kErrBadArg;
  if (h > 65535 || T > kGtTBiasMaxTypes) return kErrUnsupported;
  const long long n = (long long)gt_tbias_parts(T) * T * (h > 0 ? h : 1);
  return n > 0x7fffffffLL ? kErrUnsupported : (int)n;
}

int dfgnn_gt_fwd_tbias_rect(int m, int n_cols, int nnz, int h, int f, int T, const int *row_ptr, const int *col_ind,
                            const float *val, const int *etype, const float *B, const float *Q, const float *K,
                            const float *V, float *row_max, float *row_sum, float *out, dfgnn_stream_t stream) {
  if (T < 1) return kErrBadArg;
  if (int c = check_rect(m, n_cols, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (m == 0) return 0;  // (no row: nothing to write)
  if (!Q || !out || (n_cols > 0 && (!K || !V)) || (!row_max != !row_sum)) return kErrBadArg;  // (both statistics or neither: inference)
  if (nnz > 0 && (!etype || !B)) return kErrBadArg;
  const Csr g = rect_csr(m, n_cols, nnz, h, f, row_ptr, col_ind, val);
  return launch_gt_tbias_fwd(g, GtTBiasTable{T, etype, nullptr, B}, Q, K, V, row_max, row_sum, out, as_stream(stream));
}

int dfgnn_gt_fwd_tbias(int m, int nnz, int h, int f, int T, const int *row_ptr, const int *col_ind, const float *val,
                       const int *etype, const float *B, const float *Q, const float *K, const float *V, float *row_max,
                       float *row_sum, float *out, dfgnn_stream_t stream) {
  return dfgnn_gt_fwd_tbias_rect(m, m, nnz, h, f, T, row_ptr, col_ind, val, etype, B, Q, K, V, row_max, row_sum, out, stream);
}

int dfgnn_gt_bwd_tbias_rect(int m, int n_cols, int nnz, int h, int f, int T, const int *row_ptr, const int *col_ind,
                            const float *val, const int *etype, const int *col_ptr, const int *row_ind, const int *val_idx,
                            const int *etype_csc, const float *B, const float *Q, const float *K, const float *V,
                            const float *out, const float *row_max, const float *row_sum, const float *grad_out,
                            float *delta, float *ws, float *dQ, float *dK, float *dV, float *dB, dfgnn_stream_t stream) {
  if (T < 1) return kErrBadArg;
  const int c = check_rect(m, n_cols, nnz, h, f, row_ptr, col_ind);
  if (c < 0) return c;
  if (dB) {  // (the partials of dB are the only use of ws)
    if (!ws) return kErrBadArg;
    if (int n = dfgnn_gt_tbias_bwd_ws_floats(T, h); n < 0) return n;
  }
  if (c > 0 && (!dB || h == 0)) return 0;  // (neither rows nor columns: dB = 0 is still written, below)
  if (m > 0 && (!Q || !out || !row_max || !row_sum || !grad_out || !delta || !dQ)) return kErrBadArg;
  if (n_cols > 0 && (!K || !V || !dK || !dV || !col_ptr)) return kErrBadArg;
  if (c == 0 && nnz > 0 && (!etype || !etype_csc || !B || !row_ind || (val && !val_idx))) return kErrBadArg;  // (unit values never read val_idx)
  const Csr g = rect_csr(m, n_cols, nnz, h, f, row_ptr, col_ind, val);
  const GtTBiasTable t{T, etype, etype_csc, B};
  if (int rc = launch_gt_tbias_bwd_rows(g, t, Q, K, V, out, row_max, row_sum, grad_out, delta, dQ, ws, dB, as_stream(stream)))
    return rc;
  return launch_gt_tbias_bwd_cols(g, t, col_ptr, row_ind, val_idx, Q, K, V, row_max, row_sum, delta, grad_out, dK, dV,
                                  as_stream(stream));
}

int dfgnn_gt_bwd_tbias(int m, int nnz, int h, int f, int T, const int *row_ptr, const int *col_ind, const float *val,
                       const int *etype, const int *col_ptr, const int *row_ind, const int *val_idx, const int *etype_csc,
                       const float *B, const float *Q, const float *K, const float *V, const float *out,
                       const float *row_max, const float *row_sum, const float *grad_out, float *delta, float *ws, float *dQ,
                       float *dK, float *dV, float *dB, dfgnn_stream_t stream) {
  return dfgnn_gt_bwd_tbias_rect(m, m, nnz, h, f, T, row_ptr, col_ind, val, etype, col_ptr, row_ind, val_idx, etype_csc, B, Q,
                                 K, V, out, row_max, row_sum, grad_out, delta, ws, dQ, dK, dV, dB, stream);
}

// ---- GATv2 (gatv2_train.hip): fused inference and training pair, any graph ------------------------------------------------
int dfgnn_gatv2_bwd_ws_floats(int h, int f) {
  if (h < 0 || f < 0) return kErrBadArg;
  if (h > 65535) return kErrUnsupported;
  const long long n = (long long)kGatv2Parts * (h > 0 ? h : 1) * (f > 0 ? f : 1);
  return n > 0x7fffffffLL ? kErrUnsupported : (int)n;
}

int dfgnn_gatv2_fwd_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *attn,
                         float negative_slope, const float *X_row, const float *X_col, float *row_max, float *row_sum,
                         float *out, dfgnn_stream_t stream) {
  if (int c = check_rect(m, n_cols, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (m == 0) return 0;  // (no row: nothing to write)
  if (!attn || !X_row || (n_cols > 0 && !X_col) || !out || (!row_max != !row_sum)) return kErrBadArg;  // (both statistics or neither)
  const Csr g = rect_csr(m, n_cols, nnz, h, f, row_ptr, col_ind, nullptr);
  return launch_gatv2_fwd(g, Gatv2Graph{nullptr, nullptr, attn, negative_slope}, X_row, X_col, row_max, row_sum, out,
                          as_stream(stream));
}

int dfgnn_gatv2_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *attn,
                    float negative_slope, const float *X_row, const float *X_col, float *row_max, float *row_sum,
                    float *out, dfgnn_stream_t stream) {
  return dfgnn_gatv2_fwd_rect(m, m, nnz, h, f, row_ptr, col_ind, attn, negative_slope, X_row, X_col, row_max, row_sum, out,
                              stream);
}

int dfgnn_gatv2_bwd_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const int *col_ptr,
                         const int *row_ind, const float *attn, float negative_slope, const float *X_row, const float *X_col,
                         const float *out, const float *row_max, const float *row_sum, const float *grad_out, float *delta,
                         float *ws, float *dX_row, float *dX_col, float *dattn, dfgnn_stream_t stream) {
  if (int c = check_rect(m, n_cols, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (!attn || !ws || !dattn || (nnz > 0 && !row_ind)) return kErrBadArg;
  if (m > 0 && (!X_row || !out || !row_max || !row_sum || !grad_out || !delta || !dX_row)) return kErrBadArg;
  if (n_cols > 0 && (!X_col || !dX_col || !col_ptr)) return kErrBadArg;
  if (dX_row && dX_row == dX_col) return kErrBadArg;  // (the two passes each write their buffer in full)
  if (dfgnn_gatv2_bwd_ws_floats(h, f) < 0) return kErrUnsupported;
  const Csr g = rect_csr(m, n_cols, nnz, h, f, row_ptr, col_ind, nullptr);
  return launch_gatv2_bwd(g, Gatv2Graph{col_ptr, row_ind, attn, negative_slope}, X_row, X_col, out, row_max, row_sum,
                          grad_out, delta, ws, dX_row, dX_col, dattn, as_stream(stream));
}

int dfgnn_gatv2_bwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const int *col_ptr,
                    const int *row_ind, const float *attn, float negative_slope, const float *X_row, const float *X_col,
                    const float *out, const float *row_max, const float *row_sum, const float *grad_out, float *delta,
                    float *ws, float *dX_row, float *dX_col, float *dattn, dfgnn_stream_t stream) {
  return dfgnn_gatv2_bwd_rect(m, m, nnz, h, f, row_ptr, col_ind, col_ptr, row_ind, attn, negative_slope, X_row, X_col, out,
                              row_max, row_sum, grad_out, delta, ws, dX_row, dX_col, dattn, stream);
}

// ---- AGNN / dot-product attention with tied keys and values (agnn_train.hip): fused inference and training pair, any graph ---
int dfgnn_agnn_fwd_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *beta,
                        int cosine, const float *X_row, const float *X_col, float *row_max, float *row_sum, float *out,
                        dfgnn_stream_t stream) {
  if (cosine != 0 && cosine != 1) return kErrBadArg;
  if (int c = check_rect(m, n_cols, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (m == 0) return 0;  // (no row: nothing to write)
  if (!beta || !X_row || (n_cols > 0 && !X_col) || !out || (!row_max != !row_sum)) return kErrBadArg;  // (both statistics or neither)
  const Csr g = rect_csr(m, n_cols, nnz, h, f, row_ptr, col_ind, nullptr);
  return launch_agnn_fwd(g, AgnnGraph{nullptr, nullptr, beta, cosine == 1}, X_row, X_col, row_max, row_sum, out,
                         as_stream(stream));
}

int dfgnn_agnn_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *beta, int cosine,
                   const float *X_row, const float *X_col, float *row_max, float *row_sum, float *out,
                   dfgnn_stream_t stream) {
  return dfgnn_agnn_fwd_rect(m, m, nnz, h, f, row_ptr, col_ind, beta, cosine, X_row, X_col, row_max, row_sum, out, stream);
}

int dfgnn_agnn_bwd_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const int *col_ptr,
                        const int *row_ind, const float *beta, int cosine, const float *X_row, const float *X_col,
                        const float *out, const float *row_max, const float *row_sum, const float *grad_out, float *delta,
                        float *dX_row, float *dX_col, float *dbeta_rows, dfgnn_stream_t stream) {
  if (cosine != 0 && cosine != 1) return kErrBadArg;
  if (int c = check_rect(m, n_cols, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (!beta || (nnz > 0 && !row_ind)) return kErrBadArg;
  if (m > 0 && (!X_row || !out || !row_max || !row_sum || !grad_out || !delta || !dX_row)) return kErrBadArg;
  if (n_cols > 0 && (!X_col || !dX_col || !col_ptr)) return kErrBadArg;
  if (dX_row && dX_row == dX_col) return kErrBadArg;  // (the two passes each write their buffer in full)
  const Csr g = rect_csr(m, n_cols, nnz, h, f, row_ptr, col_ind, nullptr);
  return launch_agnn_bwd(g, AgnnGraph{col_ptr, row_ind, beta, cosine == 1}, X_row, X_col, out, row_max, row_sum, grad_out,
                         delta, dX_row, dX_col, dbeta_rows, as_stream(stream));
}

int dfgnn_agnn_bwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const int *col_ptr,
                   const int *row_ind, const float *beta, int cosine, const float *X_row, const float *X_col,
                   const float *out, const float *row_max, const float *row_sum, const float *grad_out, float *delta,
                   float *dX_row, float *dX_col, float *dbeta_rows, dfgnn_stream_t stream) {
  return dfgnn_agnn_bwd_rect(m, m, nnz, h, f, row_ptr, col_ind, col_ptr, row_ind, beta, cosine, X_row, X_col, out, row_max,
                             row_sum, grad_out, delta, dX_row, dX_col, dbeta_rows, stream);
}

// ---- GATv2 with a per-edge feature vector inside the LeakyReLU (gatv2_edge_train.hip) ---------------------------------------
int dfgnn_gatv2_fwd_edge_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                              const float *attn, float negative_slope, const float *X_row, const float *X_col, const float *E,
                              float *row_max, float *row_sum, float *out, dfgnn_stream_t stream) {
  if (int c = check_rect(m, n_cols, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (m == 0) return 0;  // (no row: nothing to write)
  if (!attn || !X_row || (n_cols > 0 && !X_col) || !out || (!row_max != !row_sum)) return kErrBadArg;  // (both statistics or neither)
  if (nnz > 0 && !E) return kErrBadArg;
  const Csr g = rect_csr(m, n_cols, nnz, h, f, row_ptr, col_ind, nullptr);
  return launch_gatv2_edge_fwd(g, Gatv2Graph{nullptr, nullptr, attn, negative_slope}, X_row, X_col, E, row_max, row_sum, out,
                               as_stream(stream));
}

int dfgnn_gatv2_fwd_edge(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *attn,
                         float negative_slope, const float *X_row, const float *X_col, const float *E, float *row_max,
                         float *row_sum, float *out, dfgnn_stream_t stream) {
  return dfgnn_gatv2_fwd_edge_rect(m, m, nnz, h, f, row_ptr, col_ind, attn, negative_slope, X_row, X_col, E, row_max, row_sum,
                                   out, stream);
}

int dfgnn_gatv2_bwd_edge_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                              const int *col_ptr, const int *row_ind, const int *val_idx, const float *attn,
                              float negative_slope, const float *X_row, const float *X_col, const float *E, const float *out,
                              const float *row_max, const float *row_sum, const float *grad_out, float *delta, float *ws,
                              float *dX_row, float *dX_col, float *dattn, float *dE, dfgnn_stream_t stream) {
  if (int c = check_rect(m, n_cols, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (!attn || !ws || !dattn) return kErrBadArg;
  if (nnz > 0 && (!E || !row_ind || !val_idx)) return kErrBadArg;  // (the CSC pass finds an entry's E row through val_idx)
  if (m > 0 && (!X_row || !out || !row_max || !row_sum || !grad_out || !delta || !dX_row)) return kErrBadArg;
  if (n_cols > 0 && (!X_col || !dX_col || !col_ptr)) return kErrBadArg;
  if (dX_row && dX_row == dX_col) return kErrBadArg;  // (the two passes each write their buffer in full)
  if (dfgnn_gatv2_bwd_ws_floats(h, f) < 0) return kErrUnsupported;
  const Csr g = rect_csr(m, n_cols, nnz, h, f, row_ptr, col_ind, nullptr);
  return launch_gatv2_edge_bwd(g, Gatv2Graph{col_ptr, row_ind, attn, negative_slope}, val_idx, X_row, X_col, E, out, row_max,
                               row_sum, grad_out, delta, ws, dX_row, dX_col, dattn, dE, as_stream(stream));
}

int dfgnn_gatv2_bwd_edge(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const int *col_ptr,
                         const int *row_ind, const int *val_idx, const float *attn, float negative_slope, const float *X_row,
                         const float *X_col, const float *E, const float *out, const float *row_max, const float *row_sum,
                         const float *grad_out, float *delta, float *ws, float *dX_row, float *dX_col, float *dattn,
                         float *dE, dfgnn_stream_t stream) {
  return dfgnn_gatv2_bwd_edge_rect(m, m, nnz, h, f, row_ptr, col_ind, col_ptr, row_ind, val_idx, attn, negative_slope, X_row,
                                   X_col, E, out, row_max, row_sum, grad_out, delta, ws, dX_row, dX_col, dattn, dE, stream);
}

// ---- GatedGCN (gatedgcn_train.hip): fused inference and training pair, any graph ------------------------------------------
static bool gatedgcn_mode_ok(int normalize, float eps) {
  return (normalize == 0 || normalize == 1) && eps >= 0.f && eps <= 3.0e38f;  // (a NaN fails both comparisons)
}

int dfgnn_gatedgcn_fwd_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                            const float *X_row, const float *X_col, const float *V, const float *E, int normalize, float eps,
                            float *den, float *out, float *Z, dfgnn_stream_t stream) {
  if (!gatedgcn_mode_ok(normalize, eps)) return kErrBadArg;
  if (int c = check_rect(m, n_cols, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (m == 0) return 0;  // (no row: nothing to write)
  if (!X_row || (n_cols > 0 && (!X_col || !V)) || !out) return kErrBadArg;
  const Csr g = rect_csr(m, n_cols, nnz, h, f, row_ptr, col_ind, nullptr);
  return launch_gatedgcn_fwd(g, GatedGcnGraph{nullptr, nullptr, nullptr, normalize == 1, eps}, X_row, X_col, V, E, den, out,
                             Z, as_stream(stream));
}

int dfgnn_gatedgcn_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *X_row,
                       const float *X_col, const float *V, const float *E, int normalize, float eps, float *den, float *out,
                       float *Z, dfgnn_stream_t stream) {
  return dfgnn_gatedgcn_fwd_rect(m, m, nnz, h, f, row_ptr, col_ind, X_row, X_col, V, E, normalize, eps, den, out, Z, stream);
}

int dfgnn_gatedgcn_bwd_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                            const int *col_ptr, const int *row_ind, const int *val_idx, const float *X_row,
                            const float *X_col, const float *V, const float *E, int normalize, float eps, const float *out,
                            const float *den, const float *grad_out, const float *G, float *dX_row, float *dX_col, float *dV,
                            float *dE, float *ws, dfgnn_stream_t stream) {
  if (!gatedgcn_mode_ok(normalize, eps)) return kErrBadArg;
  if (int c = check_rect(m, n_cols, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (nnz > 0 && (!row_ind || !val_idx)) return kErrBadArg;  // (the CSC pass finds an entry's E and G rows through val_idx)
  if (m > 0 && (!X_row || !grad_out || !dX_row)) return kErrBadArg;
  if (m > 0 && normalize == 1 && (!out || !den || !ws)) return kErrBadArg;  // (normalize = 0 reads none of the three)
  if (n_cols > 0 && (!X_col || !V || !dX_col || !dV || !col_ptr)) return kErrBadArg;
  if ((dX_row && (dX_row == dX_col || dX_row == dV)) || (dX_col && dX_col == dV)) return kErrBadArg;  // (each written in full)
  const Csr g = rect_csr(m, n_cols, nnz, h, f, row_ptr, col_ind, nullptr);
  return launch_gatedgcn_bwd(g, GatedGcnGraph{col_ptr, row_ind, val_idx, normalize == 1, eps}, X_row, X_col, V, E, out, den,
                             grad_out, G, dX_row, dX_col, dV, dE, ws, as_stream(stream));
}

int dfgnn_gatedgcn_bwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const int *col_ptr,
                       const int *row_ind, const int *val_idx, const float *X_row, const float *X_col, const float *V,
                       const float *E, int normalize, float eps, const float *out, const float *den, const float *grad_out,
                       const float *G, float *dX_row, float *dX_col, float *dV, float *dE, float *ws,
                       dfgnn_stream_t stream) {
  return dfgnn_gatedgcn_bwd_rect(m, m, nnz, h, f, row_ptr, col_ind, col_ptr, row_ind, val_idx, X_row, X_col, V, E, normalize,
                                 eps, out, den, grad_out, G, dX_row, dX_col, dV, dE, ws, stream);
}

// ---- GAT for any graph with an optional per-edge attention term (gat_edge_train.hip) --------------------------------------
int dfgnn_gat_fwd_edge_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                            const float *attn_row, const float *attn_col, float negative_slope, const float *score,
                            const float *X, const float *edge_mask, float attn_drop, float *edge_max, float *edge_sum,
                            float *out, dfgnn_stream_t stream) {
  if (edge_mask && !(attn_drop >= 0.f && attn_drop < 1.f)) return kErrBadArg;
  if (int c = check_rect(m, n_cols, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (m == 0) return 0;  // (no row: nothing to write)
  if (!attn_row || !out || (n_cols > 0 && (!attn_col || !X)) || (!edge_max != !edge_sum)) return kErrBadArg;  // (both statistics or neither: inference)
  const Csr g = rect_csr(m, n_cols, nnz, h, f, row_ptr, col_ind, nullptr);
  return launch_gat_edge_fwd(g, GatEdgeTerms{attn_row, attn_col, negative_slope, score, edge_mask, attn_drop}, X, edge_max,
                             edge_sum, out, as_stream(stream));
}

int dfgnn_gat_fwd_edge(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *attn_row,
                       const float *attn_col, float negative_slope, const float *score, const float *X,
                       const float *edge_mask, float attn_drop, float *edge_max, float *edge_sum, float *out,
                       dfgnn_stream_t stream) {
  return dfgnn_gat_fwd_edge_rect(m, m, nnz, h, f, row_ptr, col_ind, attn_row, attn_col, negative_slope, score, X, edge_mask,
                                 attn_drop, edge_max, edge_sum, out, stream);
}

int dfgnn_gat_bwd_edge_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                            const int *col_ptr, const int *row_ind, const int *val_idx, const float *attn_row,
                            const float *attn_col, float negative_slope, const float *score, const float *X,
                            const float *edge_mask, float attn_drop, const float *edge_max, const float *edge_sum,
                            const float *grad_out, float *delta, float *grad_feat, float *grad_attn_row,
                            float *grad_attn_col, float *grad_score, dfgnn_stream_t stream) {
  if (edge_mask && !(attn_drop >= 0.f && attn_drop < 1.f)) return kErrBadArg;
  if (int c = check_rect(m, n_cols, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (m > 0 && (!attn_row || !edge_max || !edge_sum || !grad_out || !delta || !grad_attn_row)) return kErrBadArg;
  if (n_cols > 0 && (!attn_col || !X || !grad_feat || !grad_attn_col || !col_ptr)) return kErrBadArg;
  if (nnz > 0 && !row_ind) return kErrBadArg;
  if (nnz > 0 && (score || edge_mask) && !val_idx) return kErrBadArg;  // (the CSC pass finds an entry's score and random through val_idx)
  const Csr g = rect_csr(m, n_cols, nnz, h, f, row_ptr, col_ind, nullptr);
  return launch_gat_edge_bwd(g, GatEdgeTerms{attn_row, attn_col, negative_slope, score, edge_mask, attn_drop}, col_ptr,
                             row_ind, val_idx, X, edge_max, edge_sum, grad_out, delta, grad_feat, grad_attn_row,
                             grad_attn_col, grad_score, as_stream(stream));
}

int dfgnn_gat_bwd_edge(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const int *col_ptr,
                       const int *row_ind, const int *val_idx, const float *attn_row, const float *attn_col,
                       float negative_slope, const float *score, const float *X, const float *edge_mask, float attn_drop,
                       const float *edge_max, const float *edge_sum, const float *grad_out, float *delta, float *grad_feat,
                       float *grad_attn_row, float *grad_attn_col, float *grad_score, dfgnn_stream_t stream) {
  return dfgnn_gat_bwd_edge_rect(m, m, nnz, h, f, row_ptr, col_ind, col_ptr, row_ind, val_idx, attn_row, attn_col,
                                 negative_slope, score, X, edge_mask, attn_drop, edge_max, edge_sum, grad_out, delta,
                                 grad_feat, grad_attn_row, grad_attn_col, grad_score, stream);
}

int dfgnn_gt_tiling_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                        const float *Q, const float *K, const float *V, float *out, dfgnn_stream_t stream) {
  if (int c = check_common(m, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (!Q || !K || !V || !out) return kErrBadArg;
  const Csr g{m, nnz, h, f, row_ptr, col_ind, nullptr, val};
  return launch_gt_tiling_fwd(g, Q, K, V, out, as_stream(stream));
}

static int gt_csr_impl(bool use_lds, int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                       const float *Q, const float *K, const float *V, float *logits, float *out, dfgnn_stream_t stream) {
  if (int c = check_common(m, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (!Q || !K || !V || !out || (nnz > 0 && !logits)) return kErrBadArg;
  const Csr g{m, nnz, h, f, row_ptr, col_ind, nullptr, val};
  return launch_gt_csr_fwd(g, Q, K, V, logits, out, use_lds, as_stream(stream));
}

int dfgnn_gt_csr_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                     const float *Q, const float *K, const float *V, float *logits, float *out, dfgnn_stream_t stream) {
  return gt_csr_impl(true, m, nnz, h, f, row_ptr, col_ind, val, Q, K, V, logits, out, stream);
}

int dfgnn_gt_csr_gm_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                        const float *Q, const float *K, const float *V, float *logits, float *out,
                        dfgnn_stream_t stream) {
  return gt_csr_impl(false, m, nnz, h, f, row_ptr, col_ind, val, Q, K, V, logits, out, stream);
}

int dfgnn_gat_recompute_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *attn_row,
                            const float *attn_col, float negative_slope, const float *X, float *out,
                            dfgnn_stream_t stream) {
  if (int c = check_common(m, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (!attn_row || !attn_col || !X || !out) return kErrBadArg;
  const Csr g{m, nnz, h, f, row_ptr, col_ind, nullptr, nullptr};
  return launch_gat_recompute_fwd(g, attn_row, attn_col, negative_slope, X, out, as_stream(stream));
}

static int gt_softmax_impl(bool use_lds, int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                           const int *rows, const float *val, const float *Q, const float *K, const float *V,
                           float *logits, float *out, dfgnn_stream_t stream) {
  if (int c = check_common(m, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (!Q || !K || !V || !out || (nnz > 0 && (!rows || !logits))) return kErrBadArg;
  const Csr g{m, nnz, h, f, row_ptr, col_ind, rows, val};
  if (int rc = launch_gt_sddmm(g, Q, K, logits, as_stream(stream))) return rc;
  return launch_softmax_spmm(g, logits, V, out, use_lds, as_stream(stream));
}

int dfgnn_gt_softmax_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const int *rows,
                         const float *val, const float *Q, const float *K, const float *V, float *logits,
                         float *out, dfgnn_stream_t stream) {
  return gt_softmax_impl(true, m, nnz, h, f, row_ptr, col_ind, rows, val, Q, K, V, logits, out, stream);
}

int dfgnn_gt_softmax_gm_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                            const int *rows, const float *val, const float *Q, const float *K, const float *V,
                            float *logits, float *out, dfgnn_stream_t stream) {
  return gt_softmax_impl(false, m, nnz, h, f, row_ptr, col_ind, rows, val, Q, K, V, logits, out, stream);
}

int dfgnn_gat_hyper_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const int *rows,
                        const float *attn_row, const float *attn_col, float negative_slope, const float *X,
                        float *edge_ws, float *out, const int *plan, const int *plan_meta, dfgnn_stream_t stream) {
  if (int c = check_common(m, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (!attn_row || !attn_col || !X || !out || (nnz > 0 && !rows)) return kErrBadArg;
  const Csr g{m, nnz, h, f, row_ptr, col_ind, rows, nullptr};
  Plan p;
  const bool v4 = (f % 4 == 0) && aligned16(X) && aligned16(out);
  if (v4 && make_plan(p, plan, plan_meta, m, nnz, h, f) && plan_usable(p, f, true, rows)) {
    if (int rc = launch_gat_block_fwd(g, p, attn_row, attn_col, negative_slope, X, edge_ws, out, as_stream(stream)))
      return rc;
    return launch_gat_hyper_fwd(g, attn_row, attn_col, negative_slope, X, out, p.spill(), p.num_spill,
                                as_stream(stream));
  }
  return launch_gat_hyper_fwd(g, attn_row, attn_col, negative_slope, X, out, nullptr, 0, as_stream(stream));
}

static int gat_softmax_impl(bool use_lds, int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                            const int *rows, const float *attn_row, const float *attn_col, float negative_slope,
                            const float *X, float *logits, float *out, dfgnn_stream_t stream) {
  if (int c = check_common(m, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (!attn_row || !attn_col || !X || !out || (nnz > 0 && (!rows || !logits))) return kErrBadArg;
  const Csr g{m, nnz, h, f, row_ptr, col_ind, rows, nullptr};
  if (int rc = launch_gat_sddmm(g, attn_row, attn_col, negative_slope, logits, as_stream(stream))) return rc;
  return launch_softmax_spmm(g, logits, X, out, use_lds, as_stream(stream));
}

int dfgnn_gat_softmax_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const int *rows,
                          const float *attn_row, const float *attn_col, float negative_slope, const float *X,
                          float *logits, float *out, dfgnn_stream_t stream) {
  return gat_softmax_impl(true, m, nnz, h, f, row_ptr, col_ind, rows, attn_row, attn_col, negative_slope, X,
                          logits, out, stream);
}

int dfgnn_gat_softmax_gm_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                             const int *rows, const float *attn_row, const float *attn_col, float negative_slope,
                             const float *X, float *logits, float *out, dfgnn_stream_t stream) {
  return gat_softmax_impl(false, m, nnz, h, f, row_ptr, col_ind, rows, attn_row, attn_col, negative_slope, X,
                          logits, out, stream);
}

int dfgnn_gat_tiling_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                         const float *attn_row, const float *attn_col, float negative_slope, const float *X,
                         float *out, dfgnn_stream_t stream) {
  if (int c = check_common(m, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (!attn_row || !attn_col || !X || !out) return kErrBadArg;
  const Csr g{m, nnz, h, f, row_ptr, col_ind, nullptr, nullptr};
  return launch_gat_tiling_fwd(g, attn_row, attn_col, negative_slope, X, out, as_stream(stream));
}

int dfgnn_gat_attn_scores(int m, int h, int f, const float *a_l, const float *a_r, const float *X, float *attn_row,
                          float *attn_col, dfgnn_stream_t stream) {
  if (m < 0 || h < 0 || f < 0) return kErrBadArg;
  if (m == 0 || h == 0) return 0;
  if (h > 65535) return kErrUnsupported;
  if (!a_l || !a_r || !X || !attn_row || !attn_col || f == 0) return kErrBadArg;
  return launch_gat_attn_scores(m, h, f, a_l, a_r, X, attn_row, attn_col, as_stream(stream));
}

// The GAT training pair serves the dense ranges of a plan with the matrix-core kernels and everything else (its
// non-dense fit ranges, its spill chunks) with the general kernels restricted to those ranges.
static bool gat_train_dense(Plan &p, const int *rows, const int *plan, const int *plan_meta, int m, int nnz, int h,
                            int f, bool v4) {
  if (!rows || !v4 || !dense_enabled()) return false;
  if (f != 8 && f != 16 && f != 32 && f != 64 && f != 128) return false;
  if (!make_plan(p, plan, plan_meta, m, nnz, h, f)) return false;
  return p.num_dense > 0;
}
static bool plan_has_rest(const Plan &p) { return p.num_fit - p.num_dense + p.num_spill > 0; }

int dfgnn_gat_fwd_train(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const int *rows,
                        const float *attn_row, const float *attn_col, float negative_slope, const float *X,
                        const float *edge_mask, float attn_drop, float *edge_max, float *edge_sum, float *out,
                        const int *plan, const int *plan_meta, dfgnn_stream_t stream) {
  if (int c = check_common(m, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (!attn_row || !attn_col || !X || !out || !edge_max || !edge_sum) return kErrBadArg;
  if (edge_mask && !(attn_drop >= 0.f && attn_drop < 1.f)) return kErrBadArg;
  const Csr g{m, nnz, h, f, row_ptr, col_ind, rows, nullptr};
  Plan p;
  const bool v4 = (f % 4 == 0) && aligned16(X) && aligned16(out);
  if (gat_train_dense(p, rows, plan, plan_meta, m, nnz, h, f, v4)) {
    if (int rc = launch_gat_dense_fwd(g, p, attn_row, attn_col, negative_slope, X, out, as_stream(stream), edge_max,
                                      edge_sum, edge_mask, attn_drop))
      return rc;
    if (!plan_has_rest(p)) return 0;
    return launch_gat_train_fwd(g, attn_row, attn_col, negative_slope, X, edge_mask, attn_drop, edge_max, edge_sum,
                                out, as_stream(stream), &p);
  }
  return launch_gat_train_fwd(g, attn_row, attn_col, negative_slope, X, edge_mask, attn_drop, edge_max, edge_sum,
                              out, as_stream(stream));
}

int dfgnn_gat_bwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const int *rows,
                  const int *col_ptr, const int *row_ind, const int *permute, const float *attn_row,
                  const float *attn_col, float negative_slope, const float *X, const float *edge_max,
                  const float *edge_sum, const float *edge_mask, float attn_drop, const float *grad_out,
                  float *grad_edge, float *grad_feat, float *grad_attn_row, float *grad_attn_col, const int *plan,
                  const int *plan_meta, dfgnn_stream_t stream) {
  if (int c = check_common(m, nnz, h, f, row_ptr, col_ind)) return c < 0 ? c : 0;
  if (!attn_row || !attn_col || !X || !edge_max || !edge_sum || !grad_out || !grad_feat || !grad_attn_row ||
      !grad_attn_col)
    return kErrBadArg;
  if (edge_mask && !(attn_drop >= 0.f && attn_drop < 1.f)) return kErrBadArg;
  const Csr g{m, nnz, h, f, row_ptr, col_ind, rows, nullptr};
  Plan p;
  const bool v4 = (f % 4 == 0) && aligned16(X) && aligned16(grad_out) && aligned16(grad_feat);
  const Plan *rest = nullptr;
  if (gat_train_dense(p, rows, plan, plan_meta, m, nnz, h, f, v4)) {
    if (int rc = launch_gat_dense_bwd(g, p, attn_row, attn_col, negative_slope, X, edge_max, edge_sum, grad_out,
                                      grad_feat, grad_attn_row, grad_attn_col, as_stream(stream), edge_mask, attn_drop))
      return rc;
    if (!plan_has_rest(p)) return 0;
    rest = &p;
  }
  if (!col_ptr || (nnz > 0 && (!row_ind || !permute || !grad_edge))) return kErrBadArg;
  if (int rc = launch_gat_bwd_rows(g, attn_row, attn_col, negative_slope, X, edge_max, edge_sum, edge_mask,
                                   attn_drop, grad_out, grad_edge, grad_attn_row, as_stream(stream), rest))
    return rc;
  return launch_gat_bwd_cols(g, col_ptr, row_ind, permute, attn_row, attn_col, negative_slope, edge_max, edge_sum,
                             edge_mask, attn_drop, grad_edge, grad_out, grad_feat, grad_attn_col, as_stream(stream),
                             rest);
}

}  // extern "C"
