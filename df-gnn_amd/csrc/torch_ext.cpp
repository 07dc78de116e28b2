// torch_ext.cpp -- the thin torch/extension.h shim over the C ABI of libdfgnn.so (include/dfgnn.h).
//
// This is the binding a maintainer of the reference would keep: pybind11 + torch::Tensor like
// DFGNN/src/fused_gtconv/fused_gtconv.cpp:577-602 and DFGNN/src/fused_gatconv/fused_gatconv.cpp:355-372, with each
// *_cuda host launcher (fused_gtconv_hyper.cu:679-760, fused_gtconv_backward.cu:231-265, fused_gatconv_*.cu) replaced by
// a few lines over the C ABI.  It holds no kernels: argument checks (real ones -- the reference's dtype / shape asserts
// are compiled out), output allocation, device guard + torch's CURRENT stream, one call into libdfgnn.so.
// Built by dfgnn_native.build() into df-gnn_amd/_dfgnn_ext.so (g++, in-tree, no JIT cache); the Python modules
// fused_gtconv / fused_gatconv route their hot entry points through it (a ctypes call costs ~25-60 us of host time per
// operator, this ~5) and keep the ctypes path for everything else.  Both paths end in the same dfgnn_* symbols.
//
// The optional block plan (dfgnn_plan_build, cached per batch structure by the Python side) and the "edge values are all
// ones" flag are passed in as plain integers / bool: caching lives in _binding_util.py for both bindings.
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>   // torch-ROCm: HIP devices are called "cuda"; these are the
#include <ATen/hip/impl/HIPStreamMasqueradingAsCUDA.h>      // guard / stream types behind torch.cuda.*
#include <torch/extension.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/dfgnn.h"

#ifndef DFGNN_SRC_HASH
#define DFGNN_SRC_HASH "unknown"
#endif

namespace {

using torch::Tensor;

inline void check_cuda_contig(const Tensor &t, const char *name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on CUDA");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}
inline void check_i32(const Tensor &t, const char *name) {
  check_cuda_contig(t, name);
  TORCH_CHECK(t.scalar_type() == torch::kInt32, name, " must have dtype torch.int32, got ", t.scalar_type());
}
inline void check_f32(const Tensor &t, const char *name) {
  check_cuda_contig(t, name);
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must have dtype torch.float32, got ", t.scalar_type());
}
inline void check_feat3(const Tensor &t, const Tensor &like, const char *name) {
  check_f32(t, name);
  TORCH_CHECK(t.dim() == 3, name, " must have shape [nodes, heads, feat], got ", t.sizes());
  TORCH_CHECK(t.sizes() == like.sizes(), name, " has shape ", t.sizes(), ", expected ", like.sizes());
}
inline void check_edges(const Tensor &t, int64_t nnz, const char *name) {
  TORCH_CHECK(t.dim() == 1 && t.size(0) == nnz, name, " must have shape (", nnz, ",), got ", t.sizes());
}
inline void check_same_device(const Tensor &ref, std::initializer_list<const Tensor *> ts) {
  for (const Tensor *t : ts)
    TORCH_CHECK(!t || !t->defined() || t->device() == ref.device(), "every tensor must live on one device (", ref.device(),
                "), got ", t->device(), ": a pointer of another GPU would be handed to a kernel of this one");
}
inline void check_rc(int rc, const char *what) {
  TORCH_CHECK(rc == 0, what, " failed: ", dfgnn_error_string(rc), " (code ", rc, ")");
}
inline dfgnn_stream_t cur_stream() {  // torch's current stream of the (guarded) current device
  return reinterpret_cast<dfgnn_stream_t>(c10::hip::getCurrentHIPStreamMasqueradingAsCUDA().stream());
}
inline const int *plan_ptr(int64_t p) { return reinterpret_cast<const int *>(static_cast<intptr_t>(p)); }
// typed device pointers for the C ABI; an undefined tensor / an empty optional is NULL
inline int *i32(const Tensor &t) { return t.defined() ? t.data_ptr<int>() : nullptr; }
inline float *f32(const Tensor &t) { return t.defined() ? t.data_ptr<float>() : nullptr; }
inline int *i32(const c10::optional<Tensor> &t) { return t ? t->data_ptr<int>() : nullptr; }
inline float *f32(const c10::optional<Tensor> &t) { return t ? t->data_ptr<float>() : nullptr; }
inline const Tensor *opt(const c10::optional<Tensor> &t) { return t ? &*t : nullptr; }

struct Dims {
  int m, nnz, h, f;
  int n_cols = 0;  // set by the checks of the pairs that take an m x n_cols graph (gt_rect_checks, gatv2_checks)
};
inline std::string shape_str(const Tensor &t) {  // "(2, 3, 4)", as Python prints a shape
  std::string s = "(";
  for (int64_t i = 0; i < t.dim(); ++i) s += (i ? ", " : "") + std::to_string(t.size(i));
  return s + (t.dim() == 1 ? ",)" : ")");
}
// the column side of a pair that takes an m x n_cols graph (K / V, GATv2's X_col): [n_cols, heads, feat] with the heads and
// features of the row side `rows` (Q, X_row)
inline void check_cols_feat(const Tensor &t, const char *name, const Tensor &rows, const char *rows_name) {
  check_f32(t, name);
  TORCH_CHECK(t.dim() == 3 && t.size(1) == rows.size(1) && t.size(2) == rows.size(2), name, " must have shape (n_cols, ",
              rows.size(1), ", ", rows.size(2), "): the heads and features of ", rows_name, ", got ", shape_str(t));
}
// What every GT entry point checks: the CSR arrays + Q / K / V, and -- where the entry point takes them, else nullptr --
// the COO rows and the edge values
Dims gt_checks(const Tensor &row_ptr, const Tensor &col_ind, const Tensor *rows, const Tensor *val, const Tensor &Q,
               const Tensor &K, const Tensor &V) {
  check_i32(row_ptr, "row_ptr");
  check_i32(col_ind, "col_ind");
  check_feat3(Q, Q, "Q");
  check_feat3(K, Q, "K");
  check_feat3(V, Q, "V");
  TORCH_CHECK(row_ptr.dim() == 1 && col_ind.dim() == 1, "indptr / indices must be 1-D");
  TORCH_CHECK(row_ptr.size(0) - 1 == Q.size(0), "indptr describes ", row_ptr.size(0) - 1, " rows but features have ", Q.size(0),
              " nodes");
  const int64_t nnz = col_ind.size(0);
  if (rows) {
    check_i32(*rows, "rows");
    check_edges(*rows, nnz, "rows");
  }
  if (val) {
    check_f32(*val, "val");
    check_edges(*val, nnz, "val");
  }
  check_same_device(Q, {&row_ptr, &col_ind, rows, val, &K, &V});
  return Dims{(int)Q.size(0), (int)nnz, (int)Q.size(1), (int)Q.size(2)};
}
// ... of the four pairs that take an m x n_cols graph (rowstats, bias, edge; GATv2 has its own): K and V agree with each
// other and with Q in [heads, feat]; their rows are the graph's columns
Dims gt_rect_checks(const Tensor &row_ptr, const Tensor &col_ind, const Tensor *val, const Tensor &Q, const Tensor &K,
                    const Tensor &V) {
  check_i32(row_ptr, "row_ptr");
  check_i32(col_ind, "col_ind");
  check_feat3(Q, Q, "Q");
  check_cols_feat(K, "K", Q, "Q");
  check_f32(V, "V");
  TORCH_CHECK(V.sizes() == K.sizes(), "V must have shape ", shape_str(K), " like K, got ", shape_str(V));
  TORCH_CHECK(row_ptr.dim() == 1 && col_ind.dim() == 1, "indptr / indices must be 1-D");
  TORCH_CHECK(row_ptr.size(0) - 1 == Q.size(0), "indptr describes ", row_ptr.size(0) - 1, " rows but features have ", Q.size(0),
              " nodes");
  const int64_t nnz = col_ind.size(0);
  if (val) {
    check_f32(*val, "val");
    check_edges(*val, nnz, "val");
  }
  check_same_device(Q, {&row_ptr, &col_ind, val, &K, &V});
  return Dims{(int)Q.size(0), (int)nnz, (int)Q.size(1), (int)Q.size(2), (int)K.size(0)};
}
// ... their CSC arrays: col_ptr has an entry per column and one more,
void csc_rect_checks(const Dims &d, const Tensor &ref, const Tensor &col_ptr, const Tensor &row_ind, const Tensor *val_idx,
                     const char *cols_name) {
  check_i32(col_ptr, "col_ptr");
  check_i32(row_ind, "row_ind");
  check_edges(row_ind, d.nnz, "row_ind");
  if (val_idx) {
    check_i32(*val_idx, "val_idx");
    check_edges(*val_idx, d.nnz, "val_idx");
  }
  TORCH_CHECK(col_ptr.dim() == 1 && col_ptr.size(0) == d.n_cols + 1, "col_ptr must have shape (", d.n_cols + 1,
              ",): one entry for each of the ", d.n_cols, " rows of ", cols_name, " and one more");
  check_same_device(ref, {&col_ptr, &row_ind, val_idx});
}
// ... of a backward of a square adjacency: the CSC arrays next to the CSR structure,
void csc_checks(const Dims &d, const Tensor &ref, const Tensor &col_ptr, const Tensor &row_ind, const Tensor &val_idx) {
  check_i32(col_ptr, "col_ptr");
  check_i32(row_ind, "row_ind");
  check_i32(val_idx, "val_idx");
  check_edges(row_ind, d.nnz, "row_ind");
  check_edges(val_idx, d.nnz, "val_idx");
  TORCH_CHECK(col_ptr.dim() == 1 && col_ptr.size(0) == d.m + 1, "col_ptr must have shape (", d.m + 1,
              ",): the adjacency must be square");
  check_same_device(ref, {&col_ptr, &row_ind, &val_idx});
}
// ... the row statistics [m, h] of a forward,
void row_stats_checks(const Dims &d, const Tensor &ref, const Tensor &row_max, const Tensor &row_sum) {
  check_f32(row_max, "row_max");
  check_f32(row_sum, "row_sum");
  for (const Tensor *t : {&row_max, &row_sum})
    TORCH_CHECK(t->dim() == 2 && t->size(0) == d.m && t->size(1) == d.h, "row_max / row_sum must have shape (", d.m, ", ", d.h,
                "), got ", t->sizes());
  check_same_device(ref, {&row_max, &row_sum});
}
// ... and attention values [h, nnz] in either order
void attn_checks(const Dims &d, const Tensor &ref, const Tensor &attn, const char *name) {
  check_f32(attn, name);
  TORCH_CHECK(attn.numel() == (int64_t)d.h * d.nnz, name, " must have ", d.h, "*", d.nnz, " elements, got ", attn.numel());
  check_same_device(ref, {&attn});
}

// fused_gtconv.cpp:278-314 (want_attn = false) and :79-116 (want_attn = true)
std::vector<Tensor> gt_hyper_fwd(const Tensor &row_ptr, const Tensor &col_ind, const Tensor &rows, const Tensor &val,
                                 const Tensor &Q, const Tensor &K, const Tensor &V, bool want_attn, bool unit_val,
                                 int64_t plan, int64_t meta) {
  const Dims d = gt_checks(row_ptr, col_ind, &rows, &val, Q, K, V);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Q.device());
  Tensor out = torch::empty_like(Q);
  Tensor attn, ws;
  if (want_attn) attn = torch::empty({d.h, d.nnz}, Q.options());
  else if (plan) ws = torch::empty({d.h, d.nnz}, Q.options());  // per-edge scratch of the inference call (include/dfgnn.h)
  check_rc(dfgnn_gt_hyper_fwd(d.m, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), i32(rows), unit_val ? nullptr : f32(val), f32(Q),
                              f32(K), f32(V), f32(attn), f32(ws), f32(out), plan_ptr(plan), plan_ptr(meta), cur_stream()),
           want_attn ? "gt_hyper_forward" : "gt_hyper_inference");
  if (want_attn) return {out, attn};
  return {out};
}

// fused_gtconv.cpp:125-172
std::vector<Tensor> gt_bwd(const Tensor &row_ptr, const Tensor &col_ind, const Tensor &rows, const Tensor &val,
                           const Tensor &col_ptr, const Tensor &row_ind, const Tensor &val_idx, const Tensor &Q,
                           const Tensor &K, const Tensor &V, const Tensor &attn_edge, const Tensor &grad, bool unit_val,
                           int64_t plan, int64_t meta) {
  const Dims d = gt_checks(row_ptr, col_ind, &rows, &val, Q, K, V);
  csc_checks(d, Q, col_ptr, row_ind, val_idx);
  attn_checks(d, Q, attn_edge, "attn_edge");
  check_feat3(grad, Q, "grad");
  check_same_device(Q, {&grad});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Q.device());
  Tensor grad_edge = torch::empty({d.h, d.nnz}, Q.options());
  Tensor dQ = torch::empty_like(Q), dK = torch::empty_like(K), dV = torch::empty_like(V);
  check_rc(dfgnn_gt_bwd(d.m, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), i32(rows), unit_val ? nullptr : f32(val), i32(col_ptr),
                        i32(row_ind), i32(val_idx), f32(Q), f32(K), f32(V), f32(attn_edge), f32(grad), f32(grad_edge), f32(dQ),
                        f32(dK), f32(dV), plan_ptr(plan), plan_ptr(meta), cur_stream()),
           "gt_backward");
  return {dQ, dK, dV};
}

// ---- the statistics-saving training pair (include/dfgnn.h: dfgnn_gt_hyper_fwd_stats / dfgnn_gt_bwd_stats) ---------------
// weights: the plan's dense edge values (plan_dense_weights below), or nothing for unit values
const float *weights_ptr(const c10::optional<Tensor> &weights, const Tensor &Q, int m) {
  if (!weights.has_value()) return nullptr;
  const Tensor &w = *weights;
  check_f32(w, "weights");
  TORCH_CHECK(w.numel() == (int64_t)dfgnn_plan_dense_weights_floats(m), "weights must hold ", dfgnn_plan_dense_weights_floats(m),
              " floats (dfgnn_plan_dense_weights), got ", w.numel());
  check_same_device(Q, {&w});
  return f32(w);
}

// save_stats = false: inference (nothing but `out` is produced; edge values on the matrix cores)
std::vector<Tensor> gt_hyper_fwd_stats(const Tensor &row_ptr, const Tensor &col_ind, const Tensor &Q, const Tensor &K,
                                       const Tensor &V, int64_t plan, int64_t meta, const c10::optional<Tensor> &weights,
                                       bool save_stats) {
  const Dims d = gt_checks(row_ptr, col_ind, nullptr, nullptr, Q, K, V);
  const float *w = weights_ptr(weights, Q, d.m);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Q.device());
  Tensor out = torch::empty_like(Q);
  Tensor row_max, row_sum;
  if (save_stats) {
    row_max = torch::empty({d.m, d.h}, Q.options());
    row_sum = torch::empty({d.m, d.h}, Q.options());
  }
  check_rc(dfgnn_gt_hyper_fwd_stats(d.m, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), w, f32(Q), f32(K), f32(V), f32(row_max),
                                    f32(row_sum), f32(out), plan_ptr(plan), plan_ptr(meta), cur_stream()),
           "gt_hyper_forward_stats");
  if (!save_stats) return {out};
  return {out, row_max, row_sum};
}

std::vector<Tensor> gt_bwd_stats(const Tensor &row_ptr, const Tensor &col_ind, const Tensor &Q, const Tensor &K,
                                 const Tensor &V, const Tensor &row_max, const Tensor &row_sum, const Tensor &grad,
                                 int64_t plan, int64_t meta, const c10::optional<Tensor> &weights) {
  const Dims d = gt_checks(row_ptr, col_ind, nullptr, nullptr, Q, K, V);
  const float *w = weights_ptr(weights, Q, d.m);
  check_feat3(grad, Q, "grad");
  row_stats_checks(d, Q, row_max, row_sum);
  check_same_device(Q, {&grad});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Q.device());
  Tensor dQ = torch::empty_like(Q), dK = torch::empty_like(K), dV = torch::empty_like(V);
  check_rc(dfgnn_gt_bwd_stats(d.m, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), w, f32(Q), f32(K), f32(V), f32(row_max),
                              f32(row_sum), f32(grad), f32(dQ), f32(dK), f32(dV), plan_ptr(plan), plan_ptr(meta), cur_stream()),
           "gt_backward_stats");
  return {dQ, dK, dV};
}

// ---- the general statistics pair (include/dfgnn.h: dfgnn_gt_fwd_rowstats / dfgnn_gt_bwd_rowstats): any graph, no plan ----
// val: edge values in CSR order, or nothing (unit values)
inline const float *edge_val_ptr(const c10::optional<Tensor> &val, bool unit_val) { return unit_val ? nullptr : f32(val); }

std::vector<Tensor> gt_fwd_rowstats(const Tensor &row_ptr, const Tensor &col_ind, const c10::optional<Tensor> &val, const Tensor &Q,
                                    const Tensor &K, const Tensor &V, bool unit_val) {
  const Dims d = gt_rect_checks(row_ptr, col_ind, opt(val), Q, K, V);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Q.device());
  Tensor out = torch::empty_like(Q);
  Tensor row_max = torch::empty({d.m, d.h}, Q.options()), row_sum = torch::empty({d.m, d.h}, Q.options());
  check_rc(dfgnn_gt_fwd_rowstats_rect(d.m, d.n_cols, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), edge_val_ptr(val, unit_val), f32(Q), f32(K),
                                 f32(V), f32(row_max), f32(row_sum), f32(out), cur_stream()),
           "gt_forward_rowstats");
  return {out, row_max, row_sum};
}

std::vector<Tensor> gt_bwd_rowstats(const Tensor &row_ptr, const Tensor &col_ind, const c10::optional<Tensor> &val, const Tensor &col_ptr,
                                    const Tensor &row_ind, const Tensor &val_idx, const Tensor &Q, const Tensor &K,
                                    const Tensor &V, const Tensor &out, const Tensor &row_max, const Tensor &row_sum,
                                    const Tensor &grad, bool unit_val) {
  const Dims d = gt_rect_checks(row_ptr, col_ind, opt(val), Q, K, V);
  csc_rect_checks(d, Q, col_ptr, row_ind, &val_idx, "K / V");
  check_feat3(out, Q, "out");
  check_feat3(grad, Q, "grad");
  row_stats_checks(d, Q, row_max, row_sum);
  check_same_device(Q, {&out, &grad});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Q.device());
  Tensor delta = torch::empty({d.m, d.h}, Q.options());
  Tensor dQ = torch::empty_like(Q), dK = torch::empty_like(K), dV = torch::empty_like(V);
  check_rc(dfgnn_gt_bwd_rowstats_rect(d.m, d.n_cols, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), edge_val_ptr(val, unit_val), i32(col_ptr),
                                 i32(row_ind), i32(val_idx), f32(Q), f32(K), f32(V), f32(out), f32(row_max), f32(row_sum),
                                 f32(grad), f32(delta), f32(dQ), f32(dK), f32(dV), cur_stream()),
           "gt_backward_rowstats");
  return {dQ, dK, dV};
}

// ---- the general pair with a per-edge additive attention bias (include/dfgnn.h: dfgnn_gt_fwd_bias / dfgnn_gt_bwd_bias) ----
// bias: fp32 [h, nnz] in CSR edge order
void bias_checks(const Dims &d, const Tensor &ref, const Tensor &bias) {
  check_f32(bias, "bias");
  TORCH_CHECK(bias.dim() == 2 && bias.size(0) == d.h && bias.size(1) == d.nnz, "bias must have shape (", d.h, ", ", d.nnz,
              "), got ", bias.sizes());
  check_same_device(ref, {&bias});
}

// save_stats = false: inference (-> {out})
std::vector<Tensor> gt_fwd_bias(const Tensor &row_ptr, const Tensor &col_ind, const c10::optional<Tensor> &val, const Tensor &bias,
                                const Tensor &Q, const Tensor &K, const Tensor &V, bool unit_val, bool save_stats) {
  const Dims d = gt_rect_checks(row_ptr, col_ind, opt(val), Q, K, V);
  bias_checks(d, Q, bias);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Q.device());
  Tensor out = torch::empty_like(Q);
  Tensor row_max, row_sum;
  if (save_stats) {
    row_max = torch::empty({d.m, d.h}, Q.options());
    row_sum = torch::empty({d.m, d.h}, Q.options());
  }
  check_rc(dfgnn_gt_fwd_bias_rect(d.m, d.n_cols, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), edge_val_ptr(val, unit_val), f32(bias), f32(Q),
                             f32(K), f32(V), f32(row_max), f32(row_sum), f32(out), cur_stream()),
           save_stats ? "gt_forward_bias" : "gt_inference_bias");
  if (!save_stats) return {out};
  return {out, row_max, row_sum};
}

// -> {dQ, dK, dV, dbias}, or {dQ, dK, dV} without need_dbias
std::vector<Tensor> gt_bwd_bias(const Tensor &row_ptr, const Tensor &col_ind, const c10::optional<Tensor> &val, const Tensor &bias,
                                const Tensor &col_ptr, const Tensor &row_ind, const Tensor &val_idx, const Tensor &Q,
                                const Tensor &K, const Tensor &V, const Tensor &out, const Tensor &row_max,
                                const Tensor &row_sum, const Tensor &grad, bool unit_val, bool need_dbias) {
  const Dims d = gt_rect_checks(row_ptr, col_ind, opt(val), Q, K, V);
  bias_checks(d, Q, bias);
  csc_rect_checks(d, Q, col_ptr, row_ind, &val_idx, "K / V");
  check_feat3(out, Q, "out");
  check_feat3(grad, Q, "grad");
  row_stats_checks(d, Q, row_max, row_sum);
  check_same_device(Q, {&out, &grad});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Q.device());
  Tensor delta = torch::empty({d.m, d.h}, Q.options());
  Tensor dQ = torch::empty_like(Q), dK = torch::empty_like(K), dV = torch::empty_like(V);
  Tensor dbias;
  if (need_dbias) dbias = torch::empty({d.h, d.nnz}, Q.options());
  check_rc(dfgnn_gt_bwd_bias_rect(d.m, d.n_cols, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), edge_val_ptr(val, unit_val), f32(bias),
                             i32(col_ptr), i32(row_ind), i32(val_idx), f32(Q), f32(K), f32(V), f32(out), f32(row_max),
                             f32(row_sum), f32(grad), f32(delta), f32(dQ), f32(dK), f32(dV), f32(dbias), cur_stream()),
           "gt_backward_bias");
  if (!need_dbias) return {dQ, dK, dV};
  return {dQ, dK, dV, dbias};
}

// ---- the general pair with a per-edge feature vector in keys and values (include/dfgnn.h: dfgnn_gt_fwd_edge / dfgnn_gt_bwd_edge) ----
// E: fp32 [nnz, h, f] in CSR edge order
void edge_feat_checks(const Dims &d, const Tensor &ref, const Tensor &E) {
  check_f32(E, "E");
  TORCH_CHECK(E.dim() == 3 && E.size(0) == d.nnz && E.size(1) == d.h && E.size(2) == d.f, "E must have shape (", d.nnz, ", ",
              d.h, ", ", d.f, "), got ", E.sizes());
  check_same_device(ref, {&E});
}

// save_stats = false: inference (-> {out})
std::vector<Tensor> gt_fwd_edge(const Tensor &row_ptr, const Tensor &col_ind, const c10::optional<Tensor> &val, const Tensor &E,
                                const Tensor &Q, const Tensor &K, const Tensor &V, bool unit_val, bool save_stats) {
  const Dims d = gt_rect_checks(row_ptr, col_ind, opt(val), Q, K, V);
  edge_feat_checks(d, Q, E);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Q.device());
  Tensor out = torch::empty_like(Q);
  Tensor row_max, row_sum;
  if (save_stats) {
    row_max = torch::empty({d.m, d.h}, Q.options());
    row_sum = torch::empty({d.m, d.h}, Q.options());
  }
  check_rc(dfgnn_gt_fwd_edge_rect(d.m, d.n_cols, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), edge_val_ptr(val, unit_val), f32(E), f32(Q),
                             f32(K), f32(V), f32(row_max), f32(row_sum), f32(out), cur_stream()),
           save_stats ? "gt_forward_edge" : "gt_inference_edge");
  if (!save_stats) return {out};
  return {out, row_max, row_sum};
}

// -> {dQ, dK, dV, dE}, or {dQ, dK, dV} without need_dE
std::vector<Tensor> gt_bwd_edge(const Tensor &row_ptr, const Tensor &col_ind, const c10::optional<Tensor> &val, const Tensor &E,
                                const Tensor &col_ptr, const Tensor &row_ind, const Tensor &val_idx, const Tensor &Q,
                                const Tensor &K, const Tensor &V, const Tensor &out, const Tensor &row_max,
                                const Tensor &row_sum, const Tensor &grad, bool unit_val, bool need_dE) {
  const Dims d = gt_rect_checks(row_ptr, col_ind, opt(val), Q, K, V);
  edge_feat_checks(d, Q, E);
  csc_rect_checks(d, Q, col_ptr, row_ind, &val_idx, "K / V");
  check_feat3(out, Q, "out");
  check_feat3(grad, Q, "grad");
  row_stats_checks(d, Q, row_max, row_sum);
  check_same_device(Q, {&out, &grad});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Q.device());
  Tensor delta = torch::empty({d.m, d.h}, Q.options());
  Tensor dQ = torch::empty_like(Q), dK = torch::empty_like(K), dV = torch::empty_like(V);
  Tensor dE;
  if (need_dE) dE = torch::empty_like(E);
  check_rc(dfgnn_gt_bwd_edge_rect(d.m, d.n_cols, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), edge_val_ptr(val, unit_val), f32(E),
                             i32(col_ptr), i32(row_ind), i32(val_idx), f32(Q), f32(K), f32(V), f32(out), f32(row_max),
                             f32(row_sum), f32(grad), f32(delta), f32(dQ), f32(dK), f32(dV), f32(dE), cur_stream()),
           "gt_backward_edge");
  if (!need_dE) return {dQ, dK, dV};
  return {dQ, dK, dV, dE};
}

// ---- the general pair with a per-edge multiplicative gate and an edge-output channel (include/dfgnn.h: dfgnn_gt_fwd_gate / dfgnn_gt_bwd_gate) ----
// E, W, G, dE: fp32 [nnz, h, f] in CSR edge order
void gate_grad_checks(const Dims &d, const Tensor &ref, const Tensor &G) {
  check_f32(G, "G");
  TORCH_CHECK(G.dim() == 3 && G.size(0) == d.nnz && G.size(1) == d.h && G.size(2) == d.f, "G must have shape (", d.nnz, ", ",
              d.h, ", ", d.f, "), got ", G.sizes());
  check_same_device(ref, {&G});
}

// save_stats = false: inference (-> {out}); need_W adds W at the end of either
std::vector<Tensor> gt_fwd_gate(const Tensor &row_ptr, const Tensor &col_ind, const c10::optional<Tensor> &val, const Tensor &E,
                                const Tensor &Q, const Tensor &K, const Tensor &V, bool unit_val, bool save_stats, bool need_W) {
  const Dims d = gt_rect_checks(row_ptr, col_ind, opt(val), Q, K, V);
  edge_feat_checks(d, Q, E);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Q.device());
  Tensor out = torch::empty_like(Q);
  Tensor row_max, row_sum, W;
  if (save_stats) {
    row_max = torch::empty({d.m, d.h}, Q.options());
    row_sum = torch::empty({d.m, d.h}, Q.options());
  }
  if (need_W) W = torch::empty_like(E);
  check_rc(dfgnn_gt_fwd_gate_rect(d.m, d.n_cols, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), edge_val_ptr(val, unit_val), f32(E), f32(Q),
                             f32(K), f32(V), f32(row_max), f32(row_sum), f32(out), f32(W), cur_stream()),
           save_stats ? "gt_forward_gate" : "gt_inference_gate");
  std::vector<Tensor> res = {out};
  if (save_stats) {
    res.push_back(row_max);
    res.push_back(row_sum);
  }
  if (need_W) res.push_back(W);
  return res;
}

// G: the gradient of W, or nothing (zero).  -> {dQ, dK, dV, dE}, or {dQ, dK, dV} without need_dE
std::vector<Tensor> gt_bwd_gate(const Tensor &row_ptr, const Tensor &col_ind, const c10::optional<Tensor> &val, const Tensor &E,
                                const Tensor &col_ptr, const Tensor &row_ind, const Tensor &val_idx, const Tensor &Q,
                                const Tensor &K, const Tensor &V, const Tensor &out, const Tensor &row_max,
                                const Tensor &row_sum, const Tensor &grad, const c10::optional<Tensor> &G, bool unit_val,
                                bool need_dE) {
  const Dims d = gt_rect_checks(row_ptr, col_ind, opt(val), Q, K, V);
  edge_feat_checks(d, Q, E);
  if (G) gate_grad_checks(d, Q, *G);
  csc_rect_checks(d, Q, col_ptr, row_ind, &val_idx, "K / V");
  check_feat3(out, Q, "out");
  check_feat3(grad, Q, "grad");
  row_stats_checks(d, Q, row_max, row_sum);
  check_same_device(Q, {&out, &grad});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Q.device());
  Tensor delta = torch::empty({d.m, d.h}, Q.options());
  Tensor dQ = torch::empty_like(Q), dK = torch::empty_like(K), dV = torch::empty_like(V);
  Tensor dE;
  if (need_dE) dE = torch::empty_like(E);
  check_rc(dfgnn_gt_bwd_gate_rect(d.m, d.n_cols, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), edge_val_ptr(val, unit_val), f32(E),
                             i32(col_ptr), i32(row_ind), i32(val_idx), f32(Q), f32(K), f32(V), f32(out), f32(row_max),
                             f32(row_sum), f32(grad), f32(G), f32(delta), f32(dQ), f32(dK), f32(dV), f32(dE), cur_stream()),
           "gt_backward_gate");
  if (!need_dE) return {dQ, dK, dV};
  return {dQ, dK, dV, dE};
}

// ---- the general pair with typed edges (include/dfgnn.h: dfgnn_gt_fwd_typed / dfgnn_gt_bwd_typed) -----------------------
// etype: int32 [nnz] in CSR edge order; R: fp32 [T, h, f] -> T
int typed_checks(const Dims &d, const Tensor &ref, const Tensor &etype, const Tensor &R) {
  check_i32(etype, "etype");
  TORCH_CHECK(etype.dim() == 1 && etype.size(0) == d.nnz, "etype must have shape (", d.nnz, ",), got ", shape_str(etype));
  check_f32(R, "R");
  TORCH_CHECK(R.dim() == 3 && R.size(0) >= 1 && R.size(1) == d.h && R.size(2) == d.f, "R must have shape (T >= 1, ", d.h, ", ",
              d.f, "), got ", shape_str(R));
  check_same_device(ref, {&etype, &R});
  return (int)R.size(0);
}

// save_stats = false: inference (-> {out})
std::vector<Tensor> gt_fwd_typed(const Tensor &row_ptr, const Tensor &col_ind, const c10::optional<Tensor> &val, const Tensor &etype,
                                 const Tensor &R, const Tensor &Q, const Tensor &K, const Tensor &V, bool unit_val, bool save_stats) {
  const Dims d = gt_rect_checks(row_ptr, col_ind, opt(val), Q, K, V);
  const int T = typed_checks(d, Q, etype, R);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Q.device());
  Tensor out = torch::empty_like(Q);
  Tensor row_max, row_sum;
  if (save_stats) {
    row_max = torch::empty({d.m, d.h}, Q.options());
    row_sum = torch::empty({d.m, d.h}, Q.options());
  }
  check_rc(dfgnn_gt_fwd_typed_rect(d.m, d.n_cols, d.nnz, d.h, d.f, T, i32(row_ptr), i32(col_ind), edge_val_ptr(val, unit_val),
                                   i32(etype), f32(R), f32(Q), f32(K), f32(V), f32(row_max), f32(row_sum), f32(out), cur_stream()),
           save_stats ? "gt_forward_typed" : "gt_inference_typed");
  if (!save_stats) return {out};
  return {out, row_max, row_sum};
}

// -> {dQ, dK, dV, dR}, or {dQ, dK, dV} without need_dR
std::vector<Tensor> gt_bwd_typed(const Tensor &row_ptr, const Tensor &col_ind, const c10::optional<Tensor> &val, const Tensor &etype,
                                 const Tensor &col_ptr, const Tensor &row_ind, const Tensor &val_idx, const Tensor &etype_csc,
                                 const Tensor &R, const Tensor &Q, const Tensor &K, const Tensor &V, const Tensor &out,
                                 const Tensor &row_max, const Tensor &row_sum, const Tensor &grad, bool unit_val, bool need_dR) {
  const Dims d = gt_rect_checks(row_ptr, col_ind, opt(val), Q, K, V);
  const int T = typed_checks(d, Q, etype, R);
  csc_rect_checks(d, Q, col_ptr, row_ind, &val_idx, "K / V");
  check_i32(etype_csc, "etype_csc");
  TORCH_CHECK(etype_csc.dim() == 1 && etype_csc.size(0) == d.nnz, "etype_csc must have shape (", d.nnz, ",), got ",
              shape_str(etype_csc));
  check_feat3(out, Q, "out");
  check_feat3(grad, Q, "grad");
  row_stats_checks(d, Q, row_max, row_sum);
  check_same_device(Q, {&etype_csc, &out, &grad});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Q.device());
  Tensor ws, dR;
  if (need_dR) {
    const int ws_floats = dfgnn_gt_typed_bwd_ws_floats(T, d.h, d.f);
    check_rc(ws_floats < 0 ? ws_floats : 0, "gt_backward_typed");
    ws = torch::empty({(int64_t)ws_floats}, Q.options());
    dR = torch::empty_like(R);
  }
  Tensor delta = torch::empty({d.m, d.h}, Q.options());
  Tensor dQ = torch::empty_like(Q), dK = torch::empty_like(K), dV = torch::empty_like(V);
  check_rc(dfgnn_gt_bwd_typed_rect(d.m, d.n_cols, d.nnz, d.h, d.f, T, i32(row_ptr), i32(col_ind), edge_val_ptr(val, unit_val),
                                   i32(etype), i32(col_ptr), i32(row_ind), i32(val_idx), i32(etype_csc), f32(R), f32(Q), f32(K),
                                   f32(V), f32(out), f32(row_max), f32(row_sum), f32(grad), f32(delta), f32(ws), f32(dQ),
                                   f32(dK), f32(dV), f32(dR), cur_stream()),
           "gt_backward_typed");
  if (!need_dR) return {dQ, dK, dV};
  return {dQ, dK, dV, dR};
}

// ---- the general pair with a typed attention bias (include/dfgnn.h: dfgnn_gt_fwd_tbias / dfgnn_gt_bwd_tbias) -------------
// etype: int32 [nnz] in CSR edge order; B: fp32 [T, h] -> T
int tbias_checks(const Dims &d, const Tensor &ref, const Tensor &etype, const Tensor &B) {
  check_i32(etype, "etype");
  TORCH_CHECK(etype.dim() == 1 && etype.size(0) == d.nnz, "etype must have shape (", d.nnz, ",), got ", shape_str(etype));
  check_f32(B, "B");
  TORCH_CHECK(B.dim() == 2 && B.size(0) >= 1 && B.size(1) == d.h, "B must have shape (T >= 1, ", d.h, "), got ", shape_str(B));
  check_same_device(ref, {&etype, &B});
  return (int)B.size(0);
}

// save_stats = false: inference (-> {out})
std::vector<Tensor> gt_fwd_tbias(const Tensor &row_ptr, const Tensor &col_ind, const c10::optional<Tensor> &val, const Tensor &etype,
                                 const Tensor &B, const Tensor &Q, const Tensor &K, const Tensor &V, bool unit_val, bool save_stats) {
  const Dims d = gt_rect_checks(row_ptr, col_ind, opt(val), Q, K, V);
  const int T = tbias_checks(d, Q, etype, B);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Q.device());
  Tensor out = torch::empty_like(Q);
  Tensor row_max, row_sum;
  if (save_stats) {
    row_max = torch::empty({d.m, d.h}, Q.options());
    row_sum = torch::empty({d.m, d.h}, Q.options());
  }
  check_rc(dfgnn_gt_fwd_tbias_rect(d.m, d.n_cols, d.nnz, d.h, d.f, T, i32(row_ptr), i32(col_ind), edge_val_ptr(val, unit_val),
                                   i32(etype), f32(B), f32(Q), f32(K), f32(V), f32(row_max), f32(row_sum), f32(out), cur_stream()),
           save_stats ? "gt_forward_tbias" : "gt_inference_tbias");
  if (!save_stats) return {out};
  return {out, row_max, row_sum};
}

// -> {dQ, dK, dV, dB}, or {dQ, dK, dV} without need_dB
std::vector<Tensor> gt_bwd_tbias(const Tensor &row_ptr, const Tensor &col_ind, const c10::optional<Tensor> &val, const Tensor &etype,
                                 const Tensor &col_ptr, const Tensor &row_ind, const Tensor &val_idx, const Tensor &etype_csc,
                                 const Tensor &B, const Tensor &Q, const Tensor &K, const Tensor &V, const Tensor &out,
                                 const Tensor &row_max, const Tensor &row_sum, const Tensor &grad, bool unit_val, bool need_dB) {
  const Dims d = gt_rect_checks(row_ptr, col_ind, opt(val), Q, K, V);
  const int T = tbias_checks(d, Q, etype, B);
  csc_rect_checks(d, Q, col_ptr, row_ind, &val_idx, "K / V");
  check_i32(etype_csc, "etype_csc");
  TORCH_CHECK(etype_csc.dim() == 1 && etype_csc.size(0) == d.nnz, "etype_csc must have shape (", d.nnz, ",), got ",
              shape_str(etype_csc));
  check_feat3(out, Q, "out");
  check_feat3(grad, Q, "grad");
  row_stats_checks(d, Q, row_max, row_sum);
  check_same_device(Q, {&etype_csc, &out, &grad});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Q.device());
  Tensor ws, dB;
  if (need_dB) {
    const int ws_floats = dfgnn_gt_tbias_bwd_ws_floats(T, d.h);
    check_rc(ws_floats < 0 ? ws_floats : 0, "gt_backward_tbias");
    ws = torch::empty({(int64_t)ws_floats}, Q.options());
    dB = torch::empty_like(B);
  }
  Tensor delta = torch::empty({d.m, d.h}, Q.options());
  Tensor dQ = torch::empty_like(Q), dK = torch::empty_like(K), dV = torch::empty_like(V);
  check_rc(dfgnn_gt_bwd_tbias_rect(d.m, d.n_cols, d.nnz, d.h, d.f, T, i32(row_ptr), i32(col_ind), edge_val_ptr(val, unit_val),
                                   i32(etype), i32(col_ptr), i32(row_ind), i32(val_idx), i32(etype_csc), f32(B), f32(Q), f32(K),
                                   f32(V), f32(out), f32(row_max), f32(row_sum), f32(grad), f32(delta), f32(ws), f32(dQ),
                                   f32(dK), f32(dV), f32(dB), cur_stream()),
           "gt_backward_tbias");
  if (!need_dB) return {dQ, dK, dV};
  return {dQ, dK, dV, dB};
}

// ---- the attn_edge pair in rank order (include/dfgnn.h: dfgnn_gt_hyper_fwd_ranked / dfgnn_gt_bwd_ranked) ----------------
std::vector<Tensor> gt_hyper_fwd_ranked(const Tensor &row_ptr, const Tensor &col_ind, const Tensor &Q, const Tensor &K,
                                        const Tensor &V, int64_t plan, int64_t meta) {
  const Dims d = gt_checks(row_ptr, col_ind, nullptr, nullptr, Q, K, V);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Q.device());
  Tensor out = torch::empty_like(Q);
  Tensor attn = torch::empty({d.h, d.nnz}, Q.options());
  check_rc(dfgnn_gt_hyper_fwd_ranked(d.m, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), f32(Q), f32(K), f32(V), f32(attn),
                                     f32(out), plan_ptr(plan), plan_ptr(meta), cur_stream()),
           "gt_hyper_forward_ranked");
  return {out, attn};
}

std::vector<Tensor> gt_bwd_ranked(const Tensor &row_ptr, const Tensor &col_ind, const Tensor &Q, const Tensor &K,
                                  const Tensor &V, const Tensor &attn, const Tensor &grad, int64_t plan, int64_t meta) {
  const Dims d = gt_checks(row_ptr, col_ind, nullptr, nullptr, Q, K, V);
  check_feat3(grad, Q, "grad");
  attn_checks(d, Q, attn, "attn_ranked");
  check_same_device(Q, {&grad});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Q.device());
  Tensor dQ = torch::empty_like(Q), dK = torch::empty_like(K), dV = torch::empty_like(V);
  check_rc(dfgnn_gt_bwd_ranked(d.m, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), f32(Q), f32(K), f32(V), f32(attn), f32(grad),
                               f32(dQ), f32(dK), f32(dV), plan_ptr(plan), plan_ptr(meta), cur_stream()),
           "gt_backward_ranked");
  return {dQ, dK, dV};
}

// the edge values of a plan's dense ranges in dense form (dfgnn_plan_dense_weights): fp32[256 m]
Tensor plan_dense_weights(const Tensor &row_ptr, const Tensor &val, int64_t plan, int64_t meta) {
  check_i32(row_ptr, "row_ptr");
  check_f32(val, "val");
  TORCH_CHECK(row_ptr.dim() == 1 && row_ptr.size(0) >= 1, "indptr must be 1-D");
  check_same_device(row_ptr, {&val});
  const int m = (int)row_ptr.size(0) - 1, nnz = (int)val.numel();
  c10::hip::HIPGuardMasqueradingAsCUDA guard(row_ptr.device());
  Tensor w = torch::empty({(int64_t)dfgnn_plan_dense_weights_floats(m)}, val.options());
  check_rc(dfgnn_plan_dense_weights(m, nnz, i32(row_ptr), f32(val), plan_ptr(plan), plan_ptr(meta), f32(w), cur_stream()),
           "plan_dense_weights");
  return w;
}

// What every GAT entry point checks: in_feat, the CSR arrays, the per-node scores [m, h] and (or nullptr) the COO rows
Dims gat_checks(const Tensor &attn_row, const Tensor &attn_col, const Tensor &indptr, const Tensor &indices,
                const Tensor *rows, const Tensor &in_feat) {
  check_f32(attn_row, "attn_row");
  check_f32(attn_col, "attn_col");
  check_f32(in_feat, "in_feat");
  check_i32(indptr, "indptr");
  check_i32(indices, "indices");
  TORCH_CHECK(in_feat.dim() == 3, "in_feat must have shape [nodes, heads, feat], got ", in_feat.sizes());
  const int64_t m = indptr.size(0) - 1, nnz = indices.size(0);
  TORCH_CHECK(attn_row.dim() == 2 && attn_row.size(0) == m && attn_row.size(1) == in_feat.size(1) &&
                  attn_col.sizes() == attn_row.sizes(),
              "attn_row / attn_col must have shape (", m, ", ", in_feat.size(1), "), got ", attn_row.sizes(), " / ",
              attn_col.sizes());
  TORCH_CHECK(in_feat.size(0) == m, "indptr describes ", m, " rows but in_feat has ", in_feat.size(0), " nodes");
  if (rows) {
    check_i32(*rows, "rows");
    check_edges(*rows, nnz, "rows");
  }
  check_same_device(in_feat, {&attn_row, &attn_col, &indptr, &indices, rows});
  return Dims{(int)m, (int)nnz, (int)in_feat.size(1), (int)in_feat.size(2)};
}
// ... of the training pair: the dropout rate and its randoms [nnz, h] (nothing: no dropout)
void drop_checks(const Dims &d, const Tensor &ref, double attn_drop, const c10::optional<Tensor> &edge_mask) {
  TORCH_CHECK(attn_drop >= 0.0 && attn_drop < 1.0, "attn_drop must be in [0, 1), got ", attn_drop);
  if (!edge_mask) return;
  check_f32(*edge_mask, "edge_mask");
  TORCH_CHECK(edge_mask->dim() == 2 && edge_mask->size(0) == d.nnz && edge_mask->size(1) == d.h, "edge_mask must have shape (",
              d.nnz, ", ", d.h, "), got ", edge_mask->sizes());
  check_same_device(ref, {&*edge_mask});
}

// fused_gatconv.cpp:99-119
Tensor gat_hyper_fwd(const Tensor &attn_row, const Tensor &attn_col, const Tensor &indptr, const Tensor &indices,
                     const Tensor &rows, double slope, const Tensor &in_feat, int64_t plan, int64_t meta, bool need_ws) {
  const Dims d = gat_checks(attn_row, attn_col, indptr, indices, &rows, in_feat);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(in_feat.device());
  Tensor out = torch::empty_like(in_feat), ws;
  if (need_ws) ws = torch::empty({d.h, d.nnz}, in_feat.options());
  check_rc(dfgnn_gat_hyper_fwd(d.m, d.nnz, d.h, d.f, i32(indptr), i32(indices), i32(rows), f32(attn_row), f32(attn_col),
                               (float)slope, f32(in_feat), f32(ws), f32(out), plan_ptr(plan), plan_ptr(meta), cur_stream()),
           "gat_inference_hyper");
  return out;
}

// fused_gatconv.cpp:40-61 (use_lds) and :69-90 (global-memory logits)
Tensor gat_softmax_fwd(const Tensor &attn_row, const Tensor &attn_col, const Tensor &indptr, const Tensor &indices,
                       const Tensor &rows, double slope, const Tensor &in_feat, bool use_lds) {
  const Dims d = gat_checks(attn_row, attn_col, indptr, indices, &rows, in_feat);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(in_feat.device());
  Tensor out = torch::empty_like(in_feat);
  Tensor logits = torch::empty({d.h, d.nnz}, in_feat.options());
  auto fn = use_lds ? dfgnn_gat_softmax_fwd : dfgnn_gat_softmax_gm_fwd;
  check_rc(fn(d.m, d.nnz, d.h, d.f, i32(indptr), i32(indices), i32(rows), f32(attn_row), f32(attn_col), (float)slope,
              f32(in_feat), f32(logits), f32(out), cur_stream()),
           use_lds ? "gat_inference_softmax" : "gat_inference_softmax_gm");
  return out;
}

// fused_gatconv.cpp:196-219
Tensor gat_tiling_fwd(const Tensor &attn_row, const Tensor &attn_col, const Tensor &row_ptr, const Tensor &col_ind,
                      double slope, const Tensor &in_feat) {
  const Dims d = gat_checks(attn_row, attn_col, row_ptr, col_ind, nullptr, in_feat);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(in_feat.device());
  Tensor out = torch::empty_like(in_feat);
  check_rc(dfgnn_gat_tiling_fwd(d.m, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), f32(attn_row), f32(attn_col), (float)slope,
                                f32(in_feat), f32(out), cur_stream()),
           "gat_inference_tiling");
  return out;
}

// fused_gatconv.cpp:11-32: the GAT training forward.  edge_mask: the dropout randoms [nnz, h] (undefined: no dropout);
// rows / plan / meta: the COO rows and the block plan when the batch may run on the matrix-core kernels, else undefined / 0
std::vector<Tensor> gat_fwd_train(const Tensor &attn_row, const Tensor &attn_col, const Tensor &row_ptr, const Tensor &col_ind,
                                  const c10::optional<Tensor> &rows, double slope, const Tensor &in_feat,
                                  const c10::optional<Tensor> &edge_mask, double attn_drop, int64_t plan, int64_t meta) {
  const Dims d = gat_checks(attn_row, attn_col, row_ptr, col_ind, opt(rows), in_feat);
  drop_checks(d, in_feat, attn_drop, edge_mask);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(in_feat.device());
  Tensor out = torch::empty_like(in_feat);
  Tensor edge_max = torch::empty({d.m, d.h}, in_feat.options()), edge_sum = torch::empty({d.m, d.h}, in_feat.options());
  check_rc(dfgnn_gat_fwd_train(d.m, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), i32(rows), f32(attn_row), f32(attn_col),
                               (float)slope, f32(in_feat), f32(edge_mask), (float)attn_drop, f32(edge_max), f32(edge_sum),
                               f32(out), plan_ptr(plan), plan_ptr(meta), cur_stream()),
           "gat_forward");
  return {out, edge_max, edge_sum};
}

// fused_gatconv.cpp:291-353
std::vector<Tensor> gat_bwd(double slope, double attn_drop, const Tensor &row_ptr, const Tensor &col_ind,
                            const c10::optional<Tensor> &rows, const Tensor &col_ptr, const Tensor &row_ind, const Tensor &permute,
                            const Tensor &edge_max, const Tensor &edge_sum, const c10::optional<Tensor> &edge_mask,
                            const Tensor &in_feat, const Tensor &attn_row, const Tensor &attn_col, const Tensor &grad,
                            int64_t plan, int64_t meta) {
  const Dims d = gat_checks(attn_row, attn_col, row_ptr, col_ind, opt(rows), in_feat);
  check_i32(col_ptr, "col_ptr");
  check_i32(row_ind, "row_ind");
  check_i32(permute, "permute");
  check_f32(edge_max, "edge_max");
  check_f32(edge_sum, "edge_sum");
  check_f32(grad, "grad");
  TORCH_CHECK(grad.sizes() == in_feat.sizes(), "grad has shape ", grad.sizes(), ", expected ", in_feat.sizes());
  TORCH_CHECK(edge_max.dim() == 2 && edge_max.size(0) == d.m && edge_max.size(1) == d.h && edge_sum.sizes() == edge_max.sizes(),
              "edge_max / edge_sum must have shape (", d.m, ", ", d.h, ")");
  TORCH_CHECK(col_ptr.size(0) == d.m + 1 && row_ind.size(0) == d.nnz && permute.size(0) == d.nnz,
              "col_ptr / row_ind / permute do not match the CSR structure");
  check_same_device(in_feat, {&col_ptr, &row_ind, &permute, &edge_max, &edge_sum, &grad});
  drop_checks(d, in_feat, attn_drop, edge_mask);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(in_feat.device());
  Tensor grad_feat = torch::empty_like(in_feat);
  Tensor grad_row = torch::empty({d.m, d.h}, in_feat.options()), grad_col = torch::empty({d.m, d.h}, in_feat.options());
  Tensor grad_edge = torch::empty({d.h, d.nnz}, in_feat.options());
  check_rc(dfgnn_gat_bwd(d.m, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), i32(rows), i32(col_ptr), i32(row_ind), i32(permute),
                         f32(attn_row), f32(attn_col), (float)slope, f32(in_feat), f32(edge_max), f32(edge_sum), f32(edge_mask),
                         (float)attn_drop, f32(grad), f32(grad_edge), f32(grad_feat), f32(grad_row), f32(grad_col),
                         plan_ptr(plan), plan_ptr(meta), cur_stream()),
           "gat_backward");
  return {grad_feat, grad_row, grad_col};
}

// ---- GATv2 (include/dfgnn.h: dfgnn_gatv2_fwd / dfgnn_gatv2_bwd): any graph, no plan ----------------------------------------
// What both entry points check: X_row / X_col fp32 [nodes, heads, feat] of one shape, attn fp32 [heads, feat], the CSR arrays
Dims gatv2_checks(const Tensor &attn, const Tensor &row_ptr, const Tensor &col_ind, const Tensor &X_row, const Tensor &X_col) {
  check_i32(row_ptr, "row_ptr");
  check_i32(col_ind, "col_ind");
  check_feat3(X_row, X_row, "X_row");
  check_cols_feat(X_col, "X_col", X_row, "X_row");
  check_f32(attn, "attn");
  TORCH_CHECK(attn.dim() == 2 && attn.size(0) == X_row.size(1) && attn.size(1) == X_row.size(2), "attn must have shape (",
              X_row.size(1), ", ", X_row.size(2), "), got ", attn.sizes());
  TORCH_CHECK(row_ptr.dim() == 1 && col_ind.dim() == 1, "indptr / indices must be 1-D");
  TORCH_CHECK(row_ptr.size(0) - 1 == X_row.size(0), "indptr describes ", row_ptr.size(0) - 1, " rows but features have ",
              X_row.size(0), " nodes");
  check_same_device(X_row, {&attn, &row_ptr, &col_ind, &X_col});
  return Dims{(int)X_row.size(0), (int)col_ind.size(0), (int)X_row.size(1), (int)X_row.size(2), (int)X_col.size(0)};
}

// save_stats = false: inference -> {out}; else the training forward -> {out, row_max, row_sum}
std::vector<Tensor> gatv2_fwd(const Tensor &attn, const Tensor &row_ptr, const Tensor &col_ind, double slope, const Tensor &X_row,
                              const Tensor &X_col, bool save_stats) {
  const Dims d = gatv2_checks(attn, row_ptr, col_ind, X_row, X_col);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(X_row.device());
  Tensor out = torch::empty_like(X_row);
  Tensor row_max, row_sum;
  if (save_stats) {
    row_max = torch::empty({d.m, d.h}, X_row.options());
    row_sum = torch::empty({d.m, d.h}, X_row.options());
  }
  check_rc(dfgnn_gatv2_fwd_rect(d.m, d.n_cols, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), f32(attn), (float)slope, f32(X_row), f32(X_col),
                           f32(row_max), f32(row_sum), f32(out), cur_stream()),
           save_stats ? "gatv2_forward" : "gatv2_inference");
  if (!save_stats) return {out};
  return {out, row_max, row_sum};
}

std::vector<Tensor> gatv2_bwd(double slope, const Tensor &row_ptr, const Tensor &col_ind, const Tensor &col_ptr, const Tensor &row_ind,
                              const Tensor &attn, const Tensor &X_row, const Tensor &X_col, const Tensor &out, const Tensor &row_max,
                              const Tensor &row_sum, const Tensor &grad) {
  const Dims d = gatv2_checks(attn, row_ptr, col_ind, X_row, X_col);
  csc_rect_checks(d, X_row, col_ptr, row_ind, nullptr, "X_col");
  check_feat3(out, X_row, "out");
  check_feat3(grad, X_row, "grad");
  row_stats_checks(d, X_row, row_max, row_sum);
  check_same_device(X_row, {&out, &grad});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(X_row.device());
  Tensor dX_row = torch::empty_like(X_row), dX_col = torch::empty_like(X_col);
  if (d.m == 0 && d.n_cols == 0) return {dX_row, dX_col, torch::zeros_like(attn)};  // (nothing to launch: no edge adds to dattn)
  const int ws_floats = dfgnn_gatv2_bwd_ws_floats(d.h, d.f);
  check_rc(ws_floats < 0 ? ws_floats : 0, "gatv2_backward");
  Tensor delta = torch::empty({d.m, d.h}, X_row.options()), ws = torch::empty({(int64_t)ws_floats}, X_row.options());
  Tensor dattn = torch::empty_like(attn);
  check_rc(dfgnn_gatv2_bwd_rect(d.m, d.n_cols, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), i32(col_ptr), i32(row_ind), f32(attn), (float)slope,
                           f32(X_row), f32(X_col), f32(out), f32(row_max), f32(row_sum), f32(grad), f32(delta), f32(ws),
                           f32(dX_row), f32(dX_col), f32(dattn), cur_stream()),
           "gatv2_backward");
  return {dX_row, dX_col, dattn};
}

// ---- AGNN / dot-product attention with tied keys and values (include/dfgnn.h: dfgnn_agnn_fwd / dfgnn_agnn_bwd): any graph ----
// What both entry points check: X_row fp32 [m, heads, feat], X_col fp32 [n_cols, heads, feat], beta fp32 [heads], the CSR arrays
Dims agnn_checks(const Tensor &beta, const Tensor &row_ptr, const Tensor &col_ind, const Tensor &X_row, const Tensor &X_col) {
  check_i32(row_ptr, "row_ptr");
  check_i32(col_ind, "col_ind");
  check_feat3(X_row, X_row, "X_row");
  check_cols_feat(X_col, "X_col", X_row, "X_row");
  check_f32(beta, "beta");
  TORCH_CHECK(beta.dim() == 1 && beta.size(0) == X_row.size(1), "beta must have shape (", X_row.size(1), ",), got ",
              shape_str(beta));
  TORCH_CHECK(row_ptr.dim() == 1 && col_ind.dim() == 1, "indptr / indices must be 1-D");
  TORCH_CHECK(row_ptr.size(0) - 1 == X_row.size(0), "indptr describes ", row_ptr.size(0) - 1, " rows but features have ",
              X_row.size(0), " nodes");
  check_same_device(X_row, {&beta, &row_ptr, &col_ind, &X_col});
  return Dims{(int)X_row.size(0), (int)col_ind.size(0), (int)X_row.size(1), (int)X_row.size(2), (int)X_col.size(0)};
}

// save_stats = false: inference -> {out}; else the training forward -> {out, row_max, row_sum}
std::vector<Tensor> agnn_fwd(const Tensor &row_ptr, const Tensor &col_ind, const Tensor &beta, bool cosine, const Tensor &X_row,
                             const Tensor &X_col, bool save_stats) {
  const Dims d = agnn_checks(beta, row_ptr, col_ind, X_row, X_col);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(X_row.device());
  Tensor out = torch::empty_like(X_row);
  Tensor row_max, row_sum;
  if (save_stats) {
    row_max = torch::empty({d.m, d.h}, X_row.options());
    row_sum = torch::empty({d.m, d.h}, X_row.options());
  }
  check_rc(dfgnn_agnn_fwd_rect(d.m, d.n_cols, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), f32(beta), cosine ? 1 : 0, f32(X_row),
                               f32(X_col), f32(row_max), f32(row_sum), f32(out), cur_stream()),
           save_stats ? "agnn_forward" : "agnn_inference");
  if (!save_stats) return {out};
  return {out, row_max, row_sum};
}

// -> {dX_row, dX_col} and, with need_dbeta, dbeta [h]: the column sum of the rows' shares the CSR pass writes
std::vector<Tensor> agnn_bwd(const Tensor &row_ptr, const Tensor &col_ind, const Tensor &col_ptr, const Tensor &row_ind,
                             const Tensor &beta, bool cosine, const Tensor &X_row, const Tensor &X_col, const Tensor &out,
                             const Tensor &row_max, const Tensor &row_sum, const Tensor &grad, bool need_dbeta) {
  const Dims d = agnn_checks(beta, row_ptr, col_ind, X_row, X_col);
  csc_rect_checks(d, X_row, col_ptr, row_ind, nullptr, "X_col");
  check_feat3(out, X_row, "out");
  check_feat3(grad, X_row, "grad");
  row_stats_checks(d, X_row, row_max, row_sum);
  check_same_device(X_row, {&out, &grad});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(X_row.device());
  Tensor dX_row = torch::empty_like(X_row), dX_col = torch::empty_like(X_col);
  Tensor delta = torch::empty({d.m, d.h}, X_row.options()), dbeta_rows;
  if (need_dbeta) dbeta_rows = torch::empty({d.m, d.h}, X_row.options());
  check_rc(dfgnn_agnn_bwd_rect(d.m, d.n_cols, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), i32(col_ptr), i32(row_ind), f32(beta),
                               cosine ? 1 : 0, f32(X_row), f32(X_col), f32(out), f32(row_max), f32(row_sum), f32(grad),
                               f32(delta), f32(dX_row), f32(dX_col), f32(dbeta_rows), cur_stream()),
           "agnn_backward");
  if (!need_dbeta) return {dX_row, dX_col};
  return {dX_row, dX_col, dbeta_rows.sum(0)};
}

// ---- GATv2 with a per-edge feature vector inside the LeakyReLU (include/dfgnn.h: dfgnn_gatv2_fwd_edge / dfgnn_gatv2_bwd_edge) ----
// a dtype as Python prints it, so that a dtype error reads the same through either transport (_binding_util._family)
std::string py_dtype(const Tensor &t) {
  switch (t.scalar_type()) {
    case torch::kInt32: return "torch.int32";
    case torch::kInt64: return "torch.int64";
    case torch::kFloat32: return "torch.float32";
    case torch::kFloat64: return "torch.float64";
    case torch::kFloat16: return "torch.float16";
    case torch::kBFloat16: return "torch.bfloat16";
    default: return std::string("torch.") + c10::toString(t.scalar_type());
  }
}
// the CSR arrays' dtype, named and worded as the ctypes transport does (check_csr); everything else: gatv2_checks
void gatv2_edge_csr_dtype(const Tensor &row_ptr, const Tensor &col_ind) {
  TORCH_CHECK(!row_ptr.is_cuda() || !row_ptr.is_contiguous() || row_ptr.scalar_type() == torch::kInt32,
              "indptr must have dtype torch.int32, got ", py_dtype(row_ptr));
  TORCH_CHECK(!col_ind.is_cuda() || !col_ind.is_contiguous() || col_ind.scalar_type() == torch::kInt32,
              "indices must have dtype torch.int32, got ", py_dtype(col_ind));
}
// E: fp32 [nnz, h, f] in CSR edge order
void gatv2_edge_feat_checks(const Dims &d, const Tensor &ref, const Tensor &E) {
  check_cuda_contig(E, "E");
  TORCH_CHECK(E.scalar_type() == torch::kFloat32, "E must have dtype torch.float32, got ", py_dtype(E));
  TORCH_CHECK(E.dim() == 3 && E.size(0) == d.nnz && E.size(1) == d.h && E.size(2) == d.f, "E must have shape (", d.nnz, ", ",
              d.h, ", ", d.f, "), got ", shape_str(E));
  check_same_device(ref, {&E});
}

// save_stats = false: inference -> {out}; else the training forward -> {out, row_max, row_sum}
std::vector<Tensor> gatv2_fwd_edge(const Tensor &attn, const Tensor &row_ptr, const Tensor &col_ind, double slope,
                                   const Tensor &X_row, const Tensor &X_col, const Tensor &E, bool save_stats) {
  gatv2_edge_csr_dtype(row_ptr, col_ind);
  const Dims d = gatv2_checks(attn, row_ptr, col_ind, X_row, X_col);
  gatv2_edge_feat_checks(d, X_row, E);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(X_row.device());
  Tensor out = torch::empty_like(X_row);
  Tensor row_max, row_sum;
  if (save_stats) {
    row_max = torch::empty({d.m, d.h}, X_row.options());
    row_sum = torch::empty({d.m, d.h}, X_row.options());
  }
  check_rc(dfgnn_gatv2_fwd_edge_rect(d.m, d.n_cols, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), f32(attn), (float)slope, f32(X_row),
                                     f32(X_col), f32(E), f32(row_max), f32(row_sum), f32(out), cur_stream()),
           save_stats ? "gatv2_forward_edge" : "gatv2_inference_edge");
  if (!save_stats) return {out};
  return {out, row_max, row_sum};
}

// -> {dX_row, dX_col, dattn, dE}, or {dX_row, dX_col, dattn} without want_dE
std::vector<Tensor> gatv2_bwd_edge(double slope, const Tensor &row_ptr, const Tensor &col_ind, const Tensor &col_ptr,
                                   const Tensor &row_ind, const Tensor &val_idx, const Tensor &attn, const Tensor &X_row,
                                   const Tensor &X_col, const Tensor &E, const Tensor &out, const Tensor &row_max,
                                   const Tensor &row_sum, const Tensor &grad, bool want_dE) {
  gatv2_edge_csr_dtype(row_ptr, col_ind);
  const Dims d = gatv2_checks(attn, row_ptr, col_ind, X_row, X_col);
  gatv2_edge_feat_checks(d, X_row, E);
  csc_rect_checks(d, X_row, col_ptr, row_ind, &val_idx, "X_col");
  check_feat3(out, X_row, "out");
  check_feat3(grad, X_row, "grad");
  row_stats_checks(d, X_row, row_max, row_sum);
  check_same_device(X_row, {&out, &grad});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(X_row.device());
  Tensor dX_row = torch::empty_like(X_row), dX_col = torch::empty_like(X_col);
  Tensor dE;
  if (want_dE) dE = torch::empty_like(E);
  std::vector<Tensor> res;
  if (d.m == 0 && d.n_cols == 0) {  // (nothing to launch: no edge adds to dattn)
    res = {dX_row, dX_col, torch::zeros_like(attn)};
  } else {
    const int ws_floats = dfgnn_gatv2_bwd_ws_floats(d.h, d.f);
    check_rc(ws_floats < 0 ? ws_floats : 0, "gatv2_backward_edge");
    Tensor delta = torch::empty({d.m, d.h}, X_row.options()), ws = torch::empty({(int64_t)ws_floats}, X_row.options());
    Tensor dattn = torch::empty_like(attn);
    check_rc(dfgnn_gatv2_bwd_edge_rect(d.m, d.n_cols, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), i32(col_ptr), i32(row_ind),
                                       i32(val_idx), f32(attn), (float)slope, f32(X_row), f32(X_col), f32(E), f32(out), f32(row_max),
                                       f32(row_sum), f32(grad), f32(delta), f32(ws), f32(dX_row), f32(dX_col), f32(dattn), f32(dE),
                                       cur_stream()),
             "gatv2_backward_edge");
    res = {dX_row, dX_col, dattn};
  }
  if (want_dE) res.push_back(dE);
  return res;
}

// ---- GatedGCN (include/dfgnn.h: dfgnn_gatedgcn_fwd / dfgnn_gatedgcn_bwd): any graph -----------------------------------------
// What both entry points check: X_row fp32 [m, heads, feat], X_col and V fp32 [n_cols, heads, feat], the CSR arrays
Dims gatedgcn_checks(const Tensor &row_ptr, const Tensor &col_ind, const Tensor &X_row, const Tensor &X_col, const Tensor &V) {
  gatv2_edge_csr_dtype(row_ptr, col_ind);
  check_i32(row_ptr, "row_ptr");
  check_i32(col_ind, "col_ind");
  check_feat3(X_row, X_row, "X_row");
  check_cols_feat(X_col, "X_col", X_row, "X_row");
  check_f32(V, "V");
  TORCH_CHECK(V.sizes() == X_col.sizes(), "V must have shape ", shape_str(X_col), " like X_col, got ", shape_str(V));
  TORCH_CHECK(row_ptr.dim() == 1 && col_ind.dim() == 1, "indptr / indices must be 1-D");
  TORCH_CHECK(row_ptr.size(0) - 1 == X_row.size(0), "indptr describes ", row_ptr.size(0) - 1, " rows but features have ",
              X_row.size(0), " nodes");
  check_same_device(X_row, {&row_ptr, &col_ind, &X_col, &V});
  return Dims{(int)X_row.size(0), (int)col_ind.size(0), (int)X_row.size(1), (int)X_row.size(2), (int)X_col.size(0)};
}
// E, G: fp32 [nnz, h, f] in CSR edge order; worded as the ctypes transport does (_binding_util._family)
void gatedgcn_edge_checks(const Dims &d, const Tensor &ref, const Tensor &T, const char *name) {
  check_cuda_contig(T, name);
  TORCH_CHECK(T.scalar_type() == torch::kFloat32, name, " must have dtype torch.float32, got ", py_dtype(T));
  TORCH_CHECK(T.dim() == 3 && T.size(0) == d.nnz && T.size(1) == d.h && T.size(2) == d.f, name, " must have shape (", d.nnz,
              ", ", d.h, ", ", d.f, "), got ", shape_str(T));
  check_same_device(ref, {&T});
}

// -> {out}, then den with save_den (training), then Z with need_Z
std::vector<Tensor> gatedgcn_fwd(const Tensor &row_ptr, const Tensor &col_ind, const Tensor &X_row, const Tensor &X_col,
                                 const Tensor &V, const c10::optional<Tensor> &E, bool normalize, double eps, bool save_den,
                                 bool need_Z) {
  const Dims d = gatedgcn_checks(row_ptr, col_ind, X_row, X_col, V);
  if (E) gatedgcn_edge_checks(d, X_row, *E, "E");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(X_row.device());
  Tensor out = torch::empty_like(X_row), den, Z;
  if (save_den) den = torch::empty_like(X_row);
  if (need_Z) Z = torch::empty({d.nnz, d.h, d.f}, X_row.options());
  check_rc(dfgnn_gatedgcn_fwd_rect(d.m, d.n_cols, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), f32(X_row), f32(X_col), f32(V),
                                   f32(E), normalize ? 1 : 0, (float)eps, f32(den), f32(out), f32(Z), cur_stream()),
           save_den ? "gatedgcn_forward" : "gatedgcn_inference");
  std::vector<Tensor> res = {out};
  if (save_den) res.push_back(den);
  if (need_Z) res.push_back(Z);
  return res;
}

// out, den: the forward's (read with normalize only).  G: the gradient of Z, or nothing (zero).
// -> {dX_row, dX_col, dV, dE}, or {dX_row, dX_col, dV} without need_dE
std::vector<Tensor> gatedgcn_bwd(const Tensor &row_ptr, const Tensor &col_ind, const Tensor &col_ptr, const Tensor &row_ind,
                                 const Tensor &val_idx, const Tensor &X_row, const Tensor &X_col, const Tensor &V,
                                 const c10::optional<Tensor> &E, bool normalize, double eps, const c10::optional<Tensor> &out,
                                 const c10::optional<Tensor> &den, const Tensor &grad, const c10::optional<Tensor> &G,
                                 bool need_dE) {
  const Dims d = gatedgcn_checks(row_ptr, col_ind, X_row, X_col, V);
  if (E) gatedgcn_edge_checks(d, X_row, *E, "E");
  if (G) gatedgcn_edge_checks(d, X_row, *G, "G");
  csc_rect_checks(d, X_row, col_ptr, row_ind, &val_idx, "X_col");
  check_feat3(grad, X_row, "grad");
  check_same_device(X_row, {&grad});
  TORCH_CHECK(!normalize || (out && den), "out and den of the forward are required with normalize");
  if (normalize) {
    check_feat3(*out, X_row, "out");
    check_feat3(*den, X_row, "den");
    check_same_device(X_row, {&*out, &*den});
  }
  c10::hip::HIPGuardMasqueradingAsCUDA guard(X_row.device());
  Tensor dX_row = torch::empty_like(X_row), dX_col = torch::empty_like(X_col), dV = torch::empty_like(V);
  Tensor dE, ws;
  if (need_dE) dE = torch::empty({d.nnz, d.h, d.f}, X_row.options());
  if (normalize) ws = torch::empty_like(X_row);  // s_i = dO_i / (den_i + eps), CSR pass -> CSC pass
  check_rc(dfgnn_gatedgcn_bwd_rect(d.m, d.n_cols, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), i32(col_ptr), i32(row_ind),
                                   i32(val_idx), f32(X_row), f32(X_col), f32(V), f32(E), normalize ? 1 : 0, (float)eps,
                                   normalize ? f32(out) : nullptr, normalize ? f32(den) : nullptr, f32(grad), f32(G),
                                   f32(dX_row), f32(dX_col), f32(dV), f32(dE), f32(ws), cur_stream()),
           "gatedgcn_backward");
  if (!need_dE) return {dX_row, dX_col, dV};
  return {dX_row, dX_col, dV, dE};
}

// ---- GAT for any graph with an optional per-edge attention term (include/dfgnn.h: dfgnn_gat_fwd_edge / dfgnn_gat_bwd_edge) ----
// an fp32 array of shape (a, b) or (a, b, c), with the text of the ctypes transport's check (_binding_util._family)
void check_shape_f32(const Tensor &t, const char *name, std::initializer_list<int64_t> shape) {
  check_cuda_contig(t, name);
  TORCH_CHECK(t.scalar_type() == torch::kFloat32, name, " must have dtype torch.float32, got ", py_dtype(t));
  if (t.sizes() == c10::IntArrayRef(shape.begin(), shape.size())) return;
  std::string want = "(";
  for (auto it = shape.begin(); it != shape.end(); ++it) want += (it != shape.begin() ? ", " : "") + std::to_string(*it);
  TORCH_CHECK(false, name, " must have shape ", want, "), got ", shape_str(t));
}
// What both entry points check: X fp32 [n_cols, heads, feat] (the sources), the CSR arrays of the m rows, the per-node scores
// attn_row [m, h] / attn_col [n_cols, h], the optional score [h, nnz] and the dropout rate with its optional randoms
Dims gat_edge_checks(const Tensor &attn_row, const Tensor &attn_col, const Tensor &row_ptr, const Tensor &col_ind,
                     const c10::optional<Tensor> &score, const Tensor &X, double attn_drop,
                     const c10::optional<Tensor> &edge_mask) {
  check_f32(X, "X");
  TORCH_CHECK(X.dim() == 3, "X must have shape [nodes, heads, feat], got ", shape_str(X));
  check_i32(row_ptr, "indptr");
  check_i32(col_ind, "indices");
  TORCH_CHECK(row_ptr.dim() == 1 && col_ind.dim() == 1, "indptr / indices must be 1-D");
  TORCH_CHECK(row_ptr.size(0) >= 1, "indptr must have at least one entry");
  const Dims d{(int)(row_ptr.size(0) - 1), (int)col_ind.size(0), (int)X.size(1), (int)X.size(2), (int)X.size(0)};
  check_shape_f32(attn_row, "attn_row", {d.m, d.h});
  check_shape_f32(attn_col, "attn_col", {d.n_cols, d.h});
  if (score) check_shape_f32(*score, "score", {d.h, d.nnz});
  check_same_device(X, {&row_ptr, &col_ind, &attn_row, &attn_col, opt(score)});
  TORCH_CHECK(attn_drop >= 0.0 && attn_drop < 1.0, "attn_drop must be in [0, 1), got ", attn_drop);
  if (edge_mask) {
    check_shape_f32(*edge_mask, "edge_mask", {d.nnz, d.h});
    check_same_device(X, {&*edge_mask});
  }
  return d;
}

// save_stats = false: inference -> {out}; else the training forward -> {out, edge_max, edge_sum}
std::vector<Tensor> gat_fwd_edge(const Tensor &attn_row, const Tensor &attn_col, const Tensor &row_ptr, const Tensor &col_ind,
                                 double slope, const c10::optional<Tensor> &score, const Tensor &X,
                                 const c10::optional<Tensor> &edge_mask, double attn_drop, bool save_stats) {
  const Dims d = gat_edge_checks(attn_row, attn_col, row_ptr, col_ind, score, X, attn_drop, edge_mask);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(X.device());
  Tensor out = torch::empty({d.m, d.h, d.f}, X.options());
  Tensor edge_max, edge_sum;
  if (save_stats) {
    edge_max = torch::empty({d.m, d.h}, X.options());
    edge_sum = torch::empty({d.m, d.h}, X.options());
  }
  check_rc(dfgnn_gat_fwd_edge_rect(d.m, d.n_cols, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), f32(attn_row), f32(attn_col),
                                   (float)slope, f32(score), f32(X), f32(edge_mask), (float)attn_drop, f32(edge_max),
                                   f32(edge_sum), f32(out), cur_stream()),
           save_stats ? "gat_forward_edge" : "gat_inference_edge");
  if (!save_stats) return {out};
  return {out, edge_max, edge_sum};
}

// -> {grad_feat, grad_attn_row, grad_attn_col, grad_score}, or the first three without want_grad_score
std::vector<Tensor> gat_bwd_edge(double slope, double attn_drop, const Tensor &row_ptr, const Tensor &col_ind,
                                 const Tensor &col_ptr, const Tensor &row_ind, const Tensor &val_idx, const Tensor &attn_row,
                                 const Tensor &attn_col, const c10::optional<Tensor> &score, const Tensor &X,
                                 const c10::optional<Tensor> &edge_mask, const Tensor &edge_max, const Tensor &edge_sum,
                                 const Tensor &grad, bool want_grad_score) {
  const Dims d = gat_edge_checks(attn_row, attn_col, row_ptr, col_ind, score, X, attn_drop, edge_mask);
  csc_rect_checks(d, X, col_ptr, row_ind, &val_idx, "X");
  check_shape_f32(grad, "grad", {d.m, d.h, d.f});
  check_shape_f32(edge_max, "edge_max", {d.m, d.h});
  check_shape_f32(edge_sum, "edge_sum", {d.m, d.h});
  check_same_device(X, {&grad, &edge_max, &edge_sum});
  c10::hip::HIPGuardMasqueradingAsCUDA guard(X.device());
  Tensor delta = torch::empty({d.m, d.h}, X.options());
  Tensor grad_feat = torch::empty_like(X);
  Tensor grad_row = torch::empty({d.m, d.h}, X.options()), grad_col = torch::empty({d.n_cols, d.h}, X.options());
  Tensor grad_score;
  if (want_grad_score) grad_score = torch::empty({d.h, d.nnz}, X.options());
  check_rc(dfgnn_gat_bwd_edge_rect(d.m, d.n_cols, d.nnz, d.h, d.f, i32(row_ptr), i32(col_ind), i32(col_ptr), i32(row_ind),
                                   i32(val_idx), f32(attn_row), f32(attn_col), (float)slope, f32(score), f32(X), f32(edge_mask),
                                   (float)attn_drop, f32(edge_max), f32(edge_sum), f32(grad), f32(delta),
                                   f32(grad_feat), f32(grad_row), f32(grad_col), f32(grad_score), cur_stream()),
           "gat_backward_edge");
  if (!want_grad_score) return {grad_feat, grad_row, grad_col};
  return {grad_feat, grad_row, grad_col, grad_score};
}

// fused_gtconv.cpp:244-276 (tiling), :174-242 (csr, csr_gm), :316-389 (softmax, softmax_gm): the GT inference variants that
// take CSR (+ the COO rows for the two-kernel forms).  which: 0 tiling, 1 csr, 2 csr_gm, 3 softmax, 4 softmax_gm
Tensor gt_variant_fwd(int64_t which, const Tensor &indptr, const Tensor &indices, const c10::optional<Tensor> &rows, const Tensor &val,
                      const Tensor &Q, const Tensor &K, const Tensor &V, bool unit_val) {
  TORCH_CHECK(which >= 0 && which <= 4, "unknown GT variant ", which);
  TORCH_CHECK(which < 3 || rows.has_value(), "rows is required by the softmax variants");
  const Dims d = gt_checks(indptr, indices, which >= 3 ? &*rows : nullptr, &val, Q, K, V);
  const int m = d.m, nnz = d.nnz, h = d.h, f = d.f;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(Q.device());
  Tensor out = torch::empty_like(Q), logits;
  if (which != 0) logits = torch::empty({h, nnz}, Q.options());
  const int *ip = i32(indptr), *ci = i32(indices);
  const float *q = f32(Q), *k = f32(K), *v = f32(V);
  float *lg = f32(logits), *o = f32(out);
  // (the two-kernel 'softmax' forms multiply the values in as they are; the others take NULL for all ones)
  const float *vl = (which >= 3 || !unit_val) ? f32(val) : nullptr;
  int rc = 0;
  switch (which) {
    case 0: rc = dfgnn_gt_tiling_fwd(m, nnz, h, f, ip, ci, f32(val), q, k, v, o, cur_stream()); break;
    case 1: rc = dfgnn_gt_csr_fwd(m, nnz, h, f, ip, ci, vl, q, k, v, lg, o, cur_stream()); break;
    case 2: rc = dfgnn_gt_csr_gm_fwd(m, nnz, h, f, ip, ci, vl, q, k, v, lg, o, cur_stream()); break;
    case 3: rc = dfgnn_gt_softmax_fwd(m, nnz, h, f, ip, ci, i32(rows), vl, q, k, v, lg, o, cur_stream()); break;
    default: rc = dfgnn_gt_softmax_gm_fwd(m, nnz, h, f, ip, ci, i32(rows), vl, q, k, v, lg, o, cur_stream()); break;
  }
  static const char *names[] = {"gt_tiling_inference", "gt_csr_inference", "gt_csr_gm_inference", "gt_softmax_inference",
                                "gt_softmax_gm_inference"};
  check_rc(rc, names[which]);
  return out;
}

// dfgnn_plan_build: -> (plan buffer int32[dfgnn_plan_ints], its 12 header words); synchronises the current stream once
std::pair<Tensor, std::vector<int64_t>> plan_build(const Tensor &indptr, const Tensor &indices, int64_t f) {
  check_i32(indptr, "indptr");
  check_i32(indices, "indices");
  TORCH_CHECK(indptr.dim() == 1 && indices.dim() == 1 && indptr.size(0) >= 1, "indptr / indices must be 1-D");
  check_same_device(indptr, {&indices});
  const int m = (int)indptr.size(0) - 1, nnz = (int)indices.size(0);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(indptr.device());
  Tensor buf = torch::empty({(int64_t)dfgnn_plan_ints(m, nnz)}, indptr.options());
  int meta[12];
  check_rc(dfgnn_plan_build(m, nnz, (int)f, i32(indptr), i32(indices), i32(buf), meta, cur_stream()), "dfgnn_plan_build");
  return {buf, std::vector<int64_t>(meta, meta + 12)};
}

// dfgnn_preprocess_hyper: COO -> (row_ptr, col_ind, rows, edge_order[, col_ptr, row_ind, val_idx]) (DFGNN/layers/util.py:82-142)
// num_cols: the column extent of a rectangular graph (num_nodes then counts its rows); < 0: square
std::vector<Tensor> preprocess_hyper(const Tensor &src, const Tensor &dst, int64_t num_nodes, bool csc, int64_t num_cols) {
  TORCH_CHECK(src.is_cuda() && dst.is_cuda(), "src / dst must be on CUDA");
  TORCH_CHECK(src.scalar_type() == dst.scalar_type() && (src.scalar_type() == torch::kInt64 || src.scalar_type() == torch::kInt32),
              "src / dst must both be int64 or int32, got ", src.scalar_type(), " / ", dst.scalar_type());
  TORCH_CHECK(src.dim() == 1 && src.sizes() == dst.sizes(), "src / dst must be 1-D and of equal length, got ", src.sizes(), " / ",
              dst.sizes());
  check_same_device(src, {&dst});
  const Tensor s = src.contiguous(), t = dst.contiguous();
  const int64_t nnz = s.numel();
  if (num_cols < 0) num_cols = num_nodes;
  TORCH_CHECK(nnz < (int64_t(1) << 31) && num_nodes < (int64_t(1) << 31) && num_nodes >= 0 && num_cols < (int64_t(1) << 31),
              "graphs with 2^31 or more nodes / edges are not supported (int32 index arrays)");
  const int m = (int)num_nodes, n_cols = (int)num_cols;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(s.device());
  const auto i32o = s.options().dtype(torch::kInt32);
  std::vector<Tensor> outs = {torch::empty({m + 1}, i32o), torch::empty({nnz}, i32o), torch::empty({nnz}, i32o), torch::empty({nnz}, i32o)};
  if (csc) outs.insert(outs.end(), {torch::empty({n_cols + 1}, i32o), torch::empty({nnz}, i32o), torch::empty({nnz}, i32o)});
  size_t ws_bytes = 0;
  check_rc(dfgnn_preprocess_ws_bytes_rect(m, n_cols, (int)nnz, &ws_bytes), "dfgnn_preprocess_hyper");
  Tensor ws = torch::empty({(int64_t)ws_bytes}, s.options().dtype(torch::kUInt8));
  const Tensor none;
  check_rc(dfgnn_preprocess_hyper_rect(m, n_cols, (int)nnz, s.data_ptr(), t.data_ptr(), s.scalar_type() == torch::kInt64 ? 1 : 0, i32(outs[0]),
                                  i32(outs[1]), i32(outs[2]), i32(outs[3]), i32(csc ? outs[4] : none), i32(csc ? outs[5] : none),
                                  i32(csc ? outs[6] : none), ws.data_ptr(), ws_bytes, cur_stream()),
           "dfgnn_preprocess_hyper");
  return outs;
}

}  // namespace

PYBIND11_MODULE(_dfgnn_ext, m) {
  m.doc() = "torch C++ binding of libdfgnn.so (include/dfgnn.h); see df-gnn_amd/fused_gtconv.py / fused_gatconv.py";
  // compile-time constants of THIS extension (not the library's answers: comparing those with the library would compare
  // the library with itself): dfgnn_native.ext() takes the extension only if both equal the library's
  m.def("abi_version", [] { return (int)DFGNN_ABI_VERSION; });
  m.def("build_id", [] { return std::string(DFGNN_SRC_HASH); });
  m.def("plan_desc_off", [](int64_t m_, int64_t nnz) { return (int64_t)dfgnn_plan_desc_off((int)m_, (int)nnz); },
        "int32 offset of the dense ranges' descriptors in a plan buffer");
  m.def("gt_hyper_fwd", &gt_hyper_fwd, "fused GT conv 'hyper' forward (inference / training)");
  m.def("gt_bwd", &gt_bwd, "fused GT conv backward");
  m.def("gt_hyper_fwd_stats", &gt_hyper_fwd_stats, "fused GT conv 'hyper' training forward, row statistics instead of attn_edge");
  m.def("gt_bwd_stats", &gt_bwd_stats, "fused GT conv backward from the row statistics");
  m.def("gt_fwd_rowstats", &gt_fwd_rowstats, "fused GT conv training forward of any graph, row statistics instead of attn_edge");
  m.def("gt_bwd_rowstats", &gt_bwd_rowstats, "fused GT conv backward of any graph from the forward's output and row statistics");
  m.def("gt_fwd_bias", &gt_fwd_bias, "fused GT conv forward of any graph with a per-edge additive attention bias");
  m.def("gt_bwd_bias", &gt_bwd_bias, "fused GT conv backward of any graph with a per-edge additive attention bias");
  m.def("gt_fwd_edge", &gt_fwd_edge, "fused GT conv forward of any graph with a per-edge feature vector in keys and values");
  m.def("gt_bwd_edge", &gt_bwd_edge, "fused GT conv backward of any graph with a per-edge feature vector in keys and values");
  m.def("gt_fwd_gate", &gt_fwd_gate, "fused GT conv forward of any graph with a per-edge multiplicative gate and an edge output");
  m.def("gt_bwd_gate", &gt_bwd_gate, "fused GT conv backward of any graph with a per-edge multiplicative gate and an edge output");
  m.def("gt_fwd_typed", &gt_fwd_typed, "fused GT conv forward of any graph with typed edges: key / value vectors from a table");
  m.def("gt_bwd_typed", &gt_bwd_typed, "fused GT conv backward of any graph with typed edges: key / value vectors from a table");
  m.def("gt_fwd_tbias", &gt_fwd_tbias, "fused GT conv forward of any graph with a typed attention bias: scalars from a table");
  m.def("gt_bwd_tbias", &gt_bwd_tbias, "fused GT conv backward of any graph with a typed attention bias: scalars from a table");
  m.def("gt_hyper_fwd_ranked", &gt_hyper_fwd_ranked, "fused GT conv 'hyper' training forward, attention values in rank order");
  m.def("gt_bwd_ranked", &gt_bwd_ranked, "fused GT conv backward from rank-ordered attention values");
  m.def("plan_dense_weights", &plan_dense_weights, "edge values of a plan's dense ranges in dense form (dfgnn_plan_dense_weights)");
  m.def("gat_hyper_fwd", &gat_hyper_fwd, "fused GAT conv 'hyper' inference");
  m.def("gat_softmax_fwd", &gat_softmax_fwd, "fused GAT conv 'softmax' / 'softmax_gm' inference");
  m.def("gat_tiling_fwd", &gat_tiling_fwd, "fused GAT conv 'tiling' inference");
  m.def("gat_fwd_train", &gat_fwd_train, "fused GAT conv training forward (row statistics, attention dropout)");
  m.def("gat_bwd", &gat_bwd, "fused GAT conv backward");
  m.def("gatv2_fwd", &gatv2_fwd, "fused GATv2 conv forward of any graph (inference, or training with row statistics)");
  m.def("gatv2_bwd", &gatv2_bwd, "fused GATv2 conv backward of any graph from the forward's output and row statistics");
  m.def("agnn_fwd", &agnn_fwd, "fused AGNN / dot-product conv forward of any graph, keys = values (inference, or training with row statistics)");
  m.def("agnn_bwd", &agnn_bwd, "fused AGNN / dot-product conv backward of any graph from the forward's output and row statistics");
  m.def("gatv2_fwd_edge", &gatv2_fwd_edge, "fused GATv2 conv forward of any graph with a per-edge feature vector inside the LeakyReLU");
  m.def("gatv2_bwd_edge", &gatv2_bwd_edge, "fused GATv2 conv backward of any graph with a per-edge feature vector inside the LeakyReLU");
  m.def("gat_fwd_edge", &gat_fwd_edge, "fused GAT forward of any graph with an optional per-edge attention term (inference, or training with statistics)");
  m.def("gat_bwd_edge", &gat_bwd_edge, "fused GAT backward of any graph from the forward's row statistics");
  m.def("gatedgcn_fwd", &gatedgcn_fwd, "fused GatedGCN conv forward of any graph (inference, or training with den; optional edge output)");
  m.def("gatedgcn_bwd", &gatedgcn_bwd, "fused GatedGCN conv backward of any graph from the forward's out and den");
  m.def("gt_variant_fwd", &gt_variant_fwd, "fused GT conv inference: tiling / csr / csr_gm / softmax / softmax_gm");
  m.def("plan_build", &plan_build, "block plan of a CSR structure (dfgnn_plan_build)");
  m.def("preprocess_hyper", &preprocess_hyper, "COO -> CSR / COO rows / CSC on the GPU (dfgnn_preprocess_hyper)");
}
