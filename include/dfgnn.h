/*
 * dfgnn.h -- C ABI of the MI355X (gfx950) fused attention-GNN convolution library (libdfgnn.so).
 *
 * One entry point per live function of the reference's two extension modules
 * (`fused_gtconv`, `fused_gatconv`).  Plain pointers and sizes only: no torch types, no
 * allocation, no host synchronisation inside (every call is graph-capturable); the caller
 * owns all buffers (device memory) and passes the HIP stream to launch on.
 *
 * Common conventions (reference: DFGNN/src/fused_gtconv/fused_gtconv_hyper.cu:679-691)
 *   m        number of nodes  (= row_ptr length - 1)
 *   nnz      number of edges  (= col_ind length)
 *   h, f     heads, per-head feature width; features are fp32 [m, h, f] row-major, contiguous
 *   row_ptr  int32[m+1]  CSR row pointers        col_ind int32[nnz] CSR column ids
 *   rows     int32[nnz]  sorted COO row ids (the COO half of the "hyper" CSR+COO format:
 *                        rows[e] = row of CSR edge e); required wherever it appears
 *   val      fp32[nnz]   edge values multiplied into the GT logits; NULL means all ones
 *   attn_edge / grad_edge  fp32[h, nnz], head-major, CSR edge order
 *   stream   hipStream_t (passed as void*), NULL = the legacy default stream
 *
 * Return value: 0 on success; a positive value is the hipError_t of the failed launch; a
 * negative value is one of the DFGNN_E_* argument errors below.  dfgnn_error_string() decodes
 * both.  Zero-sized problems (m == 0) succeed without launching.
 *
 * All functions compute, per head, for every row i with CSR neighbours j (duplicates kept):
 *   P_e = softmax_j(s_e),  out[i,h,:] = sum_e P_e * V[j,h,:],  empty row -> 0
 * with s_e = val_e * <Q[i,h,:],K[j,h,:]> (GT) or LeakyReLU(attn_row[i,h] + attn_col[j,h]) (GAT).
 */
#ifndef DFGNN_H_
#define DFGNN_H_

#ifdef __cplusplus
extern "C" {
#endif

#define DFGNN_ABI_VERSION 11

#define DFGNN_E_BADARG (-1)      /* negative size / NULL required pointer                      */
#define DFGNN_E_UNSUPPORTED (-2) /* feature width outside the compiled range (f > 1024, or     */
                                 /* f % 4 != 0 with f > 256)                                   */

typedef void *dfgnn_stream_t; /* hipStream_t */

int dfgnn_abi_version(void);
const char *dfgnn_error_string(int code);
/* 16 hex digits: sha256 of the library's sources (csrc Makefile list, in that order) at build time -- lets a
 * caller detect a stale libdfgnn.so whose ABI number still matches. */
const char *dfgnn_build_id(void);

/* ---- block plan (optional, MI355X-specific; no counterpart in the reference) --------------------
 * A batch of small graphs (DGL GraphDataLoader, DFGNN/script/test/test_batch_graph.py:67-71) is a
 * block-diagonal adjacency: each member graph is a contiguous node range whose edges stay inside it.
 * dfgnn_plan_build finds those closed ranges on the GPU and marks the ones whose feature rows
 * (f floats per node and head) plus per-edge scratch fit one CU's 160 KB LDS; the 'hyper' entry points
 * that accept a plan then run one workgroup per range with K/V (GAT: X) resident in LDS, and cut
 * everything else into 16-row chunks for the general kernels.  Results are identical with or
 * without a plan.  The plan depends on the graph structure and on f only; build it once per batch
 * (it belongs to preprocessing, like the reference's preprocess_Hyper, DFGNN/layers/util.py:82-100).
 * Ranges that are dense (>= 1 edge per 32 node pairs), have at most 255 nodes, f in {8, 16, 32, 64, 128} and no
 * duplicate edges are additionally marked for the matrix-core kernels, which the GT
 * forward / backward use for them when val == NULL (unit edge values): masked dense attention on MFMA with
 * fp32-equivalent arithmetic (operands as fp16 hi + lo halves under power-of-two scales, fp32 accumulation:
 * ~3 x 2^-24 relative error per product, that of an fp32 FMA chain).
 *   plan       device buffer of dfgnn_plan_ints(m, nnz) int32 (lists of ranges, build scratch and, for the
 *              matrix-core kernels, 2 bytes per edge -- its row and column within its dense range -- and two edge
 *              bitmaps of 32 bytes per node: the out- and the in-neighbours of a node within its dense range; over
 *              the build scratch, from int32 offset dfgnn_plan_desc_off(m, nnz), one 16-byte descriptor per dense range in the order
 *              of the range list: n0, n1 | flags, row_ptr[n0], row_ptr[n1] - row_ptr[n0] -- what a matrix-core kernel
 *              reads of its range before anything else)
 *   meta_host  host buffer of 12 int32 filled on return: num_fit, num_spill, max_fit_nodes,
 *              max_fit_edges, m, nnz, f, lds_budget, num_edge_global, num_dense, num_dense_wide (dense ranges of
 *              more than 128 nodes), coords_offset (int32 offset of the per-edge coordinates in `plan`)
 * dfgnn_plan_build synchronises `stream` (it copies the 12 header words back); nothing else in this
 * library does. */
size_t dfgnn_plan_ints(int m, int nnz);
int dfgnn_plan_desc_off(int m, int nnz);
/* 1 if the entry points below would use a plan with this host header for (m, nnz, h, f), else 0 (they then take the
 * general kernels, same results): the header must have been built for the same m, nnz, f; graphs with fewer than 8 edges
 * per row on average and feature matrices of 4 GiB or more (m h f 4 >= 2^32: the plan kernels address a feature row
 * with 32-bit byte offsets) do not use it.  Host-only, no GPU call. */
int dfgnn_plan_applies(int m, int nnz, int h, int f, const int *plan_meta);
int dfgnn_plan_build(int m, int nnz, int f, const int *row_ptr, const int *col_ind, int *plan,
                     int *meta_host, dfgnn_stream_t stream);

/* ---- graph preprocessing on the GPU -----------------------------------------------------------------
 * COO edge list -> the arrays of the reference's preprocess_Hyper / preprocess_Hyper_fw_bw
 * (DFGNN/layers/util.py:82-100, 116-142: A.csr(), torch.sort(A.row), dglsp.from_csr(...).csc()), which the
 * reference counts inside a training epoch (DFGNN/script/train/train_batch_graph_timing.py:115-143).
 *   src, dst    node ids of the nnz edges (row = src, column = dst, DFGNN/layers/util.py:53-56); int64 when
 *               idx64 != 0 (DGL's default idtype), else int32; ids are clamped to [0, m)
 *   row_ptr int32[m+1], col_ind int32[nnz], rows int32[nnz]: CSR = stable sort by row (COO order kept inside a
 *               row), rows = the sorted row ids
 *   edge_order  int32[nnz]: COO position of each CSR slot (A.csr()'s value indices: val = A.val[edge_order])
 *   col_ptr int32[m+1], row_ind int32[nnz], val_idx int32[nnz]: CSC = stable sort of the CSR list by column,
 *               val_idx = CSR slot of each CSC entry; pass all three as NULL to skip the CSC half
 *   ws          device workspace of dfgnn_preprocess_ws_bytes(m, nnz) bytes
 * No host synchronisation, no allocation.  Two rocPRIM radix sorts over the ceil(log2 m) low key bits + three
 * small kernels. */
size_t dfgnn_preprocess_ws_bytes(int m, int nnz);
int dfgnn_preprocess_hyper(int m, int nnz, const void *src, const void *dst, int idx64, int *row_ptr,
                           int *col_ind, int *rows, int *edge_order, int *col_ptr, int *row_ind,
                           int *val_idx, void *ws, size_t ws_bytes, dfgnn_stream_t stream);
/* The same for a RECTANGULAR graph of m rows and n_cols columns (a neighbour-sampled block, cross-attention): src ids are
 * clamped to [0, m), dst ids to [0, n_cols); the row sort runs over the ceil(log2 m) low key bits, the column sort over
 * ceil(log2 n_cols).  Extents:  row_ptr int32[m+1];  col_ptr int32[n_cols+1];  col_ind, rows, edge_order, row_ind, val_idx
 * int32[nnz] as above.  ws: dfgnn_preprocess_ws_bytes_rect(m, n_cols, nnz, &bytes) bytes -- the larger of
 * dfgnn_preprocess_ws_bytes(m, nnz) and dfgnn_preprocess_ws_bytes(n_cols, nnz); it returns 0 and writes *bytes (host), or a
 * DFGNN_E_* code (a negative extent or bytes == NULL: BADARG).  nnz > 0 with m == 0 or n_cols == 0: DFGNN_E_BADARG.
 * dfgnn_preprocess_hyper is this call with n_cols = m. */
int dfgnn_preprocess_ws_bytes_rect(int m, int n_cols, int nnz, size_t *bytes);
int dfgnn_preprocess_hyper_rect(int m, int n_cols, int nnz, const void *src, const void *dst, int idx64, int *row_ptr,
                                int *col_ind, int *rows, int *edge_order, int *col_ptr, int *row_ind, int *val_idx,
                                void *ws, size_t ws_bytes, dfgnn_stream_t stream);

/* ---- GT (graph transformer) ------------------------------------------------------------------
 * replaces gt_hyper_inference  (DFGNN/src/fused_gtconv/fused_gtconv.cpp:278-314,
 *                               fused_gtconv_hyper.cu:679-725) when attn_edge == NULL, and
 *          gt_hyper_forward    (fused_gtconv.cpp:79-116, fused_gtconv_hyper.cu:727-760)
 *          when attn_edge != NULL (training forward: also writes the normalised attention).
 * plan / plan_meta: device plan + its 12 host header words from dfgnn_plan_build, or NULL/NULL.
 * edge_ws: scratch fp32[h, nnz], needed only for inference (attn_edge == NULL) with a plan whose
 *          meta[8] > 0 (ranges whose per-edge values do not fit LDS next to their rows); else NULL. */
int dfgnn_gt_hyper_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                       const int *rows, const float *val, const float *Q, const float *K,
                       const float *V, float *attn_edge, float *edge_ws, float *out,
                       const int *plan, const int *plan_meta, dfgnn_stream_t stream);

/* replaces gt_backward (fused_gtconv.cpp:125-172, fused_gtconv_backward.cu:193-265).
 * col_ptr int32[m+1], row_ind int32[nnz], val_idx int32[nnz] (CSR slot of each CSC entry).
 * grad_edge is caller-provided scratch fp32[h, nnz] (the reference allocates it inside); with a
 * plan, ranges that run LDS-resident keep dS on chip and leave their part of grad_edge untouched.
 * dQ, dK, dV are fully written (no pre-zeroing needed).  plan / plan_meta as in dfgnn_gt_hyper_fwd. */
int dfgnn_gt_bwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                 const int *rows, const float *val, const int *col_ptr, const int *row_ind,
                 const int *val_idx, const float *Q, const float *K, const float *V,
                 const float *attn_edge, const float *grad_out, float *grad_edge, float *dQ,
                 float *dK, float *dV, const int *plan, const int *plan_meta,
                 dfgnn_stream_t stream);

/* The statistics-saving form of the training pair above: what FusedGTFunction_hyper (DFGNN/operators/fused_gtconv.py:
 * 79-158) needs from its forward is enough to rebuild the attention in the backward, not the attention itself.  Instead
 * of attn_edge[h, nnz] (written by gt_hyper_forward, fused_gtconv_hyper.cu:146-149, read back by gt_backward,
 * fused_gtconv_backward.cu:132-136: 8 h nnz bytes through HBM) the forward saves, per (row, head), the logit maximum and
 * the sum of exponentials -- row_max, row_sum: fp32[m, h]; an empty row has row_max = -1e38, row_sum = 0 -- and the
 * backward recomputes P_e = exp(s_e - row_max) / row_sum with one more Q K^T product on the matrix cores.
 * Only for batches that the matrix-core kernels cover completely: dfgnn_gt_stats_applies(m, nnz, h, f, plan_meta) == 1
 * (host-only; every range of the plan dense, nothing spilled); otherwise both calls return DFGNN_E_UNSUPPORTED and the
 * caller uses dfgnn_gt_hyper_fwd / dfgnn_gt_bwd.  The sparse structure reaches these kernels through the plan's edge
 * bitmaps alone: rows, CSC arrays, grad_edge are not needed.
 * Edge values (the reference's `attn * val`, fused_gtconv_hyper.cu:88-90): `weights` = NULL for unit values, else the
 * values in the dense form of dfgnn_plan_dense_weights below (built once per (plan, val), e.g. per batch of a dataset
 * whose edge weights do not change): s_e = val_e <Q_i, K_j> in the forward, d s_e / d <Q_i, K_j> = val_e in the backward.
 * row_max = row_sum = NULL in the forward: nothing is saved (inference with edge values on the matrix cores).
 * Results equal the attn_edge form's (same arithmetic for out; dQ, dK, dV to fp32 rounding). */
int dfgnn_gt_stats_applies(int m, int nnz, int h, int f, const int *plan_meta);
int dfgnn_gt_hyper_fwd_stats(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *weights,
                             const float *Q, const float *K, const float *V, float *row_max, float *row_sum, float *out,
                             const int *plan, const int *plan_meta, dfgnn_stream_t stream);
int dfgnn_gt_bwd_stats(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *weights,
                       const float *Q, const float *K, const float *V, const float *row_max, const float *row_sum,
                       const float *grad_out, float *dQ, float *dK, float *dV, const int *plan, const int *plan_meta,
                       dfgnn_stream_t stream);
/* The attn_edge pair with the attention values in RANK order (one head, unit edge values, dfgnn_gt_stats_applies == 1).
 * attn_edge[h, nnz] between gt_hyper_forward and gt_backward is internal to FusedGTFunction_hyper
 * (DFGNN/operators/fused_gtconv.py:79-158): all the pair needs is that both sides agree on an order.  Here the value of
 * row i's k-th edge BY INCREASING COLUMN is stored at attn_ranked[row_ptr[i] + k] (fp32[nnz]): the forward then finds an
 * edge's slot from the plan's bitmap (the number of set bits before it) instead of loading the edge list and building a
 * position map, and the backward is dfgnn_gt_bwd's matrix-core kernel reading the plan's rank-ordered coordinates.  For
 * rows whose columns are already increasing attn_ranked == attn_edge.  Results equal dfgnn_gt_hyper_fwd / dfgnn_gt_bwd
 * (same arithmetic).  Other shapes: DFGNN_E_UNSUPPORTED. */
int dfgnn_gt_hyper_fwd_ranked(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *Q,
                              const float *K, const float *V, float *attn_ranked, float *out, const int *plan,
                              const int *plan_meta, dfgnn_stream_t stream);
int dfgnn_gt_bwd_ranked(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *Q,
                        const float *K, const float *V, const float *attn_ranked, const float *grad_out, float *dQ,
                        float *dK, float *dV, const int *plan, const int *plan_meta, dfgnn_stream_t stream);

/* The statistics-saving training pair for ANY graph (csrc/gt_train.hip): no plan, no degree limit, any f -- full graphs,
 * batches with a sparse, oversized or spilled range, low-degree batches; everything the dense pair above returns
 * DFGNN_E_UNSUPPORTED for.  Replaces what FusedGTFunction_hyper (DFGNN/operators/fused_gtconv.py:79-158) keeps between
 * forward and backward: instead of attn_edge[h, nnz] (gt_hyper_forward, fused_gtconv_hyper.cu:146-149) and the
 * grad_edge[h, nnz] scratch of gt_backward (fused_gtconv_backward.cu:40-191) -- 8 h nnz bytes alive per layer -- the
 * forward saves row_max, row_sum: fp32[m, h] (conventions as above: an empty row has out = 0, row_max = -1e38,
 * row_sum = 0) and the backward, given the forward's `out`, rebuilds each edge from rows it gathers anyway:
 *   delta_i = <grad_out_i, out_i>,  P_e = exp(val_e <Q_i, K_j> - row_max_i) / row_sum_i,
 *   dS_e = P_e (<grad_out_i, V_j> - delta_i),  dQ_i = sum dS_e val_e K_j,  dK_j = sum dS_e val_e Q_i,  dV_j = sum P_e grad_out_i
 * in a CSR pass (delta, dQ; one sweep per row) and a CSC pass (dK, dV).
 *   val      fp32[nnz], CSR order, NULL = unit values (then val_idx is not read and may be NULL)
 *   delta    caller scratch fp32[m, h], written by the CSR pass and read by the CSC pass
 *   row_max = row_sum = NULL in the forward: nothing is saved (inference; same result as dfgnn_gt_tiling_fwd)
 * dQ, dK, dV are written in full (an empty row / column gives zeros; no pre-zeroing, no atomics: the sums are
 * deterministic).  Graphs with fewer than 8 edges per row on average run a lane group per row, others a wave per row. */
int dfgnn_gt_fwd_rowstats(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                          const float *Q, const float *K, const float *V, float *row_max, float *row_sum, float *out,
                          dfgnn_stream_t stream);
int dfgnn_gt_bwd_rowstats(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                          const int *col_ptr, const int *row_ind, const int *val_idx, const float *Q, const float *K,
                          const float *V, const float *out, const float *row_max, const float *row_sum,
                          const float *grad_out, float *delta, float *dQ, float *dK, float *dV, dfgnn_stream_t stream);
/* RECTANGULAR graphs.  The four any-graph pairs -- the one above, its two variants below and GATv2 -- each have *_rect
 * entries for a graph of m rows (queries, outputs) and n_cols columns (keys, values): what a neighbour-sampled block, a
 * bipartite graph or cross-attention onto virtual nodes hands a layer as (x_src, x_dst).  Leading extents:
 *   m          Q, out, grad_out, dQ            (GATv2: X_row, dX_row, out, grad_out)
 *   [m, h]     row_max, row_sum, delta
 *   n_cols     K, V, dK, dV                    (GATv2: X_col, dX_col)
 *   m + 1      row_ptr
 *   n_cols + 1 col_ptr
 *   unchanged  the per-edge arrays: col_ind, val, bias[h, nnz], E[nnz, h, f], row_ind, val_idx
 * col_ind[e] < n_cols and row_ind[t] < m are the caller's contract (as col_ind < m is for the square entries): the kernels
 * gather by these ids without a check.  Everything else -- arithmetic, conventions, return codes -- is that of the square
 * entry, which IS the *_rect entry with n_cols = m (same kernels, same grids, same bits).  Additionally:
 *   DFGNN_E_BADARG       a negative extent; nnz > 0 with m == 0 or n_cols == 0 (an edge needs a row and a column)
 *   DFGNN_E_UNSUPPORTED  h > 65535 or f outside the compiled range, as for the square entries (feature rows are addressed
 *                        with 64-bit offsets: extent x h x f itself has no limit below the int32 extents)
 * Degenerate extents launch no empty grid: m == 0 with n_cols > 0 -- the forward has nothing to write, the backward writes
 * dK = dV = 0 in full (GATv2: dX_col = 0, dattn = 0); n_cols == 0 (then nnz == 0) -- out = 0, row_max = -1e38, row_sum = 0,
 * dQ = 0.  The arrays of an empty side may be NULL.
 * Each pass picks its form by the average degree of what it walks: forward and CSR pass a lane group per row when
 * nnz < 8 m, the CSC pass a lane group per column when nnz < 8 n_cols (a fanout-10 block: a wave per row, a lane group
 * per column). */
int dfgnn_gt_fwd_rowstats_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                               const float *val, const float *Q, const float *K, const float *V, float *row_max,
                               float *row_sum, float *out, dfgnn_stream_t stream);
int dfgnn_gt_bwd_rowstats_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                               const float *val, const int *col_ptr, const int *row_ind, const int *val_idx, const float *Q,
                               const float *K, const float *V, const float *out, const float *row_max, const float *row_sum,
                               const float *grad_out, float *delta, float *dQ, float *dK, float *dV, dfgnn_stream_t stream);

/* The pair above with a per-edge, per-head ADDITIVE attention bias (csrc/gt_bias_train.hip): any graph, no plan, any f.
 *   s_e = val_e <Q_i, K_j> + bias[h, e],  P_e = exp(s_e - row_max_i) / row_sum_i,  out_i = sum_e P_e V_j
 *   delta_i = <grad_out_i, out_i>,  dS_e = P_e (<grad_out_i, V_j> - delta_i)
 *   dQ_i = sum dS_e val_e K_j,  dK_j = sum dS_e val_e Q_i,  dV_j = sum P_e grad_out_i,  dbias[h, e] = dS_e
 * (Graphormer's spatial / edge encodings, GraphGPS / GRIT-style attention, relative positional and edge-type biases.)
 *   bias     fp32[h, nnz] in CSR edge order (the layout of attn_edge); required when nnz > 0.  -inf masks an edge: P_e = 0,
 *            dbias_e = 0, nothing added to any sum; a (row, head) whose edges are all masked is an empty row (out = 0,
 *            row_max = -1e38, row_sum = 0, dQ = 0).  No output holds a NaN or an inf.  +inf and NaN in bias are the
 *            caller's error
 *   dbias    fp32[h, nnz], every slot written by plain stores (no pre-zeroing), or NULL: the bias needs no gradient and
 *            nothing of size h nnz is written
 *   val      fp32[nnz], CSR order, NULL = unit values
 *   val_idx  required when nnz > 0 (also for unit values): the CSC pass finds an entry's bias through it
 *   row_max = row_sum = NULL in the forward: nothing is saved (inference)
 * Everything else as dfgnn_gt_fwd_rowstats / dfgnn_gt_bwd_rowstats: delta is caller scratch fp32[m, h]; dQ, dK, dV are
 * written in full; no atomics, the sums are deterministic; the same two forms by average degree. */
int dfgnn_gt_fwd_bias(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                      const float *bias, const float *Q, const float *K, const float *V, float *row_max, float *row_sum,
                      float *out, dfgnn_stream_t stream);
int dfgnn_gt_bwd_bias(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                      const float *bias, const int *col_ptr, const int *row_ind, const int *val_idx, const float *Q,
                      const float *K, const float *V, const float *out, const float *row_max, const float *row_sum,
                      const float *grad_out, float *delta, float *dQ, float *dK, float *dV, float *dbias,
                      dfgnn_stream_t stream);
/* ... for an m x n_cols graph (extents: see dfgnn_gt_fwd_rowstats_rect) */
int dfgnn_gt_fwd_bias_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                           const float *bias, const float *Q, const float *K, const float *V, float *row_max,
                           float *row_sum, float *out, dfgnn_stream_t stream);
int dfgnn_gt_bwd_bias_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                           const float *bias, const int *col_ptr, const int *row_ind, const int *val_idx, const float *Q,
                           const float *K, const float *V, const float *out, const float *row_max, const float *row_sum,
                           const float *grad_out, float *delta, float *dQ, float *dK, float *dV, float *dbias,
                           dfgnn_stream_t stream);

/* The general statistics pair with a per-edge FEATURE VECTOR added to keys and values (csrc/gt_edge_train.hip): any graph,
 * no plan, any f.  Edge e = (i, j) carries E_e in R^f per head; one E serves key and value (PyG's TransformerConv(edge_dim),
 * Shaw-style relative position vectors, the edge channel of GPS / GRIT-type models):
 *   k~_e = K_j + E_e,  v~_e = V_j + E_e
 *   s_e = val_e <Q_i, k~_e>,  P_e = exp(s_e - row_max_i) / row_sum_i,  out_i = sum_e P_e v~_e
 *   delta_i = <grad_out_i, out_i>,  dS_e = P_e (<grad_out_i, v~_e> - delta_i)
 *   dQ_i = sum dS_e val_e k~_e,  dK_j = sum dS_e val_e Q_i,  dV_j = sum P_e grad_out_i
 *   dE_e = dS_e val_e Q_i + P_e grad_out_i
 *   E        fp32[nnz, h, f] in CSR edge order (the feature layout with the edge in place of the node: the row of
 *            (edge e, head) starts at (e h + head) f); required when nnz > 0.  Duplicate edges each have their own row
 *   dE       fp32[nnz, h, f], every slot written by plain stores (no pre-zeroing), or NULL: E needs no gradient and nothing
 *            of size nnz h f is written
 *   val      fp32[nnz], CSR order, NULL = unit values
 *   val_idx  required when nnz > 0 (also for unit values): the CSC pass finds an entry's E row through it
 *   row_max = row_sum = NULL in the forward: nothing is saved (inference)
 * An empty row has out = 0, row_max = -1e38, row_sum = 0, dQ = 0.  Everything else as dfgnn_gt_fwd_rowstats /
 * dfgnn_gt_bwd_rowstats: delta is caller scratch fp32[m, h]; dQ, dK, dV are written in full; no atomics, the sums are
 * deterministic; the same two forms by average degree; nothing allocates or synchronises (capturable in a HIP graph). */
int dfgnn_gt_fwd_edge(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                      const float *E, const float *Q, const float *K, const float *V, float *row_max, float *row_sum,
                      float *out, dfgnn_stream_t stream);
int dfgnn_gt_bwd_edge(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                      const float *E, const int *col_ptr, const int *row_ind, const int *val_idx, const float *Q,
                      const float *K, const float *V, const float *out, const float *row_max, const float *row_sum,
                      const float *grad_out, float *delta, float *dQ, float *dK, float *dV, float *dE,
                      dfgnn_stream_t stream);
/* ... for an m x n_cols graph (extents: see dfgnn_gt_fwd_rowstats_rect) */
int dfgnn_gt_fwd_edge_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                           const float *E, const float *Q, const float *K, const float *V, float *row_max, float *row_sum,
                           float *out, dfgnn_stream_t stream);
int dfgnn_gt_bwd_edge_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                           const float *E, const int *col_ptr, const int *row_ind, const int *val_idx, const float *Q,
                           const float *K, const float *V, const float *out, const float *row_max, const float *row_sum,
                           const float *grad_out, float *delta, float *dQ, float *dK, float *dV, float *dE,
                           dfgnn_stream_t stream);

/* The general statistics pair with a per-edge MULTIPLICATIVE GATE on the keys and an EDGE-OUTPUT channel
 * (csrc/gt_gate_train.hip): any graph, no plan, any f.  Edge e = (i, j) carries E_e in R^f per head, which scales the key
 * dimension by dimension; the per-dimension products are returned as the next layer's edge features (the Graph Transformer
 * layer with edge features of Dwivedi & Bresson, SAN, the GT variants of GraphGPS-type stacks):
 *   ke_e = K_j (.) E_e                       (formed first, in every pass alike)
 *   s_e = val_e <Q_i, ke_e>,  W_e[d] = val_e Q_i[d] ke_e[d],  P_e = exp(s_e - row_max_i) / row_sum_i,  out_i = sum_e P_e V_j
 *   delta_i = <grad_out_i, out_i>,  dS_e = P_e (<grad_out_i, V_j> - delta_i),  g_e[d] = dS_e + G_e[d]
 *   dQ_i[d] = sum val_e g_e[d] ke_e[d],  dK_j[d] = sum val_e g_e[d] Q_i[d] E_e[d],  dV_j = sum P_e grad_out_i
 *   dE_e[d] = val_e g_e[d] Q_i[d] K_j[d]
 * The caller applies the 1/sqrt(f) scale to Q; there is NO clamp on the logit.
 *   E        fp32[nnz, h, f] in CSR edge order (the layout of dfgnn_gt_fwd_edge's E: the row of (edge e, head) starts at
 *            (e h + head) f); required when nnz > 0.  Duplicate edges each have their own row
 *   W        fp32[nnz, h, f], every slot written by plain stores, or NULL: the forward writes nothing of size nnz h f
 *   G        fp32[nnz, h, f], the gradient of the loss with respect to W -- a second gradient stream next to grad_out, read
 *            by both backward passes (the CSC pass through val_idx) -- or NULL = zero: nothing of it is read, and the
 *            results equal those of G = zeros
 *   dE       fp32[nnz, h, f], every slot written by plain stores (no pre-zeroing), or NULL: E needs no gradient and nothing
 *            of size nnz h f is written
 *   val      fp32[nnz], CSR order, NULL = unit values
 *   val_idx  required when nnz > 0 (also for unit values): the CSC pass finds an entry's E and G rows through it
 *   row_max = row_sum = NULL in the forward: nothing is saved (inference)
 * ke = K (.) E is formed before the dot product, which is the routine of dfgnn_gt_fwd_rowstats: with E all ones, W = NULL and
 * G = NULL, out, row_max, row_sum, dQ, dK and dV are those of dfgnn_gt_fwd_rowstats / dfgnn_gt_bwd_rowstats bit for bit.
 * The float4 paths need f % 4 == 0 and 16-byte aligned feature arrays, E, W, G and dE included; otherwise the scalar layouts
 * run (f <= 256).  An empty row has out = 0, row_max = -1e38, row_sum = 0, dQ = 0; an empty column dK = dV = 0.  Everything
 * else as dfgnn_gt_fwd_edge / dfgnn_gt_bwd_edge: delta is caller scratch fp32[m, h]; every output is written in full; no
 * atomics, the sums are deterministic; the same two forms by average degree; the same size limits and DFGNN_E_* codes;
 * nothing allocates or synchronises (capturable in a HIP graph). */
int dfgnn_gt_fwd_gate(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                      const float *E, const float *Q, const float *K, const float *V, float *row_max, float *row_sum,
                      float *out, float *W, dfgnn_stream_t stream);
int dfgnn_gt_bwd_gate(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                      const float *E, const int *col_ptr, const int *row_ind, const int *val_idx, const float *Q,
                      const float *K, const float *V, const float *out, const float *row_max, const float *row_sum,
                      const float *grad_out, const float *G, float *delta, float *dQ, float *dK, float *dV, float *dE,
                      dfgnn_stream_t stream);
/* ... for an m x n_cols graph (extents: see dfgnn_gt_fwd_rowstats_rect) */
int dfgnn_gt_fwd_gate_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                           const float *E, const float *Q, const float *K, const float *V, float *row_max, float *row_sum,
                           float *out, float *W, dfgnn_stream_t stream);
int dfgnn_gt_bwd_gate_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                           const float *E, const int *col_ptr, const int *row_ind, const int *val_idx, const float *Q,
                           const float *K, const float *V, const float *out, const float *row_max, const float *row_sum,
                           const float *grad_out, const float *G, float *delta, float *dQ, float *dK, float *dV, float *dE,
                           dfgnn_stream_t stream);

/* The general statistics pair with TYPED edges (csrc/gt_typed_train.hip): any graph, no plan, any f.  The vector an edge
 * adds to key and value is a row of a small table R[T, h, f], chosen by the edge's type (Shaw-style relative positions,
 * RGAT / HGT-style relation vectors, bucketed distances, bond types).  With t = etype[e]:
 *   k~_e = K_j + R_t,  v~_e = V_j + R_t,  s_e, P_e, out_i, delta_i, dS_e, dQ_i, dK_j, dV_j as in dfgnn_gt_*_edge
 *   dR_t = sum_{e : etype[e] = t} (dS_e val_e Q_i + P_e grad_out_i)
 * i.e. the edge pair on E = R[etype] with dR = index_add(dE, etype) -- out, the statistics, dQ, dK, dV are the edge pair's
 * to the bit -- but an edge costs 4 bytes of type instead of 4 h f bytes of E, and nothing of size nnz h f is read or written.
 *   T          number of types, >= 1
 *   etype      int32[nnz] in CSR edge order, 0 <= etype < T (the caller's contract: not checked); duplicate edges each
 *              carry their own type.  Required when nnz > 0
 *   etype_csc  int32[nnz], the same types in CSC entry order: etype_csc[t] = etype[val_idx[t]].  Graph data, made once per
 *              graph by the caller; the CSC pass streams it.  Required by the backward when nnz > 0
 *   R          fp32[T, h, f]: the row of (type t, head) starts at (t h + head) f.  Required when nnz > 0
 *   val        fp32[nnz], CSR order, NULL = unit values
 *   val_idx    read only when val != NULL
 *   dR         fp32[T, h, f], written in full (a type without an edge: zeros; m == 0 or nnz == 0: all zeros), or NULL: the
 *              table is frozen, the CSR pass is the plain one with the edge pair's grid, any T, and ws is not used
 *   ws         caller scratch of dfgnn_gt_typed_bwd_ws_floats(T, h, f) floats, 16-byte aligned; required when dR != NULL.
 *              The CSR pass then runs a bounded number of persistent workgroups per head, each wave summing into a table
 *              [T, f] of its own in LDS; a workgroup stores one partial per head to ws and a reduction in the same call
 *              adds the partials in a fixed order.  No atomics: two calls give the same bits
 *   row_max = row_sum = NULL in the forward: nothing is saved (inference)
 * dfgnn_gt_typed_bwd_ws_floats: > 0 = the number of floats (independent of m and nnz); < 0 = a DFGNN_E_* code: BADARG for
 * T < 1 or a negative size; UNSUPPORTED for h > 65535, for T f > 8192 (the LDS tables: 64 types at f = 128, 512 at f = 16)
 * or a size that does not fit an int.  dfgnn_gt_bwd_typed with dR != NULL answers the same code before any launch.
 * An empty row has out = 0, row_max = -1e38, row_sum = 0, dQ = 0.  Everything else as dfgnn_gt_fwd_edge / dfgnn_gt_bwd_edge;
 * the _rect entries take an m x n_cols graph (extents: see dfgnn_gt_fwd_rowstats_rect) and the square ones are these with
 * n_cols = m.  Nothing allocates or synchronises (capturable in a HIP graph).  With tables above 64 KB (T f > 4096) the first
 * backward with dR of a process, per device and lane layout, raises the kernel's dynamic-LDS limit (hipFuncSetAttribute): run
 * the step once before capturing it, as a warm-up does. */
int dfgnn_gt_typed_bwd_ws_floats(int T, int h, int f);
int dfgnn_gt_fwd_typed(int m, int nnz, int h, int f, int T, const int *row_ptr, const int *col_ind, const float *val,
                       const int *etype, const float *R, const float *Q, const float *K, const float *V, float *row_max,
                       float *row_sum, float *out, dfgnn_stream_t stream);
int dfgnn_gt_bwd_typed(int m, int nnz, int h, int f, int T, const int *row_ptr, const int *col_ind, const float *val,
                       const int *etype, const int *col_ptr, const int *row_ind, const int *val_idx, const int *etype_csc,
                       const float *R, const float *Q, const float *K, const float *V, const float *out,
                       const float *row_max, const float *row_sum, const float *grad_out, float *delta, float *ws, float *dQ,
                       float *dK, float *dV, float *dR, dfgnn_stream_t stream);
int dfgnn_gt_fwd_typed_rect(int m, int n_cols, int nnz, int h, int f, int T, const int *row_ptr, const int *col_ind,
                            const float *val, const int *etype, const float *R, const float *Q, const float *K,
                            const float *V, float *row_max, float *row_sum, float *out, dfgnn_stream_t stream);
int dfgnn_gt_bwd_typed_rect(int m, int n_cols, int nnz, int h, int f, int T, const int *row_ptr, const int *col_ind,
                            const float *val, const int *etype, const int *col_ptr, const int *row_ind, const int *val_idx,
                            const int *etype_csc, const float *R, const float *Q, const float *K, const float *V,
                            const float *out, const float *row_max, const float *row_sum, const float *grad_out,
                            float *delta, float *ws, float *dQ, float *dK, float *dV, float *dR, dfgnn_stream_t stream);

/* The general statistics pair with a TYPED attention bias (csrc/gt_tbias_train.hip): any graph, no plan, any f.  The scalar
 * an edge adds to its logit is an entry of a small table B[T, h], chosen by the edge's type (Graphormer's spatial encoding,
 * T5 / Swin-style relative-position bias, any bucketed-distance or edge-type bias).  With t = etype[e], per head hd:
 *   s_e = val_e <Q_i, K_j> + B[t, hd],  P_e, out_i, delta_i, dS_e, dQ_i, dK_j, dV_j as in dfgnn_gt_*_bias
 *   dB[t, hd] = sum_{e : etype[e] = t} dS_e
 * i.e. the bias pair on bias[hd, e] = B[etype[e], hd] with dB = index_add(dbias.t(), etype) -- out, the statistics, dQ, dK,
 * dV are the bias pair's to the bit -- but an edge costs 4 bytes of type per pass instead of 4 h bytes of bias, and nothing
 * of size h nnz is read or written.
 *   T          number of types, >= 1
 *   etype      int32[nnz] in CSR edge order, 0 <= etype < T (the caller's contract: not checked); duplicate edges each
 *              carry their own type.  Required when nnz > 0
 *   etype_csc  int32[nnz], the same types in CSC entry order: etype_csc[t] = etype[val_idx[t]].  Graph data, made once per
 *              graph by the caller; the CSC pass streams it.  Required by the backward when nnz > 0
 *   B          fp32[T, h] (the layout of an embedding weight): the bias of (type t, head) is B[t h + head].  -inf masks
 *              every edge of that type for that head: P_e = 0, dB[t, head] = 0, and a (row, head) whose edges are all masked
 *              is an empty row (out = 0, row_max = -1e38, row_sum = 0, dQ = 0); no output holds a NaN or an inf.  +inf and
 *              NaN are the caller's error.  Required when nnz > 0
 *   val        fp32[nnz], CSR order, NULL = unit values
 *   val_idx    read only when val != NULL
 *   dB         fp32[T, h], written in full (a type without an edge: zeros; m == 0 or nnz == 0: all zeros), or NULL: the
 *              table is frozen, the CSR pass is the plain one with the bias pair's grid, any T, and ws is not used
 *   ws         caller scratch of dfgnn_gt_tbias_bwd_ws_floats(T, h) floats; required when dB != NULL.  The CSR pass then
 *              runs a bounded number of persistent workgroups per head, each wave summing into a table of T floats of its
 *              own in LDS; a workgroup stores one partial per head to ws and a reduction in the same call adds the partials
 *              in a fixed order.  No atomics: two calls give the same bits
 *   row_max = row_sum = NULL in the forward: nothing is saved (inference)
 * dfgnn_gt_tbias_bwd_ws_floats: > 0 = the number of floats, P(T) T max(h, 1) with P(T) = 1024 partials per head up to
 * T = 2560, 768 up to 3413, 512 up to 4096 (independent of m and nnz); < 0 = a DFGNN_E_* code: BADARG for T < 1 or a
 * negative h; UNSUPPORTED for h > 65535 and for T > 4096 (four wave tables of T floats in the 64 KB of dynamic LDS a kernel
 * gets without an attribute call).  dfgnn_gt_bwd_tbias with dB != NULL answers the same code before any launch.
 * Everything else as dfgnn_gt_fwd_bias / dfgnn_gt_bwd_bias; the _rect entries take an m x n_cols graph (extents: see
 * dfgnn_gt_fwd_rowstats_rect) and the square ones are these with n_cols = m.  Nothing allocates or synchronises, and no call
 * sets a function attribute: a step is capturable in a HIP graph without a warm-up. */
int dfgnn_gt_tbias_bwd_ws_floats(int T, int h);
int dfgnn_gt_fwd_tbias(int m, int nnz, int h, int f, int T, const int *row_ptr, const int *col_ind, const float *val,
                       const int *etype, const float *B, const float *Q, const float *K, const float *V, float *row_max,
                       float *row_sum, float *out, dfgnn_stream_t stream);
int dfgnn_gt_bwd_tbias(int m, int nnz, int h, int f, int T, const int *row_ptr, const int *col_ind, const float *val,
                       const int *etype, const int *col_ptr, const int *row_ind, const int *val_idx, const int *etype_csc,
                       const float *B, const float *Q, const float *K, const float *V, const float *out,
                       const float *row_max, const float *row_sum, const float *grad_out, float *delta, float *ws, float *dQ,
                       float *dK, float *dV, float *dB, dfgnn_stream_t stream);
int dfgnn_gt_fwd_tbias_rect(int m, int n_cols, int nnz, int h, int f, int T, const int *row_ptr, const int *col_ind,
                            const float *val, const int *etype, const float *B, const float *Q, const float *K,
                            const float *V, float *row_max, float *row_sum, float *out, dfgnn_stream_t stream);
int dfgnn_gt_bwd_tbias_rect(int m, int n_cols, int nnz, int h, int f, int T, const int *row_ptr, const int *col_ind,
                            const float *val, const int *etype, const int *col_ptr, const int *row_ind, const int *val_idx,
                            const int *etype_csc, const float *B, const float *Q, const float *K, const float *V,
                            const float *out, const float *row_max, const float *row_sum, const float *grad_out,
                            float *delta, float *ws, float *dQ, float *dK, float *dV, float *dB, dfgnn_stream_t stream);

/* GATv2 convolution (csrc/gatv2_train.hip): fused inference and training pair for ANY graph, no plan, no degree limit,
 * any f.  The logit of edge (i, j) is neither rank-one (dfgnn_gat_*) nor a dot product (dfgnn_gt_*):
 *   z_e = X_row[i,h,:] + X_col[j,h,:],  s_e = sum_d attn[h,d] lrelu(z_e[d]),  lrelu(x) = x > 0 ? x : negative_slope x
 *   P_e = exp(s_e - row_max_i) / row_sum_i,  out[i,h,:] = sum_e P_e X_col[j,h,:]
 * so a formulation with index ops materialises z[nnz, h, f]; here nothing of size nnz exists.  The neighbour row
 * X_col[j] is both the logit operand and the message: the lane-group form of the forward gathers it once per edge.
 * Saved between forward and backward: row_max, row_sum fp32[m, h] (empty row: out = 0, row_max = -1e38, row_sum = 0), as
 * for dfgnn_gt_fwd_rowstats.  The backward, given the forward's `out`, rebuilds each edge in a CSR pass and a CSC pass:
 *   delta_i = <grad_out_i, out_i>,  dS_e = P_e (<grad_out_i, X_col_j> - delta_i),
 *   g_e[d] = dS_e attn[h,d] (z_e[d] > 0 ? 1 : negative_slope)     (at z == 0 the derivative is negative_slope, as in torch)
 *   dX_row[i] = sum_{e of row i} g_e            dX_col[j] = sum_{e into j} (P_e grad_out_i + g_e)
 *   dattn[h,d] = sum_{all e} dS_e lrelu(z_e[d])
 * dattn is a sum over every edge: the CSR pass runs a bounded number of persistent workgroups, each keeps its share in
 * registers over all the rows it walks and stores ONE partial [h, f] into `ws`; a small kernel in the same call sums the
 * partials in a fixed order.  No atomics: every output is written in full by plain stores and is deterministic.
 *   attn     fp32[h, f]
 *   X_row, X_col  fp32[m, h, f]; may be the same pointer (shared weights).  dX_row and dX_col are distinct buffers
 *   row_max = row_sum = NULL in the forward: nothing is saved (inference); otherwise both are set
 *   delta    caller scratch fp32[m, h], written by the CSR pass and read by the CSC pass
 *   ws       caller scratch of dfgnn_gatv2_bwd_ws_floats(h, f) floats (independent of m and nnz), 16-byte aligned for
 *            the float4 path
 * dfgnn_gatv2_bwd_ws_floats: > 0 = the number of floats; < 0 = a DFGNN_E_* code (negative size: BADARG; h > 65535 or a
 * size that does not fit an int: UNSUPPORTED, as dfgnn_gatv2_bwd then answers too). */
int dfgnn_gatv2_bwd_ws_floats(int h, int f);
int dfgnn_gatv2_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *attn,
                    float negative_slope, const float *X_row, const float *X_col, float *row_max, float *row_sum,
                    float *out, dfgnn_stream_t stream);
int dfgnn_gatv2_bwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const int *col_ptr,
                    const int *row_ind, const float *attn, float negative_slope, const float *X_row, const float *X_col,
                    const float *out, const float *row_max, const float *row_sum, const float *grad_out, float *delta,
                    float *ws, float *dX_row, float *dX_col, float *dattn, dfgnn_stream_t stream);
/* ... for an m x n_cols graph: X_row, dX_row, out, grad_out fp32[m, h, f]; X_col, dX_col fp32[n_cols, h, f]; row_max,
 * row_sum, delta fp32[m, h]; row_ptr int32[m+1], col_ptr int32[n_cols+1] (see dfgnn_gt_fwd_rowstats_rect).  The CSR pass
 * keeps its bound of persistent workgroups, so `ws` is the same size. */
int dfgnn_gatv2_fwd_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *attn,
                         float negative_slope, const float *X_row, const float *X_col, float *row_max, float *row_sum,
                         float *out, dfgnn_stream_t stream);
int dfgnn_gatv2_bwd_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const int *col_ptr,
                         const int *row_ind, const float *attn, float negative_slope, const float *X_row, const float *X_col,
                         const float *out, const float *row_max, const float *row_sum, const float *grad_out, float *delta,
                         float *ws, float *dX_row, float *dX_col, float *dattn, dfgnn_stream_t stream);

/* GATv2 with a per-edge FEATURE VECTOR inside the LeakyReLU (csrc/gatv2_edge_train.hip): the pair above with E, what PyG's
 * GATv2Conv(edge_dim) computes with E = lin_edge(edge_attr) viewed [nnz, h, f]:
 *   z_e = X_row[i,h,:] + X_col[j,h,:] + E[e,h,:],  s_e, P_e as above,  out[i,h,:] = sum_e P_e X_col[j,h,:]  (E is NOT in
 *   the message),  g_e, dX_row, dX_col, dattn as above with this z_e,  dE[e,h,:] = g_e
 *   E        fp32[nnz, h, f] in CSR edge order (the feature layout with the edge in place of the node: the row of
 *            (edge e, head) starts at (e h + head) f); required when nnz > 0.  Duplicate edges each have their own row
 *   dE       fp32[nnz, h, f], every slot written by plain stores (no pre-zeroing), or NULL: E needs no gradient and nothing
 *            of size nnz h f is written
 *   val_idx  int32[nnz], the CSR position of each CSC entry; required when nnz > 0: the CSC pass finds an entry's E row
 *            through it
 *   ws       dfgnn_gatv2_bwd_ws_floats(h, f) floats, as above
 * E and dE take part in the float4 path's alignment rule (f % 4 == 0 and every base 16-byte aligned), as for
 * dfgnn_gt_fwd_edge.  With E = 0 every output equals the pair above bit for bit.  Everything else as there: empty rows and
 * columns, X_row == X_col, the size limits (DFGNN_E_UNSUPPORTED), no atomics, nothing allocates or synchronises.  The
 * square entries are the n_cols = m case of the *_rect ones. */
int dfgnn_gatv2_fwd_edge(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *attn,
                         float negative_slope, const float *X_row, const float *X_col, const float *E, float *row_max,
                         float *row_sum, float *out, dfgnn_stream_t stream);
int dfgnn_gatv2_bwd_edge(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const int *col_ptr,
                         const int *row_ind, const int *val_idx, const float *attn, float negative_slope, const float *X_row,
                         const float *X_col, const float *E, const float *out, const float *row_max, const float *row_sum,
                         const float *grad_out, float *delta, float *ws, float *dX_row, float *dX_col, float *dattn,
                         float *dE, dfgnn_stream_t stream);
int dfgnn_gatv2_fwd_edge_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                              const float *attn, float negative_slope, const float *X_row, const float *X_col, const float *E,
                              float *row_max, float *row_sum, float *out, dfgnn_stream_t stream);
int dfgnn_gatv2_bwd_edge_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                              const int *col_ptr, const int *row_ind, const int *val_idx, const float *attn,
                              float negative_slope, const float *X_row, const float *X_col, const float *E, const float *out,
                              const float *row_max, const float *row_sum, const float *grad_out, float *delta, float *ws,
                              float *dX_row, float *dX_col, float *dattn, float *dE, dfgnn_stream_t stream);

/* AGNN / dot-product attention with TIED keys and values (csrc/agnn_train.hip): fused inference and training pair for ANY
 * graph, no plan, no degree limit, any f.  The neighbour row X_col[j] is the key AND the value of edge (i, j) -- up to one
 * scalar per node, which is computed from the registers that hold the row -- so every pass gathers it once per edge and
 * nothing per node is precomputed.  Per head:
 *   cosine = 1:  r_i = 1 / max(|X_row[i]|_2, 1e-12),  q_j = 1 / max(|X_col[j]|_2, 1e-12)     (F.normalize's eps)
 *   cosine = 0:  r_i = q_j = 1
 *   c_e = r_i q_j <X_row[i], X_col[j]>,  s_e = beta[h] c_e
 *   P_e = exp(s_e - row_max_i) / row_sum_i,  out_i = sum_e P_e X_col[j]
 *   delta_i = <grad_out_i, out_i>,  dS_e = P_e (<grad_out_i, X_col[j]> - delta_i)
 *   g_i  = sum_{e of row i} dS_e c_e  -> dbeta_rows[i, h]        (dbeta[h] = sum_i g_i: the caller's column sum)
 *   g'_j = sum_{e into j} dS_e c_e
 *   dX_row[i] = beta r_i ( sum_{e of i} dS_e q_j X_col[j]  -  k g_i r_i X_row[i] )
 *   dX_col[j] = sum_{e into j} P_e grad_out_i  +  beta q_j ( sum_{e into j} dS_e r_i X_row[i]  -  k g'_j q_j X_col[j] ),  k = cosine
 * cosine = 1 is AGNN (softmax_j(beta cos(h_i, h_j)), PyG's / DGL's AGNNConv); cosine = 0 with beta = f^-1/2 is dot-product
 * graph attention (DotGatConv).  A feature row of zeros has norm 0, c = 0 and a gradient of order beta / 1e-12, exactly as
 * F.normalize's autograd gives: no special case.
 *   beta     fp32[h] on the device (a parameter)
 *   cosine   0 or 1
 *   X_row, X_col  fp32[m, h, f]; may be the same pointer.  dX_row and dX_col are distinct buffers
 *   row_max = row_sum = NULL in the forward: nothing is saved (inference); otherwise both are set.  Empty row: out = 0,
 *            row_max = -1e38, row_sum = 0, dX_row = 0, dbeta_rows = 0; empty column: dX_col = 0
 *   delta    caller scratch fp32[m, h], written by the CSR pass and read by the CSC pass
 *   dbeta_rows  fp32[m, h], written in full, or NULL: beta needs no gradient (everything else is bit-identical)
 * No edge values.  No atomics, no workspace: every output is written in full by plain stores and is deterministic.
 * Return codes as dfgnn_gatv2_*: DFGNN_E_BADARG for a missing pointer, one statistic without the other, a cosine other than
 * 0 / 1, dX_row == dX_col; DFGNN_E_UNSUPPORTED for h > 65535 or f outside the compiled range.  The square entries are the
 * n_cols = m case of the *_rect ones (X_col, dX_col fp32[n_cols, h, f], col_ptr int32[n_cols+1]; see
 * dfgnn_gt_fwd_rowstats_rect, also for the degenerate extents): same kernels, same bits. */
int dfgnn_agnn_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *beta, int cosine,
                   const float *X_row, const float *X_col, float *row_max, float *row_sum, float *out,
                   dfgnn_stream_t stream);
int dfgnn_agnn_bwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const int *col_ptr,
                   const int *row_ind, const float *beta, int cosine, const float *X_row, const float *X_col,
                   const float *out, const float *row_max, const float *row_sum, const float *grad_out, float *delta,
                   float *dX_row, float *dX_col, float *dbeta_rows, dfgnn_stream_t stream);
int dfgnn_agnn_fwd_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *beta,
                        int cosine, const float *X_row, const float *X_col, float *row_max, float *row_sum, float *out,
                        dfgnn_stream_t stream);
int dfgnn_agnn_bwd_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const int *col_ptr,
                        const int *row_ind, const float *beta, int cosine, const float *X_row, const float *X_col,
                        const float *out, const float *row_max, const float *row_sum, const float *grad_out, float *delta,
                        float *dX_row, float *dX_col, float *dbeta_rows, dfgnn_stream_t stream);

/* Residual gated graph convolution, GatedGCN (csrc/gatedgcn_train.hip): fused inference and training pair for ANY graph,
 * no plan, no degree limit, any f.  The attention is per dimension: a sigmoid gate in place of a softmax over a logit.
 * For edge e = (i, j), per head:
 *   z_e   = (X_row[i] + X_col[j]) + E_e                     elementwise, [f]
 *   sg_e  = 1 / (1 + exp(-z_e))                             finite for every finite z
 *   den_i = sum_{e of row i} sg_e
 *   out_i = sum_{e of row i} sg_e (.) V_j / (den_i + eps)   normalize = 1 (Dwivedi et al., GraphGPS; eps = 1e-6 there)
 *   out_i = sum_{e of row i} sg_e (.) V_j                   normalize = 0 (PyG's ResGatedGraphConv)
 *   Z_e   = z_e                                             the edge output: the next layer's edge features (optional)
 * and, with dO = d loss / d out and G = d loss / d Z (optional, NULL = zero),
 *   s_i   = dO_i / (den_i + eps)   (normalize = 0: dO_i)
 *   dsg_e = s_i (.) (V_j - out_i)  (normalize = 0: s_i (.) V_j)
 *   g_e   = dsg_e (.) sg_e (.) (1 - sg_e) + G_e
 *   dX_row_i = sum_{e of row i} g_e    dX_col_j = sum_{e into j} g_e    dV_j = sum_{e into j} sg_e (.) s_i    dE_e = g_e
 * Saved between forward and backward: out and den, fp32[m, h, f]; nothing of size nnz.  Both backward passes rebuild z_e
 * and sg_e with the forward's expression and routine: the bits are the forward's.
 *   X_row    fp32[m, h, f]; X_col, V fp32[n_cols, h, f] (square entries: n_cols = m).  X_row and X_col may be one pointer
 *   E        fp32[nnz, h, f] in CSR edge order (the row of (edge e, head) starts at (e h + head) f), or NULL: no edge
 *            term, the bits of E = zeros and nothing of it is read
 *   den      fp32[m, h, f], or NULL in the forward: not wanted (inference).  Written in either mode
 *   Z        fp32[nnz, h, f], every slot written by plain stores, or NULL: not wanted.  `out` and `den` are the same bits
 *   G        fp32[nnz, h, f] or NULL: zero (the bits of G = zeros; nothing of it is read)
 *   dE       fp32[nnz, h, f], every slot written, or NULL: not wanted.  Every other output is the same bits
 *   out, den of the backward: the forward's.  normalize = 0 reads neither and accepts NULL for both
 *   ws       caller scratch fp32[m, h, f] (16-byte aligned for the float4 path): the CSR pass leaves s_i there for the CSC
 *            pass.  Required when normalize = 1 and m > 0; not touched when normalize = 0
 *   val_idx  int32[nnz], the CSR position of each CSC entry; required by the backward when nnz > 0
 * An empty row: out = 0, den = 0, dX_row = 0; an empty column: dX_col = dV = 0.  No edge values.  No atomics: every output
 * is written in full by plain stores, the summation order is fixed, two calls give the same bits.  Nothing allocates or
 * synchronises.  Return codes: DFGNN_E_BADARG for a negative size, a missing pointer, a normalize other than 0 / 1, a
 * negative or non-finite eps, two of dX_row / dX_col / dV being one buffer; DFGNN_E_UNSUPPORTED for h > 65535 or f outside
 * the compiled range; m == 0 or nnz == 0 reads no edge.  The square entries are the n_cols = m case of the *_rect ones
 * (col_ptr int32[n_cols+1]; see dfgnn_gt_fwd_rowstats_rect): same kernels, same bits. */
int dfgnn_gatedgcn_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *X_row,
                       const float *X_col, const float *V, const float *E, int normalize, float eps, float *den, float *out,
                       float *Z, dfgnn_stream_t stream);
int dfgnn_gatedgcn_bwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const int *col_ptr,
                       const int *row_ind, const int *val_idx, const float *X_row, const float *X_col, const float *V,
                       const float *E, int normalize, float eps, const float *out, const float *den, const float *grad_out,
                       const float *G, float *dX_row, float *dX_col, float *dV, float *dE, float *ws,
                       dfgnn_stream_t stream);
int dfgnn_gatedgcn_fwd_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                            const float *X_row, const float *X_col, const float *V, const float *E, int normalize, float eps,
                            float *den, float *out, float *Z, dfgnn_stream_t stream);
int dfgnn_gatedgcn_bwd_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                            const int *col_ptr, const int *row_ind, const int *val_idx, const float *X_row,
                            const float *X_col, const float *V, const float *E, int normalize, float eps, const float *out,
                            const float *den, const float *grad_out, const float *G, float *dX_row, float *dX_col, float *dV,
                            float *dE, float *ws, dfgnn_stream_t stream);

/* GAT (v1) for ANY graph with an optional per-edge attention term (csrc/gat_edge_train.hip): fused inference and training
 * pair, no plan, no degree limit, any f, square or m x n_cols.  Opt-in: dfgnn_gat_fwd_train / dfgnn_gat_bwd stay what the
 * GAT layers use on dense batches.  For edge e = (row i, column j), per head (rows are the outputs, columns the sources):
 *   pre_e = (attn_row[i] + attn_col[j]) + score[head, e]
 *   s_e   = pre_e > 0 ? pre_e : negative_slope pre_e
 *   P_e   = exp(s_e - edge_max_i) / edge_sum_i              statistics over ALL edges of the row, dropped or not
 *   k_e   = edge_mask ? (edge_mask[e, head] > attn_drop) / (1 - attn_drop) : 1
 *   out_i = sum_{e of row i} k_e P_e X[j]
 * and, with dO = d loss / d out,
 *   delta_i = <dO_i, out_i>     dS_e = P_e (k_e <dO_i, X[j]> - delta_i)     G_e = dS_e (pre_e > 0 ? 1 : negative_slope)
 *   grad_attn_row[i] = sum_{e of row i} G_e    grad_attn_col[j] = sum_{e into j} G_e    grad_score[head, e] = G_e
 *   grad_feat[j]     = sum_{e into j} k_e P_e dO_i
 * Saved between forward and backward: edge_max, edge_sum (and the caller's edge_mask).  The CSR pass sums delta_i = sum_e k_e
 * P_e <dO_i, X[j]> over the edges it walks anyway -- the forward's `out` is not an argument of the backward; summed this way
 * delta carries the rounding of the dot products alone, which keeps rows of a few edges at fp32 level -- and hands only
 * delta to the CSC pass, which recomputes <dO_i, X[j]> from the rows it gathers anyway.  Nothing else of size nnz exists.
 *   attn_row, edge_max, edge_sum, delta, grad_attn_row   fp32[m, h]
 *   attn_col, grad_attn_col                              fp32[n_cols, h]  (square entries: n_cols = m)
 *   X, grad_feat                                         fp32[n_cols, h, f]: the message is the source's; no row-side features
 *   out, grad_out                                        fp32[m, h, f]
 *   score       fp32[h, nnz] in CSR edge order (the layout of bias in dfgnn_gt_fwd_bias), or NULL: no edge term, the bits of
 *               score = zeros.  -inf masks an edge: P_e = 0, G_e = 0.  A (row, head) whose edges are all masked is an empty
 *               row.  +inf and NaN are the caller's error
 *   grad_score  fp32[h, nnz], every slot written by plain stores, or NULL: not wanted, every other output keeps its bits
 *   edge_mask   fp32[nnz, h] uniform randoms with attn_drop in [0, 1) exactly as in dfgnn_gat_fwd_train, or NULL: no dropout
 *               (attn_drop is then ignored).  A row whose edges are all dropped has out = 0 and finite gradients
 *   edge_max, edge_sum of the forward: both NULL = inference
 *   delta       caller scratch fp32[m, h], written by the backward
 *   val_idx     int32[nnz], the CSR position of each CSC entry; required when nnz > 0 and score or edge_mask is given
 * An empty row: out = 0, edge_max = -1e38, edge_sum = 0, grad_attn_row = 0, delta = 0; an empty column: grad_feat = 0,
 * grad_attn_col = 0.  No atomics: every output is written in full by plain stores, the summation order is fixed, two calls
 * give the same bits.  Nothing allocates or synchronises.  X / out (forward), X / grad_out / grad_feat (backward) 16-byte aligned with f % 4 == 0
 * take the float4 path, anything else the scalar one (f <= 256).  Degenerate extents and return codes as for
 * dfgnn_gt_fwd_rowstats_rect; DFGNN_E_BADARG also for an edge_mask with attn_drop outside [0, 1).  The square entries are
 * the n_cols = m case of the *_rect ones: same kernels, same bits. */
int dfgnn_gat_fwd_edge(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *attn_row,
                       const float *attn_col, float negative_slope, const float *score, const float *X,
                       const float *edge_mask, float attn_drop, float *edge_max, float *edge_sum, float *out,
                       dfgnn_stream_t stream);
int dfgnn_gat_bwd_edge(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const int *col_ptr,
                       const int *row_ind, const int *val_idx, const float *attn_row, const float *attn_col,
                       float negative_slope, const float *score, const float *X, const float *edge_mask, float attn_drop,
                       const float *edge_max, const float *edge_sum, const float *grad_out, float *delta, float *grad_feat,
                       float *grad_attn_row, float *grad_attn_col, float *grad_score, dfgnn_stream_t stream);
int dfgnn_gat_fwd_edge_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                            const float *attn_row, const float *attn_col, float negative_slope, const float *score,
                            const float *X, const float *edge_mask, float attn_drop, float *edge_max, float *edge_sum,
                            float *out, dfgnn_stream_t stream);
int dfgnn_gat_bwd_edge_rect(int m, int n_cols, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                            const int *col_ptr, const int *row_ind, const int *val_idx, const float *attn_row,
                            const float *attn_col, float negative_slope, const float *score, const float *X,
                            const float *edge_mask, float attn_drop, const float *edge_max, const float *edge_sum,
                            const float *grad_out, float *delta, float *grad_feat, float *grad_attn_row,
                            float *grad_attn_col, float *grad_score, dfgnn_stream_t stream);

/* weights[256 i + c] = val[e] for the edge e from node i to the c-th node of i's range of the plan, 0 elsewhere:
 * dfgnn_plan_dense_weights_floats(m) = 256 m floats (device, 16-byte aligned), written by one memset + one kernel on
 * `stream`.  val: fp32[nnz] in CSR order.  Only the dense ranges of the plan are filled (dfgnn_gt_stats_applies == 1:
 * all of them). */
size_t dfgnn_plan_dense_weights_floats(int m);
int dfgnn_plan_dense_weights(int m, int nnz, const int *row_ptr, const float *val, const int *plan, const int *plan_meta,
                             float *weights, dfgnn_stream_t stream);

/* The two launches of the plan-less dfgnn_gt_bwd, exposed separately so each can be timed / profiled on its own
 * (dfgnn_gt_bwd == rows pass then cols pass on the same stream):
 *   rows pass (CSR): dP = <dO[i],V[j]>, dS = P (dP - sum_row P dP) -> grad_edge, dQ   (fused_backward_kernel,
 *                    fused_gtconv_backward.cu:73-191)
 *   cols pass (CSC): dV[j] = sum P dO[i], dK[j] = sum dS val Q[i]                      (spmm_backward_kernel,
 *                    fused_gtconv_backward.cu:40-70) */
int dfgnn_gt_bwd_rows(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                      const int *rows, const float *val, const float *K, const float *V,
                      const float *attn_edge, const float *grad_out, float *grad_edge, float *dQ,
                      dfgnn_stream_t stream);
int dfgnn_gt_bwd_cols(int m, int nnz, int h, int f, const float *val, const int *col_ptr,
                      const int *row_ind, const int *val_idx, const float *Q, const float *attn_edge,
                      const float *grad_edge, const float *grad_out, float *dK, float *dV,
                      dfgnn_stream_t stream);

/* replaces gt_tiling_inference (fused_gtconv.cpp:244-276, fused_gtconv_tiling.cu:92-118):
 * CSR only, online softmax over fixed-size neighbour tiles, no degree limit. */
int dfgnn_gt_tiling_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                        const float *val, const float *Q, const float *K, const float *V,
                        float *out, dfgnn_stream_t stream);

/* replaces gt_softmax_inference (fused_gtconv.cpp:316-352, fused_gtconv_softmax.cu:10-54) and
 * gt_softmax_gm_inference (fused_gtconv.cpp:354-389, fused_gtconv_softmax_gm.cu:81-125):
 * two kernels, edge-parallel SDDMM into `logits` (caller scratch fp32[h, nnz]) then
 * node-parallel softmax+SpMM; the _gm form re-reads logits from global memory on every pass. */
int dfgnn_gt_softmax_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                         const int *rows, const float *val, const float *Q, const float *K,
                         const float *V, float *logits, float *out, dfgnn_stream_t stream);
int dfgnn_gt_softmax_gm_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                            const int *rows, const float *val, const float *Q, const float *K,
                            const float *V, float *logits, float *out, dfgnn_stream_t stream);

/* ---- GAT ---------------------------------------------------------------------------------------
 * attn_row, attn_col fp32[m, h]; X (in_feat) fp32[m, h, f].
 * replaces gat_inference_hyper (DFGNN/src/fused_gatconv/fused_gatconv.cpp:99-119,
 *                               fused_gatconv_hyper.cu:251-272)
 * plan / plan_meta / edge_ws as in dfgnn_gt_hyper_fwd (edge_ws is needed whenever meta[8] > 0). */
int dfgnn_gat_hyper_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                        const int *rows, const float *attn_row, const float *attn_col,
                        float negative_slope, const float *X, float *edge_ws, float *out,
                        const int *plan, const int *plan_meta, dfgnn_stream_t stream);

/* replaces gt_csr_inference / gt_csr_gm_inference (fused_gtconv.cpp:174-242; fused_gt_csr,
 * fused_gt_csr_global_memory, fused_gtconv_csr.cu:10-219): the node-parallel CSR baselines of the reference's sweeps --
 * a wave per row, the row's logits materialised (in LDS: 'csr', rows longer than the 2048-float buffer use `logits`;
 * in global memory: 'csr_gm'), then max / sum / weighted-sum sweeps.  logits: fp32[h, nnz] scratch. */
int dfgnn_gt_csr_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                     const float *Q, const float *K, const float *V, float *logits, float *out,
                     dfgnn_stream_t stream);
int dfgnn_gt_csr_gm_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind, const float *val,
                        const float *Q, const float *K, const float *V, float *logits, float *out,
                        dfgnn_stream_t stream);

/* replaces gat_inference_hyper_recompute (fused_gatconv.cpp:124-142; fused_gat_hyper_recompute_inference_vec4,
 * fused_gatconv_hyper_recompute.cu:118-216): node-parallel, no logit storage -- the rank-one logits are recomputed in
 * each of the three sweeps.  Any f (the reference exit(0)s unless f % 128 == 0). */
int dfgnn_gat_recompute_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                            const float *attn_row, const float *attn_col, float negative_slope, const float *X,
                            float *out, dfgnn_stream_t stream);

/* replaces gat_inference_softmax (fused_gatconv.cpp:40-61, fused_gatconv_softmax.cu:33-56) and
 * gat_inference_softmax_gm (fused_gatconv.cpp:69-90, fused_gatconv_softmax_gm.cu) */
int dfgnn_gat_softmax_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                          const int *rows, const float *attn_row, const float *attn_col,
                          float negative_slope, const float *X, float *logits, float *out,
                          dfgnn_stream_t stream);
int dfgnn_gat_softmax_gm_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                             const int *rows, const float *attn_row, const float *attn_col,
                             float negative_slope, const float *X, float *logits, float *out,
                             dfgnn_stream_t stream);

/* replaces gat_inference_tiling (fused_gatconv.cpp:196-219, fused_gatconv_tiling.cu:78-103) */
int dfgnn_gat_tiling_fwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                         const float *attn_row, const float *attn_col, float negative_slope,
                         const float *X, float *out, dfgnn_stream_t stream);

/* dfgnn_gat_tiling_fwd for super-node full graphs whose feature table [m, h, f] does not fit the L2s (reddit: 119 MB): the
 * columns are cut into chunks of `chunk_rows` nodes (<= 32768; 8192 x 512 B = one XCD's 4 MiB L2), the edges are
 * re-ordered chunk-major, every (row, chunk) segment gives an online-softmax partial state and a second kernel merges
 * a row's states (csrc/gat_tiling_chunked.hip).  Same result as dfgnn_gat_tiling_fwd to fp32 rounding.
 *   seg_ptr  int32[nchunks * m + 1], nchunks = ceil(m / chunk_rows): the edges of row r into chunk c are
 *            seg_ptr[c m + r] .. seg_ptr[c m + r + 1] of the chunk-major edge order (= the CSR order sorted stably by
 *            the chunk of the column)
 *   ccol     int16[nnz]: column - chunk * chunk_rows of every edge in that order
 *   ws       device workspace of dfgnn_gat_tiling_chunked_ws_bytes(m, h, f, chunk_rows) bytes (partial states)
 * seg_ptr / ccol depend on the graph only: preprocessing, built once (the Python binding builds and caches them). */
size_t dfgnn_gat_tiling_chunked_ws_bytes(int m, int h, int f, int chunk_rows);
int dfgnn_gat_tiling_chunked_fwd(int m, int nnz, int h, int f, int chunk_rows, const int *seg_ptr, const short *ccol,
                                 const float *attn_row, const float *attn_col, float negative_slope, const float *X,
                                 float *out, void *ws, size_t ws_bytes, dfgnn_stream_t stream);

/* First kernel of the reference's 'hyper_v2' variant (gat_inference_hyper_v2, fused_gatconv.cpp:148-158;
 * fused_gat_dot_attn_weight, fused_gatconv_hyper_v2.cu:212-249): the per-node attention scores from the layer's
 * attention vectors a_l, a_r fp32[h, f]:  attn_row[i, hd] = <a_l[hd], X[i, hd]>,  attn_col[i, hd] = <a_r[hd], X[i, hd]>.
 * X is read once for both.  The second kernel of 'hyper_v2' is dfgnn_gat_hyper_fwd / dfgnn_gat_tiling_fwd. */
int dfgnn_gat_attn_scores(int m, int h, int f, const float *a_l, const float *a_r, const float *X,
                          float *attn_row, float *attn_col, dfgnn_stream_t stream);

/* ---- GAT training pair (FusedGATFunction, DFGNN/operators/fused_gatconv.py:95-176) --------------------
 * edge_max, edge_sum fp32[m, h]: per-row maximum of the LeakyReLU logits (-1e38 for an empty row) and
 *   sum_e exp(s_e - max); the backward recomputes P_e from them, as the reference does.
 * edge_mask fp32[nnz, h], EDGE-major (index e*h + head, fused_gatconv_kernel.cu:101): uniform randoms for
 *   attention dropout, an INPUT here (the reference draws it inside with cuRAND seeded by clock(),
 *   fused_gatconv_kernel.cu:1074-1083; the binding draws it with torch.rand so runs are reproducible).
 *   Edge e of head hd is kept iff edge_mask[e*h + hd] > attn_drop and its attention is scaled by
 *   1 / (1 - attn_drop).  NULL = no dropout (attn_drop is then ignored); with a mask, 0 <= attn_drop < 1.
 * rows / plan / plan_meta: optional (NULL = general CSR kernels).  With all three, the plan's dense ranges
 *   (meta[9] of them: small dense member graphs of a batch) run on the matrix-core kernels, one workgroup per
 *   range as in dfgnn_gt_hyper_fwd / dfgnn_gt_bwd, and the general kernels cover only the remaining ranges.
 *   The reference's gat_forward / gat_backward take no COO rows: the binding derives them from row_ptr once per
 *   batch structure, next to the plan.
 *
 * dfgnn_gat_fwd_train replaces gat_forward (fused_gatconv.cpp:11-32, fused_gatconv_kernel.cu:24-125, 1062-1129):
 *   writes out[m, h, f], edge_max, edge_sum. */
int dfgnn_gat_fwd_train(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                        const int *rows, const float *attn_row, const float *attn_col,
                        float negative_slope, const float *X, const float *edge_mask, float attn_drop,
                        float *edge_max, float *edge_sum, float *out, const int *plan,
                        const int *plan_meta, dfgnn_stream_t stream);

/* replaces gat_backward (fused_gatconv.cpp:291-353, fused_gatconv_kernel.cu:609-865, 1172-1244).
 * col_ptr int32[m+1], row_ind int32[nnz], permute int32[nnz] (CSR slot of each CSC entry; the GT path calls
 * it val_idx).  grad_edge: caller scratch fp32[h, nnz] (untouched on the matrix-core path).  Writes grad_feat
 * fp32[m, h, f], grad_attn_row and grad_attn_col fp32[m, h] in full (no pre-zeroing, no atomics: the column
 * sums are deterministic). */
int dfgnn_gat_bwd(int m, int nnz, int h, int f, const int *row_ptr, const int *col_ind,
                  const int *rows, const int *col_ptr, const int *row_ind, const int *permute,
                  const float *attn_row, const float *attn_col, float negative_slope, const float *X,
                  const float *edge_max, const float *edge_sum, const float *edge_mask,
                  float attn_drop, const float *grad_out, float *grad_edge, float *grad_feat,
                  float *grad_attn_row, float *grad_attn_col, const int *plan, const int *plan_meta,
                  dfgnn_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DFGNN_H_ */
