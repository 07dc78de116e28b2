/* dfgnn_segment.h -- C ABI of the segment multi-head attention pair (csrc/segment_mha.hip), next to the conv ABI of dfgnn.h.
 *
 * The global half of a GraphGPS-style layer: every node of a batch of graphs attends to all nodes of its own graph.  Nodes
 * are ordered by graph and the whole structure is seg_ptr: int32[n_seg + 1], non-decreasing, seg_ptr[0] = 0,
 * seg_ptr[n_seg] = m; empty segments are allowed anywhere.  For row i of segment [lo, hi), per head:
 *   s_ij = scale <Q_i, K_j>,   P_ij = softmax over j in [lo, hi) of s_ij,   out_i = sum_j P_ij V_j
 * No edge list, plan or bitmap exists and nothing of size n^2 is saved: the forward keeps row_max_i = max_j s_ij and
 * row_sum_i = sum_j exp(s_ij - row_max_i), the backward recomputes P from them.  The products run on the matrix cores with
 * split fp16 operands and fp32 accumulation (fp32-level results); graphs of any size are served by the same kernels.
 *
 *   dfgnn_segment_bounds    once per batch: bounds[2 i] = lo_i, bounds[2 i + 1] = hi_i, both clamped into [0, m] -- a
 *                           seg_ptr that breaks the rules above gives wrong numbers, never an access outside the arrays.
 *                           Every layer, head, forward and backward of the batch reads the same bounds
 *   dfgnn_segment_mha_fwd   out, and row_max / row_sum unless both are NULL (inference)
 *   dfgnn_segment_mha_bwd   dQ, dK, dV from the statistics; delta is scratch the call writes (sum_j P_ij dP_ij per row and head)
 *                           and reads back on the same stream.  `out` is accepted for symmetry with the other pairs and not
 *                           read (it may be NULL): delta is formed from P and dP
 * No call allocates, synchronises or reads the device from the host; the grids follow from m and h alone, so the calls can
 * be captured in a HIP graph.  All kernels run on `stream`; two calls give the same bits (no atomics, fixed summation order).
 *
 *   m, n_seg, h, f   nodes, segments, heads, features per head
 *   seg_ptr          int32[n_seg + 1]
 *   bounds           int32[2 m]
 *   Q, K, V, out, dO, dQ, dK, dV   fp32[m, h, f], row-major, 16-byte aligned
 *   row_max, row_sum, delta        fp32[m, h]
 *
 * Return codes: DFGNN_E_BADARG for a negative extent, h < 1, f < 1, m > 0 with n_seg == 0, one of row_max / row_sum
 * without the other, a NULL required pointer; DFGNN_E_UNSUPPORTED for f outside {16, 32, 64, 128}, h > 65535 or a feature
 * array of 4 GiB or more (rows are addressed with 32-bit byte offsets).  The extents are checked first, then the limits,
 * then (for m > 0) the pointers, all before any device call.  m == 0 is a valid no-op.
 * dfgnn_segment_mha_applies is host-only: 1 when the pair serves (h, f), else 0. */
#ifndef DFGNN_SEGMENT_H_
#define DFGNN_SEGMENT_H_

#include "dfgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DFGNN_SEGMENT_ABI_VERSION 1

int dfgnn_segment_abi_version(void);
int dfgnn_segment_mha_applies(int h, int f);
int dfgnn_segment_bounds(int m, int n_seg, const int *seg_ptr, int *bounds, dfgnn_stream_t stream);
int dfgnn_segment_mha_fwd(int m, int h, int f, float scale, const int *bounds, const float *Q, const float *K, const float *V,
                          float *out, float *row_max, float *row_sum, dfgnn_stream_t stream);
int dfgnn_segment_mha_bwd(int m, int h, int f, float scale, const int *bounds, const float *Q, const float *K, const float *V,
                          const float *out, const float *row_max, const float *row_sum, const float *dO, float *dQ, float *dK,
                          float *dV, float *delta, dfgnn_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DFGNN_SEGMENT_H_ */
