/* dfgnn_segment_bias.h -- C ABI of the segment multi-head attention pair WITH A PAIR BIAS (csrc/segment_mha.hip), next to the
 * unbiased pair of dfgnn_segment.h: Graphormer-style global attention over a batch of graphs.
 *
 * Nodes, seg_ptr and bounds are those of dfgnn_segment.h.  For row i of segment [lo, hi) with n = hi - lo, per head:
 *   s_ij = scale <Q_i, K_j> + bias[head, row_off_i + (j - lo)],   P_ij = softmax over j in [lo, hi) of s_ij,
 *   out_i = sum_j P_ij V_j
 * bias is fp32[h, n_pairs] with n_pairs = sum_g n_g^2: within a head's plane the graphs follow each other, each one a packed
 * row-major n_g x n_g block (row = query, column = key).  No padding and no alignment: a row starts wherever it starts.
 * The values are finite; a large negative finite value masks a pair.  row_off_i = pair_ptr[g(i)] + (i - lo_i) n_g is the
 * offset of pair (i, lo_i) in a plane, pair_ptr the exclusive prefix sum of n_g^2.
 * The backward, with dS_ij = P_ij (dP_ij - delta_i): dQ = scale dS K, dK = scale dS^T Q, dV = P^T dO and
 * dbias[head, pair(i, j)] = dS_ij -- every valid pair written exactly once, nothing else written.  Nothing of size n^2 is
 * saved by the library: the forward keeps row_max / row_sum of the biased logits, the backward recomputes P from them.
 *
 *   dfgnn_segment_pair_rows      once per batch, next to dfgnn_segment_bounds: pair_ptr (a device scan, no host read) and
 *                                row_off.  A seg_ptr that breaks its rules gives wrong numbers; the attention kernels clamp
 *                                row_off_i into [0, n_pairs - n_i], so no address outside bias[h, n_pairs] is ever formed
 *                                (a row whose n_i exceeds n_pairs runs without bias and writes no dbias)
 *   dfgnn_segment_mha_bias_fwd   out, and row_max / row_sum unless both are NULL (inference)
 *   dfgnn_segment_mha_bias_bwd   dQ, dK, dV and, unless it is NULL, dbias; delta is scratch the call writes and reads back
 *                                on the same stream
 * No call allocates, synchronises or reads the device from the host; the grids follow from m, n_seg and h alone, so the
 * calls can be captured in a HIP graph.  All kernels run on `stream`; no atomics, two calls give the same bits.  The bias
 * planes are addressed with 64-bit offsets (h n_pairs passes 2^32 long before the features do).
 *
 *   m, n_seg, h, f   nodes, segments, heads, features per head
 *   seg_ptr          int32[n_seg + 1]
 *   bounds           int32[2 m]           (dfgnn_segment_bounds)
 *   pair_ptr         int64[n_seg + 1]     (out)
 *   row_off          int64[m]
 *   n_pairs          sum_g n_g^2 = pair_ptr[n_seg]: the length of a bias plane
 *   bias, dbias      fp32[h, n_pairs], 4-byte aligned
 *   Q, K, V, out, dO, dQ, dK, dV   fp32[m, h, f], row-major, 16-byte aligned
 *   row_max, row_sum, delta        fp32[m, h]
 *
 * Return codes: DFGNN_E_BADARG for a negative extent (n_pairs included), h < 1, f < 1, m > 0 with n_seg == 0, one of
 * row_max / row_sum without the other, a NULL required pointer (dbias is optional); DFGNN_E_UNSUPPORTED for f outside
 * {16, 32, 64, 128}, h > 65535, m >= 2^30 or a feature array of 4 GiB or more.  The extents are checked first, then the
 * limits, then (for m > 0) the pointers, all before any device call.  m == 0 is a valid no-op that writes nothing. */
#ifndef DFGNN_SEGMENT_BIAS_H_
#define DFGNN_SEGMENT_BIAS_H_

#include "dfgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DFGNN_SEGMENT_BIAS_ABI_VERSION 1

int dfgnn_segment_bias_abi_version(void);
int dfgnn_segment_pair_rows(int m, int n_seg, const int *seg_ptr, long long *pair_ptr, long long *row_off, dfgnn_stream_t stream);
int dfgnn_segment_mha_bias_fwd(int m, int h, int f, float scale, const int *bounds, const long long *row_off, long long n_pairs,
                               const float *bias, const float *Q, const float *K, const float *V, float *out, float *row_max,
                               float *row_sum, dfgnn_stream_t stream);
int dfgnn_segment_mha_bias_bwd(int m, int h, int f, float scale, const int *bounds, const long long *row_off, long long n_pairs,
                               const float *bias, const float *Q, const float *K, const float *V, const float *row_max,
                               const float *row_sum, const float *dO, float *dQ, float *dK, float *dV, float *dbias,
                               float *delta, dfgnn_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DFGNN_SEGMENT_BIAS_H_ */
