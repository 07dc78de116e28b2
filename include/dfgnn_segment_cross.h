/* dfgnn_segment_cross.h -- C ABI of the segment multi-head CROSS attention pair (csrc/segment_cross.hip): the pair of
 * dfgnn_segment.h with the attending and the attended rows in two arrays.
 *
 * Two node arrays, each ordered by graph: m_q query rows with seg_ptr_q int32[n_seg + 1], m_k key / value rows with
 * seg_ptr_k int32[n_seg + 1]; both follow the rules of dfgnn_segment.h (non-decreasing, first entry 0, last entry m_q / m_k)
 * and either side of a segment may be empty.  Segment g of the queries attends to segment g of the keys.  Per head, for
 * query i of segment g with keys [lo, hi):
 *   s_ij = scale <Q_i, K_j>,   P_ij = softmax over j in [lo, hi) of s_ij,   out_i = sum_j P_ij V_j
 * Uses: attention readout (a few seed queries per graph over its nodes), virtual nodes and latent arrays, two node sets per
 * sample (decoder over encoder, the dst over the src nodes of a sampled block).
 *
 *   dfgnn_segment_cross_bounds    once per batch: qbounds[2 i], qbounds[2 i + 1] = the key range of query i, clamped into
 *                                 [0, m_k]; kbounds[2 j], kbounds[2 j + 1] = the query range of key j, clamped into [0, m_q].
 *                                 A seg_ptr that breaks the rules gives wrong numbers, never an access outside the arrays
 *   dfgnn_segment_mha_cross_fwd   out, and row_max / row_sum unless both are NULL (inference)
 *   dfgnn_segment_mha_cross_bwd   dQ, dK, dV from the statistics; delta is scratch the call writes and reads back on the
 *                                 same stream
 * `form` chooses the kernels of the forward and of dQ (dK / dV has one form, key strips of 128 rows):
 *   DFGNN_SEGMENT_CROSS_WIDE   a work item is a 128-row query window and a head, one 16-row strip per wave: the kernels of
 *                              dfgnn_segment.h.  With seg_ptr_q == seg_ptr_k and the same arrays on both sides it returns
 *                              the bits of dfgnn_segment_mha_fwd / _bwd
 *   DFGNN_SEGMENT_CROSS_SPLIT  a work item is ONE 16-row query strip and a head; the workgroup's waves divide every staged
 *                              key tile between them and merge their partial results in a fixed order: few queries, many keys
 *   DFGNN_SEGMENT_CROSS_AUTO   one of the two, chosen from m_q, m_k, h, f alone
 * No call allocates, synchronises or reads the device from the host; the grids follow from m_q, m_k and h alone, so the
 * calls can be captured in a HIP graph.  All kernels run on `stream`; two calls give the same bits (no atomics, fixed
 * summation order).
 *
 *   Q, out, dO, dQ            fp32[m_q, h, f], row-major, 16-byte aligned
 *   K, V, dK, dV              fp32[m_k, h, f]
 *   row_max, row_sum, delta   fp32[m_q, h]
 *   qbounds int32[2 m_q], kbounds int32[2 m_k]
 *
 * A query whose key segment is empty gets out = 0, row_max = -1e38, row_sum = 0 and dQ = 0; a key whose query segment is
 * empty gets dK = dV = 0; every output row is written.  m_q == 0 and m_k == 0 are both valid: with m_k == 0 the forward
 * still writes all of out and the statistics and the backward all of dQ; with m_q == 0 the backward writes dK and dV as
 * zeros.  An array of no rows may be NULL.
 *
 * Return codes: DFGNN_E_BADARG for a negative extent, h < 1, f < 1, a form outside 0..2, rows with n_seg == 0, one of row_max
 * / row_sum without the other, a NULL pointer to an array that has rows; DFGNN_E_UNSUPPORTED for f outside {16, 32, 64, 128},
 * h > 65535 or a feature array of 4 GiB or more on either side.  The extents are checked first, then the limits, then the
 * pointers, all before any device call.
 *
 * The pair bias and the typed pair bias (dfgnn_segment_bias.h, dfgnn_segment_tbias.h) stay square only: their planes are
 * packed n x n blocks of one node array. */
#ifndef DFGNN_SEGMENT_CROSS_H_
#define DFGNN_SEGMENT_CROSS_H_

#include "dfgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DFGNN_SEGMENT_CROSS_ABI_VERSION 1

#define DFGNN_SEGMENT_CROSS_AUTO 0
#define DFGNN_SEGMENT_CROSS_WIDE 1
#define DFGNN_SEGMENT_CROSS_SPLIT 2

int dfgnn_segment_cross_abi_version(void);
int dfgnn_segment_cross_bounds(int m_q, int m_k, int n_seg, const int *seg_ptr_q, const int *seg_ptr_k, int *qbounds,
                               int *kbounds, dfgnn_stream_t stream);
int dfgnn_segment_mha_cross_fwd(int m_q, int m_k, int h, int f, float scale, int form, const int *qbounds, const float *Q,
                                const float *K, const float *V, float *out, float *row_max, float *row_sum,
                                dfgnn_stream_t stream);
int dfgnn_segment_mha_cross_bwd(int m_q, int m_k, int h, int f, float scale, int form, const int *qbounds, const int *kbounds,
                                const float *Q, const float *K, const float *V, const float *row_max, const float *row_sum,
                                const float *dO, float *dQ, float *dK, float *dV, float *delta, dfgnn_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DFGNN_SEGMENT_CROSS_H_ */
