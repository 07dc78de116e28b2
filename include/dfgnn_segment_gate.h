/* dfgnn_segment_gate.h -- C ABI of the segment multi-head attention pair WITH PAIR GATES AND A LOGIT OUTPUT
 * (csrc/segment_gate.hip), next to the biased pair of dfgnn_segment_bias.h: EGT-style global attention over a batch of graphs,
 * for the transformers that keep a feature per node pair (EGT, GRIT / SAN-style layers).
 *
 * Nodes, seg_ptr, bounds, pair_ptr, row_off, n_pairs and the layout of a plane are those of dfgnn_segment_bias.h
 * (dfgnn_segment_bounds, dfgnn_segment_pair_rows).  For row i of segment [lo, hi), key j of the same segment, per head:
 *   x_ij = fma(<Q_i, K_j>, scale, bias_ij),   P_ij = softmax over j in [lo, hi) of x_ij   (row_max / row_sum are those of x)
 *   g_ij = 1 / (1 + exp(-gate_ij))            fp32; finite gates of any size give 0 .. 1, never NaN
 *   out_i = sum_j P_ij g_ij V_j,              logits_ij = x_ij
 * The gate acts AFTER the softmax: it is not renormalised.  The backward, with dA_ij = <dO_i, V_j>:
 *   t_i = sum_j P_ij g_ij dA_ij,   dS_ij = P_ij (g_ij dA_ij - t_i) + dlogits_ij
 *   dQ = scale dS K,   dK = scale dS^T Q,   dV = (P o g)^T dO,   dbias_ij = dS_ij,   dgate_ij = dA_ij P_ij g_ij (1 - g_ij)
 * Every valid pair of logits / dbias / dgate is written exactly once, nothing else of those planes is written.  Nothing of
 * size n^2 is saved by the library: the forward keeps row_max / row_sum, the backward recomputes P and g.
 *
 *   dfgnn_segment_mha_gate_fwd   out, row_max / row_sum unless both are NULL (inference), logits unless it is NULL
 *   dfgnn_segment_mha_gate_bwd   dQ, dK, dV and, unless NULL, dbias and dgate; delta (t_i) is scratch the call writes and reads
 *                                back on the same stream
 * gate == NULL means g = 1 everywhere; dlogits == NULL means that term of dS is absent.  With gate, logits and dlogits all
 * NULL the calls give the bits of dfgnn_segment_mha_bias_fwd / _bwd.  The kernels clamp row_off_i into [0, n_pairs - n_i], so
 * no address outside a plane [h, n_pairs] is ever formed; a row whose n_i exceeds n_pairs runs without bias and gate, reads
 * no dlogits and writes no logits, dbias or dgate.
 * No call allocates, synchronises or reads the device from the host; the grids follow from m and h alone, so the calls can
 * be captured in a HIP graph.  All kernels run on `stream`; no atomics, two calls give the same bits.  The planes are
 * addressed with 64-bit offsets.
 *
 *   m, h, f          nodes, heads, features per head
 *   bounds           int32[2 m]           (dfgnn_segment_bounds)
 *   row_off          int64[m]             (dfgnn_segment_pair_rows)
 *   n_pairs          sum_g n_g^2: the length of a plane
 *   bias, gate, logits, dlogits, dbias, dgate   fp32[h, n_pairs], 4-byte aligned
 *   Q, K, V, out, dO, dQ, dK, dV   fp32[m, h, f], row-major, 16-byte aligned
 *   row_max, row_sum, delta        fp32[m, h]
 *
 * Return codes: DFGNN_E_BADARG for a negative extent (n_pairs included), h < 1, f < 1, one of row_max / row_sum without the
 * other, dgate without gate, a NULL required pointer (gate, logits, dlogits, dbias and dgate are optional);
 * DFGNN_E_UNSUPPORTED for f outside {16, 32, 64, 128}, h > 65535 or a feature array of 4 GiB or more.  The extents are
 * checked first, then the limits, then (for m > 0) the pointers, all before any device call.  m == 0 is a valid no-op that
 * writes nothing. */
#ifndef DFGNN_SEGMENT_GATE_H_
#define DFGNN_SEGMENT_GATE_H_

#include "dfgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DFGNN_SEGMENT_GATE_ABI_VERSION 1

int dfgnn_segment_gate_abi_version(void);
int dfgnn_segment_mha_gate_fwd(int m, int h, int f, float scale, const int *bounds, const long long *row_off, long long n_pairs,
                               const float *bias, const float *gate, const float *Q, const float *K, const float *V,
                               float *out, float *row_max, float *row_sum, float *logits, dfgnn_stream_t stream);
int dfgnn_segment_mha_gate_bwd(int m, int h, int f, float scale, const int *bounds, const long long *row_off, long long n_pairs,
                               const float *bias, const float *gate, const float *Q, const float *K, const float *V,
                               const float *row_max, const float *row_sum, const float *dO, const float *dlogits,
                               float *dQ, float *dK, float *dV, float *dbias, float *dgate, float *delta, dfgnn_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DFGNN_SEGMENT_GATE_H_ */
