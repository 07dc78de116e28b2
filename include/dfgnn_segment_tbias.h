/* dfgnn_segment_tbias.h -- C ABI of the segment multi-head attention pair WITH A TYPED PAIR BIAS (csrc/segment_mha.hip): the
 * pair of dfgnn_segment_bias.h with the bias looked up in the kernels from a small table instead of read from a plane of
 * h n_pairs floats.  Every pair carries one byte of type, shared by all heads; the learnable table is B[T, h].
 *
 * Nodes, seg_ptr, bounds and row_off are those of dfgnn_segment.h and dfgnn_segment_bias.h (dfgnn_segment_bounds,
 * dfgnn_segment_pair_rows).  For row i of segment [lo, hi), per head hd:
 *   t_ij = min(types[row_off_i + (j - lo)], T - 1)
 *   s_ij = fma(<Q_i, K_j>, scale, B[t_ij, hd])            (the bias pair's logit, the same expression)
 *   P, out, dQ, dK, dV as in dfgnn_segment_bias.h
 *   dB[t, hd] = sum over the valid pairs with t_ij = t of dS_ij
 * types is uint8[n_pairs] in the packed layout of ONE bias plane: graph after graph, each a row-major n_g x n_g block, no
 * padding, a row starts at any byte.  B holds finite values; a large negative finite entry masks a type for a head.
 * row_off is clamped into [0, n_pairs - n_i] and a type into [0, T - 1], so no address outside types, B or the kernels'
 * tables is ever formed (a row whose n_i exceeds n_pairs runs without bias and adds nothing to dB).
 * out, row_max, row_sum, dQ, dK and dV equal TO THE BIT what dfgnn_segment_mha_bias_fwd / _bwd give on the materialised
 * plane bias[hd, p] = B[min(types[p], T - 1), hd].  Nothing of size h n_pairs is read, written or allocated.
 *
 *   dfgnn_segment_mha_tbias_ws_floats   host only: floats of the dB partials workspace `ws` for (m, h, T) -- one [T] per
 *                                       128-row window and head; 0 for m == 0; a negative return code for bad arguments
 *   dfgnn_segment_mha_tbias_fwd         out, and row_max / row_sum unless both are NULL (inference)
 *   dfgnn_segment_mha_tbias_bwd         dQ, dK, dV and, unless dB is NULL, dB[T, h] -- fully written, zeros for absent types
 *                                       and for m without pairs.  dB NULL is a frozen table: no table work at all, ws may be
 *                                       NULL.  delta and ws are scratch the call writes and reads back on the same stream
 * No call allocates, synchronises or reads the device from the host; the grids follow from m, h and T alone, so the calls
 * can be captured in a HIP graph.  All kernels run on `stream`.  No atomics, global or LDS: two calls give the same bits,
 * dB included (per-lane tables in LDS, folded and reduced in a fixed order).
 *
 *   m, h, f          nodes, heads, features per head
 *   bounds           int32[2 m]           (dfgnn_segment_bounds)
 *   row_off          int64[m]             (dfgnn_segment_pair_rows)
 *   n_pairs          sum_g n_g^2: the length of types
 *   types            uint8[n_pairs]
 *   T                number of types, 1 <= T <= 256
 *   B, dB            fp32[T, h], row-major
 *   ws               fp32[dfgnn_segment_mha_tbias_ws_floats(m, h, T)]
 *   Q, K, V, out, dO, dQ, dK, dV   fp32[m, h, f], row-major, 16-byte aligned
 *   row_max, row_sum, delta        fp32[m, h]
 *
 * Return codes: DFGNN_E_BADARG for a negative extent (n_pairs included), h < 1, f < 1, T < 1, one of row_max / row_sum
 * without the other, a NULL required pointer (dB is optional, ws is required only with dB and m > 0); DFGNN_E_UNSUPPORTED for
 * f outside {16, 32, 64, 128}, T > 256, h > 65535, m >= 2^30 or a feature array of 4 GiB or more.  The extents are checked
 * first, then the limits, then the pointers, all before any device call.  m == 0 is a valid no-op, except that a wanted dB
 * is still zeroed. */
#ifndef DFGNN_SEGMENT_TBIAS_H_
#define DFGNN_SEGMENT_TBIAS_H_

#include "dfgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DFGNN_SEGMENT_TBIAS_ABI_VERSION 1

int dfgnn_segment_tbias_abi_version(void);
long long dfgnn_segment_mha_tbias_ws_floats(int m, int h, int T);
int dfgnn_segment_mha_tbias_fwd(int m, int h, int f, float scale, const int *bounds, const long long *row_off, long long n_pairs,
                                const unsigned char *types, int T, const float *B, const float *Q, const float *K, const float *V,
                                float *out, float *row_max, float *row_sum, dfgnn_stream_t stream);
int dfgnn_segment_mha_tbias_bwd(int m, int h, int f, float scale, const int *bounds, const long long *row_off, long long n_pairs,
                                const unsigned char *types, int T, const float *B, const float *Q, const float *K, const float *V,
                                const float *row_max, const float *row_sum, const float *dO, float *dQ, float *dK, float *dV,
                                float *dB, float *ws, float *delta, dfgnn_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DFGNN_SEGMENT_TBIAS_H_ */
