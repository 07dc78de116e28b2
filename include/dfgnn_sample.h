/* dfgnn_sample.h -- C ABI of the GPU neighbour sampler (csrc/sample.hip), next to the conv ABI of dfgnn.h.
 *
 * One hop of uniform neighbour sampling without replacement on a parent graph in CSR form.  The sampled block comes back
 * with its CSR and CSC arrays already made -- what dfgnn_preprocess_hyper_rect would make of its edge list -- so the pairs
 * that take an m x n_cols graph run on it directly.  Nothing is sorted by row, nothing of parent-graph size in ints is
 * initialised; the only sort is the column sort of the kept edges (the CSC half).
 *
 * WHICH EDGES ARE KEPT is defined by result, so that a host reference reproduces the device bit for bit:
 *   mix(x), uint32:  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16      (a bijection)
 *   key(p) = mix(p ^ mix(seed))     for the parent edge at CSR position p; distinct positions have distinct keys
 *   a seed row of parent degree d keeps all its edges if d <= fanout, otherwise the `fanout` edges of smallest key;
 *   kept edges stand in parent order (increasing p) inside their row; duplicate parent edges are distinct edges.
 * THE BLOCK: row r is seeds[r] (distinct node ids in [0, n)); col_nodes begins with the seeds in the given order, every
 * other sampled node follows in increasing id; the block's column ids index col_nodes.
 *
 * Two calls per hop, with one device-to-host read between them (the two sizes the output shapes need):
 *   dfgnn_sample_select   writes blk_row_ptr, chooses the edges, marks the nodes they reach, writes counts = {nnz_b,
 *                         n_cols_b} (device) and leaves its choice in ws
 *   ... the caller reads counts and allocates ...
 *   dfgnn_sample_emit     reads that ws (it must not be refilled in between) and writes the edge list and the CSC half
 * Neither call synchronises or allocates; both run on `stream`.  Every array is int32.  The kernels use integer
 * arithmetic only and nothing whose order can change a result: two calls give the same bits.
 *
 *   n, m           nodes of the parent graph; seeds (= rows of the block)
 *   fanout         edges kept per row at most, >= 1.  The workspace grows with m * fanout: a caller that wants every
 *                  neighbour passes the parent's largest degree, not INT_MAX
 *   seed           the 32-bit seed of the key function
 *   row_ptr        int32[n + 1], col_ind int32[row_ptr[n]]: the parent graph; col_ind is read at kept edges only and may be
 *                  NULL for a parent without edges.  An id outside [0, n) in col_ind or seeds is clamped into it
 *   seeds          int32[m]
 *   blk_row_ptr    int32[m + 1]: written by select, read by emit
 *   counts         int32[2], device: nnz_b = blk_row_ptr[m] and n_cols_b = m + the sampled nodes that are no seeds
 *   parent_edge    int32[nnz_b]: the parent CSR position of each kept edge -- what a caller gathers etype, score or E through
 *   blk_col_ind    int32[nnz_b]: column ids into col_nodes, CSR order
 *   rows           int32[nnz_b]: the sorted row ids (the `rows` of dfgnn_preprocess_hyper_rect)
 *   col_nodes      int32[n_cols_b]
 *   col_ptr        int32[n_cols_b + 1], row_ind, val_idx int32[nnz_b]: the CSC half with the meaning of
 *                  dfgnn_preprocess_hyper_rect -- a stable sort of the CSR list by column, val_idx the CSR slot.  All three
 *                  NULL: no CSC.  With nnz_b == 0 the per-edge pointers may be NULL and col_ptr is all zero
 *   nnz_b, n_cols_b  what select wrote to counts; emit writes no slot at or past them whatever ws holds
 *   ws, ws_bytes   dfgnn_sample_ws_bytes(n, m, fanout, &bytes) bytes, 256-byte aligned, shared by the two calls.  With
 *                  W = ceil(n / 32), E = m * fanout and a(x) = x rounded up to a multiple of 256:
 *                    a(8 W)         two bitmaps of n bits, seeds and reached nodes (the only part zeroed per call)
 *                  + a(4 (W + 1))   nodes that are reached and no seeds, counted before each bitmap word (written by a scan)
 *                  + a(4 n)         block row of a node, written at the seeds and read only where the seed bitmap is set
 *                  + a(4 (m + 1))   per row, the largest key kept; then the key function's mixed seed
 *                  + a(10 E + 65536)  storage of the column sort of the kept edges
 *                  + a(4 E)         the sorted column keys
 *
 * Return codes: DFGNN_E_BADARG for a negative extent, fanout < 1, bytes == NULL, m > 0 with n == 0, a NULL required
 * pointer, a workspace smaller than dfgnn_sample_ws_bytes, nnz_b > m * fanout, n_cols_b < m or > m + nnz_b, one CSC pointer
 * without col_ptr; DFGNN_E_UNSUPPORTED for m * fanout >= 2^31 or m = 2^31 - 1.  The extents are checked first, then the size limit, then
 * the pointers.  m == 0 is a valid no-op: select writes blk_row_ptr[0] = 0 and counts = {0, 0}, emit col_ptr[0] = 0.
 * dfgnn_sample_ws_bytes is host-only. */
#ifndef DFGNN_SAMPLE_H_
#define DFGNN_SAMPLE_H_

#include <stddef.h>

#include "dfgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DFGNN_SAMPLE_ABI_VERSION 1

int dfgnn_sample_abi_version(void);
int dfgnn_sample_ws_bytes(int n, int m, int fanout, size_t *bytes);
int dfgnn_sample_select(int n, int m, int fanout, unsigned seed, const int *row_ptr, const int *col_ind, const int *seeds,
                        int *blk_row_ptr, int *counts, void *ws, size_t ws_bytes, dfgnn_stream_t stream);
int dfgnn_sample_emit(int n, int m, int fanout, int nnz_b, int n_cols_b, const int *row_ptr, const int *col_ind,
                      const int *seeds, const int *blk_row_ptr, int *parent_edge, int *blk_col_ind, int *rows,
                      int *col_nodes, int *col_ptr, int *row_ind, int *val_idx, void *ws, size_t ws_bytes,
                      dfgnn_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* DFGNN_SAMPLE_H_ */
