"""GPU-side graph preprocessing through the C ABI (include/dfgnn.h: dfgnn_preprocess_hyper).

COO edge list -> the CSR / sorted-COO-rows / CSC arrays of the reference's preprocess_Hyper and
preprocess_Hyper_fw_bw (DFGNN/layers/util.py:82-100, 116-142), for graphs that live on the GPU.  The reference gets
them from dgl.sparse (`A.csr()`, `torch.sort(A.row)`, `from_csr(...).csc()`); DFGNN/layers/util.py calls this module
instead when the graph is on a CUDA device (CPU graphs keep the torch restatement in DFGNN/utils/sparse.py).
"""
import ctypes

import torch

import dfgnn_native as _n
from _binding_util import call


def coo_to_hyper(src, dst, num_nodes, csc=True):
    """(row_ptr, col_ind, rows, edge_order[, col_ptr, row_ind, val_idx]) as int32 device tensors.

    src / dst: int64 or int32 CUDA tensors of equal length (row = src, column = dst).  Stable: the CSR keeps the COO
    order inside a row, the CSC keeps the CSR order inside a column -- the same arrays as the torch path.
    num_nodes: an int (square adjacency) or a (rows, cols) pair -- a rectangular graph such as a sampled block: src is
    clamped to [0, rows), dst to [0, cols); row_ptr has rows + 1 entries, col_ptr cols + 1."""
    m, n_cols = (int(x) for x in num_nodes) if isinstance(num_nodes, (tuple, list)) else (int(num_nodes), int(num_nodes))
    ext = _n.ext()
    if ext is not None and src.is_cuda and dst.is_cuda:
        return tuple(ext.preprocess_hyper(src, dst, m, bool(csc), n_cols))
    if not (src.is_cuda and dst.is_cuda):
        raise RuntimeError("src / dst must be on CUDA")
    if src.device != dst.device:
        raise RuntimeError(f"every tensor must live on one device ({src.device}), got dst on {dst.device}")
    if src.dtype != dst.dtype or src.dtype not in (torch.int64, torch.int32):
        raise RuntimeError(f"src / dst must both be int64 or int32, got {src.dtype} / {dst.dtype}")
    if src.dim() != 1 or src.shape != dst.shape:
        raise RuntimeError(f"src / dst must be 1-D and of equal length, got {tuple(src.shape)} / {tuple(dst.shape)}")
    src, dst = src.contiguous(), dst.contiguous()
    nnz = src.numel()
    if nnz >= 2 ** 31 or m >= 2 ** 31 or n_cols >= 2 ** 31:
        raise RuntimeError("graphs with 2^31 or more nodes / edges are not supported (int32 index arrays)")
    i32 = dict(dtype=torch.int32, device=src.device)
    outs = [torch.empty(m + 1, **i32), torch.empty(nnz, **i32), torch.empty(nnz, **i32), torch.empty(nnz, **i32)]
    if csc:
        outs += [torch.empty(n_cols + 1, **i32), torch.empty(nnz, **i32), torch.empty(nnz, **i32)]
    size = ctypes.c_size_t(0)
    _n.check(_n.lib().dfgnn_preprocess_ws_bytes_rect(m, n_cols, nnz, ctypes.addressof(size)), "dfgnn_preprocess_hyper")
    ws_bytes = int(size.value)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=src.device)
    call("dfgnn_preprocess_hyper_rect", "dfgnn_preprocess_hyper", src.device, m, n_cols, nnz, src, dst, int(src.dtype == torch.int64),
         *outs, *[None] * (7 - len(outs)), ws, ws_bytes)
    return tuple(outs)
