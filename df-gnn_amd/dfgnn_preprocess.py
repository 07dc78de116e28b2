"""GPU-side graph preprocessing through the C ABI (include/dfgnn.h: dfgnn_preprocess_hyper) and the native neighbour
sampler (include/dfgnn_sample.h: sample_hop).

COO edge list -> the CSR / sorted-COO-rows / CSC arrays of the reference's preprocess_Hyper and
preprocess_Hyper_fw_bw (DFGNN/layers/util.py:82-100, 116-142), for graphs that live on the GPU.  The reference gets
them from dgl.sparse (`A.csr()`, `torch.sort(A.row)`, `from_csr(...).csc()`); DFGNN/layers/util.py calls this module
instead when the graph is on a CUDA device (CPU graphs keep the torch restatement in DFGNN/utils/sparse.py).
"""
import ctypes

import torch

import dfgnn_native as _n
from _binding_util import _KeyedCache, as_int32, call


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


_degree_cache = _KeyedCache()


def max_degree(row_ptr):
    """The largest degree of a CSR structure, computed once per row_ptr tensor (one reduction and one host read) and cached
    like the block plans: a parent graph is sampled every step."""
    key = _KeyedCache.key_of(row_ptr)
    d = _degree_cache.get(key)
    if d is None:
        d = int((row_ptr[1:] - row_ptr[:-1]).max()) if row_ptr.numel() > 1 else 0
        _degree_cache.put(key, d, row_ptr)
    return d


def sample_hop(row_ptr, col_ind, seeds, fanout, seed, csc=True):
    """One hop of the native neighbour sampler (include/dfgnn_sample.h: dfgnn_sample_select, one read of the two output
    sizes, dfgnn_sample_emit) on torch's current stream -> dict of int32 device tensors: row_ptr [m + 1] (the block's),
    parent_edge, col_ind, rows [nnz_b], col_nodes [n_cols_b] and, with csc, col_ptr [n_cols_b + 1], row_ind, val_idx [nnz_b].

    row_ptr / col_ind: the parent graph's int32 CSR arrays on a GPU; seeds: distinct node ids (any integer dtype); seed: 32
    bits.  fanout is clamped to the parent's largest degree (max_degree), which bounds the workspace."""
    if not (row_ptr.is_cuda and col_ind.is_cuda):
        raise RuntimeError("row_ptr / col_ind must be on CUDA")
    dev = row_ptr.device
    if col_ind.device != dev:
        raise RuntimeError(f"every tensor must live on one device ({dev}), got col_ind on {col_ind.device}")
    if row_ptr.dim() != 1 or col_ind.dim() != 1 or row_ptr.numel() < 1:
        raise RuntimeError("row_ptr / col_ind must be 1-D and row_ptr must have n + 1 entries")
    if int(fanout) < 1:
        raise RuntimeError(f"fanout must be at least 1, got {fanout}")
    row_ptr, col_ind = as_int32(row_ptr).contiguous(), as_int32(col_ind).contiguous()
    seeds = torch.as_tensor(seeds, device=dev).to(torch.int32).contiguous().reshape(-1)
    n, m = row_ptr.numel() - 1, seeds.numel()
    fanout = max(1, min(int(fanout), max_degree(row_ptr)))
    i32 = dict(dtype=torch.int32, device=dev)
    size = ctypes.c_size_t(0)
    _n.check(_n.lib().dfgnn_sample_ws_bytes(n, m, fanout, ctypes.addressof(size)), "dfgnn_sample_ws_bytes")
    ws_bytes = int(size.value)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    blk_row_ptr, counts = torch.empty(m + 1, **i32), torch.empty(2, **i32)
    call("dfgnn_sample_select", "dfgnn_sample_select", dev, n, m, fanout, int(seed) & 0xFFFFFFFF, row_ptr, col_ind, seeds,
         blk_row_ptr, counts, ws, ws_bytes)
    nnz_b, n_cols_b = counts.tolist()          # the one host read of a hop
    edge = lambda: torch.empty(nnz_b, **i32)   # noqa: E731
    out = dict(row_ptr=blk_row_ptr, parent_edge=edge(), col_ind=edge(), rows=edge(), col_nodes=torch.empty(n_cols_b, **i32))
    if csc:
        out.update(col_ptr=torch.empty(n_cols_b + 1, **i32), row_ind=edge(), val_idx=edge())
    ptr = lambda name: out[name] if name in out and out[name].numel() else None  # noqa: E731  (an empty tensor has no address)
    call("dfgnn_sample_emit", "dfgnn_sample_emit", dev, n, m, fanout, nnz_b, n_cols_b, row_ptr, col_ind, seeds, blk_row_ptr,
         ptr("parent_edge"), ptr("col_ind"), ptr("rows"), ptr("col_nodes"), out.get("col_ptr"), ptr("row_ind"), ptr("val_idx"),
         ws, ws_bytes)
    return out
