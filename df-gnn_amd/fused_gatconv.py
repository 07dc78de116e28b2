"""`fused_gatconv` -- drop-in for the reference's extension module of the same name
(PYBIND11_MODULE(fused_gatconv), DFGNN/src/fused_gatconv/fused_gatconv.cpp:355-372), bound to the
MI355X HIP library through its C ABI (include/dfgnn.h).  See fused_gtconv.py for the conventions.

In scope: the four inference entry points of the hyper / softmax /
softmax_gm / tiling variants, and the training pair gat_forward / gat_backward
behind FusedGATFunction and (8f rank 3) the hyper_v2 / hyper_recompute entry points of the reference's comparison
sweeps.  gat_forward_tb (the reference's tile-scheduler experiment, no Python caller there) returns the same three
tensors from the training forward; its schedule argument only distributes work and is validated, not followed.
"""
import torch

import dfgnn_native as _n
from _binding_util import (_KeyedCache, as_int32, call, check_2d, check_3d, check_cols, check_csc, check_csc_rect, check_csr, check_edges,
                           check_family, check_feats, get_plan_obj, get_rows, plan_ptrs)

# Set to False to force the general (plan-less) kernels; results are identical either way.
USE_BLOCK_PLAN = True


def _check(attn_row, attn_col, indptr, indices, rows, in_feat):
    """What every GAT operator checks: in_feat fp32 [nodes, heads, feat], the CSR arrays of those nodes, the per-node
    scores [m, h] and -- where the operator takes them -- the COO rows -> (m, nnz, h, f)."""
    m, h, f = check_feats(in_feat=in_feat)
    nnz = check_csr(in_feat, m, indptr, indices)
    check_2d(in_feat, m, h, attn_row=attn_row, attn_col=attn_col)
    if rows is not None:
        check_edges(in_feat, nnz, torch.int32, rows=rows)
    return m, nnz, h, f


def _empty(like, *shape):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def gat_inference_hyper(smem_consume, attn_row, attn_col, indptr, indices, rows, negative_slope, in_feat):
    """fused_gatconv.cpp:99-119 -> Tensor out[m, h, f]"""
    plan = get_plan_obj(indptr, indices, in_feat, USE_BLOCK_PLAN)
    need_ws = plan is not None and plan.num_edge_global > 0   # scratch for per-edge values of the plan's edge-global ranges
    ext = _n.ext()
    if ext is not None:  # torch C++ binding (csrc/torch_ext.cpp): same checks, same C ABI call
        return ext.gat_hyper_fwd(attn_row, attn_col, indptr, indices, rows, float(negative_slope), in_feat,
                                 *plan_ptrs(plan), need_ws)
    m, nnz, h, f = _check(attn_row, attn_col, indptr, indices, rows, in_feat)
    out = torch.empty_like(in_feat)
    ws = _empty(in_feat, h, nnz) if need_ws else None
    call("dfgnn_gat_hyper_fwd", "gat_inference_hyper", in_feat.device, m, nnz, h, f, indptr, indices, rows, attn_row,
         attn_col, float(negative_slope), in_feat, ws, out, *plan_ptrs(plan))
    return out


def gat_inference_hyper_ablation(smem_consume, attn_row, attn_col, indptr, indices, rows, negative_slope,
                                 in_feat):
    """fused_gatconv.cpp (ablation study entry): served by the production kernel."""
    return gat_inference_hyper(smem_consume, attn_row, attn_col, indptr, indices, rows, negative_slope, in_feat)


def _softmax(name, attn_row, attn_col, indptr, indices, rows, negative_slope, in_feat):
    """name: 'softmax' (logits staged in LDS) or 'softmax_gm' (re-read from global memory)."""
    ext = _n.ext()
    if ext is not None:
        return ext.gat_softmax_fwd(attn_row, attn_col, indptr, indices, rows, float(negative_slope), in_feat,
                                   name == "softmax")
    m, nnz, h, f = _check(attn_row, attn_col, indptr, indices, rows, in_feat)
    out, logits = torch.empty_like(in_feat), _empty(in_feat, h, nnz)
    call(f"dfgnn_gat_{name}_fwd", f"gat_inference_{name}", in_feat.device, m, nnz, h, f, indptr, indices, rows, attn_row,
         attn_col, float(negative_slope), in_feat, logits, out)
    return out


def gat_inference_softmax(smem_consume, attn_row, attn_col, indptr, indices, rows, negative_slope, in_feat):
    """fused_gatconv.cpp:40-61 -> Tensor"""
    return _softmax("softmax", attn_row, attn_col, indptr, indices, rows, negative_slope, in_feat)


def gat_inference_softmax_gm(attn_row, attn_col, indptr, indices, rows, negative_slope, in_feat):
    """fused_gatconv.cpp:69-90 -> Tensor"""
    return _softmax("softmax_gm", attn_row, attn_col, indptr, indices, rows, negative_slope, in_feat)


# ---- 'tiling' on super-node full graphs: column chunks that fit an XCD's L2 (csrc/gat_tiling_chunked.hip) -----------------
# The chunk-major edge order of a graph is preprocessing, like the block plan of a batch: built on first use, cached by
# the identity of the CSR arrays' memory.  TILING_CHUNK_ROWS = 0 keeps the single-kernel form everywhere.
# Rows of a chunk: TILING_CHUNK_BYTES / (4 f), a multiple of 1024, at most 32768 (16-bit column offsets).  6 MiB per chunk
# measured best on the reddit-like graph at f = 128 (12288 rows: 4.28 ms; 8192 rows = one XCD's 4 MiB L2: 4.89 ms -- more
# chunks, more partial states; 16384 rows: 4.74 ms; the single-kernel form: 8.27 ms).  0 = the single-kernel form everywhere.
TILING_CHUNK_BYTES = 6 << 20
TILING_CHUNK_ROWS = None           # tests: a fixed number of rows per chunk instead
TILING_CHUNK_MIN_TABLE = 64 << 20  # feature table (bytes) below which the L2s hold it anyway
TILING_CHUNK_MIN_DEGREE = 64       # average degree below which a row of X is not re-used enough to pay for the partial states
_chunk_cache = _KeyedCache(entries=4)


def _tiling_chunks(row_ptr, col_ind, chunk_rows):
    """(seg_ptr int32[nchunks m + 1], ccol int16[nnz]) of include/dfgnn.h: dfgnn_gat_tiling_chunked_fwd."""
    key = _KeyedCache.key_of(row_ptr, col_ind, extra=(chunk_rows,))
    hit = _chunk_cache.get(key)
    if hit is None:
        m, nnz = row_ptr.size(0) - 1, col_ind.size(0)
        nchunks = (m + chunk_rows - 1) // chunk_rows
        with torch.cuda.device(col_ind.device):
            chunk = torch.div(col_ind, chunk_rows, rounding_mode="floor").to(torch.int16)
            order = torch.sort(chunk, stable=True).indices           # CSR (row-major) order survives inside a chunk
            ccol = (col_ind - chunk.to(torch.int32) * chunk_rows).to(torch.int16)[order].contiguous()
            rows = get_rows(row_ptr, nnz)
            counts = torch.bincount(chunk.long() * m + rows.long(), minlength=nchunks * m)
            seg_ptr = torch.zeros(nchunks * m + 1, dtype=torch.int32, device=col_ind.device)
            seg_ptr[1:] = torch.cumsum(counts, 0).to(torch.int32)
            del chunk, order, counts
        hit = _chunk_cache.put(key, (seg_ptr, ccol), row_ptr, col_ind)
    return hit


def _chunk_rows(f):
    if TILING_CHUNK_ROWS is not None:
        return int(TILING_CHUNK_ROWS)
    return min(32768, (TILING_CHUNK_BYTES // (4 * f)) // 1024 * 1024)


def _use_chunked_tiling(m, nnz, h, f):
    return (_chunk_rows(f) > 0 and m * h * f * 4 >= TILING_CHUNK_MIN_TABLE and nnz >= TILING_CHUNK_MIN_DEGREE * m and
            nnz < 2 ** 31)


def gat_inference_tiling(attn_row, attn_col, row_ptr, col_ind, negative_slope, in_feat):
    """fused_gatconv.cpp:196-219 -> Tensor"""
    if in_feat.dim() == 3 and in_feat.is_cuda and row_ptr.dim() == 1 and col_ind.dim() == 1 and \
            _use_chunked_tiling(row_ptr.size(0) - 1, col_ind.size(0), in_feat.size(1), in_feat.size(2)):
        m, nnz, h, f = _check(attn_row, attn_col, row_ptr, col_ind, None, in_feat)
        chunk_rows = _chunk_rows(f)
        seg_ptr, ccol = _tiling_chunks(row_ptr, col_ind, chunk_rows)
        out = torch.empty_like(in_feat)
        ws_bytes = int(_n.lib().dfgnn_gat_tiling_chunked_ws_bytes(m, h, f, chunk_rows))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=in_feat.device)
        call("dfgnn_gat_tiling_chunked_fwd", "gat_inference_tiling (chunked)", in_feat.device, m, nnz, h, f, chunk_rows,
             seg_ptr, ccol, attn_row, attn_col, float(negative_slope), in_feat, out, ws, ws_bytes)
        return out
    ext = _n.ext()
    if ext is not None:
        return ext.gat_tiling_fwd(attn_row, attn_col, row_ptr, col_ind, float(negative_slope), in_feat)
    m, nnz, h, f = _check(attn_row, attn_col, row_ptr, col_ind, None, in_feat)
    out = torch.empty_like(in_feat)
    call("dfgnn_gat_tiling_fwd", "gat_inference_tiling", in_feat.device, m, nnz, h, f, row_ptr, col_ind, attn_row, attn_col,
         float(negative_slope), in_feat, out)
    return out


def gat_inference(attn_row, attn_col, row_ptr, col_ind, negative_slope, in_feat):
    """fused_gatconv.cpp (dgNN node-parallel CSR inference): same function as the
    tiling kernel, which serves it."""
    return gat_inference_tiling(attn_row, attn_col, row_ptr, col_ind, negative_slope, in_feat)


def gat_inference_hyper_recompute(attn_row, attn_col, indptr, indices, negative_slope, in_feat):
    """fused_gatconv.cpp:124-142 -> Tensor.  CSR only; node-parallel, no logit storage: the rank-one logits are recomputed
    in each of the three sweeps (max, sum, weighted sum), like the reference's kernel
    (fused_gatconv_hyper_recompute.cu:118-216) -- csrc/csr_fwd.hip:gat_recompute_fwd_kernel; any f (the reference exit(0)s
    unless f % 128 == 0)."""
    m, nnz, h, f = _check(attn_row, attn_col, indptr, indices, None, in_feat)
    out = torch.empty_like(in_feat)
    call("dfgnn_gat_recompute_fwd", "gat_inference_hyper_recompute", in_feat.device, m, nnz, h, f, indptr, indices,
         attn_row, attn_col, float(negative_slope), in_feat, out)
    return out


def gat_inference_hyper_v2(smem_consume, a_l, a_r, indptr, indices, negative_slope, in_feat):
    """fused_gatconv.cpp:148-158 -> Tensor.  a_l, a_r: the layer's attention vectors, [heads, f] (a leading 1 is
    accepted, as the layers pass them).  Two kernels like the reference's (fused_gatconv_hyper_v2.cu:251-281): the
    per-node scores <a_l, X_i>, <a_r, X_i> in one pass over X, then the fused 'hyper' convolution -- with a block plan
    and the COO rows derived from indptr (this entry point takes CSR only), else the CSR tiling kernel.
    The reference reads a_l / a_r as contiguous [heads, f] whatever their strides (the layers hand it a transposed
    view: only right for heads == 1); here they are made contiguous first."""
    m, h, f = check_feats(in_feat=in_feat)
    a_l, a_r = a_l.reshape(-1, a_l.shape[-1]).contiguous(), a_r.reshape(-1, a_r.shape[-1]).contiguous()
    check_family(in_feat, torch.float32, a_l=a_l, a_r=a_r)
    if tuple(a_l.shape) != (h, f) or tuple(a_r.shape) != (h, f):
        raise RuntimeError(f"a_l / a_r must have shape ({h}, {f}), got {tuple(a_l.shape)} / {tuple(a_r.shape)}")
    attn_row, attn_col = _empty(in_feat, m, h), _empty(in_feat, m, h)
    call("dfgnn_gat_attn_scores", "gat_inference_hyper_v2 (scores)", in_feat.device, m, h, f, a_l, a_r, in_feat, attn_row,
         attn_col)
    _check(attn_row, attn_col, indptr, indices, None, in_feat)
    if get_plan_obj(indptr, indices, f, USE_BLOCK_PLAN) is not None:
        return gat_inference_hyper(smem_consume, attn_row, attn_col, indptr, indices, get_rows(indptr, indices.size(0)),
                                   negative_slope, in_feat)
    return gat_inference_tiling(attn_row, attn_col, indptr, indices, negative_slope, in_feat)


def _train_plan(row_ptr, col_ind, f, attn_drop):
    """(rows, plan, meta) for the training pair: the block plan and the COO row ids when the batch may qualify for
    the matrix-core kernels (the library checks that every range of the plan is dense), else Nones."""
    plan = get_plan_obj(row_ptr, col_ind, f, USE_BLOCK_PLAN)
    if plan is None:
        return None, None, None
    return (get_rows(row_ptr, col_ind.size(0)),) + plan.ptrs()


def _drop(attn_drop):
    attn_drop = float(attn_drop)
    if not 0.0 <= attn_drop < 1.0:
        raise RuntimeError(f"attn_drop must be in [0, 1), got {attn_drop}")
    return attn_drop


def gat_forward(attn_row, attn_col, row_ptr, col_ind, negative_slope, in_feat, attn_drop):
    """fused_gatconv.cpp:11-32 -> [out_feat[m,h,f], edge_max[m,h], edge_sum[m,h], edge_mask[nnz,h]]

    edge_mask holds the uniform randoms of the attention dropout (the reference fills it with cuRAND seeded by
    clock(), fused_gatconv_kernel.cu:1074-1083; here torch.rand, so torch.manual_seed reproduces a run).  With
    attn_drop == 0 nothing is dropped and no randoms are drawn: edge_mask is then a stride-0 view of a single 1.0
    (same shape, no memory), which gat_backward accepts for attn_drop == 0."""
    ext = _n.ext()
    if ext is None or in_feat.dim() != 3 or not in_feat.is_cuda:   # (the ctypes transport, or its error for such an in_feat)
        m, nnz, h, f = _check(attn_row, attn_col, row_ptr, col_ind, None, in_feat)
        attn_drop = _drop(attn_drop)
    else:
        attn_drop, nnz, h, f = float(attn_drop), col_ind.size(0), in_feat.size(1), in_feat.size(2)
    if attn_drop > 0.0:
        edge_mask = torch.rand((nnz, h), dtype=torch.float32, device=in_feat.device)
    else:
        edge_mask = torch.ones((1, 1), dtype=torch.float32, device=in_feat.device).expand(nnz, h)
    rows, plan, meta = _train_plan(row_ptr, col_ind, f, attn_drop)
    mask = edge_mask if attn_drop > 0.0 else None
    if ext is not None:
        # torch C++ binding (csrc/torch_ext.cpp): same checks, same C ABI call, ~5 us of host time instead of ~50
        out, edge_max, edge_sum = ext.gat_fwd_train(attn_row, attn_col, row_ptr, col_ind, rows, float(negative_slope), in_feat,
                                                    mask, attn_drop, plan or 0, meta or 0)
        return [out, edge_max, edge_sum, edge_mask]
    out, edge_max, edge_sum = torch.empty_like(in_feat), _empty(in_feat, m, h), _empty(in_feat, m, h)
    call("dfgnn_gat_fwd_train", "gat_forward", in_feat.device, m, nnz, h, f, row_ptr, col_ind, rows, attn_row, attn_col,
         float(negative_slope), in_feat, mask, attn_drop, edge_max, edge_sum, out, plan, meta)
    return [out, edge_max, edge_sum, edge_mask]


def gat_backward(negative_slope, attn_drop, row_ptr, col_ind, col_ptr, row_ind, permute, edge_max, edge_sum,
                 edge_mask, in_feat, attn_row, attn_col, grad):
    """fused_gatconv.cpp:291-353 -> [grad_feat[m,h,f], grad_attn_row[m,h], grad_attn_col[m,h]]"""
    permute = as_int32(permute)      # (dgl hands the CSC -> CSR permutation over as int64, like GT's val_idx)
    ext = _n.ext()
    if ext is not None and in_feat.dim() == 3 and in_feat.is_cuda:
        attn_drop = float(attn_drop)
        rows, plan, meta = _train_plan(row_ptr, col_ind, in_feat.size(2), attn_drop)
        return ext.gat_bwd(float(negative_slope), attn_drop, row_ptr, col_ind, rows, col_ptr, row_ind, permute,
                           edge_max, edge_sum, edge_mask if attn_drop > 0.0 else None, in_feat, attn_row, attn_col, grad,
                           plan or 0, meta or 0)
    m, nnz, h, f = _check(attn_row, attn_col, row_ptr, col_ind, None, in_feat)
    attn_drop = _drop(attn_drop)
    check_feats(in_feat=in_feat, grad=grad)
    check_2d(in_feat, m, h, edge_max=edge_max, edge_sum=edge_sum)
    check_csc(in_feat, m, nnz, col_ptr, row_ind=row_ind, permute=permute)
    if attn_drop > 0.0:
        check_2d(in_feat, nnz, h, edge_mask=edge_mask)
    grad_feat, grad_edge = torch.empty_like(in_feat), _empty(in_feat, h, nnz)
    grad_attn_row, grad_attn_col = _empty(in_feat, m, h), _empty(in_feat, m, h)
    rows, plan, meta = _train_plan(row_ptr, col_ind, f, attn_drop)
    call("dfgnn_gat_bwd", "gat_backward", in_feat.device, m, nnz, h, f, row_ptr, col_ind, rows, col_ptr, row_ind, permute,
         attn_row, attn_col, float(negative_slope), in_feat, edge_max, edge_sum, edge_mask if attn_drop > 0.0 else None,
         attn_drop, grad, grad_edge, grad_feat, grad_attn_row, grad_attn_col, plan, meta)
    return [grad_feat, grad_attn_row, grad_attn_col]


def gat_forward_tb(attn_row, attn_col, row_ptr, col_ind, negative_slope, in_feat, tile_scheduler):
    """fused_gatconv.cpp:256-282 -> [out_feat[m,h,f], edge_max[m,h], edge_sum[m,h]].

    The reference's kernel (fused_gatconv_kernel.cu:976-1060) walks `tile_scheduler` -- int32 (row, 32-edge tile of the
    row) pairs -- one workgroup per entry, and combines the tiles of a row through atomics on edge_max / edge_sum with
    no grid-wide synchronisation (its result depends on workgroup timing).  The schedule only says who computes what;
    the values it is meant to produce are those of gat_forward without dropout, which is what this returns (the MI355X
    kernels split heavy rows themselves)."""
    check_feats(in_feat=in_feat)
    check_family(in_feat, torch.int32, tile_scheduler=tile_scheduler)
    out, edge_max, edge_sum, _ = gat_forward(attn_row, attn_col, row_ptr, col_ind, negative_slope, in_feat, 0.0)
    return [out, edge_max, edge_sum]


# ---- GATv2 (include/dfgnn.h: dfgnn_gatv2_fwd / dfgnn_gatv2_bwd; csrc/gatv2_train.hip) -----------------------------------
# Not part of the reference's module.  The logit of edge (i, j) is sum_d attn[h, d] LeakyReLU(X_row[i, h, d] + X_col[j, h, d]):
# not rank-one, so no per-node scores exist to hand over -- the operators take the attention vector and the two projected
# feature tensors themselves.  Any graph, no plan, any f; nothing of size nnz is allocated.


def _check_v2(attn, row_ptr, col_ind, X_row, X_col, **like_X):
    """What every GATv2 operator checks: X_row (and `like_X`: out, grad) fp32 [m, heads, feat], X_col fp32 [n_cols, heads,
    feat] -- the graph may be rectangular: m rows, n_cols columns --, attn fp32 [heads, feat], the CSR arrays of the m rows
    -> (m, n_cols, nnz, h, f)."""
    m, h, f = check_feats(X_row=X_row, **like_X)
    n_cols = check_cols("X_row", X_row, X_col=X_col)
    check_2d(X_row, h, f, attn=attn)
    return m, n_cols, check_csr(X_row, m, row_ptr, col_ind), h, f


def _gatv2_fwd(what, save_stats, attn, row_ptr, col_ind, negative_slope, X_row, X_col):
    ext = _n.ext()
    if ext is not None:
        return ext.gatv2_fwd(attn, row_ptr, col_ind, float(negative_slope), X_row, X_col, save_stats)
    m, n_cols, nnz, h, f = _check_v2(attn, row_ptr, col_ind, X_row, X_col)
    out = torch.empty_like(X_row)
    row_max, row_sum = (_empty(X_row, m, h), _empty(X_row, m, h)) if save_stats else (None, None)
    call("dfgnn_gatv2_fwd_rect", what, X_row.device, m, n_cols, nnz, h, f, row_ptr, col_ind, attn, float(negative_slope), X_row, X_col,
         row_max, row_sum, out)
    return [out, row_max, row_sum] if save_stats else [out]


def gatv2_inference(attn, row_ptr, col_ind, negative_slope, X_row, X_col):
    """-> out[m, h, f].  X_row and X_col may be the same tensor (shared weights)."""
    return _gatv2_fwd("gatv2_inference", False, attn, row_ptr, col_ind, negative_slope, X_row, X_col)[0]


def gatv2_forward(attn, row_ptr, col_ind, negative_slope, X_row, X_col):
    """-> [out, row_max[m, h], row_sum[m, h]]: the training forward; the same `out` as gatv2_inference."""
    return _gatv2_fwd("gatv2_forward", True, attn, row_ptr, col_ind, negative_slope, X_row, X_col)


def gatv2_backward(negative_slope, row_ptr, col_ind, col_ptr, row_ind, attn, X_row, X_col, out, row_max, row_sum, grad):
    """-> [dX_row, dX_col, dattn[h, f]] from the forward's output and row statistics (each edge is recomputed).  With
    X_row is X_col the gradient of the shared tensor is dX_row + dX_col."""
    ext = _n.ext()
    if ext is not None:
        return ext.gatv2_bwd(float(negative_slope), row_ptr, col_ind, col_ptr, row_ind, attn, X_row, X_col, out, row_max,
                             row_sum, grad)
    m, n_cols, nnz, h, f = _check_v2(attn, row_ptr, col_ind, X_row, X_col, out=out, grad=grad)
    check_csc_rect(X_row, n_cols, nnz, col_ptr, "X_col", row_ind=row_ind)
    check_2d(X_row, m, h, row_max=row_max, row_sum=row_sum)
    dX_row, dX_col = torch.empty_like(X_row), torch.empty_like(X_col)
    if m == 0 and n_cols == 0:
        return [dX_row, dX_col, torch.zeros_like(attn)]    # (nothing to launch: no edge adds to dattn)
    ws_floats = int(_n.lib().dfgnn_gatv2_bwd_ws_floats(h, f))
    if ws_floats < 0:
        _n.check(ws_floats, "gatv2_backward")
    delta, ws, dattn = _empty(X_row, m, h), _empty(X_row, ws_floats), torch.empty_like(attn)
    call("dfgnn_gatv2_bwd_rect", "gatv2_backward", X_row.device, m, n_cols, nnz, h, f, row_ptr, col_ind, col_ptr, row_ind, attn,
         float(negative_slope), X_row, X_col, out, row_max, row_sum, grad, delta, ws, dX_row, dX_col, dattn)
    return [dX_row, dX_col, dattn]


# ---- GATv2 with a per-edge feature vector inside the LeakyReLU (include/dfgnn.h: dfgnn_gatv2_fwd_edge / dfgnn_gatv2_bwd_edge) ---
# Not part of the reference's module.  The pair above with z_e = X_row[i] + X_col[j] + E_e (csrc/gatv2_edge_train.hip), what
# PyG's GATv2Conv(edge_dim) computes: E is fp32[nnz, h, f] in CSR edge order and is not part of the message.
# DFGNN.operators.fused_gatconv.GATv2ConvFuse_edge takes it.


def _gatv2_fwd_edge(what, save_stats, attn, row_ptr, col_ind, negative_slope, X_row, X_col, E):
    ext = _n.ext()
    if ext is not None:
        return ext.gatv2_fwd_edge(attn, row_ptr, col_ind, float(negative_slope), X_row, X_col, E, save_stats)
    m, n_cols, nnz, h, f = _check_v2(attn, row_ptr, col_ind, X_row, X_col)
    check_3d(X_row, nnz, h, f, E=E)
    out = torch.empty_like(X_row)
    row_max, row_sum = (_empty(X_row, m, h), _empty(X_row, m, h)) if save_stats else (None, None)
    call("dfgnn_gatv2_fwd_edge_rect", what, X_row.device, m, n_cols, nnz, h, f, row_ptr, col_ind, attn, float(negative_slope),
         X_row, X_col, E, row_max, row_sum, out)
    return [out, row_max, row_sum] if save_stats else [out]


def gatv2_inference_edge(attn, row_ptr, col_ind, negative_slope, X_row, X_col, E):
    """-> out[m, h, f] with the edge features fp32[nnz, h, f] (CSR order) added inside the LeakyReLU.  X_row and X_col may be
    the same tensor (shared weights)."""
    return _gatv2_fwd_edge("gatv2_inference_edge", False, attn, row_ptr, col_ind, negative_slope, X_row, X_col, E)[0]


def gatv2_forward_edge(attn, row_ptr, col_ind, negative_slope, X_row, X_col, E):
    """-> [out, row_max[m, h], row_sum[m, h]]: the training forward; the same `out` as gatv2_inference_edge."""
    return _gatv2_fwd_edge("gatv2_forward_edge", True, attn, row_ptr, col_ind, negative_slope, X_row, X_col, E)


def gatv2_backward_edge(negative_slope, row_ptr, col_ind, col_ptr, row_ind, val_idx, attn, X_row, X_col, E, out, row_max,
                        row_sum, grad, want_dE=True):
    """-> [dX_row, dX_col, dattn[h, f], dE[nnz, h, f]] from the forward's output and row statistics (each edge is
    recomputed); dE is None without want_dE (then nothing of size nnz h f is allocated or written).  val_idx: the CSR
    position of each CSC entry, through which the column pass finds an entry's row of E."""
    if val_idx is None:
        raise RuntimeError("gatv2_backward_edge: val_idx is required (the column pass finds an entry's row of E through it)")
    val_idx = as_int32(val_idx)
    ext = _n.ext()
    if ext is not None:
        res = ext.gatv2_bwd_edge(float(negative_slope), row_ptr, col_ind, col_ptr, row_ind, val_idx, attn, X_row, X_col, E, out,
                                 row_max, row_sum, grad, want_dE)
        return res if want_dE else res + [None]
    m, n_cols, nnz, h, f = _check_v2(attn, row_ptr, col_ind, X_row, X_col, out=out, grad=grad)
    check_3d(X_row, nnz, h, f, E=E)
    check_csc_rect(X_row, n_cols, nnz, col_ptr, "X_col", row_ind=row_ind, val_idx=val_idx)
    check_2d(X_row, m, h, row_max=row_max, row_sum=row_sum)
    dX_row, dX_col = torch.empty_like(X_row), torch.empty_like(X_col)
    dE = torch.empty_like(E) if want_dE else None
    if m == 0 and n_cols == 0:
        return [dX_row, dX_col, torch.zeros_like(attn), dE]    # (nothing to launch: no edge adds to dattn)
    ws_floats = int(_n.lib().dfgnn_gatv2_bwd_ws_floats(h, f))
    if ws_floats < 0:
        _n.check(ws_floats, "gatv2_backward_edge")
    delta, ws, dattn = _empty(X_row, m, h), _empty(X_row, ws_floats), torch.empty_like(attn)
    call("dfgnn_gatv2_bwd_edge_rect", "gatv2_backward_edge", X_row.device, m, n_cols, nnz, h, f, row_ptr, col_ind, col_ptr, row_ind,
         val_idx, attn, float(negative_slope), X_row, X_col, E, out, row_max, row_sum, grad, delta, ws, dX_row, dX_col, dattn, dE)
    return [dX_row, dX_col, dattn, dE]


# ---- GAT for any graph with an optional per-edge attention term (include/dfgnn.h: dfgnn_gat_fwd_edge / dfgnn_gat_bwd_edge) ------
# Not part of the reference's module.  The logit of edge (i, j) is LeakyReLU(attn_row[i] + attn_col[j] + score[h, e]): the
# rank-one GAT of gat_forward / gat_backward on an m x n_cols graph (csrc/gat_edge_train.hip), with what PyG's
# GATConv(edge_dim) adds inside the LeakyReLU.  in_feat holds the SOURCES, fp32[n_cols, h, f]; attn_row is [m, h], attn_col
# [n_cols, h]; score is fp32[h, nnz] in CSR edge order or None.  No plan, any f; nothing of size nnz is allocated beyond the
# dropout randoms and, when wanted, grad_score.  DFGNN.operators.fused_gatconv.GATConvFuse_edge takes it.


def _check_edge(attn_row, attn_col, row_ptr, col_ind, score, in_feat):
    """What every operator of the pair checks -> (m, n_cols, nnz, h, f)."""
    n_cols, h, f = check_feats(X=in_feat)
    check_family(in_feat, torch.int32, indptr=row_ptr, indices=col_ind)
    if row_ptr.dim() != 1 or col_ind.dim() != 1:
        raise RuntimeError("indptr / indices must be 1-D")
    if row_ptr.size(0) < 1:
        raise RuntimeError("indptr must have at least one entry")
    m, nnz = row_ptr.size(0) - 1, col_ind.size(0)
    check_2d(in_feat, m, h, attn_row=attn_row)
    check_2d(in_feat, n_cols, h, attn_col=attn_col)
    if score is not None:
        check_2d(in_feat, h, nnz, score=score)
    return m, n_cols, nnz, h, f


def _edge_mask(in_feat, nnz, h, attn_drop, edge_mask):
    """The dropout randoms [nnz, h]: the caller's, or drawn here -- only when something is dropped."""
    if edge_mask is None and attn_drop > 0.0:
        edge_mask = torch.rand((nnz, h), dtype=torch.float32, device=in_feat.device)
    return edge_mask


def _gat_fwd_edge(what, save_stats, attn_row, attn_col, row_ptr, col_ind, negative_slope, in_feat, score, attn_drop, edge_mask):
    ext = _n.ext()
    if ext is not None and in_feat.dim() == 3 and in_feat.is_cuda and col_ind.dim() == 1:
        attn_drop = float(attn_drop)
        if 0.0 <= attn_drop < 1.0:   # (else: the extension's error, before any randoms are drawn)
            edge_mask = _edge_mask(in_feat, col_ind.size(0), in_feat.size(1), attn_drop, edge_mask)
        return ext.gat_fwd_edge(attn_row, attn_col, row_ptr, col_ind, float(negative_slope), score, in_feat, edge_mask,
                                attn_drop, save_stats) + [edge_mask]
    m, n_cols, nnz, h, f = _check_edge(attn_row, attn_col, row_ptr, col_ind, score, in_feat)
    attn_drop = _drop(attn_drop)
    edge_mask = _edge_mask(in_feat, nnz, h, attn_drop, edge_mask)
    if edge_mask is not None:
        check_2d(in_feat, nnz, h, edge_mask=edge_mask)
    out = _empty(in_feat, m, h, f)
    edge_max, edge_sum = (_empty(in_feat, m, h), _empty(in_feat, m, h)) if save_stats else (None, None)
    call("dfgnn_gat_fwd_edge_rect", what, in_feat.device, m, n_cols, nnz, h, f, row_ptr, col_ind, attn_row, attn_col,
         float(negative_slope), score, in_feat, edge_mask, attn_drop, edge_max, edge_sum, out)
    return ([out, edge_max, edge_sum] if save_stats else [out]) + [edge_mask]


def gat_inference_edge(attn_row, attn_col, row_ptr, col_ind, negative_slope, in_feat, score=None, attn_drop=0.0,
                       edge_mask=None):
    """-> out[m, h, f].  attn_drop > 0 drops edges here too (randoms from torch.rand unless edge_mask is given): the
    training forward's `out`, bit for bit, without saving the statistics."""
    return _gat_fwd_edge("gat_inference_edge", False, attn_row, attn_col, row_ptr, col_ind, negative_slope, in_feat, score,
                         attn_drop, edge_mask)[0]


def gat_forward_edge(attn_row, attn_col, row_ptr, col_ind, negative_slope, in_feat, score=None, attn_drop=0.0, edge_mask=None):
    """-> [out[m, h, f], edge_max[m, h], edge_sum[m, h], edge_mask]: the training forward.  edge_mask holds the uniform
    randoms [nnz, h] of the attention dropout -- the caller's, or drawn with torch.rand when attn_drop > 0 -- and is None
    when there are none: no dropout, nothing of size nnz allocated.  A given edge_mask with attn_drop = 0 keeps every edge."""
    return _gat_fwd_edge("gat_forward_edge", True, attn_row, attn_col, row_ptr, col_ind, negative_slope, in_feat, score,
                         attn_drop, edge_mask)


def gat_backward_edge(negative_slope, attn_drop, row_ptr, col_ind, col_ptr, row_ind, val_idx, attn_row, attn_col, in_feat,
                      edge_max, edge_sum, grad, score=None, edge_mask=None, want_grad_score=True):
    """-> [grad_feat[n_cols, h, f], grad_attn_row[m, h], grad_attn_col[n_cols, h], grad_score[h, nnz]] from the forward's
    row statistics alone (each edge is recomputed; the forward's `out` is not needed); grad_score is None without want_grad_score (then nothing of size
    nnz is allocated or written).  val_idx: the CSR position of each CSC entry, through which the column pass finds an
    entry's score and random."""
    if val_idx is None:
        raise RuntimeError("gat_backward_edge: val_idx is required (the column pass finds an entry's score and random through it)")
    val_idx = as_int32(val_idx)
    want_grad_score = bool(want_grad_score)
    ext = _n.ext()
    if ext is not None and in_feat.dim() == 3 and in_feat.is_cuda:
        res = ext.gat_bwd_edge(float(negative_slope), float(attn_drop), row_ptr, col_ind, col_ptr, row_ind, val_idx, attn_row,
                               attn_col, score, in_feat, edge_mask, edge_max, edge_sum, grad, want_grad_score)
        return res if want_grad_score else res + [None]
    m, n_cols, nnz, h, f = _check_edge(attn_row, attn_col, row_ptr, col_ind, score, in_feat)
    attn_drop = _drop(attn_drop)
    if edge_mask is not None:
        check_2d(in_feat, nnz, h, edge_mask=edge_mask)
    check_csc_rect(in_feat, n_cols, nnz, col_ptr, "X", row_ind=row_ind, val_idx=val_idx)
    check_3d(in_feat, m, h, f, grad=grad)
    check_2d(in_feat, m, h, edge_max=edge_max, edge_sum=edge_sum)
    delta, grad_feat = _empty(in_feat, m, h), torch.empty_like(in_feat)
    grad_attn_row, grad_attn_col = _empty(in_feat, m, h), _empty(in_feat, n_cols, h)
    grad_score = _empty(in_feat, h, nnz) if want_grad_score else None
    call("dfgnn_gat_bwd_edge_rect", "gat_backward_edge", in_feat.device, m, n_cols, nnz, h, f, row_ptr, col_ind, col_ptr,
         row_ind, val_idx, attn_row, attn_col, float(negative_slope), score, in_feat, edge_mask, attn_drop, edge_max, edge_sum,
         grad, delta, grad_feat, grad_attn_row, grad_attn_col, grad_score)
    return [grad_feat, grad_attn_row, grad_attn_col, grad_score]
