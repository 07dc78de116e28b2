"""`fused_gtconv` -- drop-in for the reference's extension module of the same name
(PYBIND11_MODULE(fused_gtconv), DFGNN/src/fused_gtconv/fused_gtconv.cpp:577-602), bound to the
MI355X HIP library through its C ABI (include/dfgnn.h).

Same function names, positional signatures, return conventions (list vs bare tensor) and error
type (RuntimeError) as the reference.  Differences, all deliberate:
  * kernels launch on torch's *current* stream of the tensors' device (reference: legacy default
    stream, no device guard);
  * dtype / shape checks are real (reference: asserts compiled out);
  * `smem_consume` is accepted and ignored: LDS sizing is decided per workgroup inside the
    kernels, with an online-softmax fallback instead of the reference's silent overflow.
"""
import torch

import dfgnn_native as _n
import os

from _binding_util import (as_int32, call, check_2d, check_3d, check_cols, check_csc, check_csc_rect, check_csr, check_edges,
                           check_family, check_feats, get_plan_obj, plan_dense_weights, plan_ptrs, val_ptr)

# Set to False to force the general (plan-less) kernels; results are identical either way.
USE_BLOCK_PLAN = True

# Every operator below: the block plan / val_ptr look-ups (shared by both transports), the torch C++ binding when there is
# one (csrc/torch_ext.cpp: same checks, same C ABI call), else the ctypes transport: checks by family, allocations, call().


def _checks(indptr, indices, Q, K, V, rows=None, val=None, **like_Q):
    """What every GT operator checks: Q / K / V (and `like_Q`: grad, out) fp32 [nodes, heads, feat] of one shape, the CSR
    arrays of those nodes, and -- where the operator takes them -- the COO rows and the edge values -> (m, nnz, h, f)."""
    m, h, f = check_feats(Q=Q, K=K, V=V, **like_Q)
    nnz = check_csr(Q, m, indptr, indices)
    if rows is not None:
        check_edges(Q, nnz, torch.int32, rows=rows)
    if val is not None:
        check_edges(Q, nnz, torch.float32, val=val)
    return m, nnz, h, f


def _checks_rect(indptr, indices, Q, K, V, val=None, **like_Q):
    """_checks of the pairs that take an m x n_cols graph (rowstats, bias, edge): Q (and `like_Q`: grad, out) fp32
    [m, heads, feat]; K and V agree with each other and with Q in [heads, feat], their rows are the graph's columns
    -> (m, n_cols, nnz, h, f)."""
    m, h, f = check_feats(Q=Q, **like_Q)
    n_cols = check_cols("Q", Q, K=K, V=V)
    nnz = check_csr(Q, m, indptr, indices)
    if val is not None:
        check_edges(Q, nnz, torch.float32, val=val)
    return m, n_cols, nnz, h, f


def _empty(like, *shape):
    return torch.empty(shape, dtype=torch.float32, device=like.device)


def gt_hyper_inference(indptr, indices, rows, val, smem_consume, Q, K, V):
    """fused_gtconv.cpp:278-314 -> [out]"""
    if val_ptr(val) is not None and Q.dim() == 3 and Q.is_cuda:
        # edge values: the matrix-core forward reads them in the plan's dense form (csrc/gt_dense_stats_w.hip) when
        # every range of the batch is dense; anything else takes the edge-walking kernels below
        plan = gt_stats_pair_applies(indptr, indices, val, Q)
        if plan is not None:
            return gt_hyper_forward_stats(indptr, indices, Q, K, V, plan=plan, val=val, save_stats=False)
    plan = get_plan_obj(indptr, indices, Q, USE_BLOCK_PLAN)
    ext = _n.ext()
    if ext is not None:
        return ext.gt_hyper_fwd(indptr, indices, rows, val, Q, K, V, False, val_ptr(val) is None, *plan_ptrs(plan))
    m, nnz, h, f = _checks(indptr, indices, Q, K, V, rows, val)
    out = torch.empty_like(Q)
    ws = _empty(Q, h, nnz) if plan is not None else None   # scratch for per-edge values (the plan's edge-global ranges)
    call("dfgnn_gt_hyper_fwd", "gt_hyper_inference", Q.device, m, nnz, h, f, indptr, indices, rows, val_ptr(val), Q, K, V,
         None, ws, out, *plan_ptrs(plan))
    return [out]


def gt_hyper_inference_ablation(indptr, indices, rows, val, smem_consume, Q, K, V):
    """fused_gtconv.cpp:538-575.  The reference's de-optimised ablation kernels are a paper study
    (out of scope); the entry point is kept and runs the production kernel."""
    return gt_hyper_inference(indptr, indices, rows, val, smem_consume, Q, K, V)


def gt_hyper_forward(row_ptr, col_ind, rows, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V):
    """fused_gtconv.cpp:79-116 -> [out, attn_edge[h, nnz]] (training forward)."""
    pp, mp = plan_ptrs(get_plan_obj(row_ptr, col_ind, Q, USE_BLOCK_PLAN))
    ext = _n.ext()
    if ext is not None:
        return ext.gt_hyper_fwd(row_ptr, col_ind, rows, val, Q, K, V, True, val_ptr(val) is None, pp, mp)
    m, nnz, h, f = _checks(row_ptr, col_ind, Q, K, V, rows, val)
    out, attn_edge = torch.empty_like(Q), _empty(Q, h, nnz)
    call("dfgnn_gt_hyper_fwd", "gt_hyper_forward", Q.device, m, nnz, h, f, row_ptr, col_ind, rows, val_ptr(val), Q, K, V,
         attn_edge, None, out, pp, mp)
    return [out, attn_edge]


def gt_backward(row_ptr, col_ind, rows, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V, attn_edge,
                grad):
    """fused_gtconv.cpp:125-172 -> [dQ, dK, dV]."""
    val_idx = as_int32(val_idx)
    pp, mp = plan_ptrs(get_plan_obj(row_ptr, col_ind, Q, USE_BLOCK_PLAN))
    ext = _n.ext()
    if ext is not None:
        return ext.gt_bwd(row_ptr, col_ind, rows, val, col_ptr, row_ind, val_idx, Q, K, V, attn_edge, grad,
                          val_ptr(val) is None, pp, mp)
    m, nnz, h, f = _checks(row_ptr, col_ind, Q, K, V, rows, val, grad=grad)
    check_csc(Q, m, nnz, col_ptr, row_ind=row_ind, val_idx=val_idx)
    check_family(Q, torch.float32, attn_edge=attn_edge)
    if attn_edge.numel() != h * nnz:
        raise RuntimeError(f"attn_edge must have {h}*{nnz} elements, got {attn_edge.numel()}")
    grad_edge = _empty(Q, h, nnz)
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    call("dfgnn_gt_bwd", "gt_backward", Q.device, m, nnz, h, f, row_ptr, col_ind, rows, val_ptr(val), col_ptr, row_ind,
         val_idx, Q, K, V, attn_edge, grad, grad_edge, dQ, dK, dV, pp, mp)
    return [dQ, dK, dV]


# ---- the statistics-saving training pair (include/dfgnn.h: dfgnn_gt_hyper_fwd_stats / dfgnn_gt_bwd_stats) ------------
# Not part of the reference's module: FusedGTFunction_hyper (DFGNN/operators/fused_gtconv.py) takes this pair instead of
# gt_hyper_forward / gt_backward when the whole batch runs on the matrix-core kernels -- same results, no attn_edge.
# Which pair the autograd Function takes is a measured choice: the statistics pair saves the attn_edge
# round trip (8 h nnz bytes) and pays one more K image pass in the backward -- from two heads on it is the faster one
# (8 x 16 heads: 0.58 against 0.65 ms per step), at one head the attn_edge pair is (0.263 against 0.267 ms).
# DFGNN_STATS in the environment: 0 = the attn_edge pair everywhere, 1 = the statistics pair wherever it applies (A/B runs).
_STATS_ENV = os.environ.get("DFGNN_STATS", "auto")
USE_STATS_PAIR = _STATS_ENV != "0"
STATS_PAIR_MIN_HEADS = 1 if _STATS_ENV == "1" else 2
# the attn_edge pair in rank order (further down): DFGNN_RANKED=0 switches it off, DFGNN_RANKED_HEADS lists the head counts
# it is taken at (default: one head)
USE_RANKED_PAIR = os.environ.get("DFGNN_RANKED", "1") != "0"
RANKED_HEADS = tuple(int(x) for x in os.environ.get("DFGNN_RANKED_HEADS", "1").split(",") if x)



def gt_stats_pair_applies(row_ptr, col_ind, val, Q):
    """The block plan (a true value) when gt_hyper_forward_stats / gt_backward_stats can serve this call -- a plan whose
    ranges are all dense (dfgnn_gt_stats_applies) -- else None.  The plan may be handed to the two calls (`plan=`), which
    then skip their own look-up; edge values other than ones go along as `val=` (the calls turn them into the plan's
    dense weights, _binding_util.plan_dense_weights)."""
    if not (USE_STATS_PAIR and USE_BLOCK_PLAN) or Q.dim() != 3 or not Q.is_cuda:
        return None
    plan = get_plan_obj(row_ptr, col_ind, Q)
    if plan is not None and plan.stats_applies(Q.size(1)):
        return plan
    return None


def gt_stats_pair_chosen(row_ptr, col_ind, val, Q):
    """gt_stats_pair_applies under the policy above: the plan when the autograd Function should take the statistics pair
    for this call, else None.  With edge values it is always the pair to take where it applies: the attn_edge pair has
    no matrix-core form for them."""
    if Q.dim() != 3 or (Q.size(1) < STATS_PAIR_MIN_HEADS and val_ptr(val) is None):
        return None
    if _STATS_ENV != "1" and Q.size(1) in RANKED_HEADS and gt_ranked_pair_chosen(row_ptr, col_ind, val, Q) is not None:
        return None     # (a head count handed to the rank-ordered attn_edge pair: DFGNN_RANKED_HEADS)
    return gt_stats_pair_applies(row_ptr, col_ind, val, Q)


def _stats_weights(plan, row_ptr, val):
    """None without a plan and for unit edge values (or no `val`), else the plan's dense weights of `val`."""
    if plan is None or val is None or val_ptr(val) is None:
        return None
    return plan_dense_weights(plan, row_ptr, val)


# ---- the attn_edge pair in rank order (include/dfgnn.h: dfgnn_gt_hyper_fwd_ranked / dfgnn_gt_bwd_ranked) --------------
# What FusedGTFunction_hyper takes at ONE head on an all-dense batch with unit edge values: the attention values travel from
# forward to backward like in the reference, but ordered by column within a row, which lets the forward find an edge's slot
# from the plan's bitmap instead of the edge list (csrc/gt_dense_stats_w.hip: gt_dense_fwd_ranked_kernel).


def gt_ranked_pair_applies(row_ptr, col_ind, val, Q):
    """The block plan when gt_hyper_forward_ranked / gt_backward_ranked can serve this call, else None."""
    if not (USE_RANKED_PAIR and USE_BLOCK_PLAN) or Q.dim() != 3 or not Q.is_cuda or val_ptr(val) is not None:
        return None
    plan = get_plan_obj(row_ptr, col_ind, Q)
    if plan is not None and plan.stats_applies(Q.size(1)):
        return plan
    return None


def gt_ranked_pair_chosen(row_ptr, col_ind, val, Q):
    """gt_ranked_pair_applies under the measured policy: at one head (C3: forward 95 -> 85 us; batches without a range of
    more than 128 nodes take the 256-thread form of the same forward, two workgroups per CU).  With several heads the
    rank-ordered forward times like the CSR-ordered one and the statistics pair is the faster choice; RANKED_HEADS widens
    the head counts for A/B runs (DFGNN_RANKED_HEADS=1,2,4)."""
    if Q.dim() != 3 or Q.size(1) not in RANKED_HEADS:
        return None
    return gt_ranked_pair_applies(row_ptr, col_ind, val, Q)


def gt_training_pair(row_ptr, col_ind, val, Q):
    """Which training pair FusedGTFunction_hyper takes for this call -> (pair, plan): ("stats", plan) where the policy
    chooses the statistics pair, else ("ranked", plan) where it chooses the rank-ordered attn_edge pair, else
    ("attn_edge", None): the reference's form, gt_hyper_forward / gt_backward."""
    plan = gt_stats_pair_chosen(row_ptr, col_ind, val, Q)
    if plan is not None:
        return "stats", plan
    plan = gt_ranked_pair_chosen(row_ptr, col_ind, val, Q)
    return ("ranked", plan) if plan is not None else ("attn_edge", None)


def gt_hyper_forward_ranked(row_ptr, col_ind, Q, K, V, plan=None):
    """-> [out, attn_ranked[1, nnz]] (row i's k-th edge by increasing column at row_ptr[i] + k)."""
    if plan is None:
        plan = get_plan_obj(row_ptr, col_ind, Q, USE_BLOCK_PLAN)
    pp, mp = plan_ptrs(plan)
    ext = _n.ext()
    if ext is not None:
        return ext.gt_hyper_fwd_ranked(row_ptr, col_ind, Q, K, V, pp, mp)
    m, nnz, h, f = _checks(row_ptr, col_ind, Q, K, V)
    out, attn = torch.empty_like(Q), _empty(Q, h, nnz)
    call("dfgnn_gt_hyper_fwd_ranked", "gt_hyper_forward_ranked", Q.device, m, nnz, h, f, row_ptr, col_ind, Q, K, V, attn,
         out, pp, mp)
    return [out, attn]


def gt_backward_ranked(row_ptr, col_ind, Q, K, V, attn_ranked, grad, plan=None):
    """-> [dQ, dK, dV] from the rank-ordered attention values of gt_hyper_forward_ranked."""
    if plan is None:
        plan = get_plan_obj(row_ptr, col_ind, Q, USE_BLOCK_PLAN)
    pp, mp = plan_ptrs(plan)
    ext = _n.ext()
    if ext is not None:
        return ext.gt_bwd_ranked(row_ptr, col_ind, Q, K, V, attn_ranked, grad, pp, mp)
    m, nnz, h, f = _checks(row_ptr, col_ind, Q, K, V, grad=grad)
    check_family(Q, torch.float32, attn_ranked=attn_ranked)
    if attn_ranked.numel() != h * nnz:
        raise RuntimeError(f"attn_ranked must have {h}*{nnz} elements, got {attn_ranked.numel()}")
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    call("dfgnn_gt_bwd_ranked", "gt_backward_ranked", Q.device, m, nnz, h, f, row_ptr, col_ind, Q, K, V, attn_ranked, grad,
         dQ, dK, dV, pp, mp)
    return [dQ, dK, dV]


def gt_hyper_step_raw(row_ptr, col_ind, rows, val, col_ptr, row_ind, val_idx, smem, Q, K, V, grad):
    """-> [out, dQ, dK, dV]: the launches of one FusedGTFunction_hyper forward + backward as explicit operator calls (no
    autograd graph), choosing the pair the way the autograd function does -- what the HIP-graph replays capture."""
    pair, plan = gt_training_pair(row_ptr, col_ind, val, Q)
    if pair == "stats":
        out, rmax, rsum = gt_hyper_forward_stats(row_ptr, col_ind, Q, K, V, plan=plan, val=val)
        return [out] + list(gt_backward_stats(row_ptr, col_ind, Q, K, V, rmax, rsum, grad, plan=plan, val=val))
    if pair == "ranked":
        out, attn = gt_hyper_forward_ranked(row_ptr, col_ind, Q, K, V, plan=plan)
        return [out] + list(gt_backward_ranked(row_ptr, col_ind, Q, K, V, attn, grad, plan=plan))
    out, attn = gt_hyper_forward(row_ptr, col_ind, rows, val, col_ptr, row_ind, val_idx, smem, Q, K, V)
    return [out] + list(gt_backward(row_ptr, col_ind, rows, val, col_ptr, row_ind, val_idx, smem, Q, K, V, attn, grad))


def gt_hyper_forward_stats(row_ptr, col_ind, Q, K, V, plan=None, val=None, save_stats=True):
    """-> [out, row_max[m, h], row_sum[m, h]]: the training forward without attn_edge (call gt_stats_pair_applies first).
    val: edge values (None or all ones: unit values).  save_stats=False -> [out] (inference)."""
    if plan is None:
        plan = get_plan_obj(row_ptr, col_ind, Q, USE_BLOCK_PLAN)
    weights = _stats_weights(plan, row_ptr, val)
    pp, mp = plan_ptrs(plan)
    ext = _n.ext()
    if ext is not None:
        return ext.gt_hyper_fwd_stats(row_ptr, col_ind, Q, K, V, pp, mp, weights, save_stats)
    m, nnz, h, f = _checks(row_ptr, col_ind, Q, K, V)
    out = torch.empty_like(Q)
    row_max, row_sum = (_empty(Q, m, h), _empty(Q, m, h)) if save_stats else (None, None)
    call("dfgnn_gt_hyper_fwd_stats", "gt_hyper_forward_stats", Q.device, m, nnz, h, f, row_ptr, col_ind, weights, Q, K, V,
         row_max, row_sum, out, pp, mp)
    return [out, row_max, row_sum] if save_stats else [out]


def gt_backward_stats(row_ptr, col_ind, Q, K, V, row_max, row_sum, grad, plan=None, val=None):
    """-> [dQ, dK, dV] from the row statistics of gt_hyper_forward_stats (P is recomputed on the matrix cores)."""
    if plan is None:
        plan = get_plan_obj(row_ptr, col_ind, Q, USE_BLOCK_PLAN)
    weights = _stats_weights(plan, row_ptr, val)
    pp, mp = plan_ptrs(plan)
    ext = _n.ext()
    if ext is not None:
        return ext.gt_bwd_stats(row_ptr, col_ind, Q, K, V, row_max, row_sum, grad, pp, mp, weights)
    m, nnz, h, f = _checks(row_ptr, col_ind, Q, K, V, grad=grad)
    check_2d(Q, m, h, row_max=row_max, row_sum=row_sum)
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    call("dfgnn_gt_bwd_stats", "gt_backward_stats", Q.device, m, nnz, h, f, row_ptr, col_ind, weights, Q, K, V, row_max,
         row_sum, grad, dQ, dK, dV, pp, mp)
    return [dQ, dK, dV]


# ---- the general statistics pair (include/dfgnn.h: dfgnn_gt_fwd_rowstats / dfgnn_gt_bwd_rowstats) --------------------
# Not part of the reference's module.  The same saved state as the pair above -- two floats per (row, head) -- but for
# ANY graph: no plan, no degree limit, any f (csrc/gt_train.hip).  Opt-in: DFGNN.operators.fused_gtconv.GTConvFuse_rowstats
# takes it; FusedGTFunction_hyper does not.
# This pair and its two variants below also take a RECTANGULAR graph (a neighbour-sampled block, cross-attention): Q [m, h, f]
# with row_ptr (m + 1,), K / V [n_cols, h, f] with col_ptr (n_cols + 1,), col_ind < n_cols; out, dQ and the statistics have
# m rows, dK / dV n_cols.  Every other GT operator of this module is square-only and rejects Q / K / V of different shapes.


def gt_forward_rowstats(row_ptr, col_ind, val, Q, K, V):
    """-> [out, row_max[m, h], row_sum[m, h]]: the training forward of any graph without attn_edge.
    val: edge values fp32[nnz] in CSR order; None or all ones: unit values."""
    ext = _n.ext()
    if ext is not None:
        return ext.gt_fwd_rowstats(row_ptr, col_ind, val, Q, K, V, val_ptr(val) is None)
    m, n_cols, nnz, h, f = _checks_rect(row_ptr, col_ind, Q, K, V, val=val)
    out, row_max, row_sum = torch.empty_like(Q), _empty(Q, m, h), _empty(Q, m, h)
    call("dfgnn_gt_fwd_rowstats_rect", "gt_forward_rowstats", Q.device, m, n_cols, nnz, h, f, row_ptr, col_ind, val_ptr(val), Q, K, V,
         row_max, row_sum, out)
    return [out, row_max, row_sum]


def gt_backward_rowstats(row_ptr, col_ind, val, col_ptr, row_ind, val_idx, Q, K, V, out, row_max, row_sum, grad):
    """-> [dQ, dK, dV] from the forward's output and row statistics (the attention is recomputed edge by edge).
    val as in gt_forward_rowstats."""
    val_idx = as_int32(val_idx)
    ext = _n.ext()
    if ext is not None:
        return ext.gt_bwd_rowstats(row_ptr, col_ind, val, col_ptr, row_ind, val_idx, Q, K, V, out, row_max, row_sum, grad,
                                   val_ptr(val) is None)
    m, n_cols, nnz, h, f = _checks_rect(row_ptr, col_ind, Q, K, V, val=val, out=out, grad=grad)
    check_csc_rect(Q, n_cols, nnz, col_ptr, "K / V", row_ind=row_ind, val_idx=val_idx)
    check_2d(Q, m, h, row_max=row_max, row_sum=row_sum)
    delta = _empty(Q, m, h)
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    call("dfgnn_gt_bwd_rowstats_rect", "gt_backward_rowstats", Q.device, m, n_cols, nnz, h, f, row_ptr, col_ind, val_ptr(val), col_ptr,
         row_ind, val_idx, Q, K, V, out, row_max, row_sum, grad, delta, dQ, dK, dV)
    return [dQ, dK, dV]


# ---- the general pair with a per-edge additive attention bias (include/dfgnn.h: dfgnn_gt_fwd_bias / dfgnn_gt_bwd_bias) ---
# Not part of the reference's module.  The pair above with s_e = val_e <Q_i, K_j> + bias[h, e] (csrc/gt_bias_train.hip):
# bias is fp32[h, nnz] in CSR edge order, -inf masks an edge.  DFGNN.operators.fused_gtconv.GTConvFuse_bias takes it.


def _check_bias(Q, h, nnz, bias):
    check_2d(Q, h, nnz, bias=bias)


def _forward_bias(what, save_stats, row_ptr, col_ind, val, bias, Q, K, V):
    ext = _n.ext()
    if ext is not None:
        return ext.gt_fwd_bias(row_ptr, col_ind, val, bias, Q, K, V, val_ptr(val) is None, save_stats)
    m, n_cols, nnz, h, f = _checks_rect(row_ptr, col_ind, Q, K, V, val=val)
    _check_bias(Q, h, nnz, bias)
    out = torch.empty_like(Q)
    row_max, row_sum = (_empty(Q, m, h), _empty(Q, m, h)) if save_stats else (None, None)
    call("dfgnn_gt_fwd_bias_rect", what, Q.device, m, n_cols, nnz, h, f, row_ptr, col_ind, val_ptr(val), bias, Q, K, V, row_max, row_sum,
         out)
    return [out, row_max, row_sum] if save_stats else [out]


def gt_inference_bias(row_ptr, col_ind, val, bias, Q, K, V):
    """-> out: inference of any graph with the additive bias fp32[h, nnz] (CSR order; -inf masks an edge).
    val: edge values fp32[nnz] in CSR order; None or all ones: unit values."""
    return _forward_bias("gt_inference_bias", False, row_ptr, col_ind, val, bias, Q, K, V)[0]


def gt_forward_bias(row_ptr, col_ind, val, bias, Q, K, V):
    """-> [out, row_max[m, h], row_sum[m, h]]: the training forward; a (row, head) without an unmasked edge has out = 0,
    row_max = -1e38, row_sum = 0."""
    return _forward_bias("gt_forward_bias", True, row_ptr, col_ind, val, bias, Q, K, V)


def gt_backward_bias(row_ptr, col_ind, val, bias, col_ptr, row_ind, val_idx, Q, K, V, out, row_max, row_sum, grad,
                     need_dbias=True):
    """-> [dQ, dK, dV, dbias[h, nnz]] from the forward's output and row statistics; dbias is None without need_dbias (then
    nothing of size h nnz is allocated or written)."""
    val_idx = as_int32(val_idx)
    ext = _n.ext()
    if ext is not None:
        res = ext.gt_bwd_bias(row_ptr, col_ind, val, bias, col_ptr, row_ind, val_idx, Q, K, V, out, row_max, row_sum, grad,
                              val_ptr(val) is None, need_dbias)
        return res if need_dbias else res + [None]
    m, n_cols, nnz, h, f = _checks_rect(row_ptr, col_ind, Q, K, V, val=val, out=out, grad=grad)
    _check_bias(Q, h, nnz, bias)
    check_csc_rect(Q, n_cols, nnz, col_ptr, "K / V", row_ind=row_ind, val_idx=val_idx)
    check_2d(Q, m, h, row_max=row_max, row_sum=row_sum)
    delta = _empty(Q, m, h)
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    dbias = _empty(Q, h, nnz) if need_dbias else None
    call("dfgnn_gt_bwd_bias_rect", "gt_backward_bias", Q.device, m, n_cols, nnz, h, f, row_ptr, col_ind, val_ptr(val), bias, col_ptr,
         row_ind, val_idx, Q, K, V, out, row_max, row_sum, grad, delta, dQ, dK, dV, dbias)
    return [dQ, dK, dV, dbias]


# ---- the general pair with a per-edge feature vector in keys and values (include/dfgnn.h: dfgnn_gt_fwd_edge / _bwd_edge) ---
# Not part of the reference's module.  The row-statistics pair with k~_e = K_j + E_e, v~_e = V_j + E_e (csrc/gt_edge_train.hip):
# E is fp32[nnz, h, f] in CSR edge order.  DFGNN.operators.fused_gtconv.GTConvFuse_edge takes it.


def _check_edge_feat(Q, nnz, h, f, E):
    check_3d(Q, nnz, h, f, E=E)


def _forward_edge(what, save_stats, row_ptr, col_ind, val, E, Q, K, V):
    ext = _n.ext()
    if ext is not None:
        return ext.gt_fwd_edge(row_ptr, col_ind, val, E, Q, K, V, val_ptr(val) is None, save_stats)
    m, n_cols, nnz, h, f = _checks_rect(row_ptr, col_ind, Q, K, V, val=val)
    _check_edge_feat(Q, nnz, h, f, E)
    out = torch.empty_like(Q)
    row_max, row_sum = (_empty(Q, m, h), _empty(Q, m, h)) if save_stats else (None, None)
    call("dfgnn_gt_fwd_edge_rect", what, Q.device, m, n_cols, nnz, h, f, row_ptr, col_ind, val_ptr(val), E, Q, K, V, row_max, row_sum, out)
    return [out, row_max, row_sum] if save_stats else [out]


def gt_inference_edge(row_ptr, col_ind, val, E, Q, K, V):
    """-> out: inference of any graph with the edge features fp32[nnz, h, f] (CSR order) added to keys and values.
    val: edge values fp32[nnz] in CSR order; None or all ones: unit values."""
    return _forward_edge("gt_inference_edge", False, row_ptr, col_ind, val, E, Q, K, V)[0]


def gt_forward_edge(row_ptr, col_ind, val, E, Q, K, V):
    """-> [out, row_max[m, h], row_sum[m, h]]: the training forward; an empty row has out = 0, row_max = -1e38,
    row_sum = 0."""
    return _forward_edge("gt_forward_edge", True, row_ptr, col_ind, val, E, Q, K, V)


def gt_backward_edge(row_ptr, col_ind, val, E, col_ptr, row_ind, val_idx, Q, K, V, out, row_max, row_sum, grad,
                     need_dE=True):
    """-> [dQ, dK, dV, dE[nnz, h, f]] from the forward's output and row statistics; dE is None without need_dE (then
    nothing of size nnz h f is allocated or written)."""
    val_idx = as_int32(val_idx)
    ext = _n.ext()
    if ext is not None:
        res = ext.gt_bwd_edge(row_ptr, col_ind, val, E, col_ptr, row_ind, val_idx, Q, K, V, out, row_max, row_sum, grad,
                              val_ptr(val) is None, need_dE)
        return res if need_dE else res + [None]
    m, n_cols, nnz, h, f = _checks_rect(row_ptr, col_ind, Q, K, V, val=val, out=out, grad=grad)
    _check_edge_feat(Q, nnz, h, f, E)
    check_csc_rect(Q, n_cols, nnz, col_ptr, "K / V", row_ind=row_ind, val_idx=val_idx)
    check_2d(Q, m, h, row_max=row_max, row_sum=row_sum)
    delta = _empty(Q, m, h)
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    dE = torch.empty_like(E) if need_dE else None
    call("dfgnn_gt_bwd_edge_rect", "gt_backward_edge", Q.device, m, n_cols, nnz, h, f, row_ptr, col_ind, val_ptr(val), E, col_ptr,
         row_ind, val_idx, Q, K, V, out, row_max, row_sum, grad, delta, dQ, dK, dV, dE)
    return [dQ, dK, dV, dE]


# ---- the general pair with a per-edge multiplicative gate and an edge output (include/dfgnn.h: dfgnn_gt_fwd_gate / _bwd_gate)
# Not part of the reference's module.  The row-statistics pair with ke_e = K_j (.) E_e, s_e = val_e <Q_i, ke_e> and the
# edge output W_e = val_e Q_i (.) ke_e (csrc/gt_gate_train.hip): E, W, the gradient G of W and dE are fp32[nnz, h, f] in CSR
# edge order.  No clamp on the logit.  DFGNN.operators.fused_gtconv.GTConvFuse_gate takes it.


def _forward_gate(what, save_stats, need_W, row_ptr, col_ind, val, E, Q, K, V):
    ext = _n.ext()
    if ext is not None:
        return ext.gt_fwd_gate(row_ptr, col_ind, val, E, Q, K, V, val_ptr(val) is None, save_stats, need_W)
    m, n_cols, nnz, h, f = _checks_rect(row_ptr, col_ind, Q, K, V, val=val)
    _check_edge_feat(Q, nnz, h, f, E)
    out = torch.empty_like(Q)
    row_max, row_sum = (_empty(Q, m, h), _empty(Q, m, h)) if save_stats else (None, None)
    W = torch.empty_like(E) if need_W else None
    call("dfgnn_gt_fwd_gate_rect", what, Q.device, m, n_cols, nnz, h, f, row_ptr, col_ind, val_ptr(val), E, Q, K, V, row_max, row_sum,
         out, W)
    return [out] + ([row_max, row_sum] if save_stats else []) + ([W] if need_W else [])


def gt_inference_gate(row_ptr, col_ind, val, E, Q, K, V, need_W=False):
    """-> out, or (out, W) with need_W: inference of any graph with the keys gated by the edge features fp32[nnz, h, f]
    (CSR order).  val: edge values fp32[nnz] in CSR order; None or all ones: unit values."""
    res = _forward_gate("gt_inference_gate", False, need_W, row_ptr, col_ind, val, E, Q, K, V)
    return tuple(res) if need_W else res[0]


def gt_forward_gate(row_ptr, col_ind, val, E, Q, K, V, need_W=True):
    """-> [out, row_max[m, h], row_sum[m, h], W[nnz, h, f]]: the training forward; W is None without need_W (then nothing
    of size nnz h f is allocated or written).  An empty row has out = 0, row_max = -1e38, row_sum = 0."""
    res = _forward_gate("gt_forward_gate", True, need_W, row_ptr, col_ind, val, E, Q, K, V)
    return res if need_W else res + [None]


def gt_backward_gate(row_ptr, col_ind, val, E, col_ptr, row_ind, val_idx, Q, K, V, out, row_max, row_sum, grad, G=None,
                     need_dE=True):
    """-> [dQ, dK, dV, dE[nnz, h, f]] from the forward's output and row statistics, the gradient `grad` of out and the
    gradient G[nnz, h, f] of W (None: zero, nothing of it is read); dE is None without need_dE (then nothing of size
    nnz h f is allocated or written)."""
    val_idx = as_int32(val_idx)
    ext = _n.ext()
    if ext is not None:
        res = ext.gt_bwd_gate(row_ptr, col_ind, val, E, col_ptr, row_ind, val_idx, Q, K, V, out, row_max, row_sum, grad, G,
                              val_ptr(val) is None, need_dE)
        return res if need_dE else res + [None]
    m, n_cols, nnz, h, f = _checks_rect(row_ptr, col_ind, Q, K, V, val=val, out=out, grad=grad)
    _check_edge_feat(Q, nnz, h, f, E)
    if G is not None:
        check_3d(Q, nnz, h, f, G=G)
    check_csc_rect(Q, n_cols, nnz, col_ptr, "K / V", row_ind=row_ind, val_idx=val_idx)
    check_2d(Q, m, h, row_max=row_max, row_sum=row_sum)
    delta = _empty(Q, m, h)
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    dE = torch.empty_like(E) if need_dE else None
    call("dfgnn_gt_bwd_gate_rect", "gt_backward_gate", Q.device, m, n_cols, nnz, h, f, row_ptr, col_ind, val_ptr(val), E, col_ptr,
         row_ind, val_idx, Q, K, V, out, row_max, row_sum, grad, G, delta, dQ, dK, dV, dE)
    return [dQ, dK, dV, dE]


# ---- the general pair with typed edges (include/dfgnn.h: dfgnn_gt_fwd_typed / dfgnn_gt_bwd_typed) ------------------------
# Not part of the reference's module.  The edge pair with E_e = R[etype[e]] (csrc/gt_typed_train.hip): R is fp32[T, h, f],
# etype int32[nnz] in CSR edge order, etype_csc the same types in CSC entry order (etype[val_idx];
# DFGNN.layers.preprocess_types makes both).  Nothing of size nnz h f exists; dR comes from per-workgroup partial sums and a
# fixed-order reduction.  DFGNN.operators.fused_gtconv.GTConvFuse_typed takes it.


def _check_typed(Q, nnz, h, f, R, **types):
    """The table fp32[T >= 1, h, f] and the per-edge type arrays int32[nnz] -> T."""
    check_edges(Q, nnz, torch.int32, **types)
    check_family(Q, torch.float32, R=R)
    if R.dim() != 3 or R.shape[0] < 1 or tuple(R.shape[1:]) != (h, f):
        raise RuntimeError(f"R must have shape (T >= 1, {h}, {f}), got {tuple(R.shape)}")
    return R.shape[0]


def gt_typed_dR_supported(T, h, f):
    """Whether gt_backward_typed computes dR for a table of T types at h heads of f features (include/dfgnn.h:
    dfgnn_gt_typed_bwd_ws_floats; the limit is T f <= 8192).  The forward and the backward without dR take any T."""
    return int(_n.lib().dfgnn_gt_typed_bwd_ws_floats(int(T), int(h), int(f))) > 0


def _forward_typed(what, save_stats, row_ptr, col_ind, val, etype, R, Q, K, V):
    ext = _n.ext()
    if ext is not None:
        return ext.gt_fwd_typed(row_ptr, col_ind, val, etype, R, Q, K, V, val_ptr(val) is None, save_stats)
    m, n_cols, nnz, h, f = _checks_rect(row_ptr, col_ind, Q, K, V, val=val)
    T = _check_typed(Q, nnz, h, f, R, etype=etype)
    out = torch.empty_like(Q)
    row_max, row_sum = (_empty(Q, m, h), _empty(Q, m, h)) if save_stats else (None, None)
    call("dfgnn_gt_fwd_typed_rect", what, Q.device, m, n_cols, nnz, h, f, T, row_ptr, col_ind, val_ptr(val), etype, R, Q, K, V,
         row_max, row_sum, out)
    return [out, row_max, row_sum] if save_stats else [out]


def gt_inference_typed(row_ptr, col_ind, val, etype, R, Q, K, V):
    """-> out: inference of any graph with R[etype[e]] (R fp32[T, h, f], etype int32[nnz] in CSR order, 0 <= etype < T:
    not checked here) added to keys and values.  val: edge values fp32[nnz] in CSR order; None or all ones: unit values."""
    return _forward_typed("gt_inference_typed", False, row_ptr, col_ind, val, etype, R, Q, K, V)[0]


def gt_forward_typed(row_ptr, col_ind, val, etype, R, Q, K, V):
    """-> [out, row_max[m, h], row_sum[m, h]]: the training forward; an empty row has out = 0, row_max = -1e38,
    row_sum = 0."""
    return _forward_typed("gt_forward_typed", True, row_ptr, col_ind, val, etype, R, Q, K, V)


def gt_backward_typed(row_ptr, col_ind, val, etype, col_ptr, row_ind, val_idx, etype_csc, R, Q, K, V, out, row_max, row_sum,
                      grad, need_dR=True):
    """-> [dQ, dK, dV, dR[T, h, f]] from the forward's output and row statistics; etype_csc = etype[val_idx].  dR is None
    without need_dR (a frozen table: any T).  With need_dR the table must satisfy gt_typed_dR_supported, else the call
    raises the library's "unsupported" RuntimeError before anything is launched."""
    val_idx = as_int32(val_idx)
    ext = _n.ext()
    if ext is not None:
        res = ext.gt_bwd_typed(row_ptr, col_ind, val, etype, col_ptr, row_ind, val_idx, etype_csc, R, Q, K, V, out, row_max,
                               row_sum, grad, val_ptr(val) is None, need_dR)
        return res if need_dR else res + [None]
    m, n_cols, nnz, h, f = _checks_rect(row_ptr, col_ind, Q, K, V, val=val, out=out, grad=grad)
    T = _check_typed(Q, nnz, h, f, R, etype=etype, etype_csc=etype_csc)
    check_csc_rect(Q, n_cols, nnz, col_ptr, "K / V", row_ind=row_ind, val_idx=val_idx)
    check_2d(Q, m, h, row_max=row_max, row_sum=row_sum)
    ws = dR = None
    if need_dR:
        ws_floats = int(_n.lib().dfgnn_gt_typed_bwd_ws_floats(T, h, f))
        if ws_floats < 0:
            _n.check(ws_floats, "gt_backward_typed")
        ws, dR = _empty(Q, ws_floats), torch.empty_like(R)
    delta = _empty(Q, m, h)
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    call("dfgnn_gt_bwd_typed_rect", "gt_backward_typed", Q.device, m, n_cols, nnz, h, f, T, row_ptr, col_ind, val_ptr(val), etype,
         col_ptr, row_ind, val_idx, etype_csc, R, Q, K, V, out, row_max, row_sum, grad, delta, ws, dQ, dK, dV, dR)
    return [dQ, dK, dV, dR]


# ---- the general pair with a typed attention bias (include/dfgnn.h: dfgnn_gt_fwd_tbias / dfgnn_gt_bwd_tbias) --------------
# Not part of the reference's module.  The bias pair with bias[hd, e] = B[etype[e], hd] (csrc/gt_tbias_train.hip): B is
# fp32[T, h] (an embedding weight's layout), etype int32[nnz] in CSR edge order, etype_csc the same types in CSC entry order
# (etype[val_idx]; DFGNN.layers.preprocess_types makes both).  Nothing of size h nnz exists; dB comes from per-workgroup
# partial sums and a fixed-order reduction.  DFGNN.operators.fused_gtconv.GTConvFuse_tbias takes it.


def _check_tbias(Q, nnz, h, B, **types):
    """The table fp32[T >= 1, h] and the per-edge type arrays int32[nnz] -> T."""
    check_edges(Q, nnz, torch.int32, **types)
    check_family(Q, torch.float32, B=B)
    if B.dim() != 2 or B.shape[0] < 1 or B.shape[1] != h:
        raise RuntimeError(f"B must have shape (T >= 1, {h}), got {tuple(B.shape)}")
    return B.shape[0]


def gt_tbias_dB_supported(T, h):
    """Whether gt_backward_tbias computes dB for a table of T types at h heads (include/dfgnn.h:
    dfgnn_gt_tbias_bwd_ws_floats; the limit is T <= 4096).  The forward and the backward without dB take any T."""
    return int(_n.lib().dfgnn_gt_tbias_bwd_ws_floats(int(T), int(h))) > 0


def _forward_tbias(what, save_stats, row_ptr, col_ind, val, etype, B, Q, K, V):
    ext = _n.ext()
    if ext is not None:
        return ext.gt_fwd_tbias(row_ptr, col_ind, val, etype, B, Q, K, V, val_ptr(val) is None, save_stats)
    m, n_cols, nnz, h, f = _checks_rect(row_ptr, col_ind, Q, K, V, val=val)
    T = _check_tbias(Q, nnz, h, B, etype=etype)
    out = torch.empty_like(Q)
    row_max, row_sum = (_empty(Q, m, h), _empty(Q, m, h)) if save_stats else (None, None)
    call("dfgnn_gt_fwd_tbias_rect", what, Q.device, m, n_cols, nnz, h, f, T, row_ptr, col_ind, val_ptr(val), etype, B, Q, K, V,
         row_max, row_sum, out)
    return [out, row_max, row_sum] if save_stats else [out]


def gt_inference_tbias(row_ptr, col_ind, val, etype, B, Q, K, V):
    """-> out: inference of any graph with B[etype[e], hd] (B fp32[T, h], etype int32[nnz] in CSR order, 0 <= etype < T:
    not checked here) added to the logit of edge e before the softmax; -inf masks a type for a head.  val: edge values
    fp32[nnz] in CSR order; None or all ones: unit values."""
    return _forward_tbias("gt_inference_tbias", False, row_ptr, col_ind, val, etype, B, Q, K, V)[0]


def gt_forward_tbias(row_ptr, col_ind, val, etype, B, Q, K, V):
    """-> [out, row_max[m, h], row_sum[m, h]]: the training forward; an empty or fully masked row has out = 0,
    row_max = -1e38, row_sum = 0."""
    return _forward_tbias("gt_forward_tbias", True, row_ptr, col_ind, val, etype, B, Q, K, V)


def gt_backward_tbias(row_ptr, col_ind, val, etype, col_ptr, row_ind, val_idx, etype_csc, B, Q, K, V, out, row_max, row_sum,
                      grad, need_dB=True):
    """-> [dQ, dK, dV, dB[T, h]] from the forward's output and row statistics; etype_csc = etype[val_idx].  dB is None
    without need_dB (a frozen table: any T).  With need_dB the table must satisfy gt_tbias_dB_supported, else the call
    raises the library's "unsupported" RuntimeError before anything is launched."""
    val_idx = as_int32(val_idx)
    ext = _n.ext()
    if ext is not None:
        res = ext.gt_bwd_tbias(row_ptr, col_ind, val, etype, col_ptr, row_ind, val_idx, etype_csc, B, Q, K, V, out, row_max,
                               row_sum, grad, val_ptr(val) is None, need_dB)
        return res if need_dB else res + [None]
    m, n_cols, nnz, h, f = _checks_rect(row_ptr, col_ind, Q, K, V, val=val, out=out, grad=grad)
    T = _check_tbias(Q, nnz, h, B, etype=etype, etype_csc=etype_csc)
    check_csc_rect(Q, n_cols, nnz, col_ptr, "K / V", row_ind=row_ind, val_idx=val_idx)
    check_2d(Q, m, h, row_max=row_max, row_sum=row_sum)
    ws = dB = None
    if need_dB:
        ws_floats = int(_n.lib().dfgnn_gt_tbias_bwd_ws_floats(T, h))
        if ws_floats < 0:
            _n.check(ws_floats, "gt_backward_tbias")
        ws, dB = _empty(Q, ws_floats), torch.empty_like(B)
    delta = _empty(Q, m, h)
    dQ, dK, dV = torch.empty_like(Q), torch.empty_like(K), torch.empty_like(V)
    call("dfgnn_gt_bwd_tbias_rect", "gt_backward_tbias", Q.device, m, n_cols, nnz, h, f, T, row_ptr, col_ind, val_ptr(val), etype,
         col_ptr, row_ind, val_idx, etype_csc, B, Q, K, V, out, row_max, row_sum, grad, delta, ws, dQ, dK, dV, dB)
    return [dQ, dK, dV, dB]


# ---- AGNN / dot-product attention with tied keys and values (include/dfgnn.h: dfgnn_agnn_fwd / dfgnn_agnn_bwd) -----------
# Not part of the reference's module.  s_e = beta[h] r_i q_j <X_row_i, X_col_j> with r, q the inverse row norms (cosine: AGNN)
# or 1 (dot-product attention), message X_col_j (csrc/agnn_train.hip): the neighbour row is key and value, gathered once per
# edge; nothing per node is precomputed.  Any graph, square or m x n_cols, no plan, any f.
# DFGNN.operators.fused_gtconv.AGNNConvFuse takes it.


def _check_agnn(row_ptr, col_ind, beta, X_row, X_col, **like_X):
    """X_row (and `like_X`: out, grad) fp32 [m, heads, feat], X_col fp32 [n_cols, heads, feat], beta fp32 [heads], the CSR
    arrays of the m rows -> (m, n_cols, nnz, h, f)."""
    m, h, f = check_feats(X_row=X_row, **like_X)
    n_cols = check_cols("X_row", X_row, X_col=X_col)
    check_family(X_row, torch.float32, beta=beta)
    if tuple(beta.shape) != (h,):
        raise RuntimeError(f"beta must have shape ({h},), got {tuple(beta.shape)}")
    return m, n_cols, check_csr(X_row, m, row_ptr, col_ind), h, f


def _agnn_fwd(what, save_stats, row_ptr, col_ind, beta, X_row, X_col, cosine):
    ext = _n.ext()
    if ext is not None:
        return ext.agnn_fwd(row_ptr, col_ind, beta, bool(cosine), X_row, X_col, save_stats)
    m, n_cols, nnz, h, f = _check_agnn(row_ptr, col_ind, beta, X_row, X_col)
    out = torch.empty_like(X_row)
    row_max, row_sum = (_empty(X_row, m, h), _empty(X_row, m, h)) if save_stats else (None, None)
    call("dfgnn_agnn_fwd_rect", what, X_row.device, m, n_cols, nnz, h, f, row_ptr, col_ind, beta, int(bool(cosine)), X_row, X_col,
         row_max, row_sum, out)
    return [out, row_max, row_sum] if save_stats else [out]


def agnn_inference(row_ptr, col_ind, beta, X_row, X_col, cosine=True):
    """-> out[m, h, f].  beta fp32[h]; X_row and X_col may be the same tensor.  cosine=False: plain dot-product logits."""
    return _agnn_fwd("agnn_inference", False, row_ptr, col_ind, beta, X_row, X_col, cosine)[0]


def agnn_forward(row_ptr, col_ind, beta, X_row, X_col, cosine=True):
    """-> [out, row_max[m, h], row_sum[m, h]]: the training forward; the same `out` as agnn_inference."""
    return _agnn_fwd("agnn_forward", True, row_ptr, col_ind, beta, X_row, X_col, cosine)


def agnn_backward(row_ptr, col_ind, col_ptr, row_ind, beta, X_row, X_col, out, row_max, row_sum, grad, cosine=True,
                  need_dbeta=True):
    """-> [dX_row, dX_col, dbeta[h]] from the forward's output and row statistics (each edge is recomputed); dbeta is None
    without need_dbeta (then the rows' shares [m, h] are neither allocated nor written; dX_row and dX_col are the same
    bits).  With X_row is X_col the gradient of the shared tensor is dX_row + dX_col."""
    ext = _n.ext()
    if ext is not None:
        res = ext.agnn_bwd(row_ptr, col_ind, col_ptr, row_ind, beta, bool(cosine), X_row, X_col, out, row_max, row_sum, grad,
                           bool(need_dbeta))
        return res if need_dbeta else res + [None]
    m, n_cols, nnz, h, f = _check_agnn(row_ptr, col_ind, beta, X_row, X_col, out=out, grad=grad)
    check_csc_rect(X_row, n_cols, nnz, col_ptr, "X_col", row_ind=row_ind)
    check_2d(X_row, m, h, row_max=row_max, row_sum=row_sum)
    dX_row, dX_col, delta = torch.empty_like(X_row), torch.empty_like(X_col), _empty(X_row, m, h)
    dbeta_rows = _empty(X_row, m, h) if need_dbeta else None
    call("dfgnn_agnn_bwd_rect", "agnn_backward", X_row.device, m, n_cols, nnz, h, f, row_ptr, col_ind, col_ptr, row_ind, beta,
         int(bool(cosine)), X_row, X_col, out, row_max, row_sum, grad, delta, dX_row, dX_col, dbeta_rows)
    return [dX_row, dX_col, dbeta_rows.sum(0) if need_dbeta else None]


# ---- GatedGCN (include/dfgnn.h: dfgnn_gatedgcn_fwd / dfgnn_gatedgcn_bwd) -----------------------------------------------
# Not part of the reference's module.  z_e = X_row_i + X_col_j + E_e, sg_e = sigmoid(z_e) per dimension, out_i = sum sg_e (.)
# V_j [/ (sum sg_e + eps)], edge output Z = z (csrc/gatedgcn_train.hip): E, Z, the gradient G of Z and dE are fp32[nnz, h, f]
# in CSR edge order.  Any graph, square or m x n_cols, no plan, any f.  DFGNN.operators.fused_gtconv.GatedGCNConvFuse takes it.


def _check_gatedgcn(row_ptr, col_ind, X_row, X_col, V, E=None, G=None, **like_X):
    """X_row (and `like_X`: grad, out, den) fp32 [m, heads, feat], X_col and V fp32 [n_cols, heads, feat], the CSR arrays of
    the m rows, E and G (each optional) fp32 [nnz, heads, feat] -> (m, n_cols, nnz, h, f)."""
    m, h, f = check_feats(X_row=X_row, **like_X)
    n_cols = check_cols("X_row", X_row, X_col=X_col, V=V)
    nnz = check_csr(X_row, m, row_ptr, col_ind)
    if E is not None:
        check_3d(X_row, nnz, h, f, E=E)
    if G is not None:
        check_3d(X_row, nnz, h, f, G=G)
    return m, n_cols, nnz, h, f


def _gatedgcn_fwd(what, save_den, need_Z, row_ptr, col_ind, X_row, X_col, V, E, normalize, eps):
    ext = _n.ext()
    if ext is not None:
        return ext.gatedgcn_fwd(row_ptr, col_ind, X_row, X_col, V, E, bool(normalize), float(eps), save_den, bool(need_Z))
    m, n_cols, nnz, h, f = _check_gatedgcn(row_ptr, col_ind, X_row, X_col, V, E)
    out = torch.empty_like(X_row)
    den = torch.empty_like(X_row) if save_den else None
    Z = _empty(X_row, nnz, h, f) if need_Z else None
    call("dfgnn_gatedgcn_fwd_rect", what, X_row.device, m, n_cols, nnz, h, f, row_ptr, col_ind, X_row, X_col, V, E,
         int(bool(normalize)), float(eps), den, out, Z)
    return [out] + ([den] if save_den else []) + ([Z] if need_Z else [])


def gatedgcn_inference(row_ptr, col_ind, X_row, X_col, V, E=None, normalize=True, eps=1e-6, need_Z=False):
    """-> out[m, h, f], or (out, Z[nnz, h, f]) with need_Z.  E fp32[nnz, h, f] in CSR edge order or None (no edge term);
    X_row and X_col may be the same tensor.  normalize=False: the plain gated sum (PyG's ResGatedGraphConv)."""
    res = _gatedgcn_fwd("gatedgcn_inference", False, need_Z, row_ptr, col_ind, X_row, X_col, V, E, normalize, eps)
    return tuple(res) if need_Z else res[0]


def gatedgcn_forward(row_ptr, col_ind, X_row, X_col, V, E=None, normalize=True, eps=1e-6, need_Z=False):
    """-> (out, den[m, h, f], Z): the training forward; the same `out` and Z as gatedgcn_inference.  Z is None without
    need_Z (then nothing of size nnz h f is allocated or written).  An empty row has out = 0, den = 0."""
    res = _gatedgcn_fwd("gatedgcn_forward", True, need_Z, row_ptr, col_ind, X_row, X_col, V, E, normalize, eps)
    return tuple(res) if need_Z else (res[0], res[1], None)


def gatedgcn_backward(row_ptr, col_ind, col_ptr, row_ind, val_idx, X_row, X_col, V, E, out, den, grad, G=None,
                      normalize=True, eps=1e-6, need_dE=True):
    """-> (dX_row, dX_col, dV, dE[nnz, h, f]) from the forward's out and den (each edge is recomputed), the gradient `grad`
    of out and the gradient G[nnz, h, f] of Z (None: zero, nothing of it is read); dE is None without need_dE (then nothing
    of size nnz h f is allocated or written; the other three are the same bits).  normalize=False reads neither out nor den:
    None is accepted for both."""
    val_idx = as_int32(val_idx)
    if not normalize:
        out = den = None
    ext = _n.ext()
    if ext is not None:
        res = ext.gatedgcn_bwd(row_ptr, col_ind, col_ptr, row_ind, val_idx, X_row, X_col, V, E, bool(normalize), float(eps),
                               out, den, grad, G, bool(need_dE))
        return tuple(res) if need_dE else tuple(res) + (None,)
    if normalize and (out is None or den is None):
        raise RuntimeError("out and den of the forward are required with normalize")
    saved = {"out": out, "den": den} if normalize else {}
    m, n_cols, nnz, h, f = _check_gatedgcn(row_ptr, col_ind, X_row, X_col, V, E, G, grad=grad, **saved)
    check_csc_rect(X_row, n_cols, nnz, col_ptr, "X_col", row_ind=row_ind, val_idx=val_idx)
    dX_row, dX_col, dV = torch.empty_like(X_row), torch.empty_like(X_col), torch.empty_like(V)
    dE = _empty(X_row, nnz, h, f) if need_dE else None
    ws = torch.empty_like(X_row) if normalize else None   # s_i = dO_i / (den_i + eps), CSR pass -> CSC pass
    call("dfgnn_gatedgcn_bwd_rect", "gatedgcn_backward", X_row.device, m, n_cols, nnz, h, f, row_ptr, col_ind, col_ptr, row_ind,
         val_idx, X_row, X_col, V, E, int(bool(normalize)), float(eps), out, den, grad, G, dX_row, dX_col, dV, dE, ws)
    return dX_row, dX_col, dV, dE


# ---- the CSR-taking inference variants ----------------------------------------------------------------------------------
_VARIANTS = ("gt_tiling", "gt_csr", "gt_csr_gm", "gt_softmax", "gt_softmax_gm")   # by `which` of torch_ext.cpp: gt_variant_fwd


def _variant(which, indptr, indices, rows, val, Q, K, V):
    """-> out of inference variant `which`: dfgnn_<name>_fwd, reported as <name>_inference."""
    ext = _n.ext()
    if ext is not None:
        return ext.gt_variant_fwd(which, indptr, indices, rows, val, Q, K, V, val_ptr(val) is None)
    name = _VARIANTS[which]
    m, nnz, h, f = _checks(indptr, indices, Q, K, V, rows, val)
    out = torch.empty_like(Q)
    # 'tiling' and the two-kernel 'softmax' forms multiply the values in as they are (the latter after the COO rows, and
    # like the 'csr' forms with the logits [h, nnz] as scratch); the 'csr' forms take NULL for all ones
    graph = (indptr, indices) if which < 3 else (indptr, indices, rows)
    outs = (out,) if which == 0 else (_empty(Q, h, nnz), out)
    call(f"dfgnn_{name}_fwd", f"{name}_inference", Q.device, m, nnz, h, f, *graph, val_ptr(val) if which in (1, 2) else val,
         Q, K, V, *outs)
    return out


def gt_tiling_inference(indptr, indices, val, smem_consume, Q, K, V):
    """fused_gtconv.cpp:244-276 -> [out]"""
    return [_variant(0, indptr, indices, None, val, Q, K, V)]


def gt_csr_inference(indptr, indices, val, smem_consume, Q, K, V):
    """fused_gtconv.cpp:174-207 -> [out].  The node-parallel CSR baseline of the reference's sweeps (fused_gt_csr): a wave
    per row, the row's logits materialised in LDS (csrc/csr_fwd.hip), then max / sum / weighted-sum sweeps."""
    return [_variant(1, indptr, indices, None, val, Q, K, V)]


def gt_csr_gm_inference(indptr, indices, val, Q, K, V):
    """fused_gtconv.cpp:209-242 -> [out].  As gt_csr_inference with the logits in global memory
    (fused_gt_csr_global_memory)."""
    return [_variant(2, indptr, indices, None, val, Q, K, V)]


def gt_softmax_inference(indptr, indices, rows, val, smem_consume, Q, K, V):
    """fused_gtconv.cpp:316-352 -> [out] (two kernels: COO SDDMM, then LDS softmax+SpMM)."""
    return [_variant(3, indptr, indices, rows, val, Q, K, V)]


def gt_softmax_gm_inference(indptr, indices, rows, val, Q, K, V):
    """fused_gtconv.cpp:354-389 -> bare Tensor (two kernels, logits re-read from global memory)."""
    return _variant(4, indptr, indices, rows, val, Q, K, V)
