"""GT operator surface -- same names / signatures as the reference's DFGNN/operators/fused_gtconv.py.

Each function forwards to the `fused_gtconv` binding module (MI355X HIP kernels behind the C ABI).
Return conventions follow the reference: the binding returns a list for most entry points and the
wrapper unwraps element 0; `softmax_gm` returns a bare tensor (reference :279).
Note the argument-order quirk kept from the reference: `GTConvFuse_hyper` takes `rows` first, the
binding takes `row_ptr` first (reference :51-107).
"""
import fused_gtconv as fused_gt
import torch


def GTConvFuse_inference_hyper(indptr, indices, rows, val, smem_consume, Q, K, V):
    """hyper: one kernel, CSR + COO.  reference :5-25"""
    return fused_gt.gt_hyper_inference(indptr, indices, rows, val, smem_consume, Q, K, V)[0]


def GTConvFuse_inference_hyper_ablation(indptr, indices, rows, val, smem_consume, Q, K, V):
    """reference :28-48"""
    return fused_gt.gt_hyper_inference_ablation(indptr, indices, rows, val, smem_consume, Q, K, V)[0]


class FusedGTFunction_hyper(torch.autograd.Function):
    """Fused forward + fused backward.  reference :79-158

    The reference's forward saves the normalised attention (attn_edge[h, nnz]) for the backward.  When the whole batch
    runs on the matrix-core kernels (fused_gt.gt_stats_pair_applies: a block plan of dense ranges) and has at least two
    heads or edge values other than ones (fused_gt.gt_training_pair: there it is the faster pair, measured) the
    forward saves two floats per (row, head) instead -- logit maximum and sum of exponentials -- and the backward
    recomputes the attention (include/dfgnn.h: dfgnn_gt_hyper_fwd_stats / dfgnn_gt_bwd_stats): same gradients, 8 h nnz
    bytes less through HBM.  At one head with unit values such a batch keeps the reference's form but with attn_edge in
    RANK order (by column within a row: fused_gt.gt_ranked_pair_applies), which spares the forward the edge list and the
    position map.  Any other batch takes the reference's form below them."""

    @staticmethod
    def forward(ctx, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V):
        ctx.smem = smem_consume
        ctx.pair, ctx.plan = fused_gt.gt_training_pair(row_ptr, col_ind, val, Q)   # the pair's block plan, or None
        if ctx.pair == "stats":
            out_feat, row_max, row_sum = fused_gt.gt_hyper_forward_stats(row_ptr, col_ind, Q, K, V, ctx.plan, val)
            ctx.save_for_backward(row_ptr, col_ind, Q, K, V, row_max, row_sum, val)
        elif ctx.pair == "ranked":   # one head, all dense, unit values: attn_edge in rank order (same pair, cheaper forward)
            out_feat, attn_ranked = fused_gt.gt_hyper_forward_ranked(row_ptr, col_ind, Q, K, V, ctx.plan)
            ctx.save_for_backward(row_ptr, col_ind, Q, K, V, attn_ranked)
        else:
            out_feat, attn_edge = fused_gt.gt_hyper_forward(
                row_ptr, col_ind, rows, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V)
            ctx.save_for_backward(row_ptr, col_ind, rows, val, col_ptr, row_ind, val_idx, Q, K, V, attn_edge)
        return out_feat

    @staticmethod
    def backward(ctx, grad_out):
        if ctx.pair == "stats":
            row_ptr, col_ind, Q, K, V, row_max, row_sum, val = ctx.saved_tensors
            grads = fused_gt.gt_backward_stats(row_ptr, col_ind, Q, K, V, row_max, row_sum, grad_out.contiguous(),
                                               ctx.plan, val)
        elif ctx.pair == "ranked":
            row_ptr, col_ind, Q, K, V, attn_ranked = ctx.saved_tensors
            grads = fused_gt.gt_backward_ranked(row_ptr, col_ind, Q, K, V, attn_ranked, grad_out.contiguous(), ctx.plan)
        else:
            row_ptr, col_ind, rows, val, col_ptr, row_ind, val_idx, Q, K, V, attn_edge = ctx.saved_tensors
            grads = fused_gt.gt_backward(
                row_ptr, col_ind, rows, val, col_ptr, row_ind, val_idx, ctx.smem, Q, K, V, attn_edge,
                grad_out.contiguous())
        return (None,) * 8 + tuple(grads)


def GTConvFuse_hyper(rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V):
    """Differentiable hyper conv.  reference :51-76"""
    return FusedGTFunction_hyper.apply(
        rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V)


class FusedGTFunction_rowstats(torch.autograd.Function):
    """FusedGTFunction_hyper for ANY graph without per-edge saved state (opt-in; include/dfgnn.h: dfgnn_gt_fwd_rowstats /
    dfgnn_gt_bwd_rowstats, csrc/gt_train.hip).  Saved between forward and backward: Q, K, V, out, the row statistics
    row_max / row_sum [m, h] and the graph arrays -- nothing of size nnz in floating point (the reference's form keeps
    attn_edge[h, nnz] and allocates grad_edge[h, nnz] in its backward).  The backward recomputes each edge's attention
    from the rows it gathers anyway."""

    @staticmethod
    def forward(ctx, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V):
        out_feat, row_max, row_sum = fused_gt.gt_forward_rowstats(row_ptr, col_ind, val, Q, K, V)
        # unit edge values (what every reference flow passes) are not kept: the kernels never read them
        keep_val = () if fused_gt.val_ptr(val) is None else (val,)
        ctx.save_for_backward(row_ptr, col_ind, col_ptr, row_ind, val_idx, Q, K, V, out_feat, row_max, row_sum, *keep_val)
        return out_feat

    @staticmethod
    def backward(ctx, grad_out):
        row_ptr, col_ind, col_ptr, row_ind, val_idx, Q, K, V, out_feat, row_max, row_sum, *val = ctx.saved_tensors
        val = val[0] if val else None
        grad_Q, grad_K, grad_V = fused_gt.gt_backward_rowstats(row_ptr, col_ind, val, col_ptr, row_ind, val_idx, Q, K, V,
                                                               out_feat, row_max, row_sum, grad_out.contiguous())
        return (None,) * 8 + (grad_Q, grad_K, grad_V)


def GTConvFuse_rowstats(rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V):
    """Differentiable conv of any graph that saves row statistics instead of attn_edge; the argument list of
    GTConvFuse_hyper (`rows` and `smem_consume` are accepted and not used)."""
    return FusedGTFunction_rowstats.apply(
        rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V)


# ---- AGNN / dot-product attention with tied keys and values (this build's addition; fused_gtconv.agnn_*) -----------------
def AGNNConvFuse_inference(row_ptr, col_ind, beta, X_row, X_col, cosine=True):
    """-> out[m, h, f] = softmax_j(beta[h] cos(X_row_i, X_col_j)) X_col_j (cosine=False: beta[h] <X_row_i, X_col_j>); beta
    fp32 [heads], X_row / X_col fp32 [nodes, heads, feat] (may be the same tensor)."""
    return fused_gt.agnn_inference(row_ptr, col_ind, beta, X_row, X_col, cosine)


class FusedAGNNFunction(torch.autograd.Function):
    """Training pair (include/dfgnn.h: dfgnn_agnn_fwd / dfgnn_agnn_bwd, csrc/agnn_train.hip).  Saved between forward and
    backward: beta, X_row, X_col, out, two floats per (row, head) and the graph arrays -- no normalised copy of the features,
    nothing of size nnz in floating point.  The rows' shares of dbeta are requested only when beta needs a gradient."""

    @staticmethod
    def forward(ctx, row_ptr, col_ind, col_ptr, row_ind, beta, X_row, X_col, cosine):
        out, row_max, row_sum = fused_gt.agnn_forward(row_ptr, col_ind, beta, X_row, X_col, cosine)
        ctx.save_for_backward(row_ptr, col_ind, col_ptr, row_ind, beta, X_row, X_col, out, row_max, row_sum)
        ctx.cosine = bool(cosine)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        row_ptr, col_ind, col_ptr, row_ind, beta, X_row, X_col, out, row_max, row_sum = ctx.saved_tensors
        dX_row, dX_col, dbeta = fused_gt.agnn_backward(row_ptr, col_ind, col_ptr, row_ind, beta, X_row, X_col, out, row_max,
                                                       row_sum, grad_out.contiguous(), ctx.cosine,
                                                       need_dbeta=ctx.needs_input_grad[4])
        # (one tensor passed as both X_row and X_col: autograd adds the two gradients)
        return None, None, None, None, dbeta, dX_row, dX_col, None


def AGNNConvFuse(row_ptr, col_ind, col_ptr, row_ind, beta, X_row, X_col, cosine=True):
    """Differentiable AGNN (cosine=True) / dot-product (cosine=False) conv of any graph, square or m x n_cols; the gradient
    goes to beta, X_row and X_col."""
    return FusedAGNNFunction.apply(row_ptr, col_ind, col_ptr, row_ind, beta, X_row, X_col, cosine)


# ---- GatedGCN: per-dimension sigmoid gates, optional edge term and edge output (this build's addition; fused_gtconv.gatedgcn_*)
def GatedGCNConvFuse_inference(row_ptr, col_ind, X_row, X_col, V, E=None, normalize=True, eps=1e-6, edge_out=False):
    """-> out[m, h, f] = sum_j sg_ij (.) V_j [/ (sum_j sg_ij + eps)] with sg_ij = sigmoid(X_row_i + X_col_j + E_ij), or
    (out, Z) with edge_out: Z[nnz, h, f] = X_row_i + X_col_j + E_ij in CSR edge order.  E fp32[nnz, h, f] or None."""
    return fused_gt.gatedgcn_inference(row_ptr, col_ind, X_row, X_col, V, E, normalize, eps, need_Z=edge_out)


class FusedGatedGCNFunction(torch.autograd.Function):
    """Training pair (include/dfgnn.h: dfgnn_gatedgcn_fwd / dfgnn_gatedgcn_bwd, csrc/gatedgcn_train.hip) -> (out, Z), or out
    alone with edge_out=False.  Z is an OUTPUT the model trains through: its gradient G enters the backward next to grad_out
    (None when Z was not used: then nothing of G is read).  Z is not saved -- the backward recomputes every edge from the rows
    it gathers.  Saved between forward and backward: X_row, X_col, V, E (when given), the graph arrays and, with normalize,
    out and den [m, h, f].  dE[nnz, h, f] is computed only when E requires a gradient."""

    @staticmethod
    def forward(ctx, row_ptr, col_ind, col_ptr, row_ind, val_idx, X_row, X_col, V, E, normalize, eps, edge_out):
        out, den, Z = fused_gt.gatedgcn_forward(row_ptr, col_ind, X_row, X_col, V, E, normalize, eps, need_Z=edge_out)
        keep = ((E,) if E is not None else ()) + ((out, den) if normalize else ())
        ctx.save_for_backward(row_ptr, col_ind, col_ptr, row_ind, val_idx, X_row, X_col, V, *keep)
        ctx.has_E, ctx.normalize, ctx.eps = E is not None, bool(normalize), float(eps)
        ctx.set_materialize_grads(False)       # an unused Z arrives as None, not as zeros [nnz, h, f]
        return (out, Z) if edge_out else out

    @staticmethod
    def backward(ctx, grad_out, grad_Z=None):
        row_ptr, col_ind, col_ptr, row_ind, val_idx, X_row, X_col, V, *keep = ctx.saved_tensors
        E = keep.pop(0) if ctx.has_E else None
        out, den = keep if ctx.normalize else (None, None)
        if grad_out is None:                   # only Z was used
            grad_out = torch.zeros_like(X_row)
        dX_row, dX_col, dV, dE = fused_gt.gatedgcn_backward(
            row_ptr, col_ind, col_ptr, row_ind, val_idx, X_row, X_col, V, E, out, den, grad_out.contiguous(),
            G=None if grad_Z is None else grad_Z.contiguous(), normalize=ctx.normalize, eps=ctx.eps,
            need_dE=ctx.has_E and ctx.needs_input_grad[8])
        # (one tensor passed as both X_row and X_col: autograd adds the two gradients)
        return (None,) * 5 + (dX_row, dX_col, dV, dE, None, None, None)


def GatedGCNConvFuse(row_ptr, col_ind, col_ptr, row_ind, val_idx, X_row, X_col, V, E=None, normalize=True, eps=1e-6,
                     edge_out=True):
    """Differentiable GatedGCN conv of any graph, square or m x n_cols -> (out, Z) with the edge output Z[nnz, h, f] =
    X_row_i + X_col_j + E_ij, or out alone with edge_out=False; the gradient goes to X_row, X_col, V and E."""
    return FusedGatedGCNFunction.apply(row_ptr, col_ind, col_ptr, row_ind, val_idx, X_row, X_col, V, E, normalize, eps,
                                       edge_out)


class FusedGTFunction_bias(torch.autograd.Function):
    """FusedGTFunction_rowstats with a per-edge, per-head additive attention bias (include/dfgnn.h: dfgnn_gt_fwd_bias /
    dfgnn_gt_bwd_bias, csrc/gt_bias_train.hip): s_e = val_e <Q_i, K_j> + bias[h, e], bias fp32[h, nnz] in CSR edge order,
    -inf masks an edge.  Saved between forward and backward: Q, K, V, bias, out, the row statistics and the graph arrays
    (`val` only when it is not all ones).  dbias[h, nnz] is computed only when the bias requires a gradient; otherwise the
    backward allocates and writes nothing of size h nnz."""

    @staticmethod
    def forward(ctx, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V, bias):
        out_feat, row_max, row_sum = fused_gt.gt_forward_bias(row_ptr, col_ind, val, bias, Q, K, V)
        keep_val = () if fused_gt.val_ptr(val) is None else (val,)
        ctx.save_for_backward(row_ptr, col_ind, col_ptr, row_ind, val_idx, Q, K, V, bias, out_feat, row_max, row_sum,
                              *keep_val)
        return out_feat

    @staticmethod
    def backward(ctx, grad_out):
        row_ptr, col_ind, col_ptr, row_ind, val_idx, Q, K, V, bias, out_feat, row_max, row_sum, *val = ctx.saved_tensors
        val = val[0] if val else None
        grad_Q, grad_K, grad_V, grad_bias = fused_gt.gt_backward_bias(
            row_ptr, col_ind, val, bias, col_ptr, row_ind, val_idx, Q, K, V, out_feat, row_max, row_sum,
            grad_out.contiguous(), need_dbias=ctx.needs_input_grad[11])
        return (None,) * 8 + (grad_Q, grad_K, grad_V, grad_bias)


def GTConvFuse_bias(rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V, bias):
    """Differentiable conv of any graph with the additive attention bias fp32[h, nnz] (CSR edge order); the argument list
    of GTConvFuse_rowstats plus `bias` (`rows` and `smem_consume` are accepted and not used)."""
    return FusedGTFunction_bias.apply(
        rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V, bias)


def GTConvFuse_inference_bias(row_ptr, col_ind, val, Q, K, V, bias):
    """Inference of any graph with the additive attention bias fp32[h, nnz] (CSR edge order)."""
    return fused_gt.gt_inference_bias(row_ptr, col_ind, val, bias, Q, K, V)


class FusedGTFunction_edge(torch.autograd.Function):
    """FusedGTFunction_rowstats with a per-edge feature vector added to keys and values (include/dfgnn.h: dfgnn_gt_fwd_edge /
    dfgnn_gt_bwd_edge, csrc/gt_edge_train.hip): k~_e = K_j + E_e, v~_e = V_j + E_e, E fp32[nnz, h, f] in CSR edge order.
    Saved between forward and backward: Q, K, V, E, out, the row statistics and the graph arrays (`val` only when it is not
    all ones) -- nothing of size nnz h f beyond E itself.  dE[nnz, h, f] is computed only when E requires a gradient;
    otherwise the backward allocates and writes nothing of that size."""

    @staticmethod
    def forward(ctx, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V, E):
        out_feat, row_max, row_sum = fused_gt.gt_forward_edge(row_ptr, col_ind, val, E, Q, K, V)
        keep_val = () if fused_gt.val_ptr(val) is None else (val,)
        ctx.save_for_backward(row_ptr, col_ind, col_ptr, row_ind, val_idx, Q, K, V, E, out_feat, row_max, row_sum,
                              *keep_val)
        return out_feat

    @staticmethod
    def backward(ctx, grad_out):
        row_ptr, col_ind, col_ptr, row_ind, val_idx, Q, K, V, E, out_feat, row_max, row_sum, *val = ctx.saved_tensors
        val = val[0] if val else None
        grad_Q, grad_K, grad_V, grad_E = fused_gt.gt_backward_edge(
            row_ptr, col_ind, val, E, col_ptr, row_ind, val_idx, Q, K, V, out_feat, row_max, row_sum,
            grad_out.contiguous(), need_dE=ctx.needs_input_grad[11])
        return (None,) * 8 + (grad_Q, grad_K, grad_V, grad_E)


def GTConvFuse_edge(rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V, E):
    """Differentiable conv of any graph with the edge features fp32[nnz, h, f] (CSR edge order) added to keys and values;
    the argument list of GTConvFuse_rowstats plus `E` (`rows` and `smem_consume` are accepted and not used)."""
    return FusedGTFunction_edge.apply(
        rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V, E)


def GTConvFuse_inference_edge(row_ptr, col_ind, val, Q, K, V, E):
    """Inference of any graph with the edge features fp32[nnz, h, f] (CSR edge order) added to keys and values."""
    return fused_gt.gt_inference_edge(row_ptr, col_ind, val, E, Q, K, V)


class FusedGTFunction_gate(torch.autograd.Function):
    """FusedGTFunction_rowstats with a per-edge multiplicative gate on the keys and an edge output (include/dfgnn.h:
    dfgnn_gt_fwd_gate / dfgnn_gt_bwd_gate, csrc/gt_gate_train.hip): ke_e = K_j (.) E_e, s_e = val_e <Q_i, ke_e>,
    W_e = val_e Q_i (.) ke_e, E and W fp32[nnz, h, f] in CSR edge order; no clamp on the logit.  -> (out, W), or out alone
    with edge_out=False.  W is an OUTPUT the model trains through: its gradient G enters the backward next to grad_out
    (None when W was not used: then nothing of G is read).  W is not saved -- the backward recomputes every edge from the
    rows it gathers.  Saved between forward and backward: Q, K, V, E, out, the row statistics and the graph arrays (`val`
    only when it is not all ones).  dE[nnz, h, f] is computed only when E requires a gradient."""

    @staticmethod
    def forward(ctx, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V, E, edge_out):
        out_feat, row_max, row_sum, W = fused_gt.gt_forward_gate(row_ptr, col_ind, val, E, Q, K, V, need_W=edge_out)
        keep_val = () if fused_gt.val_ptr(val) is None else (val,)
        ctx.save_for_backward(row_ptr, col_ind, col_ptr, row_ind, val_idx, Q, K, V, E, out_feat, row_max, row_sum,
                              *keep_val)
        ctx.edge_out = edge_out
        ctx.set_materialize_grads(False)       # an unused W arrives as None, not as zeros [nnz, h, f]
        return (out_feat, W) if edge_out else out_feat

    @staticmethod
    def backward(ctx, grad_out, grad_W=None):
        row_ptr, col_ind, col_ptr, row_ind, val_idx, Q, K, V, E, out_feat, row_max, row_sum, *val = ctx.saved_tensors
        val = val[0] if val else None
        if grad_out is None:                   # only W was used
            grad_out = torch.zeros_like(out_feat)
        grad_Q, grad_K, grad_V, grad_E = fused_gt.gt_backward_gate(
            row_ptr, col_ind, val, E, col_ptr, row_ind, val_idx, Q, K, V, out_feat, row_max, row_sum,
            grad_out.contiguous(), G=None if grad_W is None else grad_W.contiguous(), need_dE=ctx.needs_input_grad[11])
        return (None,) * 8 + (grad_Q, grad_K, grad_V, grad_E, None)


def GTConvFuse_gate(rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V, E, edge_out=True):
    """Differentiable conv of any graph with the keys gated by the edge features fp32[nnz, h, f] (CSR edge order) -> (out, W)
    with the edge output W[nnz, h, f] = val_e Q_i (.) K_j (.) E_e, or out alone with edge_out=False; the argument list of
    GTConvFuse_edge plus `edge_out` (`rows` and `smem_consume` are accepted and not used)."""
    return FusedGTFunction_gate.apply(
        rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V, E, edge_out)


def GTConvFuse_inference_gate(row_ptr, col_ind, val, Q, K, V, E, edge_out=True):
    """Inference of any graph with the keys gated by the edge features fp32[nnz, h, f] (CSR edge order) -> (out, W), or out
    alone with edge_out=False."""
    return fused_gt.gt_inference_gate(row_ptr, col_ind, val, E, Q, K, V, need_W=edge_out)


class FusedGTFunction_typed(torch.autograd.Function):
    """FusedGTFunction_edge with E_e = R[etype[e]] looked up in the kernels (include/dfgnn.h: dfgnn_gt_fwd_typed /
    dfgnn_gt_bwd_typed, csrc/gt_typed_train.hip): R fp32[T, h, f], etype int32[nnz] in CSR edge order, etype_csc the same types
    in CSC entry order (DFGNN.layers.preprocess_types).  Saved between forward and backward: Q, K, V, R, out, the row
    statistics and the graph arrays (`val` only when it is not all ones) -- nothing of size nnz h f exists at any point.
    dR[T, h, f] is computed (per-workgroup partial sums, a fixed-order reduction: no atomics) only when R requires a
    gradient."""

    @staticmethod
    def forward(ctx, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V, R, etype, etype_csc):
        out_feat, row_max, row_sum = fused_gt.gt_forward_typed(row_ptr, col_ind, val, etype, R, Q, K, V)
        keep_val = () if fused_gt.val_ptr(val) is None else (val,)
        ctx.save_for_backward(row_ptr, col_ind, col_ptr, row_ind, val_idx, etype, etype_csc, Q, K, V, R, out_feat, row_max,
                              row_sum, *keep_val)
        return out_feat

    @staticmethod
    def backward(ctx, grad_out):
        (row_ptr, col_ind, col_ptr, row_ind, val_idx, etype, etype_csc, Q, K, V, R, out_feat, row_max, row_sum,
         *val) = ctx.saved_tensors
        val = val[0] if val else None
        grad_Q, grad_K, grad_V, grad_R = fused_gt.gt_backward_typed(
            row_ptr, col_ind, val, etype, col_ptr, row_ind, val_idx, etype_csc, R, Q, K, V, out_feat, row_max, row_sum,
            grad_out.contiguous(), need_dR=ctx.needs_input_grad[11])
        return (None,) * 8 + (grad_Q, grad_K, grad_V, grad_R, None, None)


def GTConvFuse_typed(rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V, R, etype, etype_csc):
    """Differentiable conv of any graph with typed edges: R[etype[e]] (R fp32[T, h, f]) is added to the key and the value of
    edge e; the argument list of GTConvFuse_rowstats plus `R`, `etype` and `etype_csc` (`rows` and `smem_consume` are
    accepted and not used).
    Where R needs a gradient and the table is beyond what the kernels reduce (fused_gt.gt_typed_dR_supported: T f <=
    8192), this calls GTConvFuse_edge on the materialised R[etype]: the result is correct, but it allocates tensors of size
    nnz h f and autograd reduces dE to dR with an atomic index_add, whose sum is not reproducible bit for bit."""
    if R.requires_grad and torch.is_grad_enabled() and not fused_gt.gt_typed_dR_supported(R.shape[0], Q.shape[1], Q.shape[2]):
        return GTConvFuse_edge(rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V,
                               R[etype.long()])
    return FusedGTFunction_typed.apply(
        rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V, R, etype, etype_csc)


def GTConvFuse_inference_typed(row_ptr, col_ind, val, Q, K, V, R, etype):
    """Inference of any graph with typed edges: R[etype[e]] (R fp32[T, h, f]) added to keys and values; any T."""
    return fused_gt.gt_inference_typed(row_ptr, col_ind, val, etype, R, Q, K, V)


class FusedGTFunction_tbias(torch.autograd.Function):
    """FusedGTFunction_bias with bias[hd, e] = B[etype[e], hd] looked up in the kernels (include/dfgnn.h: dfgnn_gt_fwd_tbias /
    dfgnn_gt_bwd_tbias, csrc/gt_tbias_train.hip): B fp32[T, h], etype int32[nnz] in CSR edge order, etype_csc the same types
    in CSC entry order (DFGNN.layers.preprocess_types).  Saved between forward and backward: Q, K, V, B, out, the row
    statistics and the graph arrays (`val` only when it is not all ones) -- nothing of size h nnz exists at any point.
    dB[T, h] is computed (per-workgroup partial sums, a fixed-order reduction: no atomics) only when B requires a
    gradient."""

    @staticmethod
    def forward(ctx, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V, B, etype, etype_csc):
        out_feat, row_max, row_sum = fused_gt.gt_forward_tbias(row_ptr, col_ind, val, etype, B, Q, K, V)
        keep_val = () if fused_gt.val_ptr(val) is None else (val,)
        ctx.save_for_backward(row_ptr, col_ind, col_ptr, row_ind, val_idx, etype, etype_csc, Q, K, V, B, out_feat, row_max,
                              row_sum, *keep_val)
        return out_feat

    @staticmethod
    def backward(ctx, grad_out):
        (row_ptr, col_ind, col_ptr, row_ind, val_idx, etype, etype_csc, Q, K, V, B, out_feat, row_max, row_sum,
         *val) = ctx.saved_tensors
        val = val[0] if val else None
        grad_Q, grad_K, grad_V, grad_B = fused_gt.gt_backward_tbias(
            row_ptr, col_ind, val, etype, col_ptr, row_ind, val_idx, etype_csc, B, Q, K, V, out_feat, row_max, row_sum,
            grad_out.contiguous(), need_dB=ctx.needs_input_grad[11])
        return (None,) * 8 + (grad_Q, grad_K, grad_V, grad_B, None, None)


def GTConvFuse_tbias(rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V, B, etype, etype_csc):
    """Differentiable conv of any graph with a typed attention bias: B[etype[e], hd] (B fp32[T, h]; -inf masks a type for a
    head) is added to the logit of edge e before the softmax; the argument list of GTConvFuse_rowstats plus `B`, `etype` and
    `etype_csc` (`rows` and `smem_consume` are accepted and not used).
    Where B needs a gradient and the table is beyond what the kernels reduce (fused_gt.gt_tbias_dB_supported: T <= 4096),
    this calls GTConvFuse_bias on the materialised B[etype].t(): the result is correct, but it allocates tensors of size
    h nnz and autograd reduces dbias to dB with an atomic index_add, whose sum is not reproducible bit for bit."""
    if B.requires_grad and torch.is_grad_enabled() and not fused_gt.gt_tbias_dB_supported(B.shape[0], Q.shape[1]):
        return GTConvFuse_bias(rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V,
                               B[etype.long()].t().contiguous())
    return FusedGTFunction_tbias.apply(
        rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, Q, K, V, B, etype, etype_csc)


def GTConvFuse_inference_tbias(row_ptr, col_ind, val, Q, K, V, B, etype):
    """Inference of any graph with a typed attention bias: B[etype[e], hd] (B fp32[T, h]) added to the logits; any T."""
    return fused_gt.gt_inference_tbias(row_ptr, col_ind, val, etype, B, Q, K, V)


def GTConvFuse_inference_softmax(indptr, indices, rows, val, smem_consume, Q, K, V):
    """softmax: two kernels (COO SDDMM, then softmax + SpMM).  reference :238-259"""
    return fused_gt.gt_softmax_inference(indptr, indices, rows, val, smem_consume, Q, K, V)[0]


def GTConvFuse_inference_softmax_gm(indptr, indices, rows, val, Q, K, V):
    """softmax with logits kept in global memory; bare tensor.  reference :262-279"""
    return fused_gt.gt_softmax_gm_inference(indptr, indices, rows, val, Q, K, V)


def GTConvFuse_inference_csr(indptr, indices, val, smem_consume, Q, K, V):
    """reference :282-301"""
    return fused_gt.gt_csr_inference(indptr, indices, val, smem_consume, Q, K, V)[0]


def GTConvFuse_inference_csr_gm(indptr, indices, val, Q, K, V):
    """reference :304-321"""
    return fused_gt.gt_csr_gm_inference(indptr, indices, val, Q, K, V)[0]


def GTConvFuse_inference_tiling(indptr, indices, val, smem_consume, Q, K, V):
    """tiling: one kernel, column tiles + online softmax.  reference :324-343"""
    return fused_gt.gt_tiling_inference(indptr, indices, val, smem_consume, Q, K, V)[0]
