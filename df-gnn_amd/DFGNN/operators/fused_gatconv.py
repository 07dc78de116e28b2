"""GAT operator surface -- same names / signatures as the reference's DFGNN/operators/fused_gatconv.py.

In scope: the hyper / softmax / softmax_gm / tiling inference functions and the training
pair `GATConvFuse` / `FusedGATFunction` and the hyper_v2 / hyper_recompute / hyper_ablation
variants of the reference's comparison sweeps.
"""
import fused_gatconv as fused_gat
import torch


def GATConvFuse_inference_hyper(smem_consume, attn_row, attn_col, indptr, indices, rows, negative_slope, in_feat):
    """reference :31-36"""
    return fused_gat.gat_inference_hyper(
        smem_consume, attn_row, attn_col, indptr, indices, rows, negative_slope, in_feat)


def GATConvFuse_inference_hyper_ablation(smem_consume, attn_row, attn_col, indptr, indices, rows,
                                         negative_slope, in_feat):
    """reference :55-60"""
    return fused_gat.gat_inference_hyper_ablation(
        smem_consume, attn_row, attn_col, indptr, indices, rows, negative_slope, in_feat)


def GATConvFuse_inference_softmax(smem_consume, attn_row, attn_col, indptr, indices, rows, negative_slope, in_feat):
    """reference :63-68"""
    return fused_gat.gat_inference_softmax(
        smem_consume, attn_row, attn_col, indptr, indices, rows, negative_slope, in_feat)


def GATConvFuse_inference_softmax_gm(attn_row, attn_col, indptr, indices, rows, negative_slope, in_feat):
    """reference :71-76"""
    return fused_gat.gat_inference_softmax_gm(attn_row, attn_col, indptr, indices, rows, negative_slope, in_feat)


def GATConvFuse_inference_tiling(attn_row, attn_col, row_ptr, col_ind, negative_slope, in_feat):
    """reference :79-84"""
    return fused_gat.gat_inference_tiling(attn_row, attn_col, row_ptr, col_ind, negative_slope, in_feat)


def GATConvFuse_inference(attn_row, attn_col, row_ptr, col_ind, negative_slope, in_feat):
    """reference :87-92"""
    return fused_gat.gat_inference(attn_row, attn_col, row_ptr, col_ind, negative_slope, in_feat)


def GATConvFuse_inference_hyper_recompute(attn_row, attn_col, indptr, indices, negative_slope, in_feat):
    """reference :39-44"""
    return fused_gat.gat_inference_hyper_recompute(attn_row, attn_col, indptr, indices, negative_slope, in_feat)


def GATConvFuse_inference_hyper_v2(smem_consume, a_l, a_r, indptr, indices, negative_slope, in_feat):
    """reference :47-52"""
    return fused_gat.gat_inference_hyper_v2(smem_consume, a_l, a_r, indptr, indices, negative_slope, in_feat)


class FusedGATFunction(torch.autograd.Function):
    """reference :95-176 (training pair: fwd saves the row statistics, bwd recomputes the attention)."""

    @staticmethod
    def forward(ctx, attn_row, attn_col, row_ptr, col_ind, col_ptr, row_ind, permute, negative_slope, in_feat,
                attn_drop):
        out_feat, edge_max, edge_sum, edge_mask = fused_gat.gat_forward(
            attn_row, attn_col, row_ptr, col_ind, negative_slope, in_feat, attn_drop)
        ctx.save_for_backward(row_ptr, col_ind, col_ptr, row_ind, permute, edge_max, edge_sum, edge_mask,
                              in_feat, attn_row, attn_col)
        ctx.negative_slope, ctx.attn_drop = negative_slope, attn_drop
        return out_feat

    @staticmethod
    def backward(ctx, grad_out):
        (row_ptr, col_ind, col_ptr, row_ind, permute, edge_max, edge_sum, edge_mask, in_feat, attn_row,
         attn_col) = ctx.saved_tensors
        grad_feat, grad_attn_row, grad_attn_col = fused_gat.gat_backward(
            ctx.negative_slope, ctx.attn_drop, row_ptr, col_ind, col_ptr, row_ind, permute, edge_max, edge_sum,
            edge_mask, in_feat, attn_row, attn_col, grad_out.contiguous())
        return grad_attn_row, grad_attn_col, None, None, None, None, None, None, grad_feat, None


def GATConvFuse(attn_row, attn_col, row_ptr, col_ind, col_ptr, row_ind, permute, negative_slope, in_feat,
                attn_drop):
    """reference :5-28"""
    return FusedGATFunction.apply(attn_row, attn_col, row_ptr, col_ind, col_ptr, row_ind, permute,
                                  negative_slope, in_feat, attn_drop)


# ---- GATv2 (this build's addition; fused_gatconv.gatv2_*): logits a^T LeakyReLU(X_row[i] + X_col[j]) ---------------------
def GATv2ConvFuse_inference(attn, row_ptr, col_ind, negative_slope, X_row, X_col):
    """-> out[m, h, f]; attn fp32 [heads, feat], X_row / X_col fp32 [nodes, heads, feat] (the same tensor: shared weights)."""
    return fused_gat.gatv2_inference(attn, row_ptr, col_ind, negative_slope, X_row, X_col)


class FusedGATv2Function(torch.autograd.Function):
    """Training pair: the forward saves its output and two floats per (row, head); the backward recomputes each edge from
    the rows it gathers.  No floating-point tensor of nnz elements is created or kept."""

    @staticmethod
    def forward(ctx, attn, row_ptr, col_ind, col_ptr, row_ind, negative_slope, X_row, X_col):
        out, row_max, row_sum = fused_gat.gatv2_forward(attn, row_ptr, col_ind, negative_slope, X_row, X_col)
        ctx.save_for_backward(row_ptr, col_ind, col_ptr, row_ind, attn, X_row, X_col, out, row_max, row_sum)
        ctx.negative_slope = negative_slope
        return out

    @staticmethod
    def backward(ctx, grad_out):
        row_ptr, col_ind, col_ptr, row_ind, attn, X_row, X_col, out, row_max, row_sum = ctx.saved_tensors
        dX_row, dX_col, dattn = fused_gat.gatv2_backward(ctx.negative_slope, row_ptr, col_ind, col_ptr, row_ind, attn, X_row,
                                                         X_col, out, row_max, row_sum, grad_out.contiguous())
        # (one tensor passed as both X_row and X_col: autograd adds the two gradients)
        return dattn, None, None, None, None, None, dX_row, dX_col


def GATv2ConvFuse(attn, row_ptr, col_ind, col_ptr, row_ind, negative_slope, X_row, X_col):
    return FusedGATv2Function.apply(attn, row_ptr, col_ind, col_ptr, row_ind, negative_slope, X_row, X_col)


# ---- GATv2 with per-edge feature vectors (fused_gatconv.gatv2_*_edge): logits a^T LeakyReLU(X_row[i] + X_col[j] + E_e) ----
def GATv2ConvFuse_inference_edge(attn, row_ptr, col_ind, negative_slope, X_row, X_col, E):
    """-> out[m, h, f]; E fp32 [nnz, heads, feat] in CSR edge order, added inside the LeakyReLU and not part of the message
    (PyG's GATv2Conv(edge_dim))."""
    return fused_gat.gatv2_inference_edge(attn, row_ptr, col_ind, negative_slope, X_row, X_col, E)


class FusedGATv2Function_edge(torch.autograd.Function):
    """FusedGATv2Function with E[nnz, heads, feat] inside the LeakyReLU (include/dfgnn.h: dfgnn_gatv2_fwd_edge /
    dfgnn_gatv2_bwd_edge, csrc/gatv2_edge_train.hip).  Saved between forward and backward: attn, X_row, X_col, E, out, the row
    statistics and the graph arrays -- nothing of size nnz h f beyond E itself.  dE[nnz, heads, feat] is computed only when E
    requires a gradient; otherwise the backward allocates and writes nothing of that size."""

    @staticmethod
    def forward(ctx, attn, row_ptr, col_ind, col_ptr, row_ind, val_idx, negative_slope, X_row, X_col, E):
        out, row_max, row_sum = fused_gat.gatv2_forward_edge(attn, row_ptr, col_ind, negative_slope, X_row, X_col, E)
        ctx.save_for_backward(row_ptr, col_ind, col_ptr, row_ind, val_idx, attn, X_row, X_col, E, out, row_max, row_sum)
        ctx.negative_slope = negative_slope
        return out

    @staticmethod
    def backward(ctx, grad_out):
        row_ptr, col_ind, col_ptr, row_ind, val_idx, attn, X_row, X_col, E, out, row_max, row_sum = ctx.saved_tensors
        dX_row, dX_col, dattn, dE = fused_gat.gatv2_backward_edge(
            ctx.negative_slope, row_ptr, col_ind, col_ptr, row_ind, val_idx, attn, X_row, X_col, E, out, row_max, row_sum,
            grad_out.contiguous(), want_dE=ctx.needs_input_grad[9])
        # (one tensor passed as both X_row and X_col: autograd adds the two gradients)
        return dattn, None, None, None, None, None, None, dX_row, dX_col, dE


def GATv2ConvFuse_edge(attn, row_ptr, col_ind, col_ptr, row_ind, val_idx, negative_slope, X_row, X_col, E):
    """Differentiable GATv2 conv of any graph with the edge features fp32[nnz, h, f] (CSR edge order) inside the LeakyReLU;
    the argument list of GATv2ConvFuse plus `val_idx` (the CSR position of each CSC entry) and `E`."""
    return FusedGATv2Function_edge.apply(attn, row_ptr, col_ind, col_ptr, row_ind, val_idx, negative_slope, X_row, X_col, E)


# ---- GAT of any graph with an optional per-edge attention term (fused_gatconv.gat_*_edge) ---------------------------------
# logits LeakyReLU(attn_row[i] + attn_col[j] + score[h, e]) on an m x n_cols graph: in_feat fp32[n_cols, h, f] are the sources
def GATConvFuse_inference_edge(attn_row, attn_col, row_ptr, col_ind, negative_slope, in_feat, score=None):
    """-> out[m, h, f]; attn_row [m, heads], attn_col [n_cols, heads], score fp32[heads, nnz] in CSR edge order or None
    (PyG's GATConv(edge_dim): the term is inside the LeakyReLU and not part of the message).  No dropout."""
    return fused_gat.gat_inference_edge(attn_row, attn_col, row_ptr, col_ind, negative_slope, in_feat, score)


class FusedGATFunction_edge(torch.autograd.Function):
    """Training pair (include/dfgnn.h: dfgnn_gat_fwd_edge / dfgnn_gat_bwd_edge, csrc/gat_edge_train.hip): FusedGATFunction
    for any graph, square or m x n_cols, with the optional edge term.  Saved between forward and backward: the inputs,
    two floats per (row, head) and -- with dropout only -- the randoms [nnz, heads].  grad_score [heads, nnz] is computed only
    when score requires a gradient; otherwise the backward allocates and writes nothing of that size."""

    @staticmethod
    def forward(ctx, attn_row, attn_col, row_ptr, col_ind, col_ptr, row_ind, val_idx, negative_slope, in_feat, attn_drop,
                score):
        out, edge_max, edge_sum, edge_mask = fused_gat.gat_forward_edge(attn_row, attn_col, row_ptr, col_ind, negative_slope,
                                                                        in_feat, score, attn_drop)
        ctx.save_for_backward(row_ptr, col_ind, col_ptr, row_ind, val_idx, attn_row, attn_col, in_feat, edge_max, edge_sum,
                              score, edge_mask)
        ctx.negative_slope, ctx.attn_drop = negative_slope, attn_drop
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (row_ptr, col_ind, col_ptr, row_ind, val_idx, attn_row, attn_col, in_feat, edge_max, edge_sum, score,
         edge_mask) = ctx.saved_tensors
        grad_feat, grad_attn_row, grad_attn_col, grad_score = fused_gat.gat_backward_edge(
            ctx.negative_slope, ctx.attn_drop, row_ptr, col_ind, col_ptr, row_ind, val_idx, attn_row, attn_col, in_feat,
            edge_max, edge_sum, grad_out.contiguous(), score=score, edge_mask=edge_mask,
            want_grad_score=score is not None and ctx.needs_input_grad[10])
        return grad_attn_row, grad_attn_col, None, None, None, None, None, None, grad_feat, None, grad_score


def GATConvFuse_edge(attn_row, attn_col, row_ptr, col_ind, col_ptr, row_ind, val_idx, negative_slope, in_feat, attn_drop=0.0,
                     score=None):
    """Differentiable GAT conv of any graph; the argument list of GATConvFuse with `val_idx` (the CSR position of each CSC
    entry; GATConvFuse calls it permute) and the optional edge term `score` fp32[heads, nnz] in CSR edge order."""
    return FusedGATFunction_edge.apply(attn_row, attn_col, row_ptr, col_ind, col_ptr, row_ind, val_idx, negative_slope,
                                       in_feat, attn_drop, score)
