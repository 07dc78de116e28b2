"""AGNN layers (attention = softmax over the cosine similarity of the projected features) on the fused GT operators:
Q = K = row-normalised H, V = H.  Same class names, constructor and forward(params, feat, fuse) contract as the
reference's DFGNN/layers/AGNN/*.py (agnn_layer.py:7-19 base; agnn_layer_fused.py:13-122 csr / softmax / hyper;
agnn_layer_tiling.py, agnn_layer_csr_gm.py, agnn_layer_softmax_gm.py; agnn_layer_forward.py:8-66 training) -- no new
kernels.  Like the reference, the projection is Linear(in, out) viewed as
[N, heads, out], i.e. the layers are single-head (heads = 1) in practice.  One table-driven body instead of the reference's per-format copies: a variant is the
operator it calls plus how it picks that operator's arguments out of the preprocess tuple."""
import torch
from torch import nn
from torch.nn import functional as F

from DFGNN.operators import fused_gtconv as ops
from DFGNN.utils import sparse as dglsp


class AGNNConvDGL(nn.Module):
    def __init__(self, in_size, out_size, num_heads):
        super().__init__()
        self.in_size, self.out_size, self.num_heads = in_size, out_size, num_heads
        self.proj = nn.Linear(in_size, out_size)

    def forward_dglsp(self, A, H):
        """Non-fused branch; H is [N, out, heads] (reference agnn_layer.py:14-19)."""
        H_norm = F.normalize(H, p=2, dim=1)
        attn = dglsp.bsddmm(A, H_norm, H_norm.transpose(1, 0)).softmax()
        return dglsp.bspmm(attn, H)


class _AGNNInference(AGNNConvDGL):
    """forward(params, feat, fuse) -> (out[N, heads * out], elapsed_ms), timed like the reference (3 dry + 10 runs)."""
    op = None            # fused operator: op(*graph_args, Q, K, V)
    n_params = 0         # length of the preprocess tuple this format takes

    def conv(self, H, *graph_args):
        H_norm = F.normalize(H, p=2, dim=-1)
        return type(self).op(*graph_args, H_norm, H_norm, H)

    def graph_args(self, params):
        return params

    def forward(self, params, feat, fuse=False):
        from DFGNN.utils import benchmark
        N = len(feat)
        H = self.proj(feat).view(-1, self.num_heads, self.out_size)
        if fuse:
            assert len(params) == self.n_params
            out, elapsed = benchmark(self.conv, H.detach().contiguous(), *self.graph_args(params))
        else:
            H = H.detach().reshape(-1, self.out_size, self.num_heads)
            out, elapsed = benchmark(self.forward_dglsp, params, H)
            out = out.transpose(1, 2)
        return out.reshape(N, -1), elapsed * 1000


class AGNNConv_csr(_AGNNInference):          # params = preprocess_CSR: (indptr, indices, val, smem)
    op, n_params = staticmethod(ops.GTConvFuse_inference_csr), 4


class AGNNConv_tiling(_AGNNInference):
    op, n_params = staticmethod(ops.GTConvFuse_inference_tiling), 4


class AGNNConv_csr_gm(_AGNNInference):       # the _gm operators take no smem_consume
    op, n_params = staticmethod(ops.GTConvFuse_inference_csr_gm), 4

    def graph_args(self, params):
        return params[:3]


class AGNNConv_hyper(_AGNNInference):        # params = preprocess_Hyper: (indptr, indices, rows, val, smem)
    op, n_params = staticmethod(ops.GTConvFuse_inference_hyper), 5


class AGNNConv_softmax(_AGNNInference):
    op, n_params = staticmethod(ops.GTConvFuse_inference_softmax), 5


class AGNNConv_softmax_gm(_AGNNInference):
    op, n_params = staticmethod(ops.GTConvFuse_inference_softmax_gm), 5

    def graph_args(self, params):
        return params[:4]


class AGNNConv_forward(AGNNConvDGL):
    """Training layer on the differentiable hyper operator; params = preprocess_Hyper_fw_bw's 9-tuple; returns the
    output only (reference agnn_layer_forward.py:38-66)."""

    def conv(self, H, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume):
        H_norm = F.normalize(H, p=2, dim=-1)
        return ops.GTConvFuse_hyper(rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, H_norm, H_norm, H)

    def forward(self, params, feat, fuse=False):
        N = len(feat)
        A, graph = params[0], params[1:]
        if fuse:
            out = self.conv(self.proj(feat).view(-1, self.num_heads, self.out_size), *graph)
        else:
            out = self.forward_dglsp(A, self.proj(feat).view(-1, self.out_size, self.num_heads))
        return out.reshape(N, -1)


def index_ops_agnn(row, col, beta, x_row, x_col, cosine=True):
    """softmax_rows(beta[h] cos(x_row_i, x_col_j)) x_col_j with torch index ops over the edges (row[e], col[e]); cosine=False:
    plain dot-product logits.  x_row: [m, heads, d], x_col: [n_cols, heads, d], beta: [heads].  The normalisation
    (F.normalize, eps 1e-12) is outside the edge loop: it keeps two normalised copies of the features and materialises the
    logits [nnz, heads] and the messages [nnz, heads, d], which is what the fused operator avoids."""
    row, col = row.long(), col.long()
    q, k = (F.normalize(x_row, p=2, dim=-1, eps=1e-12), F.normalize(x_col, p=2, dim=-1, eps=1e-12)) if cosine else (x_row, x_col)
    s = (q[row] * k[col]).sum(-1) * beta                                                          # [nnz, heads]
    mx = torch.full((x_row.size(0), s.size(1)), float("-inf"), dtype=s.dtype, device=s.device)
    mx = mx.scatter_reduce(0, row[:, None].expand_as(s), s.detach(), reduce="amax", include_self=True)
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)                                   # empty row
    p = torch.exp(s - mx[row])
    den = torch.zeros_like(mx).index_add_(0, row, p)
    return torch.zeros_like(x_row).index_add_(0, row, x_col[col] * (p / den[row])[:, :, None])    # empty row: 0


class AGNNConv_beta(nn.Module):
    """AGNN as published (Thekumparampil et al.; PyG's / DGL's AGNNConv): softmax_j(beta cos(h_i, h_j)) h_j with a learnable
    temperature beta per head, trainable on ANY graph -- this build's addition; the classes above keep the reference's
    beta = 1 on the GT operators.  Multi-head: proj is Linear(in, heads * out), viewed [N, heads, out].
    forward(params, feat, fuse) -> out[N, heads * out], differentiable in both branches.  params =
    preprocess_Hyper_fw_bw's (A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem); on a rectangular graph
    preprocess_block's, with feat = (feat_cols, feat_rows) -> out[m, heads * out].  The fused branch is AGNNConvFuse
    (csrc/agnn_train.hip): the projected features go in as they are, once -- no normalised copy, one gather per edge."""

    def __init__(self, in_size, out_size, num_heads):
        super().__init__()
        self.in_size, self.out_size, self.num_heads = in_size, out_size, num_heads
        self.proj = nn.Linear(in_size, out_size * num_heads)
        self.beta = nn.Parameter(torch.ones(num_heads))

    def project(self, feat):
        """-> X_row, X_col [N, heads, out]: one tensor, or -- feat = (feat_cols, feat_rows), the two node sets of a
        rectangular graph -- the projections of the second and of the first member."""
        if isinstance(feat, (tuple, list)):
            feat_cols, feat_rows = feat
            return (self.proj(feat_rows).view(-1, self.num_heads, self.out_size),
                    self.proj(feat_cols).view(-1, self.num_heads, self.out_size))
        x = self.proj(feat).view(-1, self.num_heads, self.out_size)
        return x, x

    def conv_nofuse(self, A, x_row, x_col):
        return index_ops_agnn(A.row, A.col, self.beta, x_row, x_col, cosine=True)

    def forward(self, params, feat, fuse=False):
        A, _, row_ptr, col_ind, _, col_ptr, row_ind, _, _ = params
        x_row, x_col = self.project(feat)
        if fuse:
            shared = x_col is x_row
            x_row = x_row.contiguous()
            out = ops.AGNNConvFuse(row_ptr, col_ind, col_ptr, row_ind, self.beta, x_row,
                                   x_row if shared else x_col.contiguous(), cosine=True)
        else:
            out = self.conv_nofuse(A, x_row, x_col)
        return out.reshape(out.size(0), -1)
