"""GAT training layers on the any-graph fused pair (DFGNN/operators/fused_gatconv.py: GATConvFuse_edge /
GATConvFuse_inference_edge, csrc/gat_edge_train.hip).  This build's addition: the reference's GAT layers are inference only
and its training operator is square.  Parameters are GATConvDGL's -- W, a_l (row / destination side), a_r (column / source
side) --; the projected features are laid out as view(-1, heads, out) in both branches, so the two agree for any head count.
The logit of edge (row i, column j) is

    s_e = LeakyReLU(<a_l, W x_i> + <a_r, W x_j> [+ score_e])

normalised over row i's edges, and out_i = sum_e dropout(softmax(s))_e W x_j.  On a rectangular graph (preprocess_block) feat
is the pair (feat_cols, feat_rows); only the scalar <a_l, W x_i> is taken from the row side.

GATConv_edge is the layer with edge features, PyG's GATConv(edge_dim=...): score_e[h] = <lin_edge(edge_attr)_e[h], att_edge[h]>.
It is computed as edge_attr @ fold with fold[edge_dim, h] = sum_c W_edge[h C + c, :] att_edge[h, c], so neither branch builds
[nnz, heads, out]; autograd through the small matmul gives the gradients of lin_edge and att_edge."""
import torch
from torch import nn
from torch.nn import functional as F

from DFGNN.operators.fused_gatconv import GATConvFuse_edge, GATConvFuse_inference_edge

from .gatconv_layer import GATConvDGL


def index_ops_gat_edge(rows, col_ind, attn_row, attn_col, negative_slope, x_col, score=None, attn_drop=0.0, training=False):
    """dropout(softmax_rows(lrelu(attn_row_i + attn_col_j + score_e))) x_col_j with torch index ops.  attn_row: [m, heads],
    attn_col: [n_cols, heads], x_col: [n_cols, heads, d], score: [nnz, heads] or None; rows / col_ind: the edge list (in CSR
    order when there is a score).  Materialises x_col[col_ind], [nnz, heads, d]."""
    rows, cols = rows.long(), col_ind.long()
    pre = attn_row[rows] + attn_col[cols]
    if score is not None:
        pre = pre + score
    s = F.leaky_relu(pre, negative_slope)                                                     # [nnz, heads]
    mx = torch.full((attn_row.size(0), s.size(1)), float("-inf"), dtype=s.dtype, device=s.device)
    mx = mx.scatter_reduce(0, rows[:, None].expand_as(s), s.detach(), reduce="amax", include_self=True)
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)                               # empty row
    p = torch.exp(s - mx[rows])
    den = torch.zeros_like(mx).index_add_(0, rows, p)
    p = F.dropout(p / den[rows], attn_drop, training)
    out = torch.zeros((attn_row.size(0),) + tuple(x_col.shape[1:]), dtype=x_col.dtype, device=x_col.device)
    return out.index_add_(0, rows, x_col[cols] * p[:, :, None])                               # empty row: 0


class GATConv_forward(GATConvDGL):
    """Training: forward(params, feat, fuse) -> out[m, heads * out], differentiable in both branches.  params =
    preprocess_Hyper_fw_bw's (A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem); on a rectangular graph
    preprocess_block's, with feat = (feat_cols, feat_rows).  `dropout` is the attention dropout.  In eval mode the fused
    branch runs the inference operator."""

    def __init__(self, in_size, out_size, num_heads, dropout=0.0, negative_slope=0.2):
        super().__init__(in_size, out_size, num_heads, dropout, negative_slope)
        self.attn_drop = float(dropout)

    def project(self, feat):
        """-> attn_row [m, heads], attn_col [n_cols, heads], x_col [n_cols, heads, out]"""
        a_l, a_r = self.a_l.transpose(1, 2), self.a_r.transpose(1, 2)    # [1, heads, out]
        if isinstance(feat, (tuple, list)):
            feat_cols, feat_rows = feat
            x_col = self.W(feat_cols).view(-1, self.num_heads, self.out_size)
            x_row = self.W(feat_rows).view(-1, self.num_heads, self.out_size)
        else:
            x_col = x_row = self.W(feat).view(-1, self.num_heads, self.out_size)
        return (a_l * x_row).sum(-1), (a_r * x_col).sum(-1), x_col

    def conv(self, params, feat, score, fuse):
        """score: [nnz, heads] in CSR edge order, or None"""
        A, rows, row_ptr, col_ind, _, col_ptr, row_ind, val_idx, _ = params
        attn_row, attn_col, x_col = self.project(feat)
        if fuse:
            attn_row, attn_col, x_col = attn_row.contiguous(), attn_col.contiguous(), x_col.contiguous()
            score = None if score is None else score.t().contiguous()    # [heads, nnz]: a head's stream is contiguous
            if self.training:
                out = GATConvFuse_edge(attn_row, attn_col, row_ptr, col_ind, col_ptr, row_ind, val_idx, self.negative_slope,
                                       x_col, self.attn_drop, score)
            else:
                out = GATConvFuse_inference_edge(attn_row, attn_col, row_ptr, col_ind, self.negative_slope, x_col, score)
        else:
            # (a tuple of preprocess_*(fused=False) holds A alone: its COO order, which only a score-free call may use)
            r, c = (A.row, A.col) if rows is None else (rows, col_ind)
            out = index_ops_gat_edge(r, c, attn_row, attn_col, self.negative_slope, x_col, score, self.attn_drop, self.training)
        return out.reshape(out.size(0), -1)

    def forward(self, params, feat, fuse=False):
        return self.conv(params, feat, None, fuse)


class GATConv_edge(GATConv_forward):
    """GATConv_forward with edge features: owns lin_edge = Linear(edge_dim, heads * out, bias=False) and att_edge [heads,
    out], as PyG's GATConv(edge_dim).  forward(params, feat, edge_attr, fuse) -> out[m, heads * out]; edge_attr: [nnz,
    edge_dim] in CSR edge order (both branches take the CSR arrays)."""

    def __init__(self, in_size, out_size, num_heads, dropout=0.0, negative_slope=0.2, edge_dim=None):
        super().__init__(in_size, out_size, num_heads, dropout, negative_slope)
        self.lin_edge = nn.Linear(in_size if edge_dim is None else edge_dim, out_size * num_heads, bias=False)
        self.att_edge = nn.Parameter(torch.zeros(num_heads, out_size))
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_normal_(self.lin_edge.weight, gain=gain)
        nn.init.xavier_normal_(self.att_edge, gain=gain)

    def edge_score(self, edge_attr):
        """-> [nnz, heads]: <lin_edge(edge_attr)_e[h], att_edge[h]> without lin_edge(edge_attr) itself"""
        w = self.lin_edge.weight.view(self.num_heads, self.out_size, -1)          # [heads, out, edge_dim]
        fold = (w * self.att_edge[:, :, None]).sum(1).t()                         # [edge_dim, heads]
        return edge_attr @ fold

    def forward(self, params, feat, edge_attr, fuse=False):
        return self.conv(params, feat, self.edge_score(edge_attr), fuse)


class GATConv_edge_timing(GATConv_forward):
    """GATConv_edge for the timing scripts, which pass no edge features: a seeded random score ~ N(0, 1) [nnz, heads], drawn
    once per (edge count, device).  -> (out, milliseconds)."""

    def _random_score(self, nnz, device):
        key = (nnz, str(device))
        if getattr(self, "_score_key", None) != key:
            gen = torch.Generator().manual_seed(0)
            self._score_key = key
            self._score = torch.randn(nnz, self.num_heads, generator=gen).to(device)
        return self._score

    def forward(self, params, feat, fuse=False):
        from DFGNN.utils import benchmark
        score = self._random_score(params[0].nnz, feat.device)
        out, elapsed = benchmark(self.conv, params, feat, score, fuse)
        return out, elapsed * 1000
