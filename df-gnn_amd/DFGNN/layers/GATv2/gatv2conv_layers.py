"""GATv2 layers (Brody et al., "How Attentive are Graph Attention Networks?") on the fused GATv2 operators
(DFGNN/operators/fused_gatconv.py: GATv2ConvFuse_inference / GATv2ConvFuse).  This build's addition: the reference has no
GATv2.  Parameters as dgl.nn.GATv2Conv publishes them -- two projections (`fc_src` / `fc_dst` there; one module when
`share_weights`) and an attention vector per head -- with the logit of edge (i, j)

    s_e = sum_d attn[h, d] LeakyReLU(fc_row(x_i)[h, d] + fc_col(x_j)[h, d])

normalised over row i's out-edges (rows = sources of g.edges(), as every fused operator here; DFGNN/layers/util.py) and
out_i = sum_e softmax(s)_e fc_col(x_j).  The non-fused branch restates that with torch index ops on A.row / A.col, the way
DotGatConv (DFGNN/layers/GAT_DOT) restates its module; it materialises z[nnz, heads, out], which is what the fused
operators avoid.  Both branches lay the projections out as view(-1, heads, out), so they agree for any head count.

GATv2Conv_edge is the layer with edge features, PyG's GATv2Conv(edge_dim=...): E = lin_edge(edge_attr) viewed [nnz, heads,
out] is added inside the LeakyReLU, z_e = fc_row(x_i) + fc_col(x_j) + E_e, and is not part of the message.  Its fused branch
goes through GATv2ConvFuse_edge (csrc/gatv2_edge_train.hip); the edge features are per edge in CSR order, so both branches
take the CSR arrays."""
import torch
from torch import nn
from torch.nn import functional as F

from DFGNN.operators.fused_gatconv import (GATv2ConvFuse, GATv2ConvFuse_edge, GATv2ConvFuse_inference,
                                           GATv2ConvFuse_inference_edge)


class GATv2ConvDGL(nn.Module):
    def __init__(self, in_size, out_size, num_heads, negative_slope=0.2, share_weights=False):
        super().__init__()
        self.in_size, self.out_size, self.num_heads = in_size, out_size, num_heads
        self.negative_slope, self.share_weights = negative_slope, share_weights
        self.fc_row = nn.Linear(in_size, out_size * num_heads)
        self.fc_col = self.fc_row if share_weights else nn.Linear(in_size, out_size * num_heads)
        self.attn = nn.Parameter(torch.zeros(num_heads, out_size))
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_normal_(self.fc_row.weight, gain=gain)
        if not self.share_weights:
            nn.init.xavier_normal_(self.fc_col.weight, gain=gain)
        nn.init.xavier_normal_(self.attn, gain=gain)

    def project(self, feat):
        """-> X_row, X_col [N, heads, out]; the same tensor when the weights are shared.  feat may be a pair (feat_cols,
        feat_rows) -- the two node sets of a rectangular graph: X_col [n_cols, heads, out] is projected from the first member,
        X_row [m, heads, out] from the second."""
        if isinstance(feat, (tuple, list)):
            feat_cols, feat_rows = feat
            return (self.fc_row(feat_rows).view(-1, self.num_heads, self.out_size),
                    self.fc_col(feat_cols).view(-1, self.num_heads, self.out_size))
        x_row = self.fc_row(feat).view(-1, self.num_heads, self.out_size)
        return x_row, (x_row if self.share_weights else self.fc_col(feat).view(-1, self.num_heads, self.out_size))

    def forward_nofuse(self, A, feat):
        return self.conv_nofuse(A, *self.project(feat))

    def conv_nofuse(self, A, x_row, x_col):
        """-> [N, heads, out] with torch index ops over the edges (A.row[e], A.col[e])."""
        row, col = A.row.long(), A.col.long()
        n = x_row.size(0)
        s = (F.leaky_relu(x_row[row] + x_col[col], self.negative_slope) * self.attn).sum(-1)      # [E, heads]
        smax = torch.full((n, self.num_heads), float("-inf"), device=s.device, dtype=s.dtype)
        smax = smax.scatter_reduce(0, row[:, None].expand_as(s), s, reduce="amax", include_self=True)
        p = torch.exp(s - smax[row])
        den = torch.zeros((n, self.num_heads), device=s.device, dtype=s.dtype).index_add_(0, row, p)
        return torch.zeros_like(x_row).index_add_(0, row, x_col[col] * (p / den[row])[:, :, None])   # empty row: 0


class GATv2Conv_tiling(GATv2ConvDGL):
    """Inference: forward(params, feat, fuse) -> (out[N, heads * out], elapsed_ms), timed like the other inference layers
    (3 dry + 10 runs).  fuse: params = preprocess_CSR's (row_ptr, col_ind, val, smem); else params = A."""

    def forward(self, params, feat, fuse=False):
        from DFGNN.utils import benchmark
        N = len(feat)
        with torch.no_grad():   # (both branches time the convolution on the projected features)
            if fuse:
                row_ptr, col_ind, _, _ = params
                x_row, x_col = (x.contiguous() for x in self.project(feat))
                out, elapsed = benchmark(GATv2ConvFuse_inference, self.attn.detach(), row_ptr, col_ind, self.negative_slope,
                                         x_row, x_col)
            else:
                out, elapsed = benchmark(self.conv_nofuse, params, *self.project(feat))
        return out.reshape(N, -1), elapsed * 1000


class GATv2Conv_forward(GATv2ConvDGL):
    """Training: forward(params, feat, fuse) -> out[N, heads * out], differentiable in both branches.
    params = preprocess_Hyper_fw_bw's (A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem); on a rectangular
    graph preprocess_block's, with feat = (feat_cols, feat_rows) -> out[m, heads * out]."""

    def forward(self, params, feat, fuse=False):
        A, _, row_ptr, col_ind, _, col_ptr, row_ind, _, _ = params
        if fuse:
            x_row, x_col = self.project(feat)
            shared = x_col is x_row
            x_row = x_row.contiguous()
            out = GATv2ConvFuse(self.attn, row_ptr, col_ind, col_ptr, row_ind, self.negative_slope, x_row,
                                x_row if shared else x_col.contiguous())
        else:
            out = self.forward_nofuse(A, feat)
        return out.reshape(out.size(0), -1)


def index_ops_gatv2_edge(rows, col_ind, attn, negative_slope, x_row, x_col, e):
    """softmax_rows(sum_d attn[h, d] lrelu(x_row_i + x_col_j + e_e)) x_col_j with torch index ops.  x_row: [m, heads, d],
    x_col: [n_cols, heads, d], e: [nnz, heads, d]; rows / col_ind: the edge list in CSR order.  Materialises z[nnz, heads,
    d] and lrelu(z)."""
    rows, cols = rows.long(), col_ind.long()
    s = (F.leaky_relu(x_row[rows] + x_col[cols] + e, negative_slope) * attn).sum(-1)          # [nnz, heads]
    mx = torch.full((x_row.size(0), s.size(1)), float("-inf"), dtype=s.dtype, device=s.device)
    mx = mx.scatter_reduce(0, rows[:, None].expand_as(s), s.detach(), reduce="amax", include_self=True)
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)                               # empty row
    p = torch.exp(s - mx[rows])
    den = torch.zeros_like(mx).index_add_(0, rows, p)
    return torch.zeros_like(x_row).index_add_(0, rows, x_col[cols] * (p / den[rows])[:, :, None])   # empty row: 0


class GATv2Conv_edge(GATv2ConvDGL):
    """GATv2Conv_forward with edge features: owns lin_edge = Linear(edge_dim, heads * out, bias=False), as PyG's
    GATv2Conv(edge_dim).  forward(params, feat, edge_attr, fuse) -> out[N, heads * out], differentiable in both branches.
    params = preprocess_Hyper_fw_bw's tuple, or preprocess_block's with feat = (feat_cols, feat_rows); edge_attr: [nnz,
    edge_dim] in CSR edge order.  In eval mode the fused branch runs the inference operator."""

    def __init__(self, in_size, out_size, num_heads, negative_slope=0.2, share_weights=False, edge_dim=None):
        super().__init__(in_size, out_size, num_heads, negative_slope, share_weights)
        self.lin_edge = nn.Linear(in_size if edge_dim is None else edge_dim, out_size * num_heads, bias=False)
        nn.init.xavier_normal_(self.lin_edge.weight, gain=nn.init.calculate_gain("relu"))

    def forward(self, params, feat, edge_attr, fuse=False):
        A, rows, row_ptr, col_ind, _, col_ptr, row_ind, val_idx, _ = params
        x_row, x_col = self.project(feat)
        e = self.lin_edge(edge_attr).view(-1, self.num_heads, self.out_size)
        if fuse:
            shared = x_col is x_row
            x_row, e = x_row.contiguous(), e.contiguous()
            x_col = x_row if shared else x_col.contiguous()
            if self.training:
                out = GATv2ConvFuse_edge(self.attn, row_ptr, col_ind, col_ptr, row_ind, val_idx, self.negative_slope, x_row,
                                         x_col, e)
            else:
                out = GATv2ConvFuse_inference_edge(self.attn, row_ptr, col_ind, self.negative_slope, x_row, x_col, e)
        else:
            out = index_ops_gatv2_edge(rows, col_ind, self.attn, self.negative_slope, x_row, x_col, e)
        return out.reshape(out.size(0), -1)


class GATv2Conv_edge_timing(GATv2ConvDGL):
    """GATv2Conv_edge for the timing scripts, which pass no edge features: a seeded random E ~ N(0, 1) [nnz, heads, out],
    drawn once per (edge count, device).  -> (out, milliseconds)."""

    def _random_edge(self, nnz, device):
        key = (nnz, str(device))
        if getattr(self, "_edge_key", None) != key:
            gen = torch.Generator().manual_seed(0)
            self._edge_key = key
            self._edge = torch.randn(nnz, self.num_heads, self.out_size, generator=gen).to(device)
        return self._edge

    def forward(self, params, feat, fuse=False):
        from DFGNN.utils import benchmark
        A, rows, row_ptr, col_ind, _, col_ptr, row_ind, val_idx, _ = params
        e = self._random_edge(col_ind.numel(), feat.device)
        x_row, x_col = self.project(feat)
        if fuse:
            x_row = x_row.contiguous()
            out, elapsed = benchmark(GATv2ConvFuse_edge, self.attn, row_ptr, col_ind, col_ptr, row_ind, val_idx,
                                     self.negative_slope, x_row, x_row if self.share_weights else x_col.contiguous(), e)
        else:
            out, elapsed = benchmark(index_ops_gatv2_edge, rows, col_ind, self.attn, self.negative_slope, x_row,
                                     x_col, e)
        return out.reshape(len(feat), -1), elapsed * 1000
