"""Residual gated graph convolution, GatedGCN (Bresson & Laurent, "Residual Gated Graph ConvNets"; the layer of Dwivedi et
al.'s "Benchmarking GNNs", the default local layer of GraphGPS, PyG's ResGatedGraphConv) on the fused GatedGCN operators
(DFGNN/operators/fused_gtconv.py: GatedGCNConvFuse / GatedGCNConvFuse_inference, csrc/gatedgcn_train.hip).  This build's
addition: the reference has no GatedGCN.  The layer owns the five linear maps of the published layer -- A (self term), B
(message), D (row gate), E (column gate), C (edge gate) -- and computes, for edge e = (i, j) in CSR order,

    z_e   = D h_i + E h_j + C edge_attr_e
    sg_e  = sigmoid(z_e)                                     per dimension
    agg_i = sum_e sg_e (.) B h_j / (sum_e sg_e + eps)        normalize=True (Dwivedi / GraphGPS); else the plain sum (PyG)
    h_out = A h_i + agg_i          e_out = z_e               the next layer's edge features

Batch norm, ReLU and the residuals stay with the caller.  Heads are channel groups only: the arithmetic is per dimension, so
any head count gives the same numbers; [N, heads, out / heads] is the layout the kernels take.  The non-fused branch restates
the layer with torch index ops; it materialises x_row[rows], x_col[cols], z, sg and sg (.) v[cols], each [nnz, heads, d], which
is what the fused operators avoid."""
import torch
from torch import nn

from DFGNN.operators.fused_gtconv import GatedGCNConvFuse, GatedGCNConvFuse_inference
from DFGNN.utils import benchmark

from ..GT.gtconv_layer import split_pair


def index_ops_gatedgcn(rows, col_ind, x_row, x_col, v, e, normalize=True, eps=1e-6):
    """-> (out, z): z_e = x_row_i + x_col_j + e_e [nnz, heads, d] and out_i = sum_e sigmoid(z_e) (.) v_j [/ (sum_e sigmoid(z_e)
    + eps)] with torch index ops.  x_row: [m, heads, d]; x_col, v: [n_cols, heads, d]; e: [nnz, heads, d] or None; rows /
    col_ind: the edge list in CSR order."""
    rows, cols = rows.long(), col_ind.long()
    z = x_row[rows] + x_col[cols]
    if e is not None:
        z = z + e
    sg = torch.sigmoid(z)
    out = torch.zeros_like(x_row).index_add_(0, rows, sg * v[cols])
    if normalize:
        out = out / (torch.zeros_like(x_row).index_add_(0, rows, sg) + eps)
    return out, z


class GatedGCNConv(nn.Module):
    """forward(params, h, edge_attr=None, fuse=False) -> (h_out [m, out], e_out [nnz, out] or None), differentiable in both
    branches.  params = preprocess_Hyper_fw_bw's (A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem); on a
    rectangular graph preprocess_block's, with h = (h_cols, h_rows).  edge_attr: [nnz, edge_dim] in CSR edge order, or None:
    no edge term.  edge_out=False: the edge output is not computed (the last layer of a stack) and e_out is None.  In eval
    mode the fused branch runs the inference operator."""

    def __init__(self, in_size, out_size, num_heads=1, edge_dim=None, normalize=True, edge_out=True, eps=1e-6):
        super().__init__()
        if out_size % num_heads:
            raise ValueError(f"out_size {out_size} is not a multiple of num_heads {num_heads}")
        self.in_size, self.out_size, self.num_heads, self.head_dim = in_size, out_size, num_heads, out_size // num_heads
        self.normalize, self.edge_out, self.eps = normalize, edge_out, eps
        self.lin_self = nn.Linear(in_size, out_size)                     # A
        self.lin_msg = nn.Linear(in_size, out_size)                      # B
        self.lin_row = nn.Linear(in_size, out_size)                      # D
        self.lin_col = nn.Linear(in_size, out_size)                      # E
        self.lin_edge = nn.Linear(in_size if edge_dim is None else edge_dim, out_size, bias=False)   # C

    def project(self, h):
        """-> (self term [m, out], x_row [m, heads, d], x_col, v [n_cols, heads, d])"""
        h_cols, h_rows, _ = split_pair(h)
        shape = (-1, self.num_heads, self.head_dim)
        return (self.lin_self(h_rows), self.lin_row(h_rows).view(shape), self.lin_col(h_cols).view(shape),
                self.lin_msg(h_cols).view(shape))

    def forward(self, params, h, edge_attr=None, fuse=False):
        A, rows, row_ptr, col_ind, _, col_ptr, row_ind, val_idx, _ = params
        own, x_row, x_col, v = self.project(h)
        e = None if edge_attr is None else self.lin_edge(edge_attr).view(-1, self.num_heads, self.head_dim)
        if fuse:
            x_row, x_col, v = x_row.contiguous(), x_col.contiguous(), v.contiguous()
            e = None if e is None else e.contiguous()
            if self.training:
                res = GatedGCNConvFuse(row_ptr, col_ind, col_ptr, row_ind, val_idx, x_row, x_col, v, e, self.normalize,
                                       self.eps, edge_out=self.edge_out)
            else:
                res = GatedGCNConvFuse_inference(row_ptr, col_ind, x_row, x_col, v, e, self.normalize, self.eps,
                                                 edge_out=self.edge_out)
            agg, z = res if self.edge_out else (res, None)
        else:
            agg, z = index_ops_gatedgcn(rows, col_ind, x_row, x_col, v, e, self.normalize, self.eps)
            if not self.edge_out:
                z = None
        return own + agg.reshape(own.size(0), -1), None if z is None else z.reshape(z.size(0), -1)


class _GatedGCNTiming(GatedGCNConv):
    """The conv alone on the projected features, timed like the other training layers (3 dry + 10 runs) -> (out [N, out],
    milliseconds); the edge output, where there is one, is computed and dropped."""
    with_edge = True

    def _random_edge(self, nnz, device):
        key = (nnz, str(device))
        if getattr(self, "_edge_key", None) != key:
            gen = torch.Generator().manual_seed(0)
            self._edge_key = key
            self._edge = torch.randn(nnz, self.num_heads, self.head_dim, generator=gen).to(device)
        return self._edge

    def forward(self, params, h, fuse=False):
        A, rows, row_ptr, col_ind, _, col_ptr, row_ind, val_idx, _ = params
        _, x_row, x_col, v = self.project(h)
        e = self._random_edge(col_ind.numel(), x_row.device) if self.with_edge else None
        if fuse:
            res, elapsed = benchmark(GatedGCNConvFuse, row_ptr, col_ind, col_ptr, row_ind, val_idx, x_row.contiguous(),
                                     x_col.contiguous(), v.contiguous(), e, self.with_edge, self.eps, self.with_edge)
            out = res[0] if self.with_edge else res
        else:
            (out, _), elapsed = benchmark(index_ops_gatedgcn, rows, col_ind, x_row, x_col, v, e, self.with_edge, self.eps)
        return out.reshape(out.size(0), -1), elapsed * 1000


class GatedGCNConv_timing(_GatedGCNTiming):
    """--conv gatedgcn --format forward: the Dwivedi / GraphGPS form -- a seeded random E ~ N(0, 1) [nnz, heads, d], drawn
    once per (edge count, device), normalised, with the edge output."""
    with_edge = True


class GatedGCNConv_plain_timing(_GatedGCNTiming):
    """--conv gatedgcn --format forward_plain: PyG's ResGatedGraphConv -- no edge term, no normalisation, no edge output."""
    with_edge = False
