"""Training layers with a per-edge feature vector added to keys and messages: k~_e = k_j + E_e, v~_e = v_j + E_e with
E = lin_edge(edge_attr) viewed [nnz, heads, head_dim], s_e = <q_i, k~_e> val_e, out_i = sum_e softmax_i(s)_e v~_e -- PyG's
TransformerConv(edge_dim=...), Shaw-style relative position vectors, the edge channel of GPS / GRIT-type models.  The
fused branch goes through GTConvFuse_edge (DFGNN/operators/fused_gtconv.py: FusedGTFunction_edge; two floats per (row,
head) kept between forward and backward, any graph, dE the only thing of size nnz h f it writes), the other one is the
same arithmetic in torch index ops.  Both use the [N, heads, head_dim] layout, so they agree at any head count.
params = (A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume) of preprocess_Hyper_fw_bw(g): the edge
features are per edge in CSR order, so the CSR arrays are needed in both branches."""
import torch
from torch import nn

from DFGNN.operators.fused_gtconv import GTConvFuse_edge, GTConvFuse_inference_edge
from DFGNN.utils import benchmark

from .gtconv_layer import split_pair
from .gtconv_layer_forward import _TrainingQKV


def index_ops_mha_edge(rows, col_ind, val, q, k, v, e):
    """softmax_rows(val_e <q_i, k_j + e_e>) (v_j + e_e) with torch index ops.  q, k, v: [N, heads, d]; e: [nnz, heads, d];
    rows / col_ind: the edge list in CSR order.  Materialises several [nnz, heads, d] tensors."""
    rows, cols = rows.long(), col_ind.long()
    ke, ve = k[cols] + e, v[cols] + e                                                         # [nnz, heads, d]
    s = (q[rows] * ke).sum(-1) * val.to(q.dtype)[:, None]                                     # [nnz, heads]
    mx = torch.full((q.size(0), s.size(1)), float("-inf"), dtype=s.dtype, device=s.device)
    mx = mx.scatter_reduce(0, rows[:, None].expand_as(s), s.detach(), reduce="amax", include_self=True)
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)                               # empty row
    p = torch.exp(s - mx[rows])
    den = torch.zeros_like(mx).index_add_(0, rows, p)
    attn = p / den[rows]
    return v.new_zeros((q.size(0),) + tuple(v.shape[1:])).index_add_(0, rows, ve * attn[:, :, None])   # (k, v may have n_cols rows)


class SparseMHA_edge(_TrainingQKV):
    """SparseMHA with edge features: owns lin_edge = Linear(edge_dim, out_size, bias=False), one projection for key and
    value as in TransformerConv."""

    def __init__(self, in_size, out_size, num_heads, edge_dim=None):
        super().__init__(in_size, out_size, num_heads)
        self.lin_edge = nn.Linear(in_size if edge_dim is None else edge_dim, out_size, bias=False)

    def forward(self, params, h, edge_attr, fuse=False):
        """edge_attr: [nnz, edge_dim] in CSR edge order.  h: [N, in] or, on a rectangular graph (preprocess_block), the pair
        (h_cols, h_rows) -> [len(h_rows), out]."""
        A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume = params
        h_rows = split_pair(h)[1]
        q, k, v = self._qkv_fused(h)
        e = self.lin_edge(edge_attr).view(-1, self.num_heads, self.head_dim)
        if fuse:
            q, k, v, e = q.contiguous(), k.contiguous(), v.contiguous(), e.contiguous()
            if self.training:
                out = GTConvFuse_edge(rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, q, k, v, e)
            else:
                out = GTConvFuse_inference_edge(row_ptr, col_ind, val, q, k, v, e)
        else:
            out = index_ops_mha_edge(rows, col_ind, val, q, k, v, e)
        return out.reshape(len(h_rows), -1)


class SparseMHA_edge_timing(_TrainingQKV):
    """SparseMHA_edge for the timing scripts, which pass no edge features: a seeded random E ~ N(0, 1) [nnz, heads,
    head_dim], drawn once per (edge count, device).  -> (out, milliseconds)."""

    def _random_edge(self, nnz, device):
        key = (nnz, str(device))
        if getattr(self, "_edge_key", None) != key:
            gen = torch.Generator().manual_seed(0)
            self._edge_key = key
            self._edge = torch.randn(nnz, self.num_heads, self.head_dim, generator=gen).to(device)
        return self._edge

    def forward(self, params, h, fuse=False):
        A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume = params
        e = self._random_edge(col_ind.numel(), h.device)
        q, k, v = self._qkv_fused(h)
        if fuse:
            out, elapsed = benchmark(GTConvFuse_edge, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume,
                                     q.contiguous(), k.contiguous(), v.contiguous(), e)
        else:
            out, elapsed = benchmark(index_ops_mha_edge, rows, col_ind, val, q, k, v, e)
        return out.reshape(len(h), -1), elapsed * 1000
