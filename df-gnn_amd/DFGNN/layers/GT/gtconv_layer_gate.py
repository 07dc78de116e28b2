"""Training layers with a per-edge multiplicative gate on the keys and an edge output: with E = lin_edge(edge_attr) viewed
[nnz, heads, head_dim], w_e = val_e q_i (.) k_j (.) E_e, s_e = sum_d w_e[d], out_i = sum_e softmax_i(s)_e v_j and
e_out = w_e -- the Graph Transformer layer with edge features of Dwivedi & Bresson (benchmarking-gnns
graph_transformer_edge_layer), SAN, the GT variants inside GraphGPS-type stacks.  The edge representation is updated in
every layer: the model trains THROUGH e_out, whose gradient enters the backward next to the gradient of out.  There is no
clamp on the logit.  The fused branch goes through GTConvFuse_gate (DFGNN/operators/fused_gtconv.py: FusedGTFunction_gate;
two floats per (row, head) kept between forward and backward, any graph; W and dE the only things of size nnz h f it
writes), the other one is the same arithmetic in torch index ops.  Both use the [N, heads, head_dim] layout, so they agree
at any head count.
params = (A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume) of preprocess_Hyper_fw_bw(g): the edge
features are per edge in CSR order, so the CSR arrays are needed in both branches."""
import torch
from torch import nn

from DFGNN.operators.fused_gtconv import GTConvFuse_gate, GTConvFuse_inference_gate
from DFGNN.utils import benchmark

from .gtconv_layer import split_pair
from .gtconv_layer_forward import _TrainingQKV


def index_ops_mha_gate(rows, col_ind, val, q, k, v, e):
    """-> (out, w): w_e = val_e q_i (.) k_j (.) e_e [nnz, heads, d] and out = softmax_rows(sum_d w_e) v_j with torch index
    ops.  q, k, v: [N, heads, d]; e: [nnz, heads, d]; rows / col_ind: the edge list in CSR order.  Materialises several
    [nnz, heads, d] tensors."""
    rows, cols = rows.long(), col_ind.long()
    w = q[rows] * (k[cols] * e) * val.to(q.dtype)[:, None, None]                              # [nnz, heads, d]
    s = w.sum(-1)                                                                             # [nnz, heads]
    mx = torch.full((q.size(0), s.size(1)), float("-inf"), dtype=s.dtype, device=s.device)
    mx = mx.scatter_reduce(0, rows[:, None].expand_as(s), s.detach(), reduce="amax", include_self=True)
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)                               # empty row
    p = torch.exp(s - mx[rows])
    den = torch.zeros_like(mx).index_add_(0, rows, p)
    attn = p / den[rows]
    out = v.new_zeros((q.size(0),) + tuple(v.shape[1:])).index_add_(0, rows, v[cols] * attn[:, :, None])  # (k, v may have n_cols rows)
    return out, w


class SparseMHA_gate(_TrainingQKV):
    """SparseMHA with gating edge features and an edge output: owns lin_edge = Linear(edge_dim, out_size, bias=False).
    edge_out=False: the edge output is not computed (the last layer of a stack) and e_out is None."""

    def __init__(self, in_size, out_size, num_heads, edge_dim=None, edge_out=True):
        super().__init__(in_size, out_size, num_heads)
        self.lin_edge = nn.Linear(in_size if edge_dim is None else edge_dim, out_size, bias=False)
        self.edge_out = edge_out

    def forward(self, params, h, edge_attr, fuse=False):
        """edge_attr: [nnz, edge_dim] in CSR edge order.  h: [N, in] or, on a rectangular graph (preprocess_block), the pair
        (h_cols, h_rows).  -> (h_out [len(h_rows), out], e_out [nnz, out] or None)."""
        A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume = params
        h_rows = split_pair(h)[1]
        q, k, v = self._qkv_fused(h)
        e = self.lin_edge(edge_attr).view(-1, self.num_heads, self.head_dim)
        if fuse:
            q, k, v, e = q.contiguous(), k.contiguous(), v.contiguous(), e.contiguous()
            if self.training:
                res = GTConvFuse_gate(rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, q, k, v, e,
                                      edge_out=self.edge_out)
            else:
                res = GTConvFuse_inference_gate(row_ptr, col_ind, val, q, k, v, e, edge_out=self.edge_out)
            out, w = res if self.edge_out else (res, None)
        else:
            out, w = index_ops_mha_gate(rows, col_ind, val, q, k, v, e)
            if not self.edge_out:
                w = None
        return out.reshape(len(h_rows), -1), None if w is None else w.reshape(w.size(0), -1)


class SparseMHA_gate_timing(_TrainingQKV):
    """SparseMHA_gate for the timing scripts, which pass no edge features: a seeded random E ~ N(0, 1) [nnz, heads,
    head_dim], drawn once per (edge count, device).  -> (out, milliseconds); the edge output is computed and dropped."""

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
            (out, _), elapsed = benchmark(GTConvFuse_gate, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx,
                                          smem_consume, q.contiguous(), k.contiguous(), v.contiguous(), e)
        else:
            (out, _), elapsed = benchmark(index_ops_mha_gate, rows, col_ind, val, q, k, v, e)
        return out.reshape(len(h), -1), elapsed * 1000
