"""Training layers with a per-edge, per-head additive attention bias: s_e = <q_i, k_j> val_e + edge_bias[e, head] before
the softmax -- Graphormer's spatial / edge encodings, GraphGPS / GRIT-style attention, any relative positional or
edge-type bias; -inf in it masks an edge, and a (node, head) whose edges are all masked gets a zero output.  The fused
branch goes through GTConvFuse_bias (DFGNN/operators/fused_gtconv.py: FusedGTFunction_bias; two floats per (row, head)
kept between forward and backward, any graph), the other one is the same arithmetic in torch index ops.  Both use the
[N, heads, head_dim] layout, so they agree at any head count.
params = (A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume) of preprocess_Hyper_fw_bw(g): the bias
is per edge in CSR order, so the CSR arrays are needed in both branches."""
import torch

from DFGNN.operators.fused_gtconv import GTConvFuse_bias, GTConvFuse_inference_bias
from DFGNN.utils import benchmark

from .gtconv_layer import split_pair
from .gtconv_layer_forward import _TrainingQKV


def index_ops_mha_bias(rows, col_ind, val, q, k, v, edge_bias):
    """softmax_rows(val_e <q_i, k_j> + edge_bias[e]) v_j with torch index ops.  q: [N, heads, d]; k, v: [N, heads, d] (on a
    rectangular graph [n_cols, heads, d]); edge_bias: [nnz, heads]; rows / col_ind: the edge list in CSR order.
    Materialises [nnz, heads] logits and probabilities."""
    rows, cols = rows.long(), col_ind.long()
    s = (q[rows] * k[cols]).sum(-1) * val.to(q.dtype)[:, None] + edge_bias                    # [nnz, heads]
    mx = torch.full((q.size(0), s.size(1)), float("-inf"), dtype=s.dtype, device=s.device)
    mx = mx.scatter_reduce(0, rows[:, None].expand_as(s), s.detach(), reduce="amax", include_self=True)
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)                               # no unmasked edge: exp(-inf - 0)
    p = torch.exp(s - mx[rows])
    den = torch.zeros_like(mx).index_add_(0, rows, p)
    attn = p / torch.where(den > 0, den, torch.ones_like(den))[rows]
    return v.new_zeros((q.size(0),) + tuple(v.shape[1:])).index_add_(0, rows, v[cols] * attn[:, :, None])


class SparseMHA_bias(_TrainingQKV):
    def forward(self, params, h, edge_bias, fuse=False):
        """edge_bias: [nnz, heads] in CSR edge order -- what Linear(edge_dim, heads)(edge_attr) yields.  h: [N, in] or, on a
        rectangular graph (preprocess_block), the pair (h_cols, h_rows) -> [len(h_rows), out]."""
        A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume = params
        h_rows = split_pair(h)[1]
        q, k, v = self._qkv_fused(h)
        if fuse:
            bias = edge_bias.t().contiguous()            # [heads, nnz]: a 64-edge tile of one head is one coalesced load
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
            if self.training:
                out = GTConvFuse_bias(rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, q, k, v, bias)
            else:
                out = GTConvFuse_inference_bias(row_ptr, col_ind, val, q, k, v, bias)
        else:
            out = index_ops_mha_bias(rows, col_ind, val, q, k, v, edge_bias)
        return out.reshape(len(h_rows), -1)


class SparseMHA_bias_timing(_TrainingQKV):
    """SparseMHA_bias for the timing scripts, which pass no edge features: a seeded random bias ~ N(0, 1), drawn once per
    (edge count, device).  -> (out, milliseconds)."""

    def _random_bias(self, nnz, device):
        key = (nnz, str(device))
        if getattr(self, "_bias_key", None) != key:
            gen = torch.Generator().manual_seed(0)
            self._bias_key, self._bias = key, torch.randn(nnz, self.num_heads, generator=gen).to(device)
        return self._bias

    def forward(self, params, h, fuse=False):
        A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume = params
        edge_bias = self._random_bias(col_ind.numel(), h.device)
        q, k, v = self._qkv_fused(h)
        if fuse:
            out, elapsed = benchmark(GTConvFuse_bias, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume,
                                     q.contiguous(), k.contiguous(), v.contiguous(), edge_bias.t().contiguous())
        else:
            out, elapsed = benchmark(index_ops_mha_bias, rows, col_ind, val, q, k, v, edge_bias)
        return out.reshape(len(h), -1), elapsed * 1000
