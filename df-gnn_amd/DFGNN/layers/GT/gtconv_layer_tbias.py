"""Training layers with a TYPED attention bias: the scalar added to an edge's logit is an entry of a small trainable table,
chosen by the edge's type and the head -- s_e = <q_i, k_j> val_e + rel_bias[t_e, head] before the softmax.  Graphormer's
spatial encoding (nn.Embedding(num_spatial, num_heads) indexed by the shortest-path bucket), T5 / Swin-style
relative-position bias, any bucketed-distance or edge-type bias; -inf in the table masks a type for a head.  The fused
branch goes through GTConvFuse_tbias (DFGNN/operators/fused_gtconv.py: FusedGTFunction_tbias; two floats per (row, head)
kept between forward and backward, any graph, 4 bytes of type per edge and nothing of size heads nnz), the other one is
SparseMHA_bias's index ops on the gathered rel_bias[etype].  Both use the [N, heads, head_dim] layout, so they agree at any
head count.
params = (A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume) of preprocess_Hyper_fw_bw(g) or
preprocess_block(block); types = (etype, etype_csc) of preprocess_types(params, etype, num_types)."""
import torch
from torch import nn

from DFGNN.operators.fused_gtconv import GTConvFuse_inference_tbias, GTConvFuse_tbias
from DFGNN.utils import benchmark

from .gtconv_layer import split_pair
from .gtconv_layer_bias import index_ops_mha_bias
from .gtconv_layer_forward import _TrainingQKV
from .gtconv_layer_typed import preprocess_types


class SparseMHA_tbias(_TrainingQKV):
    """SparseMHA with a typed attention bias: owns rel_bias = Parameter[num_types, num_heads], an embedding weight."""

    def __init__(self, in_size, out_size, num_heads, num_types):
        super().__init__(in_size, out_size, num_heads)
        self.num_types = num_types
        self.rel_bias = nn.Parameter(torch.randn(num_types, num_heads) * 0.5)

    def forward(self, params, h, types, fuse=False):
        """types: (etype, etype_csc) of preprocess_types.  h: [N, in] or, on a rectangular graph (preprocess_block), the
        pair (h_cols, h_rows) -> [len(h_rows), out]."""
        A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume = params
        etype, etype_csc = types
        h_rows = split_pair(h)[1]
        q, k, v = self._qkv_fused(h)
        if fuse:
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
            if self.training:
                out = GTConvFuse_tbias(rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, q, k, v,
                                       self.rel_bias, etype, etype_csc)
            else:
                out = GTConvFuse_inference_tbias(row_ptr, col_ind, val, q, k, v, self.rel_bias, etype)
        else:
            out = index_ops_mha_bias(rows, col_ind, val, q, k, v, self.rel_bias[etype.long()])
        return out.reshape(len(h_rows), -1)


class SparseMHA_tbias_timing(SparseMHA_tbias):
    """SparseMHA_tbias for the timing scripts, which pass no edge types: seeded random types in [0, 16), drawn once per
    (edge count, device).  -> (out, milliseconds)."""

    def __init__(self, in_size, out_size, num_heads, num_types=16):
        super().__init__(in_size, out_size, num_heads, num_types)

    def _random_types(self, params, device):
        key = (params[3].numel(), str(device), params[7].data_ptr())
        if getattr(self, "_types_key", None) != key:
            gen = torch.Generator().manual_seed(0)
            etype = torch.randint(0, self.num_types, (params[3].numel(),), generator=gen, dtype=torch.int32).to(device)
            self._types_key, self._types = key, preprocess_types(params, etype, self.num_types)
        return self._types

    def forward(self, params, h, fuse=False):
        A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume = params
        etype, etype_csc = self._random_types(params, h.device)
        q, k, v = self._qkv_fused(h)
        if fuse:
            out, elapsed = benchmark(GTConvFuse_tbias, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume,
                                     q.contiguous(), k.contiguous(), v.contiguous(), self.rel_bias, etype, etype_csc)
        else:
            out, elapsed = benchmark(index_ops_mha_bias, rows, col_ind, val, q, k, v, self.rel_bias[etype.long()])
        return out.reshape(len(h), -1), elapsed * 1000
