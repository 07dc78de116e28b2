"""Training layers with TYPED edges: the vector added to keys and messages is a row of a small trainable table, chosen by
the edge's type -- k~_e = k_j + rel[t_e], v~_e = v_j + rel[t_e] with rel viewed [num_types, heads, head_dim], s_e = <q_i,
k~_e> val_e, out_i = sum_e softmax_i(s)_e v~_e.  Shaw-style relative positions, RGAT / HGT-style relation vectors,
bucketed distances, bond types.  The fused branch goes through GTConvFuse_typed (DFGNN/operators/fused_gtconv.py:
FusedGTFunction_typed; two floats per (row, head) kept between forward and backward, any graph, 4 bytes of type per edge and
nothing of size nnz h f), the other one is SparseMHA_edge's index ops on the materialised rel[etype].  Both use the [N,
heads, head_dim] layout, so they agree at any head count.
params = (A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume) of preprocess_Hyper_fw_bw(g) or
preprocess_block(block); types = (etype, etype_csc) of preprocess_types(params, etype, num_types)."""
import torch
from torch import nn

from DFGNN.operators.fused_gtconv import GTConvFuse_inference_typed, GTConvFuse_typed
from DFGNN.utils import benchmark

from .gtconv_layer import split_pair
from .gtconv_layer_edge import index_ops_mha_edge
from .gtconv_layer_forward import _TrainingQKV


def preprocess_types(params, etype, num_types):
    """-> (etype int32 in CSR edge order, etype_csc = etype[val_idx]: the same types in CSC entry order), what the typed
    layers and GTConvFuse_typed take.  etype: one integer type per edge in CSR edge order, on the device of params.  Runs
    once per graph and is the one place that validates 0 <= etype < num_types (one host synchronisation; the kernels index
    the table unchecked): ValueError otherwise.  params may be rectangular (preprocess_block)."""
    col_ind, val_idx = params[3], params[7]
    if etype.dim() != 1 or etype.numel() != col_ind.numel():
        raise ValueError(f"etype must have shape ({col_ind.numel()},): one type per edge in CSR order, got {tuple(etype.shape)}")
    if etype.is_floating_point() or etype.dtype == torch.bool:
        raise ValueError(f"etype must be an integer tensor, got {etype.dtype}")
    if num_types < 1:
        raise ValueError(f"num_types must be at least 1, got {num_types}")
    if etype.numel():
        lo, hi = torch.aminmax(etype)
        lo, hi = int(lo), int(hi)
        if lo < 0 or hi >= num_types:
            raise ValueError(f"edge types must lie in [0, {num_types}), got values from {lo} to {hi}")
    etype = etype.to(torch.int32).contiguous()
    return etype, etype[val_idx.long()].contiguous()


class SparseMHA_typed(_TrainingQKV):
    """SparseMHA with typed edges: owns rel = Parameter[num_types, out_size], one table for key and value."""

    def __init__(self, in_size, out_size, num_heads, num_types):
        super().__init__(in_size, out_size, num_heads)
        self.num_types = num_types
        self.rel = nn.Parameter(torch.randn(num_types, out_size) * out_size ** -0.5)

    def forward(self, params, h, types, fuse=False):
        """types: (etype, etype_csc) of preprocess_types.  h: [N, in] or, on a rectangular graph (preprocess_block), the
        pair (h_cols, h_rows) -> [len(h_rows), out]."""
        A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume = params
        etype, etype_csc = types
        h_rows = split_pair(h)[1]
        q, k, v = self._qkv_fused(h)
        rel = self.rel.view(self.num_types, self.num_heads, self.head_dim)
        if fuse:
            q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
            if self.training:
                out = GTConvFuse_typed(rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume, q, k, v, rel,
                                       etype, etype_csc)
            else:
                out = GTConvFuse_inference_typed(row_ptr, col_ind, val, q, k, v, rel, etype)
        else:
            out = index_ops_mha_edge(rows, col_ind, val, q, k, v, rel[etype.long()])
        return out.reshape(len(h_rows), -1)


class SparseMHA_typed_timing(SparseMHA_typed):
    """SparseMHA_typed for the timing scripts, which pass no edge types: seeded random types in [0, 16), drawn once per
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
        rel = self.rel.view(self.num_types, self.num_heads, self.head_dim)
        if fuse:
            out, elapsed = benchmark(GTConvFuse_typed, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume,
                                     q.contiguous(), k.contiguous(), v.contiguous(), rel, etype, etype_csc)
        else:
            out, elapsed = benchmark(index_ops_mha_edge, rows, col_ind, val, q, k, v, rel[etype.long()])
        return out.reshape(len(h), -1), elapsed * 1000
