"""Training layers on the general statistics pair: fused forward + fused backward through GTConvFuse_rowstats, which
keeps two floats per (row, head) between the two instead of attn_edge[h, nnz] and serves any graph (full graphs,
low-degree batches; DFGNN/operators/fused_gtconv.py: FusedGTFunction_rowstats).  Counterparts of SparseMHA_forward /
SparseMHA_forward_timing (gtconv_layer_forward.py): same parameters tuple, same return conventions.
params = (A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume)."""
from DFGNN.operators.fused_gtconv import GTConvFuse_inference_hyper, GTConvFuse_rowstats
from DFGNN.utils import benchmark

from .gtconv_layer import split_pair
from .gtconv_layer_forward import _TrainingQKV


class SparseMHA_rowstats(_TrainingQKV):
    def forward(self, params, h, fuse=False):
        """h: [N, in] or, on a rectangular graph (preprocess_block), the pair (h_cols, h_rows) -> [len(h_rows), out]."""
        A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume = params
        _, h_rows, pair = split_pair(h)
        if fuse:
            q, k, v = self._qkv_fused(h)
            if self.training or pair:   # (the 'hyper' inference operator below is square-only)
                out = GTConvFuse_rowstats(rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume,
                                          q.contiguous(), k.contiguous(), v.contiguous())
            else:
                out = GTConvFuse_inference_hyper(row_ptr, col_ind, rows, val, smem_consume, q.contiguous(),
                                                 k.contiguous(), v.contiguous())
        else:
            out = self.forward_dglsp(A, *self.prep_qkv(h))
        return out.reshape(len(h_rows), -1)


class SparseMHA_rowstats_timing(_TrainingQKV):
    def forward(self, params, h, fuse=False):
        A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem_consume = params
        if fuse:
            q, k, v = self._qkv_fused(h)
            out, elapsed = benchmark(GTConvFuse_rowstats, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx,
                                     smem_consume, q.contiguous(), k.contiguous(), v.contiguous())
            out = out.transpose(1, 2)
        else:
            out, elapsed = benchmark(self.forward_dglsp, A, *self.prep_qkv(h))
        return out.reshape(len(h), -1), elapsed * 1000
