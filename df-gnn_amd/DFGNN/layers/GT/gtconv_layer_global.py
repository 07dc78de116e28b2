"""The global half of a GraphGPS-style layer: multi-head attention of every node over all nodes of its own graph in a
batch (DFGNN/operators/fused_gtconv.py: SegmentMHAFuse, csrc/segment_mha.hip).  The nodes are ordered by graph; the only
structure is the graphs' sizes."""
import torch
import torch.nn as nn

import fused_gtconv as fused_gt
from DFGNN.operators.fused_gtconv import (SegmentCrossMHAFuse, SegmentMHABiasFuse, SegmentMHAFuse, SegmentMHAGateFuse,
                                          SegmentMHATBiasFuse)


def segment_offsets(segments, device):
    """seg_ptr int32[n_seg + 1] on `device` from what a caller has: an int32 tensor on the device IS a seg_ptr (passed through
    without a host read, so that the bounds cached on it are found again and the call can be captured); anything else is
    the graphs' sizes (Graph.batch_num_nodes(): int64)."""
    segments = torch.as_tensor(segments)
    if segments.dtype == torch.int32 and segments.device == device:
        return segments
    sizes = segments.to(torch.int64)
    seg_ptr = torch.zeros(sizes.numel() + 1, dtype=torch.int32)
    seg_ptr[1:] = torch.cumsum(sizes.cpu(), 0)
    return seg_ptr.to(device)


class GlobalMHA(nn.Module):
    """out = W_o concat_heads(softmax_graph(scale Q K^T [+ bias]) V), the softmax of a node running over its own graph's
    nodes."""

    def __init__(self, in_size, out_size, num_heads):
        super().__init__()
        self.num_heads = num_heads
        self.head_dim = out_size // num_heads
        self.scaling = self.head_dim ** -0.5
        self.q_proj = nn.Linear(in_size, out_size)
        self.k_proj = nn.Linear(in_size, out_size)
        self.v_proj = nn.Linear(in_size, out_size)
        self.out_proj = nn.Linear(out_size, out_size)

    def forward(self, h, seg_ptr, fuse=True, bias=None, pair_types=None, pair_table=None, gate=None, return_logits=False):
        """h [N, in]; seg_ptr: int32[n_seg + 1] offsets (a tensor kept across layers and steps is looked up, not rebuilt) or
        the batch's graph sizes.  bias: None or fp32 [heads, sum of n_g^2], added to the logits -- per head the graphs'
        packed row-major n_g x n_g blocks one after another (PairBias makes one from pair types).  pair_types [sum of n_g^2]
        (integers, best uint8) with pair_table fp32 [T, heads] instead of bias: the same bias, table.t()[:, pair_types],
        looked up inside the fused kernels for T <= 256 -- no plane is built and the table's gradient is summed there.
        gate: None or fp32 [heads, sum of n_g^2] like bias (which it needs): the attention weights are multiplied by
        sigmoid(gate) after the softmax.  return_logits (with a bias): -> (out, logits [heads, sum of n_g^2]), the logits
        scale Q K^T + bias as an output whose gradient flows back (EGT's pair channel; see EGTAttention).
        fuse=False, or a head shape the fused pair does not serve: plain torch, graph by graph."""
        if (gate is not None or return_logits) and (bias is None or pair_types is not None):
            raise ValueError("gate and return_logits go with a bias plane")
        if (pair_types is None) != (pair_table is None):
            raise ValueError("pair_types and pair_table go together")
        if pair_types is not None and bias is not None:
            raise ValueError("give either bias or pair_types with pair_table, not both")
        seg_ptr = segment_offsets(seg_ptr, h.device)
        n = len(h)
        q, k, v = (p(h).reshape(n, self.num_heads, self.head_dim) for p in (self.q_proj, self.k_proj, self.v_proj))
        if fuse and h.is_cuda and fused_gt.segment_mha_applies(self.num_heads, self.head_dim):
            if gate is not None or return_logits:
                out = SegmentMHAGateFuse(seg_ptr, q.contiguous(), k.contiguous(), v.contiguous(), bias.contiguous(),
                                         None if gate is None else gate.contiguous(), self.scaling, return_logits)
            elif pair_types is not None:
                if pair_table.size(0) <= fused_gt.SEGMENT_TBIAS_MAX_TYPES:
                    pair_types = pair_types.to(torch.uint8)   # (no host read; a no-op for uint8)
                out = SegmentMHATBiasFuse(seg_ptr, q.contiguous(), k.contiguous(), v.contiguous(), pair_types.contiguous(),
                                          pair_table, self.scaling)
            elif bias is None:
                out = SegmentMHAFuse(seg_ptr, q.contiguous(), k.contiguous(), v.contiguous(), self.scaling)
            else:
                out = SegmentMHABiasFuse(seg_ptr, q.contiguous(), k.contiguous(), v.contiguous(), bias.contiguous(), self.scaling)
        else:
            if pair_types is not None:
                bias = pair_table.t()[:, pair_types.long()]
            out = self.forward_plain(seg_ptr, q, k, v, bias, gate, return_logits)
        if return_logits:
            return self.out_proj(out[0].reshape(n, -1)), out[1]
        return self.out_proj(out.reshape(n, -1))

    def forward_plain(self, seg_ptr, q, k, v, bias=None, gate=None, return_logits=False):
        outs, logits = [], []
        ends = seg_ptr.tolist()
        at = 0
        for lo, hi in zip(ends[:-1], ends[1:]):
            s = torch.einsum("ihf,jhf->hij", q[lo:hi], k[lo:hi]) * self.scaling
            n = hi - lo
            if bias is not None:
                s = s + bias[:, at:at + n * n].reshape(bias.size(0), n, n)
            a = torch.softmax(s, dim=-1)
            if gate is not None:
                a = a * torch.sigmoid(gate[:, at:at + n * n].reshape(gate.size(0), n, n))
            at += n * n
            outs.append(torch.einsum("hij,jhf->ihf", a, v[lo:hi]))
            logits.append(s.reshape(s.size(0), n * n))
        out = torch.cat(outs) if outs else torch.empty_like(q)
        if return_logits:
            return out, (torch.cat(logits, dim=1) if logits else q.new_empty(q.size(1), 0))
        return out


class PairBias(nn.Module):
    """A learnable scalar per (pair type, head) as the attention bias of GlobalMHA: Graphormer's spatial encoding with the
    pair type = the (clipped) shortest-path distance.  pair_types int64[n_pairs] lists every graph's n x n type matrix,
    flattened row-major, graph after graph -> bias [heads, n_pairs]; the table's gradient comes by autograd through dbias."""

    def __init__(self, num_types, num_heads):
        super().__init__()
        self.table = nn.Parameter(torch.zeros(num_types, num_heads))
        nn.init.normal_(self.table, std=0.02)

    def forward(self, pair_types):
        return self.table.t()[:, pair_types]


class EGTAttention(nn.Module):
    """The attention of an Edge-augmented Graph Transformer layer (Hussain et al.): a feature per node PAIR gives every head a
    bias on the logit and a sigmoid gate on the attention weight, and the logits update the pair channel:
      x = scale Q K^T + W_b e,   node_out = W_o concat_heads((softmax_graph(x) * sigmoid(W_g e)) V),   pair_out = W_e x
    pair_feat [sum of n_g^2, pair_dim] lists every graph's n x n pairs row-major, graph after graph -> (node_out [N, dim],
    pair_out [sum of n_g^2, pair_dim]).  Fused (GlobalMHA, SegmentMHAGateFuse) nothing of size heads x n^2 is saved for the
    backward besides the three planes themselves."""

    def __init__(self, dim, pair_dim, heads):
        super().__init__()
        self.mha = GlobalMHA(dim, dim, heads)
        self.pair_bias = nn.Linear(pair_dim, heads)
        self.pair_gate = nn.Linear(pair_dim, heads)
        self.pair_out = nn.Linear(heads, pair_dim)

    def forward(self, x, pair_feat, seg_ptr, fuse=True):
        bias, gate = self.pair_bias(pair_feat).t().contiguous(), self.pair_gate(pair_feat).t().contiguous()
        node_out, logits = self.mha(x, seg_ptr, fuse=fuse, bias=bias, gate=gate, return_logits=True)
        return node_out, self.pair_out(logits.t())


class CrossMHA(nn.Module):
    """out = W_o concat_heads(softmax_graph(scale Q K^T) V) with the queries from one node array and the keys / values from
    another, both ordered by graph: the rows hq of graph g attend to the rows hk of graph g (DFGNN/operators/fused_gtconv.py:
    SegmentCrossMHAFuse, csrc/segment_cross.hip).  A query of a graph without keys gets W_o's bias."""

    def __init__(self, q_size, kv_size, out_size, num_heads):
        super().__init__()
        self.num_heads = num_heads
        self.head_dim = out_size // num_heads
        self.scaling = self.head_dim ** -0.5
        self.q_proj = nn.Linear(q_size, out_size)
        self.k_proj = nn.Linear(kv_size, out_size)
        self.v_proj = nn.Linear(kv_size, out_size)
        self.out_proj = nn.Linear(out_size, out_size)

    def forward(self, hq, hk, seg_q, seg_k, fuse=True):
        """hq [N_q, q_size], hk [N_k, kv_size]; seg_q, seg_k: int32 offsets on the device or the graphs' sizes (as
        GlobalMHA's seg_ptr), of the same number of graphs.  fuse=False, CPU tensors or a head shape the fused pair does not
        serve: plain torch, graph by graph."""
        seg_q, seg_k = segment_offsets(seg_q, hq.device), segment_offsets(seg_k, hk.device)
        q = self.q_proj(hq).reshape(len(hq), self.num_heads, self.head_dim)
        k = self.k_proj(hk).reshape(len(hk), self.num_heads, self.head_dim)
        v = self.v_proj(hk).reshape(len(hk), self.num_heads, self.head_dim)
        return self.out_proj(self.attend(seg_q, seg_k, q, k, v, fuse).reshape(len(hq), -1))

    def attend(self, seg_q, seg_k, q, k, v, fuse=True):
        if fuse and q.is_cuda and fused_gt.segment_mha_applies(self.num_heads, self.head_dim):
            return SegmentCrossMHAFuse(seg_q, seg_k, q.contiguous(), k.contiguous(), v.contiguous(), self.scaling)
        outs = []
        eq, ek = seg_q.tolist(), seg_k.tolist()
        for a, b, lo, hi in zip(eq[:-1], eq[1:], ek[:-1], ek[1:]):
            if hi == lo:
                outs.append(torch.zeros_like(q[a:b]))
                continue
            s = torch.einsum("ihf,jhf->hij", q[a:b], k[lo:hi]) * self.scaling
            outs.append(torch.einsum("hij,jhf->ihf", torch.softmax(s, dim=-1), v[lo:hi]))
        return torch.cat(outs) if outs else torch.empty_like(q)


class AttentionReadout(nn.Module):
    """Graph embedding by attention (Set Transformer's PMA, Graph Multiset pooling): num_seeds learnable queries per graph
    attend to that graph's nodes -> [B, num_seeds * out_size]; a graph without nodes gives zeros.  The queries of all graphs
    are the seed matrix repeated, seg_ptr_q = num_seeds * arange(B + 1) built on the device without a host read."""

    def __init__(self, in_size, out_size, num_heads, num_seeds=1):
        super().__init__()
        self.num_seeds = num_seeds
        self.seeds = nn.Parameter(torch.empty(num_seeds, out_size))
        nn.init.xavier_uniform_(self.seeds)
        self.mha = CrossMHA(out_size, in_size, out_size, num_heads)

    def forward(self, h, seg_ptr, fuse=True):
        m = self.mha
        seg_k = segment_offsets(seg_ptr, h.device)
        B = seg_k.numel() - 1
        seg_q = torch.arange(B + 1, dtype=torch.int32, device=h.device) * self.num_seeds
        q = m.q_proj(self.seeds).reshape(self.num_seeds, m.num_heads, m.head_dim).repeat(B, 1, 1)
        k, v = (p(h).reshape(len(h), m.num_heads, m.head_dim) for p in (m.k_proj, m.v_proj))
        out = m.attend(seg_q, seg_k, q, k, v, fuse).reshape(B * self.num_seeds, -1)
        has_nodes = (seg_k[1:] > seg_k[:-1]).repeat_interleave(self.num_seeds).unsqueeze(1)
        return (m.out_proj(out) * has_nodes).reshape(B, -1)
