#!/usr/bin/env python3
"""Neighbour-sampled mini-batch training on the reddit-like stand-in: a 2-layer GT (--conv gatv2: GATv2, --conv gat: GAT on the any-graph pair) whose layers run
on RECTANGULAR blocks (DFGNN.utils.graph.sample_block -> DFGNN.layers.preprocess_block -> the fused pairs that take an
m x n_cols graph; --sampler native: DFGNN.utils.graph.sample_block_fused, the native sampler of include/dfgnn_sample.h, whose
blocks carry their CSR and CSC arrays, so that preprocess_block only hands them on).  Each step: seeds, two sampled blocks, their preprocessing, forward, backward, Adam.  The same blocks
go through the index-op branch of the layers every step (same weights, no gradient, outside the timed step); the last
step's two losses and the largest gap between the two over all steps are printed.

Reported as separate JSON lines (medians over --repeats groups of --iters):
  sampling        ms per step for the two sample_block (--sampler native: sample_block_fused) calls
  preprocessing   ms per step for the two preprocess_block calls
  step            ms per training step, fused, everything included
  conv_pairs      ms for forward + backward of the convolution operators alone on the two blocks of one step, three ways:
                  rect (this build's entries), padded_square (rows padded to n_cols, the square entry: the workaround
                  without rectangular support) and index_ops (torch index ops over the edge list)
usage: python3 tools/train_sampled.py --scale 0.1 --fanout 10,25 --batch 1024 --heads 1 --dim 128 [--conv gatv2|gat]
       [--sampler torch|native]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "df-gnn_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from torch import nn  # noqa: E402

import dfgnn_preprocess  # noqa: E402
import fused_gatconv  # noqa: E402
import fused_gtconv  # noqa: E402
from DFGNN.layers import GATConv_forward, GATv2Conv_forward, SparseMHA_rowstats, index_ops_gat_edge, preprocess_block  # noqa: E402
from DFGNN.layers.GT.gtconv_layer_bias import index_ops_mha_bias  # noqa: E402
from DFGNN.utils import load_data_full_graph, sample_block, sample_block_fused  # noqa: E402

SLOPE = 0.2


class _GTLayer(nn.Module):
    """Holds a SparseMHA_rowstats.  fuse=True is its fused branch; the index-op branch is routed here explicitly through
    index_ops_mha_bias with a zero bias on the same projections: it keeps the [N, heads, head_dim] layout of the fused
    branch at any head count (SparseMHA_rowstats' own baseline lays the heads out differently and agrees at one head)."""

    def __init__(self, in_size, out_size, num_heads):
        super().__init__()
        self.mha = SparseMHA_rowstats(in_size, out_size, num_heads)

    def forward(self, params, h, fuse=False):
        if fuse:
            return self.mha(params, h, fuse=True)
        _, rows, _, col_ind, val = params[:5]
        q, k, v = self.mha._qkv_fused(h)
        zero = torch.zeros(col_ind.numel(), self.mha.num_heads, device=col_ind.device)
        return index_ops_mha_bias(rows, col_ind, val, q, k, v, zero).reshape(q.size(0), -1)


class Net(nn.Module):
    def __init__(self, conv, in_dim, dim, heads, classes):
        super().__init__()
        self.inproj = nn.Linear(in_dim, dim)
        make = {"gatv2": lambda: GATv2Conv_forward(dim, dim // heads, heads), "gat": lambda: GATConv_forward(dim, dim // heads, heads),
                "gt": lambda: _GTLayer(dim, dim, heads)}[conv]
        self.layers = nn.ModuleList(make() for _ in range(2))
        self.out = nn.Linear(dim, classes)

    def forward(self, blocks, x, fuse):
        h = self.inproj(x)
        for layer, (params, m) in zip(self.layers, blocks):
            h = layer(params, (h, h[:m]), fuse=fuse)       # the rows of a block are its first columns
        return self.out(h)


def sample(row_ptr, col_ind, seeds, fanouts, gen, hop=sample_block):
    """-> [(block, rows)] outermost first, and the input nodes of the outermost block."""
    blocks, nodes = [], seeds
    for fanout in reversed(fanouts):
        block, cols = hop(row_ptr, col_ind, nodes, fanout, gen)
        blocks.insert(0, (block, nodes.numel()))
        nodes = cols
    return blocks, nodes


def timed(fn, iters, repeats):
    """Median over `repeats` of the mean ms of `iters` calls (device time by events), and the spread (max - min) / median."""
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b) / iters)
    med = statistics.median(ms)
    return round(med, 4), round((max(ms) - min(ms)) / med, 3)


def block_jobs(conv, params, m, heads, f, gen):
    """The three forward + backward callables of ONE block: rect, padded_square, index_ops.  A function of its own so that
    each block's closures hold that block's arrays (closures made in a loop over the blocks would all see the last block's,
    and a row_ptr of one block with the col_ind of another sends a kernel out of bounds); the assert below checks the
    contract the operators leave to the caller before anything is launched."""
    A, rows, rp, ci, val, cp, ri, vi, _ = params
    dev = ci.device
    n, nnz = cp.numel() - 1, ci.numel()
    r = lambda *s: torch.randn(*s, device=dev, generator=gen)  # noqa: E731
    q, k, v, dO = r(m, heads, f) * f ** -0.25, r(n, heads, f) * f ** -0.25, r(n, heads, f), r(m, heads, f)
    pad = lambda t: torch.cat([t, torch.zeros(n - m, *t.shape[1:], device=dev)])  # noqa: E731
    rp_sq = torch.cat([rp, rp[-1:].expand(n - m)]).contiguous()       # n + 1 entries: the rows past m are empty
    q_sq, dO_sq = pad(q), pad(dO)
    assert rp.numel() == m + 1 and rp_sq.numel() == n + 1 and int(rp[-1]) == nnz and int(ci.max()) < n and int(ri.max()) < m
    rows_l, ci_l = rows.long(), ci.long()
    if conv == "gat":     # rect: the any-graph pair; padded_square: the existing (square) pair on the padded adjacency
        ar, ac = r(m, heads), r(n, heads)
        ar_sq = pad(ar)

        def rect():
            _, mx, sm, _ = fused_gatconv.gat_forward_edge(ar, ac, rp, ci, SLOPE, k)
            fused_gatconv.gat_backward_edge(SLOPE, 0.0, rp, ci, cp, ri, vi, ar, ac, k, mx, sm, dO, want_grad_score=False)

        def padded_square():
            _, mx, sm, mask = fused_gatconv.gat_forward(ar_sq, ac, rp_sq, ci, SLOPE, k, 0.0)
            fused_gatconv.gat_backward(SLOPE, 0.0, rp_sq, ci, cp, ri, vi, mx, sm, mask, k, ar_sq, ac, dO_sq)

        def index_ops():
            ar_, ac_, k_ = (t.clone().requires_grad_(True) for t in (ar, ac, k))
            index_ops_gat_edge(rows, ci, ar_, ac_, SLOPE, k_).backward(dO)
        return dict(rect=rect, padded_square=padded_square, index_ops=index_ops)
    if conv == "gatv2":
        attn = r(heads, f) * f ** -0.5

        def pair(rp_, xr, g):
            out, mx, sm = fused_gatconv.gatv2_forward(attn, rp_, ci, SLOPE, xr, k)
            fused_gatconv.gatv2_backward(SLOPE, rp_, ci, cp, ri, attn, xr, k, out, mx, sm, g)

        def index_ops():
            xr, xc, a = (t.clone().requires_grad_(True) for t in (q, k, attn))
            s = (torch.nn.functional.leaky_relu(xr[rows_l] + xc[ci_l], SLOPE) * a).sum(-1)
            p = torch.exp(s - s.detach().max())
            den = torch.zeros(m, heads, device=dev).index_add_(0, rows_l, p)
            torch.zeros_like(xr).index_add_(0, rows_l, xc[ci_l] * (p / den[rows_l])[:, :, None]).backward(dO)
    else:
        zero = torch.zeros(nnz, heads, device=dev)

        def pair(rp_, q_, g):
            out, mx, sm = fused_gtconv.gt_forward_rowstats(rp_, ci, val, q_, k, v)
            fused_gtconv.gt_backward_rowstats(rp_, ci, val, cp, ri, vi, q_, k, v, out, mx, sm, g)

        def index_ops():
            q_, k_, v_ = (t.clone().requires_grad_(True) for t in (q, k, v))
            index_ops_mha_bias(rows, ci, val, q_, k_, v_, zero).backward(dO)
    return dict(rect=lambda: pair(rp, q, dO), padded_square=lambda: pair(rp_sq, q_sq, dO_sq), index_ops=index_ops)


def conv_pairs(conv, blocks, heads, dim, iters, repeats):
    """forward + backward of the operators alone on the blocks of one step: rect, padded-square, index ops."""
    gen = torch.Generator(device=blocks[0][0][3].device).manual_seed(3)
    per_block = [block_jobs(conv, params, m, heads, dim // heads, gen) for params, m in blocks]
    res = {}
    for name in ("rect", "padded_square", "index_ops"):
        fns = [jobs[name] for jobs in per_block]
        run = lambda fns=fns: [fn() for fn in fns]  # noqa: E731
        run()
        res[name + "_ms"], res[name + "_spread"] = timed(run, iters, repeats)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=0.1)
    ap.add_argument("--conv", default="gt", choices=["gt", "gatv2", "gat"])
    ap.add_argument("--fanout", default="10,25", help="per layer, input side first")
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--heads", type=int, default=1)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sampler", default="torch", choices=["torch", "native"],
                    help="torch: sample_block (torch ops, keys from the device generator); native: sample_block_fused")
    args = ap.parse_args()
    fanouts = [int(x) for x in args.fanout.split(",")]
    assert len(fanouts) == 2, "two layers: two fanouts"
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    g = load_data_full_graph("reddit", scale=args.scale)
    N = g.num_nodes()
    x_all = g.ndata["feat"][:, :args.dim].to(dev)
    labels = torch.randint(args.classes, (N,), generator=torch.Generator().manual_seed(1)).to(dev)
    src, dst = (t.to(dev) for t in g.edges())
    row_ptr, col_ind = dfgnn_preprocess.coo_to_hyper(src, dst, N, csc=False)[:2]
    model = Net(args.conv, x_all.shape[1], args.dim, args.heads, args.classes).to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    loss_fn = nn.CrossEntropyLoss()
    gen = torch.Generator(device=dev).manual_seed(2)
    # the native sampler takes one 32-bit seed per hop: drawn on the CPU, no device work and no host read
    hop, hop_gen = (sample_block_fused, torch.Generator().manual_seed(2)) if args.sampler == "native" else (sample_block, gen)
    base = dict(tool="train_sampled", sampler=args.sampler, conv=args.conv, scale=args.scale, fanout=fanouts, batch=args.batch, heads=args.heads,
                dim=args.dim, nodes=N, edges=g.num_edges())
    t_sample, t_prep, t_step, worst_gap = [], [], [], 0.0

    def now():
        torch.cuda.synchronize()
        return time.perf_counter()

    for step in range(args.warmup + args.steps):
        t0 = now()
        seeds = torch.randperm(N, device=dev, generator=gen)[:args.batch]
        sampled, inputs = sample(row_ptr, col_ind, seeds, fanouts, hop_gen, hop)
        t1 = now()
        blocks = [(preprocess_block(b), m) for b, m in sampled]
        t2 = now()
        loss = loss_fn(model(blocks, x_all[inputs], True), labels[seeds])
        opt.zero_grad()
        loss.backward()
        t3 = now()
        with torch.no_grad():       # the index-op branch on the same blocks and weights, outside the timed step
            plain = loss_fn(model(blocks, x_all[inputs], False), labels[seeds])
        worst_gap = max(worst_gap, abs(float(loss) - float(plain)))
        t4 = now()
        opt.step()
        t3 += now() - t4
        if step >= args.warmup:
            t_sample.append((t1 - t0) * 1e3), t_prep.append((t2 - t1) * 1e3), t_step.append((t3 - t0) * 1e3)
    fused, plain = float(loss), float(plain)      # the last step's two losses
    shapes = [[m, int(p[5].numel()) - 1, int(p[3].numel())] for p, m in blocks]
    med = lambda v: round(statistics.median(v), 3)  # noqa: E731
    print(json.dumps(dict(base, what="losses", fused=round(fused, 6), index_ops=round(plain, 6), worst_gap_over_steps=float(f"{worst_gap:.2e}"),
                          blocks_rows_cols_nnz=shapes)))
    print(json.dumps(dict(base, what="sampling", ms_per_step=med(t_sample))))
    print(json.dumps(dict(base, what="preprocessing", ms_per_step=med(t_prep))))
    print(json.dumps(dict(base, what="step", ms_per_step=med(t_step))))
    print(json.dumps(dict(base, what="conv_pairs", **conv_pairs(args.conv, blocks, args.heads, args.dim, args.iters, args.repeats))))


if __name__ == "__main__":
    main()
