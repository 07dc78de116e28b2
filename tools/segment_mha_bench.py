#!/usr/bin/env python3
"""Global attention over batched graphs (DFGNN.operators.fused_gtconv.SegmentMHAFuse; csrc/segment_mha.hip) against the two
things a user could do before it, on identical inputs, forward + backward of one training step:
  new    SegmentMHAFuse(seg_ptr, Q, K, V)
  sdpa   torch scaled_dot_product_attention on the batch padded to [B, h, n_max, f] with a key-padding mask (the padding
         and the gather back are NOT timed: the baseline at its best)
  csr    GTConvFuse_rowstats on the complete-graph CSR (sum of n^2 edges), where that has at most --csr-max-edges edges
Batches: graph sizes drawn around 23 (ZINC-like), 119 (PATTERN-like), 150 (Peptides-like) and 1000-2000 nodes.  Device events
around each step, warm-up first, the forms alternating step by step; the median and the minimum go to one JSON line per
(batch, shape), appended to profiles/segment_mha_bench.jsonl.
--bias: the pair with a pair bias (SegmentMHABiasFuse, include/dfgnn_segment_bias.h), bias fp32 [h, sum of n^2] requiring a
gradient, against
  sdpa   the same padded SDPA with the bias as a float attn_mask [B, h, n_max, n_max] (-inf on the padding keys), its
         gradient included
  plain  the unbiased pair on the same Q, K, V: the difference is the price of the bias
--tbias: the pair with a typed pair bias (SegmentMHATBiasFuse, include/dfgnn_segment_tbias.h), T = --types, one training step
with the table's gradient:
  typed         SegmentMHATBiasFuse(seg_ptr, Q, K, V, types uint8, table)
  materialised  what a user ran before it: bias = table.t()[:, types int64], SegmentMHABiasFuse, autograd's index backward --
                all of it inside the timed region
  plain         the unbiased pair
and the peak of torch's allocator over one step of typed and of materialised, above what is allocated before the step.
--cross: the cross pair (SegmentCrossMHAFuse, include/dfgnn_segment_cross.h) with every batch as the KEY side and --seeds
queries per graph (0: the square row, the queries are the keys' own array), one training step of
  wide, split, auto   the three values of `form`
  sdpa                the padded SDPA with [B, h, seeds, f] queries and the key-padding mask
  self                (square row only) SegmentMHAFuse on the same arrays
one JSON line per (batch, seeds, shape), appended to profiles/segment_cross_bench.jsonl.
--gate: the pair with pair gates and a logit output (SegmentMHAGateFuse, include/dfgnn_segment_gate.h), one training step with
the gradients of Q, K, V, bias and gate, the logits an output that receives a gradient of its own:
  new    SegmentMHAGateFuse(seg_ptr, Q, K, V, bias, gate, return_logits=True)
  torch  the padded form, (softmax(Q K^T scale + b) * sigmoid(g)) @ V on [B, h, n_max, n_max] with the logits kept (SDPA
         cannot gate); the padding and the gather back are not timed
  bias   the bias pair on the same Q, K, V, bias: the difference is the price of the two streams in and the two out
one JSON line per (batch, shape), appended to profiles/segment_gate_bench.jsonl.
usage: python3 tools/segment_mha_bench.py [--shapes 4x32,8x16,1x128] [--steps 30] [--bias | --gate | --tbias [--types 20] | --cross [--seeds 1,4,16,0]]
(DESIGN.md 3.3k, 3.3l, 3.3m, 3.3n, 3.3o hold the tables)"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "df-gnn_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from torch.nn import functional as F  # noqa: E402

from DFGNN.operators.fused_gtconv import (GTConvFuse_rowstats, SegmentCrossMHAFuse, SegmentMHABiasFuse, SegmentMHAFuse,  # noqa: E402
                                          SegmentMHAGateFuse, SegmentMHATBiasFuse)

DEV = "cuda:0"
BATCHES = {"zinc": (1024, 9, 37), "pattern": (256, 44, 188), "peptides": (128, 60, 240), "long": (16, 1000, 2000)}


def complete_csr(sizes):
    """The complete graph of every segment as the arrays GTConvFuse_rowstats takes (its CSC half is its own transpose)."""
    n = torch.as_tensor(sizes, device=DEV)
    lo = torch.cumsum(n, 0) - n
    node_lo, node_n = torch.repeat_interleave(lo, n), torch.repeat_interleave(n, n)
    row_ptr = torch.zeros(node_n.numel() + 1, dtype=torch.int64, device=DEV)
    row_ptr[1:] = torch.cumsum(node_n, 0)
    rows = torch.repeat_interleave(torch.arange(node_n.numel(), device=DEV), node_n)
    col = torch.arange(int(row_ptr[-1]), device=DEV) - row_ptr[rows] + node_lo[rows]
    val_idx = row_ptr[col] + rows - node_lo[rows]
    i32 = lambda t: t.to(torch.int32)  # noqa: E731
    val = torch.ones(col.numel(), device=DEV)
    return i32(rows), i32(row_ptr), i32(col), val, i32(row_ptr), i32(col), i32(val_idx), 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="4x32,8x16,1x128", help="heads x per-head width, comma-separated")
    ap.add_argument("--batches", default=",".join(BATCHES))
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--csr-max-edges", type=int, default=40_000_000)
    ap.add_argument("--bias", action="store_true", help="time the biased pair against SDPA with a float mask and the unbiased pair")
    ap.add_argument("--tbias", action="store_true", help="time the typed pair against the materialised bias and the unbiased pair")
    ap.add_argument("--types", type=int, default=20, help="--tbias: rows of the table")
    ap.add_argument("--bias-max-pairs", type=int, default=40_000_000, help="skip batches whose padded mask would be larger")
    ap.add_argument("--cross", action="store_true", help="time the cross pair's forms against padded SDPA (and the self pair)")
    ap.add_argument("--seeds", default="1,4,16,0", help="--cross: queries per graph, comma-separated; 0: queries = keys (square)")
    ap.add_argument("--gate", action="store_true", help="time the gated pair with its logit output against padded torch and the bias pair")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    default = "segment_cross_bench.jsonl" if args.cross else "segment_gate_bench.jsonl" if args.gate else "segment_mha_bench.jsonl"
    args.out = args.out or os.path.join(ROOT, "profiles", default)
    for name in args.batches.split(","):
        count, a, b = BATCHES[name]
        sizes = np.random.default_rng(7).integers(a, b + 1, size=count)
        for shape in args.shapes.split(","):
            h, f = (int(x) for x in shape.split("x"))
            if (args.bias or args.tbias or args.gate) and len(sizes) * int(sizes.max()) ** 2 > args.bias_max_pairs:
                continue
            lines = ([bench_cross(args, name, sizes, h, f, int(k)) for k in args.seeds.split(",")] if args.cross else
                     [bench_gate(args, name, sizes, h, f)] if args.gate else [bench(args, name, sizes, h, f)])
            for line in lines:
                print(json.dumps(line), flush=True)
                with open(args.out, "a") as fh:
                    fh.write(json.dumps(line) + "\n")


def bench(args, name, sizes, h, f):
    ends = np.concatenate([[0], np.cumsum(sizes)])
    m, B, nmax, pairs = int(ends[-1]), len(sizes), int(sizes.max()), int((sizes.astype(np.int64) ** 2).sum())
    seg_ptr = torch.tensor(ends, dtype=torch.int32, device=DEV)
    gen = torch.Generator().manual_seed(5)
    Q0, K0, V0, dO = (torch.randn(m, h, f, generator=gen).to(DEV) for _ in range(4))
    scale = f ** -0.5
    # padded form: node i of graph b at [b, :, i - lo_b]
    seg = torch.repeat_interleave(torch.arange(B, device=DEV), torch.as_tensor(sizes, device=DEV))
    pos = torch.arange(m, device=DEV) - seg_ptr[seg.long()].long()
    pad = lambda x: torch.zeros(B, nmax, h, f, device=DEV).index_put_((seg, pos), x).transpose(1, 2).contiguous()  # noqa: E731
    keep = (torch.arange(nmax, device=DEV)[None, :] < torch.as_tensor(sizes, device=DEV)[:, None])[:, None, None, :]
    Qp, Kp, Vp, dOp = (pad(x) for x in (Q0, K0, V0, dO))
    forms = {"new": (lambda q, k, v: SegmentMHAFuse(seg_ptr, q, k, v, scale), (Q0, K0, V0), dO),
             "sdpa": (lambda q, k, v: F.scaled_dot_product_attention(q, k, v, attn_mask=keep, scale=scale), (Qp, Kp, Vp), dOp)}
    if args.bias:
        # bias [h, pairs] and the same numbers as a padded float mask: pair (i, j) of graph b at [b, :, i - lo, j - lo]
        n_of = torch.as_tensor(sizes, device=DEV)[seg]
        prow = torch.repeat_interleave(torch.arange(m, device=DEV), n_of)
        pcol = torch.arange(pairs, device=DEV) - torch.repeat_interleave(torch.cumsum(n_of, 0) - n_of, n_of)
        bias0 = torch.randn(h, pairs, generator=gen).to(DEV)
        mask0 = torch.zeros(B, h, nmax, nmax, device=DEV).masked_fill_(~keep, float("-inf"))
        mask0[seg[prow], :, pos[prow], pcol] = bias0.t()
        forms = {"new": (lambda q, k, v, b: SegmentMHABiasFuse(seg_ptr, q, k, v, b, scale), (Q0, K0, V0, bias0), dO),
                 "sdpa": (lambda q, k, v, b: F.scaled_dot_product_attention(q, k, v, attn_mask=b, scale=scale), (Qp, Kp, Vp, mask0), dOp),
                 "plain": (lambda q, k, v: SegmentMHAFuse(seg_ptr, q, k, v, scale), (Q0, K0, V0), dO)}
    elif args.tbias:
        types = torch.randint(0, args.types, (pairs,), generator=gen)
        t8, t64, table0 = types.to(torch.uint8).to(DEV), types.to(DEV), torch.randn(args.types, h, generator=gen).to(DEV)
        forms = {"typed": (lambda q, k, v, tb: SegmentMHATBiasFuse(seg_ptr, q, k, v, t8, tb, scale), (Q0, K0, V0, table0), dO),
                 "materialised": (lambda q, k, v, tb: SegmentMHABiasFuse(seg_ptr, q, k, v, tb.t()[:, t64], scale), (Q0, K0, V0, table0), dO),
                 "plain": (lambda q, k, v: SegmentMHAFuse(seg_ptr, q, k, v, scale), (Q0, K0, V0), dO)}
    elif pairs <= args.csr_max_edges:
        csr = complete_csr(sizes)
        forms["csr"] = (lambda q, k, v: GTConvFuse_rowstats(*csr, q * scale, k, v), (Q0, K0, V0), dO)
    times = {k: [] for k in forms}
    last, peak = {}, {}
    for it in range(args.warmup + args.steps):
        for key, (fn, inputs, grad) in forms.items():           # alternating: all forms see the same machine state
            leaves = [x.detach().requires_grad_(True) for x in inputs]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            if args.tbias and it == args.warmup - 1:
                torch.cuda.reset_peak_memory_stats()
                before = torch.cuda.memory_allocated()
            a.record()
            out = fn(*leaves)
            grads = torch.autograd.grad(out, leaves, grad)
            b.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[key].append(a.elapsed_time(b) * 1e3)
            if args.tbias and it == args.warmup - 1:
                peak[key] = torch.cuda.max_memory_allocated() - before
            last[key] = [out.detach()] + list(grads)
    unpad = lambda x: x.transpose(1, 2)[seg, pos]  # noqa: E731
    if args.tbias:
        line = {"tool": "segment_mha_bench_tbias", "batch": name, "graphs": B, "m": m, "pairs": pairs, "h": h, "f": f, "T": args.types,
                "steps": args.steps}
        for key in forms:
            line[key + "_us"], line[key + "_us_min"] = round(float(np.median(times[key])), 1), round(float(np.min(times[key])), 1)
            line[key + "_peak_mib"] = round(peak[key] / 2 ** 20, 1)
        line["max_diff"] = max(float((x - y).abs().max()) for x, y in zip(last["typed"], last["materialised"]))
        return line
    line = {"tool": "segment_mha_bench" + ("_bias" if args.bias else ""), "batch": name, "graphs": B, "m": m, "n_max": nmax, "pairs": pairs, "h": h, "f": f,
            "steps": args.steps}
    for key in forms:
        line[key + "_us"] = round(float(np.median(times[key])), 1)
        line[key + "_us_min"] = round(float(np.min(times[key])), 1)
        if key == "plain":                                       # (another function)
            continue
        if key != "new":                                         # same function: the forms agree to fp32 rounding
            other = [unpad(x) for x in last[key][:4]] if key == "sdpa" else last[key]
            if args.bias:
                other.append(last[key][4][seg[prow], :, pos[prow], pcol].t())
            line[key + "_max_diff"] = max(float((x - y).abs().max()) for x, y in zip(last["new"], other))
    return line


def bench_cross(args, name, sizes, h, f, seeds):
    """One training step of the cross pair with `sizes` as the key side and `seeds` queries per graph (0: the square row)."""
    B, nmax = len(sizes), int(sizes.max())
    qsizes = sizes if seeds == 0 else np.full(B, seeds)
    ek, eq = (np.concatenate([[0], np.cumsum(s)]) for s in (sizes, qsizes))
    m_k, m_q, qmax = int(ek[-1]), int(eq[-1]), int(qsizes.max())
    sk, sq = (torch.tensor(e, dtype=torch.int32, device=DEV) for e in (ek, eq))
    gen = torch.Generator().manual_seed(5)
    Q0, dO = (torch.randn(m_q, h, f, generator=gen).to(DEV) for _ in range(2))
    K0, V0 = (torch.randn(m_k, h, f, generator=gen).to(DEV) for _ in range(2))
    scale = f ** -0.5

    def padder(sz, ptr, m, width):        # row i of graph b at [b, :, i - lo_b]
        seg = torch.repeat_interleave(torch.arange(B, device=DEV), torch.as_tensor(sz, device=DEV))
        pos = torch.arange(m, device=DEV) - ptr[seg.long()].long()
        return seg, pos, lambda x: torch.zeros(B, width, h, f, device=DEV).index_put_((seg, pos), x).transpose(1, 2).contiguous()
    qseg, qpos, padq = padder(qsizes, sq, m_q, qmax)
    kseg, kpos, padk = padder(sizes, sk, m_k, nmax)
    keep = (torch.arange(nmax, device=DEV)[None, :] < torch.as_tensor(sizes, device=DEV)[:, None])[:, None, None, :]
    forms = {key: (lambda q, k, v, form=form: SegmentCrossMHAFuse(sq, sk, q, k, v, scale, form), (Q0, K0, V0), dO)
             for key, form in (("wide", 1), ("split", 2), ("auto", 0))}
    forms["sdpa"] = (lambda q, k, v: F.scaled_dot_product_attention(q, k, v, attn_mask=keep, scale=scale),
                     (padq(Q0), padk(K0), padk(V0)), padq(dO))
    if seeds == 0:
        forms["self"] = (lambda q, k, v: SegmentMHAFuse(sk, q, k, v, scale), (Q0, K0, V0), dO)
    times, last = {k: [] for k in forms}, {}
    for it in range(args.warmup + args.steps):
        for key, (fn, inputs, grad) in forms.items():           # alternating: all forms see the same machine state
            leaves = [x.detach().requires_grad_(True) for x in inputs]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out = fn(*leaves)
            grads = torch.autograd.grad(out, leaves, grad)
            b.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[key].append(a.elapsed_time(b) * 1e3)
            last[key] = [out.detach()] + list(grads)
    line = {"tool": "segment_cross_bench", "batch": name, "graphs": B, "seeds": seeds, "m_q": m_q, "m_k": m_k, "n_max": nmax, "h": h,
            "f": f, "steps": args.steps}
    for key in forms:
        line[key + "_us"], line[key + "_us_min"] = round(float(np.median(times[key])), 1), round(float(np.min(times[key])), 1)
        other = last[key]
        if key == "sdpa":
            unq, unk = (lambda x: x.transpose(1, 2)[qseg, qpos]), (lambda x: x.transpose(1, 2)[kseg, kpos])
            other = [unq(other[0]), unq(other[1]), unk(other[2]), unk(other[3])]
        if key != "wide":
            line[key + "_max_diff"] = max(float((x - y).abs().max()) for x, y in zip(last["wide"], other))
    return line


def bench_gate(args, name, sizes, h, f):
    """One training step of the gated pair with its logit output, of its padded torch form and of the bias pair."""
    ends = np.concatenate([[0], np.cumsum(sizes)])
    m, B, nmax, pairs = int(ends[-1]), len(sizes), int(sizes.max()), int((sizes.astype(np.int64) ** 2).sum())
    seg_ptr = torch.tensor(ends, dtype=torch.int32, device=DEV)
    gen = torch.Generator().manual_seed(5)
    Q0, K0, V0, dO = (torch.randn(m, h, f, generator=gen).to(DEV) for _ in range(4))
    bias0, gate0, dL = (torch.randn(h, pairs, generator=gen).to(DEV) for _ in range(3))
    scale = f ** -0.5
    n_t = torch.as_tensor(sizes, device=DEV)
    seg = torch.repeat_interleave(torch.arange(B, device=DEV), n_t)
    pos = torch.arange(m, device=DEV) - seg_ptr[seg.long()].long()
    pad = lambda x: torch.zeros(B, nmax, h, f, device=DEV).index_put_((seg, pos), x).transpose(1, 2).contiguous()  # noqa: E731
    keep = (torch.arange(nmax, device=DEV)[None, :] < n_t[:, None])[:, None, None, :]
    n_of = n_t[seg]
    prow = torch.repeat_interleave(torch.arange(m, device=DEV), n_of)
    pcol = torch.arange(pairs, device=DEV) - torch.repeat_interleave(torch.cumsum(n_of, 0) - n_of, n_of)
    at = (seg[prow], slice(None), pos[prow], pcol)               # pair (i, j) of graph b at [b, :, i - lo, j - lo]

    def plane(x, fill=0.0):
        p = torch.full((B, h, nmax, nmax), fill, device=DEV)
        p[at] = x.t()
        return p
    mask0 = plane(bias0).masked_fill_(~keep, float("-inf"))

    def padded(q, k, v, b, g):
        x = q @ k.transpose(-1, -2) * scale + b
        return (torch.softmax(x, dim=-1) * torch.sigmoid(g)) @ v, x
    forms = {"new": (lambda q, k, v, b, g: SegmentMHAGateFuse(seg_ptr, q, k, v, b, g, scale, return_logits=True),
                     (Q0, K0, V0, bias0, gate0), (dO, dL)),
             "torch": (padded, (pad(Q0), pad(K0), pad(V0), mask0, plane(gate0)), (pad(dO), plane(dL))),
             "bias": (lambda q, k, v, b: (SegmentMHABiasFuse(seg_ptr, q, k, v, b, scale),), (Q0, K0, V0, bias0), (dO,))}
    times, last = {k: [] for k in forms}, {}
    for it in range(args.warmup + args.steps):
        for key, (fn, inputs, grad) in forms.items():           # alternating: all forms see the same machine state
            leaves = [x.detach().requires_grad_(True) for x in inputs]
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            outs = fn(*leaves)
            grads = torch.autograd.grad(outs, leaves, grad)
            b.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[key].append(a.elapsed_time(b) * 1e3)
            last[key] = [o.detach() for o in outs] + list(grads)
    line = {"tool": "segment_mha_bench_gate", "batch": name, "graphs": B, "m": m, "n_max": nmax, "pairs": pairs, "h": h, "f": f,
            "steps": args.steps, "plane_mib": round(4 * h * pairs / 2 ** 20, 2)}
    for key in forms:
        line[key + "_us"], line[key + "_us_min"] = round(float(np.median(times[key])), 1), round(float(np.min(times[key])), 1)
    unpad, unplane = (lambda x: x.transpose(1, 2)[seg, pos]), (lambda x: x[at].t())
    o, lg, dq, dk, dv, db, dg = last["torch"]
    other = [unpad(o), unplane(lg), unpad(dq), unpad(dk), unpad(dv), unplane(db), unplane(dg)]
    line["torch_max_diff"] = max(float((x - y).abs().max()) for x, y in zip(last["new"], other))
    return line


if __name__ == "__main__":
    main()
