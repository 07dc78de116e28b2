#!/usr/bin/env python3
"""The any-graph GAT pair with a per-edge attention term (fused_gatconv.gat_forward_edge / gat_backward_edge,
csrc/gat_edge_train.hip) against the index-op branch (DFGNN/layers/GAT: index_ops_gat_edge + torch.autograd.grad) and -- on
the configurations without a score -- against the existing general GAT pair (fused_gatconv.gat_forward / gat_backward with
USE_BLOCK_PLAN = False, which hands grad_edge [h, nnz] from its CSR pass to its CSC pass) on the same inputs: the PATTERN-like
and Peptides-like batches (bs 256), the cora-like graph and the reddit-like graph at --scale (0.1), at 1 x 128 and 8 x 16, in
four configurations:
  plain        no score, no dropout
  drop         no score, attention dropout 0.5 (one set of randoms, given to every branch that takes them)
  score        score [h, nnz] and grad_score, no dropout
  score_drop   both
Per configuration, by device events (warm-up first, the branches alternating step by step, medians): the fused forward
call, the fused backward call, the whole step of each branch; the three kernels (forward, CSR pass, CSC pass) from a
torch.profiler trace of the same calls (null where the profiler reports no kernels); and the peak of allocated memory of one
step of each branch above what was allocated before it.  The index-op branch is skipped (null) where it does not fit.

The driver starts one child process per (case, shape) under its own time limit and stops at the first one that fails; a
child prints one JSON line per configuration.  --out appends the lines to a file (profiles/gat_edge_bench.jsonl).
usage: python3 tools/gat_edge_bench.py [--cases pattern,peptides,cora,reddit] [--scale 0.1] [--shapes 1x128,8x16] [--steps 10]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
SLOPE, DROP = 0.2, 0.5
CONFIGS = {"plain": (False, False), "drop": (False, True), "score": (True, False), "score_drop": (True, True)}   # (score, dropout)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="pattern,peptides,cora,reddit")
    ap.add_argument("--scale", type=float, default=0.1, help="reddit only: the index-op form fits at 0.1")
    ap.add_argument("--shapes", default="1x128,8x16", help="heads x per-head width, comma-separated")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds a (case, shape) child may take")
    ap.add_argument("--out", default=None, help="append the JSON lines to this file")
    ap.add_argument("--child", default=None, help="case:shape -- run that one in this process")
    args = ap.parse_args()
    if args.child:
        return child(args, *args.child.split(":"))
    for case in args.cases.split(","):
        for shape in args.shapes.split(","):
            cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", f"{case}:{shape}",
                   "--scale", str(args.scale), "--steps", str(args.steps), "--warmup", str(args.warmup)]
            done = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            sys.stdout.write(done.stdout)
            sys.stdout.flush()
            if done.returncode != 0:
                print(f"# {case} {shape}: exit status {done.returncode}; stopping", file=sys.stderr)
                return done.returncode
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(done.stdout)
    return 0


def child(args, case, shape):
    for p in (ROOT, os.path.join(ROOT, "df-gnn_amd")):
        sys.path.insert(0, p)
    import torch

    from DFGNN.layers import preprocess_Hyper_fw_bw
    from DFGNN.utils import synthetic as S
    t0 = time.perf_counter()
    g = {"reddit": lambda: S.reddit_like(scale=args.scale), "cora": S.cora_like, "pattern": lambda: S.pattern_like(batch_size=256),
         "peptides": lambda: S.peptides_like(batch_size=256)}[case]().to(DEV)
    graph = preprocess_Hyper_fw_bw(g)[1:]
    del g
    m, nnz = graph[1].numel() - 1, graph[2].numel()
    print(f"# {case}: m={m} nnz={nnz}, built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    h, f = (int(x) for x in shape.split("x"))
    for name, (score, drop) in CONFIGS.items():
        print(json.dumps(bench(torch, args, case, name, score, drop, graph, m, nnz, h, f)), flush=True)
    return 0


def bench(torch, args, case, name, with_score, with_drop, graph, m, nnz, h, f):
    import numpy as np

    import fused_gatconv as gat
    from DFGNN.layers import index_ops_gat_edge
    rows, row_ptr, col_ind, _, col_ptr, row_ind, val_idx, _ = graph
    gen = lambda s: torch.Generator(device=DEV).manual_seed(s)  # noqa: E731
    ar, ac = (torch.randn(m, h, generator=gen(s), device=DEV) for s in (1, 2))
    X, dO = (torch.randn(m, h, f, generator=gen(s), device=DEV) for s in (3, 4))
    score = torch.randn(h, nnz, generator=gen(5), device=DEV) * 0.5 if with_score else None
    score_t = score.t().contiguous() if with_score else None               # [nnz, h] for the index-op branch
    mask = torch.rand(nnz, h, generator=gen(6), device=DEV) if with_drop else None
    drop = DROP if with_drop else 0.0

    def fwd():
        return gat.gat_forward_edge(ar, ac, row_ptr, col_ind, SLOPE, X, score, drop, mask)

    def bwd(emax, esum):
        return gat.gat_backward_edge(SLOPE, drop, row_ptr, col_ind, col_ptr, row_ind, val_idx, ar, ac, X, emax, esum, dO,
                                     score=score, edge_mask=mask, want_grad_score=with_score)

    def fused_step():
        out, emax, esum, _ = fwd()
        return [out] + list(bwd(emax, esum))

    def general_step():                                                    # the existing pair, general kernels
        saved, gat.USE_BLOCK_PLAN = gat.USE_BLOCK_PLAN, False
        try:
            # (its forward draws its own randoms: one torch.rand more per step than the new pair is given)
            out, emax, esum, msk = gat.gat_forward(ar, ac, row_ptr, col_ind, SLOPE, X, drop)
            return [out] + list(gat.gat_backward(SLOPE, drop, row_ptr, col_ind, col_ptr, row_ind, val_idx, emax, esum, msk, X, ar,
                                                 ac, dO))
        finally:
            gat.USE_BLOCK_PLAN = saved

    def torch_step():
        leaves = [t.detach().requires_grad_(True) for t in (X, ar, ac) + ((score_t,) if with_score else ())]
        sc = leaves[3] if with_score else None
        if mask is None:
            out = index_ops_gat_edge(rows, col_ind, leaves[1], leaves[2], SLOPE, leaves[0], sc)
        else:                       # the same randoms as the fused branch, in place of F.dropout's own
            keep = (mask > drop).to(X.dtype) / (1.0 - drop)
            out = _index_ops_with_mask(torch, rows, col_ind, leaves[1], leaves[2], leaves[0], sc, keep)
        return [out.detach()] + list(torch.autograd.grad(out, leaves, dO))

    def peak_of(step):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res = step()
        torch.cuda.synchronize()
        del res
        return torch.cuda.max_memory_allocated() - base

    forms = {"fused": fused_step, "torch": torch_step}
    if not with_score:
        forms["general"] = general_step
    peaks = {}
    for form in list(forms):
        try:
            forms[form]()
            peaks[form] = peak_of(forms[form])
        except torch.OutOfMemoryError:
            peaks[form] = None
            del forms[form]
            torch.cuda.empty_cache()
    times = {k: [] for k in list(forms) + ["fwd", "bwd"]}
    results = {}
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    for it in range(args.warmup + args.steps):
        for form, step in forms.items():
            a, b = ev(), ev()
            a.record()
            res = step()
            b.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[form].append(a.elapsed_time(b) * 1e3)
            results[form] = res
            del res
        a, b, c = ev(), ev(), ev()                             # the fused step once more, call by call
        a.record()
        out, emax, esum, _ = fwd()
        b.record()
        res = bwd(emax, esum)
        c.record()
        torch.cuda.synchronize()
        del res, out
        if it >= args.warmup:
            times["fwd"].append(a.elapsed_time(b) * 1e3)
            times["bwd"].append(b.elapsed_time(c) * 1e3)
    if "torch" in results:
        for x, y, what in zip(results["fused"], results["torch"], ("out", "grad_feat", "grad_attn_row", "grad_attn_col", "grad_score")):
            if x is not None:
                y = y.t() if what == "grad_score" else y
                print(f"# {case} {h}x{f} {name} max |fused - torch| {what}: {(x - y).abs().max().item():.2e} "
                      f"(max |.| {y.abs().max().item():.2e})", file=sys.stderr)
    passes = pass_times(torch, fused_step, args.steps)
    med = {k: float(np.median(v)) for k, v in times.items()}
    us = lambda k: round(med[k], 1) if k in med else None  # noqa: E731
    return {"tool": "gat_edge_bench", "case": case, "config": name, "m": m, "nnz": nnz, "h": h, "f": f, "steps": args.steps,
            "score": with_score, "dropout": with_drop,
            "fused_us": us("fused"), "torch_us": us("torch"), "general_us": us("general"),
            "torch_over_fused": round(med["torch"] / med["fused"], 2) if "torch" in med else None,
            "general_over_fused": round(med["general"] / med["fused"], 2) if "general" in med else None,
            "fwd_us": us("fwd"), "bwd_us": us("bwd"),
            "fwd_kernel_us": passes.get(0), "csr_kernel_us": passes.get(1), "csc_kernel_us": passes.get(2),
            "fused_peak_bytes": peaks.get("fused"), "torch_peak_bytes": peaks.get("torch"),
            "general_peak_bytes": peaks.get("general"), "head_edge_array_bytes": 4 * nnz * h}


def _index_ops_with_mask(torch, rows, col_ind, attn_row, attn_col, x_col, score, keep):
    """index_ops_gat_edge with given keep factors [nnz, h] in place of F.dropout's own randoms."""
    F = torch.nn.functional
    rows, cols = rows.long(), col_ind.long()
    pre = attn_row[rows] + attn_col[cols]
    if score is not None:
        pre = pre + score
    s = F.leaky_relu(pre, SLOPE)
    mx = torch.full((attn_row.size(0), s.size(1)), float("-inf"), dtype=s.dtype, device=s.device)
    mx = mx.scatter_reduce(0, rows[:, None].expand_as(s), s.detach(), reduce="amax", include_self=True)
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    p = torch.exp(s - mx[rows])
    den = torch.zeros_like(mx).index_add_(0, rows, p)
    p = p / den[rows] * keep
    out = torch.zeros((attn_row.size(0),) + tuple(x_col.shape[1:]), dtype=x_col.dtype, device=x_col.device)
    return out.index_add_(0, rows, x_col[cols] * p[:, :, None])


def pass_times(torch, step, steps):
    """{pass: median us} of the kernels gat_edge_*_kernel<..., PASS> (0 forward, 1 CSR pass, 2 CSC pass) over `steps` fused
    steps, from a torch.profiler trace; {} when the profiler reports none."""
    import re

    import numpy as np
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(steps):
                step()
            torch.cuda.synchronize()
        found = {}
        for e in prof.events():
            hit = re.search(r"gat_edge_(?:wave|group)_kernel<.*,\s*(\d)>", e.name)
            if hit:
                found.setdefault(int(hit.group(1)), []).append(e.device_time if hasattr(e, "device_time") else e.cuda_time)
        return {k: round(float(np.median(v)), 1) for k, v in found.items()}
    except Exception as err:   # (a profiler that cannot start leaves the event times above as they are)
        print(f"# pass times unavailable: {type(err).__name__}: {err}", file=sys.stderr)
        return {}


if __name__ == "__main__":
    sys.exit(main())
