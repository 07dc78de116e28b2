#!/usr/bin/env python3
"""The two plan-less GT training pairs on identical inputs: the attn_edge form (fused_gtconv.gt_hyper_forward /
gt_backward: what GTConvFuse_hyper takes on a full graph or a low-degree batch) against the general statistics pair
(gt_forward_rowstats / gt_backward_rowstats: what GTConvFuse_rowstats takes).  Device events around each call, warm-up
first, the two forms alternating step by step; peak of allocated memory of one forward + backward; optionally the whole
step as one HIP graph.  One JSON line per (case, form).
usage: python3 tools/rowstats_bench.py --case reddit|cora|peptides [--scale 1.0] [--shapes 1x128,8x16] [--steps 20]
       [--graph]   (DESIGN.md 3.3i holds the table made from these lines)"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "df-gnn_amd")):
    sys.path.insert(0, p)
import numpy as np  # noqa: E402
import torch  # noqa: E402

import fused_gtconv as gt  # noqa: E402
from DFGNN.layers import preprocess_Hyper_fw_bw  # noqa: E402
from DFGNN.utils import GraphedStep  # noqa: E402
from DFGNN.utils import synthetic as S  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="cora", choices=["reddit", "cora", "peptides"])
    ap.add_argument("--scale", type=float, default=1.0, help="reddit only")
    ap.add_argument("--shapes", default="1x128", help="heads x per-head width, comma-separated: 1x128,8x16")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--graph", action="store_true", help="also time the step as one HIP graph")
    ap.add_argument("--forms", default="hyper,rowstats")
    args = ap.parse_args()
    t0 = time.perf_counter()
    g = {"reddit": lambda: S.reddit_like(scale=args.scale), "cora": S.cora_like,
         "peptides": lambda: S.peptides_like(batch_size=256)}[args.case]().to(DEV)
    A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem = preprocess_Hyper_fw_bw(g)
    del A, g
    m, nnz = row_ptr.numel() - 1, col_ind.numel()
    print(f"# {args.case}: m={m} nnz={nnz}, built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    graph = (rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem)
    for shape in args.shapes.split(","):
        h, f = (int(x) for x in shape.split("x"))
        bench(args, graph, m, nnz, h, f)


def bench(args, graph, m, nnz, h, f):
    rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem = graph
    Q, K, V = S.gt_features(m, h, f, seed=5, device=DEV)
    dO = torch.randn(m, h, f, generator=torch.Generator().manual_seed(3)).to(DEV)
    # the attn_edge form is what FusedGTFunction_hyper takes here (no all-dense plan)
    assert gt.gt_stats_pair_chosen(row_ptr, col_ind, val, Q) is None and gt.gt_ranked_pair_chosen(row_ptr, col_ind, val, Q) is None

    def hyper_fwd():
        return gt.gt_hyper_forward(row_ptr, col_ind, rows, val, col_ptr, row_ind, val_idx, smem, Q, K, V)

    def hyper_bwd(saved):
        return gt.gt_backward(row_ptr, col_ind, rows, val, col_ptr, row_ind, val_idx, smem, Q, K, V, saved[1], dO)

    def row_fwd():
        return gt.gt_forward_rowstats(row_ptr, col_ind, val, Q, K, V)

    def row_bwd(saved):
        return gt.gt_backward_rowstats(row_ptr, col_ind, val, col_ptr, row_ind, val_idx, Q, K, V, *saved, dO)

    forms = {"hyper": (hyper_fwd, hyper_bwd), "rowstats": (row_fwd, row_bwd)}
    forms = {k: forms[k] for k in args.forms.split(",")}
    times = {k: {"fwd": [], "bwd": []} for k in forms}
    results = {}
    for it in range(args.warmup + args.steps):
        for name, (fwd, bwd) in forms.items():           # alternating: both forms see the same machine state
            e = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
            e[0].record()
            saved = fwd()
            e[1].record()
            grads = bwd(saved)
            e[2].record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[name]["fwd"].append(e[0].elapsed_time(e[1]) * 1e3)
                times[name]["bwd"].append(e[1].elapsed_time(e[2]) * 1e3)
            results[name] = [saved[0]] + list(grads)
            del saved, grads
    if len(results) == 2:                                 # same function: the two forms agree to fp32 rounding
        for a, b, what in zip(results["hyper"], results["rowstats"], ("out", "dQ", "dK", "dV")):
            print(f"# max |hyper - rowstats| {what}: {(a - b).abs().max().item():.2e} (max |.| {a.abs().max().item():.2e})",
                  file=sys.stderr)
    results.clear()
    for name, (fwd, bwd) in forms.items():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        bwd(fwd())
        torch.cuda.synchronize()
        line = {"tool": "rowstats_bench", "case": args.case, "form": name, "m": m, "nnz": nnz, "h": h, "f": f,
                "steps": args.steps,
                "fwd_us": round(float(np.median(times[name]["fwd"])), 1), "bwd_us": round(float(np.median(times[name]["bwd"])), 1),
                "step_us_min": round(float(np.min(np.add(times[name]["fwd"], times[name]["bwd"]))), 1),
                "step_us_max": round(float(np.max(np.add(times[name]["fwd"], times[name]["bwd"]))), 1),
                "peak_bytes_one_step": torch.cuda.max_memory_allocated() - base}
        line["step_us"] = round(line["fwd_us"] + line["bwd_us"], 1)
        if args.graph:
            step = GraphedStep(lambda: bwd(fwd()))
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            for _ in range(args.warmup):
                step.replay()
            a.record()
            for _ in range(args.steps):
                step.replay()
            b.record()
            torch.cuda.synchronize()
            line["graph_step_us"] = round(a.elapsed_time(b) * 1e3 / args.steps, 1)
            del step
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
