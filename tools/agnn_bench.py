#!/usr/bin/env python3
"""The fused AGNN / dot-product pair with tied keys and values (DFGNN.operators.fused_gtconv.AGNNConvFuse;
csrc/agnn_train.hip) against what the repository did for these two convolutions before it, on identical inputs, forward and
backward timed separately, in both modes:
  new      AGNNConvFuse(beta, H, H): one tensor in, one gather per edge, norms from the gathered registers
  gt       (a) F.normalize + GTConvFuse_rowstats on (H_norm beta, H_norm, H) -- dot mode: (H beta, H, H) -- with autograd
           through the normalisation and the scaling: three tensors in, a key row and a value row gathered per edge
  nofuse   (b) the layers' index-op branch (index_ops_agnn), skipped where the messages [nnz, h, f] alone exceed
           --nofuse-max-gb
Device events around each pass, warm-up first, the forms alternating step by step; peak of allocated memory of one training
step.  One JSON line per (case, shape, mode).
usage: python3 tools/agnn_bench.py --case cora|pattern|reddit [--scale 0.1] [--shapes 1x64,8x16,1x128] [--steps 20]
       (DESIGN.md 3.2k holds the table made from these lines)"""
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
from torch.nn import functional as F  # noqa: E402

from DFGNN.layers import preprocess_Hyper_fw_bw  # noqa: E402
from DFGNN.layers.AGNN import index_ops_agnn  # noqa: E402
from DFGNN.operators.fused_gtconv import AGNNConvFuse, GTConvFuse_rowstats  # noqa: E402
from DFGNN.utils import synthetic as S  # noqa: E402

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="cora", choices=["reddit", "cora", "pattern"])
    ap.add_argument("--scale", type=float, default=0.1, help="reddit only")
    ap.add_argument("--batch-size", type=int, default=256, help="pattern only")
    ap.add_argument("--shapes", default="1x64,8x16,1x128", help="heads x per-head width, comma-separated")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nofuse-max-gb", type=float, default=4.0, help="skip the index-op form when its messages are larger")
    args = ap.parse_args()
    t0 = time.perf_counter()
    g = {"reddit": lambda: S.reddit_like(scale=args.scale), "cora": S.cora_like,
         "pattern": lambda: S.pattern_like(batch_size=args.batch_size)}[args.case]().to(DEV)
    params = preprocess_Hyper_fw_bw(g)
    m, nnz = params[2].numel() - 1, params[3].numel()
    print(f"# {args.case}: m={m} nnz={nnz}, built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    for shape in args.shapes.split(","):
        h, f = (int(x) for x in shape.split("x"))
        for cosine in (True, False):
            bench(args, params, m, nnz, h, f, cosine)


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b) * 1e3


def bench(args, params, m, nnz, h, f, cosine):
    A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem = params
    gen = torch.Generator().manual_seed(5)
    beta0 = ((torch.rand(h, generator=gen) * 4 + 0.5) * (1.0 if cosine else f ** -0.5)).to(DEV)
    H0, dO = (torch.randn(m, h, f, generator=gen).to(DEV) for _ in range(2))
    msg_bytes = nnz * h * f * 4
    nofuse = msg_bytes <= args.nofuse_max_gb * 2 ** 30

    def leaves():
        return H0.detach().requires_grad_(True), beta0.detach().requires_grad_(True)

    def new_fwd(H, beta):
        return AGNNConvFuse(row_ptr, col_ind, col_ptr, row_ind, beta, H, H, cosine)

    def gt_fwd(H, beta):
        K = F.normalize(H, p=2, dim=-1) if cosine else H
        return GTConvFuse_rowstats(rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem, K * beta[None, :, None], K, H)

    def nofuse_fwd(H, beta):
        return index_ops_agnn(A.row, A.col, beta, H, H, cosine)

    forms = {"new": new_fwd, "gt": gt_fwd}
    if nofuse:
        forms["nofuse"] = nofuse_fwd
    times = {k + p: [] for k in forms for p in ("_fwd", "_bwd")}
    last = {}

    def step(fn):
        H, beta = leaves()
        out, t_fwd = _timed(lambda: fn(H, beta))
        grads, t_bwd = _timed(lambda: torch.autograd.grad(out, (H, beta), dO))
        return [out.detach()] + list(grads), t_fwd, t_bwd

    for it in range(args.warmup + args.steps):
        for name, fn in forms.items():                    # alternating: all forms see the same machine state
            res, t_fwd, t_bwd = step(fn)
            if it >= args.warmup:
                times[name + "_fwd"].append(t_fwd)
                times[name + "_bwd"].append(t_bwd)
            last[name] = res
            del res
    for other in list(forms)[1:]:                         # same function: the forms agree to fp32 rounding
        for a, b, what in zip(last["new"], last[other], ("out", "dH", "dbeta")):
            print(f"# max |new - {other}| {what}: {(a - b).abs().max().item():.2e} (max |.| {b.abs().max().item():.2e})",
                  file=sys.stderr)
    last.clear()
    line = {"tool": "agnn_bench", "case": args.case, "mode": "cosine" if cosine else "dot", "m": m, "nnz": nnz, "h": h, "f": f,
            "steps": args.steps, "msg_bytes": msg_bytes}
    for name in times:
        line[name + "_us"] = round(float(np.median(times[name])), 1)
        line[name + "_us_min"] = round(float(np.min(times[name])), 1)
    for name, fn in forms.items():
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res = step(fn)
        torch.cuda.synchronize()
        line[name + "_step_peak_bytes"] = torch.cuda.max_memory_allocated() - base
        del res
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
