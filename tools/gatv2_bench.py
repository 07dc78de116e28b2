#!/usr/bin/env python3
"""The fused GATv2 convolution (fused_gatconv.gatv2_inference / gatv2_forward / gatv2_backward) against the layers' own
non-fused torch branch (GATv2ConvDGL.conv_nofuse: index ops that materialise z[nnz, h, f]) on identical inputs.  Device
events around each call, warm-up first, the two forms alternating step by step; peak of allocated memory of one training
step next to nnz h f 4 bytes, which the non-fused form needs for z alone.  The non-fused form is skipped where that figure
exceeds --nofuse-max-gb (it would not fit, or would only measure the allocator).  One JSON line per (case, shape).
usage: python3 tools/gatv2_bench.py --case cora|pattern|reddit [--scale 0.1] [--shapes 1x64,8x16] [--steps 20]
       (DESIGN.md 3.2c holds the table made from these lines)"""
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

import fused_gatconv as gat  # noqa: E402
from DFGNN.layers import GATv2ConvDGL, preprocess_Hyper_fw_bw  # noqa: E402
from DFGNN.utils import synthetic as S  # noqa: E402

DEV = "cuda:0"
SLOPE = 0.2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="cora", choices=["reddit", "cora", "pattern"])
    ap.add_argument("--scale", type=float, default=0.1, help="reddit only")
    ap.add_argument("--batch-size", type=int, default=256, help="pattern only")
    ap.add_argument("--shapes", default="1x64,8x16", help="heads x per-head width, comma-separated")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nofuse-max-gb", type=float, default=4.0, help="skip the non-fused form when z alone is larger")
    args = ap.parse_args()
    t0 = time.perf_counter()
    g = {"reddit": lambda: S.reddit_like(scale=args.scale), "cora": S.cora_like,
         "pattern": lambda: S.pattern_like(batch_size=args.batch_size)}[args.case]().to(DEV)
    A, _, row_ptr, col_ind, _, col_ptr, row_ind, _, _ = preprocess_Hyper_fw_bw(g)
    m, nnz = row_ptr.numel() - 1, col_ind.numel()
    print(f"# {args.case}: m={m} nnz={nnz}, built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
    for shape in args.shapes.split(","):
        h, f = (int(x) for x in shape.split("x"))
        bench(args, A, (row_ptr, col_ind, col_ptr, row_ind), m, nnz, h, f)


def _timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    torch.cuda.synchronize()
    return out, a.elapsed_time(b) * 1e3


def bench(args, A, graph, m, nnz, h, f):
    row_ptr, col_ind, col_ptr, row_ind = graph
    gen = torch.Generator().manual_seed(5)
    attn = (torch.randn(h, f, generator=gen) * f ** -0.5).to(DEV)
    x_row, x_col, dO = (torch.randn(m, h, f, generator=gen).to(DEV) for _ in range(3))
    layer = GATv2ConvDGL(f, f, h, negative_slope=SLOPE).to(DEV)   # (only its attention vector and conv_nofuse are used)
    with torch.no_grad():
        layer.attn.copy_(attn)
    z_bytes = nnz * h * f * 4
    nofuse = z_bytes <= args.nofuse_max_gb * 2 ** 30

    def fused_fwd():
        return gat.gatv2_inference(attn, row_ptr, col_ind, SLOPE, x_row, x_col)

    def fused_step():
        out, mx, sm = gat.gatv2_forward(attn, row_ptr, col_ind, SLOPE, x_row, x_col)
        return [out] + list(gat.gatv2_backward(SLOPE, row_ptr, col_ind, col_ptr, row_ind, attn, x_row, x_col, out, mx, sm, dO))

    def nofuse_fwd():
        with torch.no_grad():
            return layer.conv_nofuse(A, x_row, x_col)

    def nofuse_step():
        xr, xc = (t.detach().requires_grad_(True) for t in (x_row, x_col))
        out = layer.conv_nofuse(A, xr, xc)
        return [out.detach()] + list(torch.autograd.grad(out, (xr, xc, layer.attn), dO))

    forms = {"fused_fwd": fused_fwd, "fused_step": fused_step}
    if nofuse:
        forms.update(nofuse_fwd=nofuse_fwd, nofuse_step=nofuse_step)
    times = {k: [] for k in forms}
    last = {}
    for it in range(args.warmup + args.steps):
        for name, fn in forms.items():                    # alternating: all forms see the same machine state
            out, us = _timed(fn)
            if it >= args.warmup:
                times[name].append(us)
            last[name] = out
            del out
    if nofuse:                                            # same function: the two forms agree to fp32 rounding
        for a, b, what in zip(last["fused_step"], last["nofuse_step"], ("out", "dX_row", "dX_col", "dattn")):
            print(f"# max |fused - nofuse| {what}: {(a - b).abs().max().item():.2e} (max |.| {b.abs().max().item():.2e})",
                  file=sys.stderr)
    last.clear()
    line = {"tool": "gatv2_bench", "case": args.case, "m": m, "nnz": nnz, "h": h, "f": f, "steps": args.steps,
            "z_bytes": z_bytes}
    for name in forms:
        line[name + "_us"] = round(float(np.median(times[name])), 1)
        line[name + "_us_min"] = round(float(np.min(times[name])), 1)
    for name in ("fused_step",) + (("nofuse_step",) if nofuse else ()):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        forms[name]()
        torch.cuda.synchronize()
        line[name + "_peak_bytes"] = torch.cuda.max_memory_allocated() - base
        line[name + "_max_memory_allocated"] = torch.cuda.max_memory_allocated()
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
