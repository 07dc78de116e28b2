#!/usr/bin/env python3
"""The GATv2 pair with per-edge feature vectors inside the LeakyReLU on four graphs at 1 x 128 and 8 x 16, forward + backward
by device events (warm-up first, the forms alternating step by step, medians):
  (a) edge    fused_gatconv.gatv2_forward_edge / gatv2_backward_edge (dE wanted)
  (b) plain   gatv2_forward / gatv2_backward on the same inputs without E: the floor
  (c) torch   the index-op formulation with E (DFGNN/layers/GATv2/gatv2conv_layers.py: index_ops_gatv2_edge) and
              torch.autograd.grad: what a layer with edge features had to run before.  Skipped (null) where it does not fit
              in memory
and (a) - (b) set against the bytes E moves -- 4 nnz h f read in the forward, in the CSR pass and (gathered) in the CSC pass,
and dE written by the CSR pass: 16 nnz h f with dE, 12 nnz h f without (--no-dE) -- at the device-to-device copy rate
measured here the way bench.py does.  Next to the times, torch.cuda.max_memory_allocated of one step of (a) and of (c) above
what was allocated before it, and 4 nnz h f.
One JSON line per (case, shape) on stdout; --out appends a text table (profiles/gatv2_edge_kernel_times.txt).
usage: python3 tools/gatv2_edge_bench.py [--cases cora,peptides,pattern,reddit] [--scale 0.1] [--shapes 1x128,8x16] [--steps 10]"""
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
from DFGNN.layers import preprocess_Hyper_fw_bw  # noqa: E402
from DFGNN.layers.GATv2.gatv2conv_layers import index_ops_gatv2_edge  # noqa: E402
from DFGNN.utils import synthetic as S  # noqa: E402

DEV = "cuda:0"
SLOPE = 0.2


def copy_rate_gbs(n_bytes=1 << 28):
    """Read + written bytes of a device-to-device copy per second, in GB/s."""
    src, dst = torch.empty(n_bytes // 4, device=DEV), torch.empty(n_bytes // 4, device=DEV)
    for _ in range(2):
        dst.copy_(src)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(5):
        dst.copy_(src)
    b.record()
    torch.cuda.synchronize()
    return 2 * n_bytes * 5 / (a.elapsed_time(b) * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="cora,peptides,pattern,reddit")
    ap.add_argument("--scale", type=float, default=0.1, help="reddit only: E, dE and the index-op form fit at 0.1")
    ap.add_argument("--shapes", default="1x128,8x16", help="heads x per-head width, comma-separated")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-dE", action="store_true", help="E needs no gradient: (a) writes nothing of size nnz h f")
    ap.add_argument("--out", default=None, help="append the text table to this file")
    args = ap.parse_args()
    rate = copy_rate_gbs()
    per_edge = 12 if args.no_dE else 16
    table = [f"# tools/gatv2_edge_bench.py --scale {args.scale} --steps {args.steps}{' --no-dE' if args.no_dE else ''}; "
             f"device-to-device copy rate {rate:.0f} GB/s",
             f"# us, median of forward + backward; extra = {per_edge} nnz h f bytes / copy rate; MB: peak of one step above its start",
             f"# {'case':<9}{'h x f':>8}{'m':>8}{'nnz':>10}{'(a) edge':>11}{'(b) plain':>11}{'(c) torch':>11}"
             f"{'(a)-(b)':>10}{'extra':>9}{'(c)/(a)':>9}{'(a) MB':>9}{'(c) MB':>9}{'E MB':>8}"]
    for case in args.cases.split(","):
        t0 = time.perf_counter()
        g = {"reddit": lambda: S.reddit_like(scale=args.scale), "cora": S.cora_like,
             "peptides": lambda: S.peptides_like(batch_size=256),
             "pattern": lambda: S.pattern_like(batch_size=256)}[case]().to(DEV)
        graph = preprocess_Hyper_fw_bw(g)[1:]
        del g
        m, nnz = graph[1].numel() - 1, graph[2].numel()
        print(f"# {case}: m={m} nnz={nnz}, built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        for shape in args.shapes.split(","):
            h, f = (int(x) for x in shape.split("x"))
            line = bench(args, case, graph, m, nnz, h, f, rate, per_edge)
            print(json.dumps(line), flush=True)
            t_us, t_mb = line["torch_us"], line["torch_peak_bytes"]
            table.append(f"  {case:<9}{f'{h} x {f}':>8}{m:>8}{nnz:>10}{line['edge_us']:>11.1f}{line['plain_us']:>11.1f}"
                         + (f"{t_us:>11.1f}" if t_us is not None else f"{'-':>11}")
                         + f"{line['edge_us'] - line['plain_us']:>10.1f}{line['extra_us']:>9.1f}"
                         + (f"{t_us / line['edge_us']:>9.1f}" if t_us is not None else f"{'-':>9}")
                         + f"{line['edge_peak_bytes'] / 1e6:>9.1f}"
                         + (f"{t_mb / 1e6:>9.1f}" if t_mb is not None else f"{'-':>9}") + f"{4 * nnz * h * f / 1e6:>8.1f}")
    print("\n".join(table), file=sys.stderr)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(table) + "\n")


def peak_of(step):
    """torch.cuda.max_memory_allocated of one step above what was allocated before it."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    res = step()
    torch.cuda.synchronize()
    del res
    return torch.cuda.max_memory_allocated() - base


def bench(args, case, graph, m, nnz, h, f, rate, per_edge):
    rows, row_ptr, col_ind, _, col_ptr, row_ind, val_idx, _ = graph
    gen = torch.Generator().manual_seed(5)
    attn = (torch.randn(h, f, generator=gen) * f ** -0.5).to(DEV)
    x_row, x_col, dO = (torch.randn(m, h, f, generator=gen).to(DEV) for _ in range(3))
    E = torch.randn(nnz, h, f, generator=torch.Generator(device=DEV).manual_seed(4), device=DEV) * 0.5
    want_dE = not args.no_dE

    def edge_step():
        out, mx, sm = gat.gatv2_forward_edge(attn, row_ptr, col_ind, SLOPE, x_row, x_col, E)
        return [out] + list(gat.gatv2_backward_edge(SLOPE, row_ptr, col_ind, col_ptr, row_ind, val_idx, attn, x_row, x_col, E, out,
                                                    mx, sm, dO, want_dE=want_dE))

    def plain_step():
        out, mx, sm = gat.gatv2_forward(attn, row_ptr, col_ind, SLOPE, x_row, x_col)
        return [out] + list(gat.gatv2_backward(SLOPE, row_ptr, col_ind, col_ptr, row_ind, attn, x_row, x_col, out, mx, sm, dO))

    def torch_step():
        xr, xc, a = (t.detach().requires_grad_(True) for t in (x_row, x_col, attn))
        e = E.detach().requires_grad_(want_dE)
        out = index_ops_gatv2_edge(rows, col_ind, a, SLOPE, xr, xc, e)
        grads = torch.autograd.grad(out, (xr, xc, a, e) if want_dE else (xr, xc, a), dO)
        return [out.detach()] + list(grads)

    forms = {"edge": edge_step, "plain": plain_step, "torch": torch_step}
    peaks = {"edge": peak_of(edge_step)}
    try:
        peaks["torch"] = peak_of(torch_step)
    except torch.OutOfMemoryError:
        peaks["torch"] = None
        del forms["torch"]
        torch.cuda.empty_cache()
    times = {k: [] for k in forms}
    results = {}
    for it in range(args.warmup + args.steps):
        for name, step in forms.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            res = step()
            b.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[name].append(a.elapsed_time(b) * 1e3)
            results[name] = res
            del res
    if "torch" in results:
        for x, y, what in zip(results["edge"], results["torch"], ("out", "dX_row", "dX_col", "dattn", "dE")):
            if x is not None:
                print(f"# {case} {h}x{f} max |edge - torch| {what}: {(x - y).abs().max().item():.2e} "
                      f"(max |.| {y.abs().max().item():.2e})", file=sys.stderr)
    med = {k: float(np.median(v)) for k, v in times.items()}
    return {"tool": "gatv2_edge_bench", "case": case, "m": m, "nnz": nnz, "h": h, "f": f, "steps": args.steps, "dE": want_dE,
            "edge_us": round(med["edge"], 1), "plain_us": round(med["plain"], 1),
            "torch_us": round(med["torch"], 1) if "torch" in med else None,
            "edge_peak_bytes": peaks["edge"], "torch_peak_bytes": peaks["torch"], "E_bytes": 4 * nnz * h * f,
            "extra_bytes": per_edge * nnz * h * f, "copy_GBs": round(rate, 1),
            "extra_us": round(per_edge * nnz * h * f / rate * 1e-3, 1)}


if __name__ == "__main__":
    main()
