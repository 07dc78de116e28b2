#!/usr/bin/env python3
"""The GT pair with per-edge feature vectors in keys and values on four graphs at 1 x 128 and 8 x 16, forward + backward by
device events (warm-up first, the forms alternating step by step, medians):
  (a) edge      fused_gtconv.gt_forward_edge / gt_backward_edge (dE wanted)
  (b) rowstats  gt_forward_rowstats / gt_backward_rowstats on the same inputs without E: the floor
  (c) torch     the index-op formulation with E (DFGNN/layers/GT/gtconv_layer_edge.py: index_ops_mha_edge) and
                torch.autograd.grad: what a layer with edge features had to run before.  Skipped (null) where it does not
                fit in memory
and (a) - (b) set against the bytes E moves -- 4 nnz h f read in the forward, read and written (dE) in the CSR pass,
gathered in the CSC pass: 16 nnz h f -- at the device-to-device copy rate measured here the way bench.py does.  Next to the
times, torch.cuda.max_memory_allocated of one step of (a) and of (c) above what was allocated before it, and 4 nnz h f.
One JSON line per (case, shape) on stdout; --out appends a text table (profiles/gt_edge_kernel_times.txt).
usage: python3 tools/edge_bench.py [--cases cora,peptides,pattern,reddit] [--scale 0.1] [--shapes 1x128,8x16] [--steps 10]"""
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
from DFGNN.layers.GT.gtconv_layer_edge import index_ops_mha_edge  # noqa: E402
from DFGNN.utils import synthetic as S  # noqa: E402

DEV = "cuda:0"


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
    ap.add_argument("--out", default=None, help="append the text table to this file")
    args = ap.parse_args()
    rate = copy_rate_gbs()
    table = [f"# tools/edge_bench.py --scale {args.scale} --steps {args.steps}; device-to-device copy rate {rate:.0f} GB/s",
             "# us, median of forward + backward; extra = 16 nnz h f bytes / copy rate; MB: peak of one step above its start",
             f"# {'case':<9}{'h x f':>8}{'m':>8}{'nnz':>10}{'(a) edge':>11}{'(b) rowstats':>14}{'(c) torch':>11}"
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
            line = bench(args, case, graph, m, nnz, h, f, rate)
            print(json.dumps(line), flush=True)
            t_us, t_mb = line["torch_us"], line["torch_peak_bytes"]
            table.append(f"  {case:<9}{f'{h} x {f}':>8}{m:>8}{nnz:>10}{line['edge_us']:>11.1f}{line['rowstats_us']:>14.1f}"
                         + (f"{t_us:>11.1f}" if t_us is not None else f"{'-':>11}")
                         + f"{line['edge_us'] - line['rowstats_us']:>10.1f}{line['extra_us']:>9.1f}"
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


def bench(args, case, graph, m, nnz, h, f, rate):
    rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem = graph
    Q, K, V = S.gt_features(m, h, f, seed=5, device=DEV)
    dO = torch.randn(m, h, f, generator=torch.Generator().manual_seed(3)).to(DEV)
    E = torch.randn(nnz, h, f, generator=torch.Generator(device=DEV).manual_seed(4), device=DEV) * 0.5

    def edge_step():
        out, mx, sm = gt.gt_forward_edge(row_ptr, col_ind, val, E, Q, K, V)
        return [out] + list(gt.gt_backward_edge(row_ptr, col_ind, val, E, col_ptr, row_ind, val_idx, Q, K, V, out, mx, sm, dO))

    def rowstats_step():
        out, mx, sm = gt.gt_forward_rowstats(row_ptr, col_ind, val, Q, K, V)
        return [out] + list(gt.gt_backward_rowstats(row_ptr, col_ind, val, col_ptr, row_ind, val_idx, Q, K, V, out, mx, sm, dO))

    def torch_step():
        q, k, v, e = (t.detach().requires_grad_(True) for t in (Q, K, V, E))
        out = index_ops_mha_edge(rows, col_ind, val, q, k, v, e)
        dq, dk, dv, de = torch.autograd.grad(out, (q, k, v, e), dO)
        return [out.detach(), dq, dk, dv, de]

    forms = {"edge": edge_step, "rowstats": rowstats_step, "torch": torch_step}
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
        for x, y, what in zip(results["edge"], results["torch"], ("out", "dQ", "dK", "dV", "dE")):
            print(f"# {case} {h}x{f} max |edge - torch| {what}: {(x - y).abs().max().item():.2e} "
                  f"(max |.| {y.abs().max().item():.2e})", file=sys.stderr)
    med = {k: float(np.median(v)) for k, v in times.items()}
    return {"tool": "edge_bench", "case": case, "m": m, "nnz": nnz, "h": h, "f": f, "steps": args.steps,
            "edge_us": round(med["edge"], 1), "rowstats_us": round(med["rowstats"], 1),
            "torch_us": round(med["torch"], 1) if "torch" in med else None,
            "edge_peak_bytes": peaks["edge"], "torch_peak_bytes": peaks["torch"], "E_bytes": 4 * nnz * h * f,
            "extra_bytes": 16 * nnz * h * f, "copy_GBs": round(rate, 1), "extra_us": round(16 * nnz * h * f / rate * 1e-3, 1)}


if __name__ == "__main__":
    main()
