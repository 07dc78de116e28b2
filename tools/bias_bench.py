#!/usr/bin/env python3
"""The GT pair with a per-edge additive attention bias on three graphs at 1 and 8 heads, forward + backward by device
events (warm-up first, the forms alternating step by step, medians):
  (a) bias      fused_gtconv.gt_forward_bias / gt_backward_bias (dbias wanted)
  (b) rowstats  gt_forward_rowstats / gt_backward_rowstats on the same inputs without the bias: the floor
  (c) torch     the index-op formulation with the bias (DFGNN/layers/GT/gtconv_layer_bias.py: index_ops_mha_bias) and
                torch.autograd.grad: what a layer with an attention bias had to run before
and (a) - (b) set against the extra bytes the bias moves -- 4 h nnz read in the forward, 4 h nnz read + 4 h nnz written in
the CSR pass, 4 h nnz gathered in the CSC pass -- at the device-to-device copy rate measured here the way bench.py does.
One JSON line per (case, shape) on stdout; --out appends a text table (profiles/gt_bias_kernel_times.txt).
usage: python3 tools/bias_bench.py [--cases reddit,cora,peptides] [--scale 0.1] [--shapes 1x128,8x16] [--steps 10]"""
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
from DFGNN.layers.GT.gtconv_layer_bias import index_ops_mha_bias  # noqa: E402
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
    ap.add_argument("--cases", default="reddit,cora,peptides")
    ap.add_argument("--scale", type=float, default=0.1, help="reddit only")
    ap.add_argument("--shapes", default="1x128,8x16", help="heads x per-head width, comma-separated")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="append the text table to this file")
    args = ap.parse_args()
    rate = copy_rate_gbs()
    table = [f"# tools/bias_bench.py --scale {args.scale} --steps {args.steps}; device-to-device copy rate {rate:.0f} GB/s",
             "# us, median of forward + backward; extra = 16 h nnz bytes / copy rate",
             f"# {'case':<9}{'h x f':>8}{'m':>8}{'nnz':>10}{'(a) bias':>11}{'(b) rowstats':>14}{'(c) torch':>11}"
             f"{'(a)-(b)':>9}{'extra':>8}{'(c)/(a)':>9}"]
    for case in args.cases.split(","):
        t0 = time.perf_counter()
        g = {"reddit": lambda: S.reddit_like(scale=args.scale), "cora": S.cora_like,
             "peptides": lambda: S.peptides_like(batch_size=256)}[case]().to(DEV)
        graph = preprocess_Hyper_fw_bw(g)[1:]
        del g
        m, nnz = graph[1].numel() - 1, graph[2].numel()
        print(f"# {case}: m={m} nnz={nnz}, built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        for shape in args.shapes.split(","):
            h, f = (int(x) for x in shape.split("x"))
            line = bench(args, case, graph, m, nnz, h, f, rate)
            print(json.dumps(line), flush=True)
            table.append(f"  {case:<9}{f'{h} x {f}':>8}{m:>8}{nnz:>10}{line['bias_us']:>11.1f}{line['rowstats_us']:>14.1f}"
                         f"{line['torch_us']:>11.1f}{line['bias_us'] - line['rowstats_us']:>9.1f}{line['extra_us']:>8.1f}"
                         f"{line['torch_us'] / line['bias_us']:>9.1f}")
    print("\n".join(table), file=sys.stderr)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write("\n".join(table) + "\n")


def bench(args, case, graph, m, nnz, h, f, rate):
    rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem = graph
    Q, K, V = S.gt_features(m, h, f, seed=5, device=DEV)
    dO = torch.randn(m, h, f, generator=torch.Generator().manual_seed(3)).to(DEV)
    edge_bias = torch.randn(nnz, h, generator=torch.Generator().manual_seed(4)).to(DEV)       # [nnz, h], as a layer has it
    bias = edge_bias.t().contiguous()

    def bias_step():
        out, mx, sm = gt.gt_forward_bias(row_ptr, col_ind, val, bias, Q, K, V)
        return [out] + list(gt.gt_backward_bias(row_ptr, col_ind, val, bias, col_ptr, row_ind, val_idx, Q, K, V, out, mx, sm, dO))

    def rowstats_step():
        out, mx, sm = gt.gt_forward_rowstats(row_ptr, col_ind, val, Q, K, V)
        return [out] + list(gt.gt_backward_rowstats(row_ptr, col_ind, val, col_ptr, row_ind, val_idx, Q, K, V, out, mx, sm, dO))

    def torch_step():
        q, k, v, b = (t.detach().requires_grad_(True) for t in (Q, K, V, edge_bias))
        out = index_ops_mha_bias(rows, col_ind, val, q, k, v, b)
        dq, dk, dv, db = torch.autograd.grad(out, (q, k, v, b), dO)
        return [out.detach(), dq, dk, dv, db.t()]

    forms = {"bias": bias_step, "rowstats": rowstats_step, "torch": torch_step}
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
    for x, y, what in zip(results["bias"], results["torch"], ("out", "dQ", "dK", "dV", "dbias")):
        print(f"# {case} {h}x{f} max |bias - torch| {what}: {(x - y).abs().max().item():.2e} (max |.| {y.abs().max().item():.2e})",
              file=sys.stderr)
    med = {k: float(np.median(v)) for k, v in times.items()}
    return {"tool": "bias_bench", "case": case, "m": m, "nnz": nnz, "h": h, "f": f, "steps": args.steps,
            "bias_us": round(med["bias"], 1), "rowstats_us": round(med["rowstats"], 1), "torch_us": round(med["torch"], 1),
            "extra_bytes": 16 * h * nnz, "copy_GBs": round(rate, 1), "extra_us": round(16 * h * nnz / rate * 1e-3, 1)}


if __name__ == "__main__":
    main()
