#!/usr/bin/env python3
"""The GT pair with a per-edge multiplicative gate and an edge output on three graphs at 1 x 128 and 8 x 16, forward +
backward by device events (warm-up first, the forms alternating step by step, medians):
  (a) gate      fused_gtconv.gt_forward_gate / gt_backward_gate with W, G and dE
  (b) lean      the same pair with none of the three (E frozen, no edge output)
  (c) edge      the additive pair gt_forward_edge / gt_backward_edge with dE on the same graph: the nearest existing kernel
  (d) torch     the index-op formulation (DFGNN/layers/GT/gtconv_layer_gate.py: index_ops_mha_gate) and
                torch.autograd.grad of (out, W) with (dO, G): what such a layer had to run before.  Skipped (null) where it
                does not fit in memory
(a) is also timed pass by pass -- the forward call, and the backward call with its two passes -- and each set against the
per-edge bytes it must move at the device-to-device copy rate measured here the way bench.py does: the forward reads E and
writes W (8 nnz h f), the CSR pass reads E and G and writes dE (12 nnz h f), the CSC pass gathers E and G (8 nnz h f): 28 in
all, against the additive pair's 16.  Next to the times, torch.cuda.max_memory_allocated of one step of (a), (b) and (d)
above what was allocated before it, and 4 nnz h f.
One JSON line per (case, shape) on stdout; --out appends a text table (profiles/gt_gate_kernel_times.txt).
usage: python3 tools/gate_bench.py [--cases pattern,cora,reddit] [--scale 0.1] [--shapes 1x128,8x16] [--steps 10]"""
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
from DFGNN.layers.GT.gtconv_layer_gate import index_ops_mha_gate  # noqa: E402
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
    ap.add_argument("--cases", default="pattern,cora,reddit")
    ap.add_argument("--scale", type=float, default=0.1, help="reddit only: the per-edge arrays and the index-op form fit at 0.1")
    ap.add_argument("--shapes", default="1x128,8x16", help="heads x per-head width, comma-separated")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="append the text table to this file")
    args = ap.parse_args()
    rate = copy_rate_gbs()
    table = [f"# tools/gate_bench.py --scale {args.scale} --steps {args.steps}; device-to-device copy rate {rate:.0f} GB/s",
             "# us, median of forward + backward; fwd / bwd: the two calls of (a) alone, x: their time over the copy-rate time of",
             "# 8 / 20 nnz h f bytes; MB: peak of one step above its start",
             f"# {'case':<9}{'h x f':>8}{'m':>8}{'nnz':>10}{'(a) gate':>10}{'(b) lean':>10}{'(c) edge':>10}{'(d) torch':>11}"
             f"{'(d)/(a)':>9}{'(a)/(c)':>9}{'fwd':>9}{'x':>6}{'bwd':>9}{'x':>6}{'(a) MB':>9}{'(b) MB':>9}{'(d) MB':>9}{'E MB':>8}"]
    for case in args.cases.split(","):
        t0 = time.perf_counter()
        g = {"reddit": lambda: S.reddit_like(scale=args.scale), "cora": S.cora_like,
             "pattern": lambda: S.pattern_like(batch_size=256)}[case]().to(DEV)
        graph = preprocess_Hyper_fw_bw(g)[1:]
        del g
        m, nnz = graph[1].numel() - 1, graph[2].numel()
        print(f"# {case}: m={m} nnz={nnz}, built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        for shape in args.shapes.split(","):
            h, f = (int(x) for x in shape.split("x"))
            r = bench(args, case, graph, m, nnz, h, f, rate)
            print(json.dumps(r), flush=True)
            t_us, t_mb = r["torch_us"], r["torch_peak_bytes"]
            table.append(f"  {case:<9}{f'{h} x {f}':>8}{m:>8}{nnz:>10}{r['gate_us']:>10.1f}{r['lean_us']:>10.1f}{r['edge_us']:>10.1f}"
                         + (f"{t_us:>11.1f}{t_us / r['gate_us']:>9.1f}" if t_us is not None else f"{'-':>11}{'-':>9}")
                         + f"{r['gate_us'] / r['edge_us']:>9.2f}{r['fwd_us']:>9.1f}{r['fwd_x_copy']:>6.2f}{r['bwd_us']:>9.1f}"
                         + f"{r['bwd_x_copy']:>6.2f}{r['gate_peak_bytes'] / 1e6:>9.1f}{r['lean_peak_bytes'] / 1e6:>9.1f}"
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
    E = 1 + torch.randn(nnz, h, f, generator=torch.Generator(device=DEV).manual_seed(4), device=DEV) * 0.5
    G = torch.randn(nnz, h, f, generator=torch.Generator(device=DEV).manual_seed(6), device=DEV) * 0.25
    E_add = E - 1                                              # the additive pair's E, of the size tools/edge_bench.py uses

    def gate_fwd():
        return gt.gt_forward_gate(row_ptr, col_ind, val, E, Q, K, V)

    def gate_bwd(out, mx, sm):
        return gt.gt_backward_gate(row_ptr, col_ind, val, E, col_ptr, row_ind, val_idx, Q, K, V, out, mx, sm, dO, G=G)

    def gate_step():
        out, mx, sm, W = gate_fwd()
        return [out, W] + list(gate_bwd(out, mx, sm))

    def lean_step():
        out, mx, sm, _ = gt.gt_forward_gate(row_ptr, col_ind, val, E, Q, K, V, need_W=False)
        return [out] + list(gt.gt_backward_gate(row_ptr, col_ind, val, E, col_ptr, row_ind, val_idx, Q, K, V, out, mx, sm, dO,
                                                need_dE=False))[:3]

    def edge_step():
        out, mx, sm = gt.gt_forward_edge(row_ptr, col_ind, val, E_add, Q, K, V)
        return [out] + list(gt.gt_backward_edge(row_ptr, col_ind, val, E_add, col_ptr, row_ind, val_idx, Q, K, V, out, mx, sm, dO))

    def torch_step():
        q, k, v, e = (t.detach().requires_grad_(True) for t in (Q, K, V, E))
        out, w = index_ops_mha_gate(rows, col_ind, val, q, k, v, e)
        dq, dk, dv, de = torch.autograd.grad((out, w), (q, k, v, e), (dO, G))
        return [out.detach(), w.detach(), dq, dk, dv, de]

    forms = {"gate": gate_step, "lean": lean_step, "edge": edge_step, "torch": torch_step}
    peaks = {"gate": peak_of(gate_step), "lean": peak_of(lean_step)}
    try:
        peaks["torch"] = peak_of(torch_step)
    except torch.OutOfMemoryError:
        peaks["torch"] = None
        del forms["torch"]
        torch.cuda.empty_cache()
    times = {k: [] for k in list(forms) + ["fwd", "bwd"]}
    results = {}
    ev = lambda: torch.cuda.Event(enable_timing=True)  # noqa: E731
    for it in range(args.warmup + args.steps):
        for name, step in forms.items():
            a, b = ev(), ev()
            a.record()
            res = step()
            b.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                times[name].append(a.elapsed_time(b) * 1e3)
            results[name] = res
            del res
        a, b, c = ev(), ev(), ev()                             # (a) once more, call by call
        a.record()
        out, mx, sm, W = gate_fwd()
        b.record()
        res = gate_bwd(out, mx, sm)
        c.record()
        torch.cuda.synchronize()
        del res, W
        if it >= args.warmup:
            times["fwd"].append(a.elapsed_time(b) * 1e3)
            times["bwd"].append(b.elapsed_time(c) * 1e3)
    if "torch" in results:
        for x, y, what in zip(results["gate"], results["torch"], ("out", "W", "dQ", "dK", "dV", "dE")):
            print(f"# {case} {h}x{f} max |gate - torch| {what}: {(x - y).abs().max().item():.2e} "
                  f"(max |.| {y.abs().max().item():.2e})", file=sys.stderr)
    med = {k: float(np.median(v)) for k, v in times.items()}
    unit_us = 4 * nnz * h * f / rate * 1e-3                    # copy-rate time of one per-edge array
    return {"tool": "gate_bench", "case": case, "m": m, "nnz": nnz, "h": h, "f": f, "steps": args.steps,
            "gate_us": round(med["gate"], 1), "lean_us": round(med["lean"], 1), "edge_us": round(med["edge"], 1),
            "torch_us": round(med["torch"], 1) if "torch" in med else None,
            "fwd_us": round(med["fwd"], 1), "bwd_us": round(med["bwd"], 1),
            "fwd_x_copy": round(med["fwd"] / (2 * unit_us), 2), "bwd_x_copy": round(med["bwd"] / (5 * unit_us), 2),
            "gate_peak_bytes": peaks["gate"], "lean_peak_bytes": peaks["lean"], "torch_peak_bytes": peaks["torch"],
            "E_bytes": 4 * nnz * h * f, "copy_GBs": round(rate, 1)}


if __name__ == "__main__":
    main()
