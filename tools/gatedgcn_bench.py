#!/usr/bin/env python3
"""The fused GatedGCN pair (fused_gtconv.gatedgcn_forward / gatedgcn_backward, csrc/gatedgcn_train.hip) against the
index-op branch (DFGNN/layers/GatedGCN: index_ops_gatedgcn + torch.autograd.grad) on the same inputs: the PATTERN-like and
Peptides-like batches (bs 256), the cora-like graph and the reddit-like graph at --scale (0.1), at 1 x 128 and 8 x 16, in
four configurations:
  full        E, Z, G and dE, normalize           (the Dwivedi / GraphGPS layer inside a stack)
  lean        none of the four, normalize
  full_plain  E, Z, G and dE, no normalisation
  plain       none of the four, no normalisation  (PyG's ResGatedGraphConv)
Per configuration, by device events (warm-up first, the two branches alternating step by step, medians): the fused forward
call, the fused backward call, the whole fused step and the whole index-op step; the backward's two kernels (CSR pass, CSC
pass) from a torch.profiler trace of the same calls (null where the profiler reports no kernels); the peak of allocated
memory of one step of either branch above what was allocated before it; and next to each pass the bytes it MUST move -- the
per-edge streams once (forward: E in, Z out; CSR pass: E, G in, dE out; CSC pass: E, G in) plus every node-sized array it
reads or writes once -- with the time those bytes take at the device-to-device copy rate measured here the way bench.py does.
The index-op branch is skipped (null) where it does not fit in memory.

The driver starts one child process per (case, shape) under its own time limit and stops at the first one that fails; a
child prints one JSON line per configuration.  --out appends the lines to a file (profiles/gatedgcn_bench.jsonl).
usage: python3 tools/gatedgcn_bench.py [--cases pattern,peptides,cora,reddit] [--scale 0.1] [--shapes 1x128,8x16] [--steps 10]"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
CONFIGS = {"full": (True, True), "lean": (False, True), "full_plain": (True, False), "plain": (False, False)}   # (edge arrays, normalize)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="pattern,peptides,cora,reddit")
    ap.add_argument("--scale", type=float, default=0.1, help="reddit only: the per-edge arrays and the index-op form fit at 0.1")
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
    rate = copy_rate_gbs(torch)
    for name, (edge, normalize) in CONFIGS.items():
        print(json.dumps(bench(torch, args, case, name, edge, normalize, graph, m, nnz, h, f, rate)), flush=True)
    return 0


def copy_rate_gbs(torch, n_bytes=1 << 28):
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


def bench(torch, args, case, name, edge, normalize, graph, m, nnz, h, f, rate):
    import numpy as np

    import fused_gtconv as gt
    from DFGNN.layers import index_ops_gatedgcn
    rows, row_ptr, col_ind, _, col_ptr, row_ind, val_idx, _ = graph
    gen = lambda s: torch.Generator(device=DEV).manual_seed(s)  # noqa: E731
    X_row, X_col, V, dO = (torch.randn(m, h, f, generator=gen(s), device=DEV) for s in (1, 2, 3, 4))
    E = torch.randn(nnz, h, f, generator=gen(5), device=DEV) if edge else None
    G = torch.randn(nnz, h, f, generator=gen(6), device=DEV) * 0.25 if edge else None

    def fwd():
        return gt.gatedgcn_forward(row_ptr, col_ind, X_row, X_col, V, E, normalize, 1e-6, need_Z=edge)

    def bwd(out, den):
        return gt.gatedgcn_backward(row_ptr, col_ind, col_ptr, row_ind, val_idx, X_row, X_col, V, E, out, den, dO, G=G,
                                    normalize=normalize, eps=1e-6, need_dE=edge)

    def fused_step():
        out, den, Z = fwd()
        return [out, Z] + list(bwd(out, den))

    def torch_step():
        leaves = [t.detach().requires_grad_(True) for t in (X_row, X_col, V) + ((E,) if edge else ())]
        out, z = index_ops_gatedgcn(rows, col_ind, *leaves[:3], leaves[3] if edge else None, normalize, 1e-6)
        grads = torch.autograd.grad((out, z) if edge else out, leaves, (dO, G) if edge else dO)
        return [out.detach(), z.detach() if edge else None] + list(grads) + ([] if edge else [None])

    def peak_of(step):
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res = step()
        torch.cuda.synchronize()
        del res
        return torch.cuda.max_memory_allocated() - base

    forms = {"fused": fused_step, "torch": torch_step}
    fused_step()
    peaks = {"fused": peak_of(fused_step)}
    try:
        torch_step()
        peaks["torch"] = peak_of(torch_step)
    except torch.OutOfMemoryError:
        peaks["torch"] = None
        del forms["torch"]
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
        out, den, Z = fwd()
        b.record()
        res = bwd(out, den)
        c.record()
        torch.cuda.synchronize()
        del res, Z
        if it >= args.warmup:
            times["fwd"].append(a.elapsed_time(b) * 1e3)
            times["bwd"].append(b.elapsed_time(c) * 1e3)
    if "torch" in results:
        for x, y, what in zip(results["fused"], results["torch"], ("out", "Z", "dX_row", "dX_col", "dV", "dE")):
            if x is not None:
                print(f"# {case} {h}x{f} {name} max |fused - torch| {what}: {(x - y).abs().max().item():.2e} "
                      f"(max |.| {y.abs().max().item():.2e})", file=sys.stderr)
    passes = pass_times(torch, fused_step, args.steps)
    med = {k: float(np.median(v)) for k, v in times.items()}
    node, edge_arr = 4 * m * h * f, 4 * nnz * h * f if edge else 0
    # node-sized arrays a pass reads or writes once.  forward: X_row, X_col, V in, out, den out.  CSR pass: X_row, X_col, V, dO
    # in, dX_row out (+ out, den in, the scratch out with normalize).  CSC pass: X_row, X_col, V, dO or the scratch in, dX_col,
    # dV out (+ out in with normalize)
    must = {"fwd": 5 * node + 2 * edge_arr, "csr": (8 if normalize else 5) * node + 3 * edge_arr,
            "csc": (7 if normalize else 6) * node + 2 * edge_arr}
    at_rate = {k: v / rate * 1e-3 for k, v in must.items()}        # us
    r = {"tool": "gatedgcn_bench", "case": case, "config": name, "m": m, "nnz": nnz, "h": h, "f": f, "steps": args.steps,
         "edge_arrays": edge, "normalize": normalize,
         "fused_us": round(med["fused"], 1), "torch_us": round(med["torch"], 1) if "torch" in med else None,
         "torch_over_fused": round(med["torch"] / med["fused"], 2) if "torch" in med else None,
         "fwd_us": round(med["fwd"], 1), "fwd_must_bytes": must["fwd"], "fwd_must_us": round(at_rate["fwd"], 1),
         "bwd_us": round(med["bwd"], 1), "bwd_must_bytes": must["csr"] + must["csc"],
         "bwd_must_us": round(at_rate["csr"] + at_rate["csc"], 1),
         "fwd_kernel_us": passes.get(0), "csr_kernel_us": passes.get(1), "csr_must_bytes": must["csr"],
         "csr_must_us": round(at_rate["csr"], 1), "csc_kernel_us": passes.get(2), "csc_must_bytes": must["csc"],
         "csc_must_us": round(at_rate["csc"], 1),
         "fused_peak_bytes": peaks["fused"], "torch_peak_bytes": peaks["torch"], "edge_array_bytes": 4 * nnz * h * f,
         "copy_GBs": round(rate, 1)}
    return r


def pass_times(torch, step, steps):
    """{pass: median us} of the kernels gatedgcn_*_kernel<..., PASS> (0 forward, 1 CSR pass, 2 CSC pass) over `steps` fused
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
            hit = re.search(r"gatedgcn_(?:wave|group)_kernel<.*,\s*(\d)>", e.name)
            if hit:
                found.setdefault(int(hit.group(1)), []).append(e.device_time if hasattr(e, "device_time") else e.cuda_time)
        return {k: round(float(np.median(v)), 1) for k, v in found.items()}
    except Exception as err:   # (a profiler that cannot start leaves the event times above as they are)
        print(f"# pass times unavailable: {type(err).__name__}: {err}", file=sys.stderr)
        return {}


if __name__ == "__main__":
    sys.exit(main())
