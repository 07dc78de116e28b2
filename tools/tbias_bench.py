#!/usr/bin/env python3
"""The GT pair with a typed attention bias on the graphs of tools/typed_bench.py at 1 x 128 and 8 x 16, T = 16 and T = 512,
forward + backward by device events (warm-up first, the forms alternating step by step, medians):
  (a) tbias     fused_gtconv.gt_forward_tbias / gt_backward_tbias (dB wanted): 4 bytes of type per edge and pass, the table
                in L2
  (b) rowstats  gt_forward_rowstats / gt_backward_rowstats on the same inputs without the table: the floor
  (c) bias      GTConvFuse_bias on the materialised B[etype].t() and torch.autograd.grad: what a layer with a typed bias had
                to run before -- bias and dbias of h nnz floats, the CSC pass's gather through val_idx and autograd's
                index_add into dB.  Skipped (null) with --no-materialised
  (d) torch     the index-op formulation on B[etype] (DFGNN/layers/GT/gtconv_layer_bias.py: index_ops_mha_bias).  As (c)
Next to the times, torch.cuda.max_memory_allocated of one step of each form above what was allocated before it.
--passes: no timing table; every form runs --steps times back to back, for a `rocprofv3 --kernel-trace --stats` run of its
own that splits (a) into forward, CSR pass, CSC pass and reduction.
One JSON line per (case, shape, T) on stdout; --out appends a text table (profiles/gt_tbias_kernel_times.txt).
usage: python3 tools/tbias_bench.py [--cases cora,peptides,pattern,reddit] [--scale 0.1] [--shapes 1x128,8x16]
                                    [--types 16,512] [--steps 10] [--no-materialised] [--passes]"""
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
from DFGNN.layers import preprocess_Hyper_fw_bw, preprocess_types  # noqa: E402
from DFGNN.layers.GT.gtconv_layer_bias import index_ops_mha_bias  # noqa: E402
from DFGNN.operators.fused_gtconv import GTConvFuse_bias  # noqa: E402
from DFGNN.utils import synthetic as S  # noqa: E402

DEV = "cuda:0"
FORMS = ("tbias", "rowstats", "bias", "torch")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="cora,peptides,pattern,reddit")
    ap.add_argument("--scale", type=float, default=0.1, help="reddit only")
    ap.add_argument("--shapes", default="1x128,8x16", help="heads x per-head width, comma-separated")
    ap.add_argument("--types", default="16,512", help="table sizes T, comma-separated")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--no-materialised", action="store_true", help="forms (a) and (b) only")
    ap.add_argument("--passes", action="store_true", help="run the forms back to back for a kernel trace; no table")
    ap.add_argument("--out", default=None, help="append the text table to this file")
    args = ap.parse_args()
    table = [f"# tools/tbias_bench.py --scale {args.scale} --steps {args.steps}" + (" --no-materialised" if args.no_materialised else ""),
             "# us, median of forward + backward; MB: peak of one step above its start; bias MB = 4 h nnz; type MB = 12 h nnz,"
             " the types the three passes of (a) read (every head's workgroups read them again)",
             f"# {'case':<9}{'h x f':>8}{'T':>5}{'m':>9}{'nnz':>11}{'(a) tbias':>11}{'(b) rowstats':>14}{'(c) bias':>11}{'(d) torch':>11}"
             f"{'(a)-(b)':>10}{'(c)-(b)':>10}{'type MB':>10}{'(a) MB':>9}{'(b) MB':>9}{'(c) MB':>9}{'(d) MB':>9}{'bias MB':>9}"]
    num = lambda v, w, d=1: f"{v:>{w}.{d}f}" if v is not None else f"{'-':>{w}}"  # noqa: E731
    for case in args.cases.split(","):
        t0 = time.perf_counter()
        g = {"reddit": lambda: S.reddit_like(scale=args.scale), "cora": S.cora_like,
             "peptides": lambda: S.peptides_like(batch_size=256),
             "pattern": lambda: S.pattern_like(batch_size=256)}[case]().to(DEV)
        params = preprocess_Hyper_fw_bw(g)
        del g
        m, nnz = params[2].numel() - 1, params[3].numel()
        print(f"# {case}: m={m} nnz={nnz}, built in {time.perf_counter() - t0:.1f} s", file=sys.stderr, flush=True)
        for shape in args.shapes.split(","):
            h, f = (int(x) for x in shape.split("x"))
            for T in (int(t) for t in args.types.split(",")):
                line = bench(args, case, params, m, nnz, h, f, T)
                if line is None:
                    continue
                print(json.dumps(line), flush=True)
                us, mb = line["us"], {k: (v / 1e6 if v is not None else None) for k, v in line["peak_bytes"].items()}
                table.append(f"  {case:<9}{f'{h} x {f}':>8}{T:>5}{m:>9}{nnz:>11}{num(us['tbias'], 11)}{num(us['rowstats'], 14)}"
                             f"{num(us['bias'], 11)}{num(us['torch'], 11)}{num(us['tbias'] - us['rowstats'], 10)}"
                             f"{num(us['bias'] - us['rowstats'] if us['bias'] is not None else None, 10)}"
                             f"{12 * nnz * h / 1e6:>10.1f}{num(mb['tbias'], 9)}"
                             f"{num(mb['rowstats'], 9)}{num(mb['bias'], 9)}{num(mb['torch'], 9)}{4 * nnz * h / 1e6:>9.1f}")
    if args.passes:
        return
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


def bench(args, case, params, m, nnz, h, f, T):
    _, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem = params
    assert gt.gt_tbias_dB_supported(T, h), (T, h)
    Q, K, V = S.gt_features(m, h, f, seed=5, device=DEV)
    dO = torch.randn(m, h, f, generator=torch.Generator().manual_seed(3)).to(DEV)
    gen = torch.Generator(device=DEV).manual_seed(4)
    B = torch.randn(T, h, generator=gen, device=DEV)
    etype, etype_csc = preprocess_types(params, torch.randint(0, T, (nnz,), generator=gen, device=DEV), T)

    def tbias_step():
        out, mx, sm = gt.gt_forward_tbias(row_ptr, col_ind, val, etype, B, Q, K, V)
        return [out] + list(gt.gt_backward_tbias(row_ptr, col_ind, val, etype, col_ptr, row_ind, val_idx, etype_csc, B, Q, K, V,
                                                 out, mx, sm, dO))

    def rowstats_step():
        out, mx, sm = gt.gt_forward_rowstats(row_ptr, col_ind, val, Q, K, V)
        return [out] + list(gt.gt_backward_rowstats(row_ptr, col_ind, val, col_ptr, row_ind, val_idx, Q, K, V, out, mx, sm, dO))

    def bias_step():
        q, k, v, b = (t.detach().requires_grad_(True) for t in (Q, K, V, B))
        out = GTConvFuse_bias(rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem, q, k, v,
                              b[etype.long()].t().contiguous())
        return [out.detach()] + list(torch.autograd.grad(out, (q, k, v, b), dO))

    def torch_step():
        q, k, v, b = (t.detach().requires_grad_(True) for t in (Q, K, V, B))
        out = index_ops_mha_bias(rows, col_ind, val, q, k, v, b[etype.long()])
        return [out.detach()] + list(torch.autograd.grad(out, (q, k, v, b), dO))

    forms = {"tbias": tbias_step, "rowstats": rowstats_step}
    if not args.no_materialised:
        forms.update(bias=bias_step, torch=torch_step)
    if args.passes:
        for name, step in forms.items():
            for _ in range(args.steps):
                step()
            torch.cuda.synchronize()
        return None
    peaks = {"bias": None, "torch": None}
    for name in list(forms):
        try:
            peaks[name] = peak_of(forms[name])
        except torch.OutOfMemoryError:
            del forms[name]
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
    for other in ("bias", "torch"):
        if other in results:
            for x, y, what in zip(results["tbias"], results[other], ("out", "dQ", "dK", "dV", "dB")):
                print(f"# {case} {h}x{f} T={T} max |tbias - {other}| {what}: {(x - y).abs().max().item():.2e} "
                      f"(max |.| {y.abs().max().item():.2e})", file=sys.stderr)
    med = {k: (round(float(np.median(times[k])), 1) if k in times else None) for k in FORMS}
    return {"tool": "tbias_bench", "case": case, "m": m, "nnz": nnz, "h": h, "f": f, "T": T, "steps": args.steps, "us": med,
            "peak_bytes": peaks, "bias_bytes": 4 * nnz * h,
            "ws_bytes": 4 * int(gt._n.lib().dfgnn_gt_tbias_bwd_ws_floats(T, h))}


if __name__ == "__main__":
    main()
