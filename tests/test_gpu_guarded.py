"""Every C entry that takes a stream, called through the C ABI with raw pointers into guarded buffers (tests/guarded.py): after
each call the return code is 0, every guard of every array is untouched, every output element was written and is finite,
every input is what was copied in; then every output is held against the float64 reference of its operation and, at the
default alignment, is bit-identical to what the Python binding returns on the same inputs -- the kernels are deterministic,
so the torch.empty results the rest of the suite reads on these shapes were complete.  Table, cases, argument builder and the
bound: tests/guarded_cases.py; tests/test_guarded_host.py holds the table against include/dfgnn.h.

Family A: the eleven any-graph pairs, square and *_rect entries, training forward / inference / backward with every optional
argument and output (`full`) and with none (`min`), weighted and unit edge values, every width, and one float off a 16-byte
boundary (shift = 1: another lane layout runs, so the reference check only); and every pair on constructed boundary-degree
cases under its fp32-level bound (MARGIN x the float32 formulation's error; on the random graphs the pairs' own 1e-3 bar is
the bound and that figure is printed).  At the default alignment every entry must have been compared with the binding; an
entry that refuses a width must have written nothing.  Family B: the `hyper` path with and without a
plan (LDS-resident ranges, ranges whose per-edge values live in scratch, spilled ranges, the general kernels), the ranked pair,
every inference variant, the chunked tiling, the general GAT training pair -- on constructed boundary cases of
tests/parity_cases.py under their fp32-level bounds, and on block-diagonal batches under test_gpu_parity.py's bar.  Family C:
the preprocessing and the plan build, bit-exact.

Each test prints (pytest -s), per entry: the worst measured error over its outputs with its bound, the number of guarded
buffers, and whether the outputs were bit-identical to the binding's."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import guarded_cases as gc
import parity_cases as pc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
ATOL = RTOL = 1e-3                           # tests/test_gpu_parity.py's bar, for the batches of family B
GRAPH_KEYS = ("row_ptr", "col_ind", "rows", "col_ptr", "row_ind", "val_idx")


def _lib():
    import dfgnn_native
    return dfgnn_native.lib()


def _stream():
    from _binding_util import stream_ptr
    return stream_ptr(torch.device(DEV))


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    return t.detach().cpu().numpy()


class _Log:
    """What one entry did over a test: worst error / bound ratio, buffers, bit-identity; printed at the end."""

    def __init__(self):
        self.rows, self.fp32 = {}, {}

    def add(self, entry, name, err, bound, buffers):
        r = self.rows.setdefault(entry, dict(calls=0, buffers=0, worst=(0.0, 0.0, "-"), bits=None))
        r["calls"] += 1
        r["buffers"] += buffers
        if name is not None and (r["worst"][2] == "-" or err * r["worst"][1] > r["worst"][0] * bound):
            r["worst"] = (err, bound, name)

    def bits(self, entry, same):
        r = self.rows[entry]
        r["bits"] = same if r["bits"] is None else (r["bits"] and same)

    def require_bits(self, *uncompared):
        """At the default alignment every entry has been compared with the binding at least once, but for `uncompared`."""
        missing = sorted(e for e, r in self.rows.items() if r["bits"] is None and e not in uncompared)
        assert not missing, f"never compared with the binding: {missing}"

    def show(self, what):
        for name, (ratio, err, level, where) in sorted(self.fp32.items()):
            print(f"guarded {what} | fp32-level figure of {name}: {ratio:.2f} of MARGIN x the float32 formulation's error "
                  f"(measured {err:.3e}, {level:.3e}) at {where}")
        for entry, r in sorted(self.rows.items()):
            err, bound, name = r["worst"]
            ident = {None: "not compared with the binding", True: "bit-identical to the binding"}.get(r["bits"], "BITS DIFFER")
            print(f"guarded {what} | {entry}: {r['calls']} calls, {r['buffers']} guarded buffers, worst {name} measured "
                  f"{err:.3e} bound {bound:.3e}, {ident}")


def _run(call, log, missed, what, check=None, allow=()):
    """Launch, synchronise, verify -> the return code.  check(name, array) -> (error, bound) of every output."""
    code = call.run(_lib(), torch.cuda.synchronize)
    if code in allow:
        return code
    assert code == 0, (what, call.entry, code, _lib().dfgnn_error_string(code))
    worst = None
    for name, got in call.numpy().items():
        if check is None:
            continue
        err, bound = check(name, got)
        print(f"guarded {what} | {call.entry} {name}: measured {err:.3e}, bound {bound:.3e}")
        if not err <= bound:
            missed.append((what, call.entry, name, err, bound))
        if worst is None or err * worst[1] > worst[0] * bound:
            worst = (err, bound, name)
    log.add(call.entry, *(worst[2], worst[0], worst[1]) if worst else (None, 0.0, 0.0), buffers=len(call.arena))
    return code


def _same_bits(log, missed, what, entry, mine, theirs):
    """mine: Call outputs (name -> view); theirs: name -> the binding's tensor (None: not returned)."""
    for name, t in theirs.items():
        if t is None or name not in mine:
            continue
        same = tuple(t.shape) == tuple(mine[name].shape) and torch.equal(t, mine[name])
        log.bits(entry, same)
        if not same:
            missed.append((what, entry, name, "differs from the binding's bits"))


# ---- family A: the eleven any-graph pairs -----------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _pair_case(pair, kind, h, f, unit, which):
    """-> (inputs, scalars, forward omit, backward omit, float64 reference); shared, nobody writes to it."""
    g = gc.graph(kind)
    x, scal, fo, bo = gc.variant(pair, which, gc.inputs(pair, g, h, f, unit), f)
    ref32 = gc.reference(pair, g, x, scal, "f32") if pair in gc.FP32_PAIRS and g["nnz"] else None
    return x, scal, fo, bo, gc.reference(pair, g, x, scal), ref32


def _ws_numel(pair, g, h, f):
    L = _lib()
    if pair == "typed":
        return int(L.dfgnn_gt_typed_bwd_ws_floats(gc.TYPES, h, f))
    if pair == "tbias":
        return int(L.dfgnn_gt_tbias_bwd_ws_floats(gc.TYPES, h))
    if pair in ("gatv2", "gatv2_edge"):
        return int(L.dfgnn_gatv2_bwd_ws_floats(h, f))
    return g["m"] * h * f if pair == "gatedgcn" else 0


def _pair_binding(pair, d, t, scal, full):
    """The pair through the Python binding on device tensors t -> name -> tensor (the header's names; "inference")."""
    import fused_gatconv as gat
    import fused_gtconv as gt
    rp, ci, cp, ri, vi = (d[k] for k in ("row_ptr", "col_ind", "col_ptr", "row_ind", "val_idx"))
    dO, val = t["grad_out"], t.get("val")
    if pair in gc.TAKES_VAL:
        Q, K, V = t["Q"], t["K"], t["V"]
        if pair == "rowstats":
            out, mx, sm = gt.gt_forward_rowstats(rp, ci, val, Q, K, V)
            grads = dict(zip(("dQ", "dK", "dV"), gt.gt_backward_rowstats(rp, ci, val, cp, ri, vi, Q, K, V, out, mx, sm, dO)))
            return dict(out=out, row_max=mx, row_sum=sm, **grads)
        extra, gname, kw = dict(bias=((t.get("bias"),), "dbias", "need_dbias"), edge=((t.get("E"),), "dE", "need_dE"),
                                gate=((t.get("E"),), "dE", "need_dE"), typed=((t.get("etype"), t.get("R")), "dR", "need_dR"),
                                tbias=((t.get("etype"), t.get("B")), "dB", "need_dB"))[pair]
        fwd, inf, bwd = (getattr(gt, f"gt_{k}_{pair}") for k in ("forward", "inference", "backward"))
        res = {}
        if pair == "gate":
            out, mx, sm, res["W"] = fwd(rp, ci, val, *extra, Q, K, V, need_W=full)
        else:
            out, mx, sm = fwd(rp, ci, val, *extra, Q, K, V)
        res["inference"] = inf(rp, ci, val, *extra, Q, K, V)
        csc = (cp, ri, vi) + ((t["etype_csc"],) if pair in ("typed", "tbias") else ())
        tail = {kw: full}
        if pair == "gate":
            tail["G"] = t.get("G")
        args = (rp, ci, val, extra[0], *csc, *extra[1:], Q, K, V, out, mx, sm, dO)
        res.update(zip(("dQ", "dK", "dV", gname), bwd(*args, **tail)), out=out, row_max=mx, row_sum=sm)
        return res
    if pair in ("gatv2", "gatv2_edge"):
        a, xr, xc = t["attn"], t["X_row"], t["X_col"]
        if pair == "gatv2":
            out, mx, sm = gat.gatv2_forward(a, rp, ci, gc.SLOPE, xr, xc)
            inf = gat.gatv2_inference(a, rp, ci, gc.SLOPE, xr, xc)
            grads = gat.gatv2_backward(gc.SLOPE, rp, ci, cp, ri, a, xr, xc, out, mx, sm, dO) + [None]
        else:
            out, mx, sm = gat.gatv2_forward_edge(a, rp, ci, gc.SLOPE, xr, xc, t["E"])
            inf = gat.gatv2_inference_edge(a, rp, ci, gc.SLOPE, xr, xc, t["E"])
            grads = gat.gatv2_backward_edge(gc.SLOPE, rp, ci, cp, ri, vi, a, xr, xc, t["E"], out, mx, sm, dO, want_dE=full)
        return dict(zip(("dX_row", "dX_col", "dattn", "dE"), grads), out=out, row_max=mx, row_sum=sm, inference=inf)
    if pair == "agnn":
        cos = bool(scal["cosine"])
        out, mx, sm = gt.agnn_forward(rp, ci, t["beta"], t["X_row"], t["X_col"], cos)
        inf = gt.agnn_inference(rp, ci, t["beta"], t["X_row"], t["X_col"], cos)
        dxr, dxc, db = gt.agnn_backward(rp, ci, cp, ri, t["beta"], t["X_row"], t["X_col"], out, mx, sm, dO, cos, need_dbeta=full)
        return dict(out=out, row_max=mx, row_sum=sm, inference=inf, dX_row=dxr, dX_col=dxc, dbeta=db)
    if pair == "gatedgcn":
        nz, eps = bool(scal["normalize"]), scal["eps"]
        xr, xc, V, E = t["X_row"], t["X_col"], t["V"], t.get("E")
        out, den, Z = gt.gatedgcn_forward(rp, ci, xr, xc, V, E, nz, eps, need_Z=full)
        inf = gt.gatedgcn_inference(rp, ci, xr, xc, V, E, nz, eps)
        grads = gt.gatedgcn_backward(rp, ci, cp, ri, vi, xr, xc, V, E, out, den, dO, G=t.get("G"), normalize=nz, eps=eps,
                                     need_dE=full)
        return dict(zip(("dX_row", "dX_col", "dV", "dE"), grads), out=out, den=den, Z=Z, inference=inf)
    assert pair == "gat_edge"
    ar, ac, X, sc, mask, drop = t["attn_row"], t["attn_col"], t["X"], t.get("score"), t.get("edge_mask"), scal["attn_drop"]
    out, emax, esum, _ = gat.gat_forward_edge(ar, ac, rp, ci, gc.SLOPE, X, sc, drop, mask)
    inf = gat.gat_inference_edge(ar, ac, rp, ci, gc.SLOPE, X, sc, drop, mask)
    grads = gat.gat_backward_edge(gc.SLOPE, drop, rp, ci, cp, ri, vi, ar, ac, X, emax, esum, dO, sc, mask, want_grad_score=full)
    return dict(zip(("grad_feat", "grad_attn_row", "grad_attn_col", "grad_score"), grads), out=out, edge_max=emax,
                edge_sum=esum, inference=inf)


def _run_pair(pair, kind, h, f, unit, which, shift, rects, log, missed):
    g = gc.graph(kind)
    x, scal, fo, bo, ref, ref32 = _pair_case(pair, kind, h, f, unit, which)
    what = f"{pair} {kind} h{h} f{f} {'unit' if unit else 'weighted'} {which} shift{shift}"
    base = dict(m=g["m"], n_cols=g["n_cols"], nnz=g["nnz"], h=h, f=f, stream=_stream(), ws_numel=_ws_numel(pair, g, h, f), **scal)
    base.update({k: g[k] for k in GRAPH_KEYS})
    base.update(x)
    if unit:
        base["val"] = None
    stats = gc.stats_of(pair)

    def check(name, got):
        if ref32 is not None:                                # a figure to print, not a bound (guarded_cases.fp32_level)
            err, level = gc.fp32_level(pair, g, name, got, ref[name], ref32[name])
            if level > 0 and err / level > log.fp32.get(name, (0.0,))[0]:
                log.fp32[name] = (err / level, err, level, what)
        return gc.error_and_bound(name, got, ref[name], g["deg"])
    allow = (-2,) if (h, f) in gc.EXTRA_WIDTHS else ()
    for rect in rects:
        fwd, bwd = (e + ("_rect" if rect else "") for e in gc.PAIRS[pair])
        train = gc.Call(fwd, base, DEV, shift, omit=fo)
        if _run(train, log, missed, what, check, allow) != 0:   # (Call.run has verified that the refused call wrote nothing)
            print(f"guarded {what} | {fwd}: unsupported width")
            continue
        inf = gc.Call(fwd, base, DEV, shift, omit=fo + stats + ("W", "Z"))
        _run(inf, log, missed, what + " inference", check)
        if not torch.equal(inf.outputs["out"], train.outputs["out"]):
            missed.append((what, fwd, "inference differs from the training forward's out"))
        saved = {k: v for k, v in train.numpy().items() if k in ("out",) + stats}
        if pair == "gatedgcn" and not scal["normalize"]:
            saved = {}                                       # (normalize = 0 reads neither out nor den: NULL for both)
        back = gc.Call(bwd, dict(base, **saved), DEV, shift, omit=bo)
        _run(back, log, missed, what, check)
        if shift == 0:
            t = {k: _dev(v) for k, v in x.items()}
            if unit:
                t["val"] = None
            theirs = _pair_binding(pair, {k: _dev(g[k]) for k in GRAPH_KEYS}, t, scal, which == "full")
            torch.cuda.synchronize()
            _same_bits(log, missed, what, fwd, train.outputs, theirs)
            _same_bits(log, missed, what, fwd, dict(inference=inf.outputs["out"]), theirs)
            _same_bits(log, missed, what, bwd, back.outputs, theirs)


def _pair_test(pair, kind, widths, shift, log):
    rects = (False, True) if kind in gc.SQUARE_KINDS else (True,)
    missed = []
    for h, f in widths:
        for unit in ((True, False) if pair in gc.TAKES_VAL else (True,)):
            for which in (("full", "min") if gc.has_variants(pair) else ("full",)):
                _run_pair(pair, kind, h, f, unit, which, shift, rects, log, missed)
    log.show(f"{pair} {kind} shift{shift}")
    want = {e + sfx for e in gc.PAIRS[pair] for sfx in (("", "_rect") if kind in gc.SQUARE_KINDS else ("_rect",))}
    assert set(log.rows) == want and want <= set(gc.entries_of("pair:" + pair)), sorted(log.rows)
    if shift == 0:            # (dbeta_rows itself has no counterpart: the binding returns its column sum; dX_row / dX_col do)
        log.require_bits()
    assert not missed, missed


@pytest.mark.parametrize("kind", gc.SQUARE_KINDS + gc.RECT_KINDS)
@pytest.mark.parametrize("pair", sorted(gc.PAIRS))
def test_pair(pair, kind):
    """One pair on one graph, every width: the square entry and the *_rect entry on the square graphs (the *_rect entry
    with n_cols = m: the same bits as the binding, which calls *_rect), the *_rect entry on the rectangles."""
    g = gc.graph(kind)
    form = ("lane" if gc.rc.lane_form(g["m"], g["nnz"]) else "wave", "lane" if gc.rc.lane_form(g["n_cols"], g["nnz"]) else "wave")
    print(f"guarded {pair} {kind}: {g['m']} x {g['n_cols']}, {g['nnz']} edges, rows {form[0]}, columns {form[1]}")
    _pair_test(pair, kind, gc.WIDTHS, 0, _Log())


@pytest.mark.parametrize("case", gc.BOUNDARY_CASES, ids=str)
@pytest.mark.parametrize("pair", sorted(gc.PAIRS))
def test_pair_at_fp32_level_on_boundary_degrees(oracle_mod, pair, case):
    """The fp32-level bound of every pair under guards: on the constructed boundary-degree graphs of tests/parity_cases.py
    (rows and columns of 1 ... 257 entries and the caps; wave and lane-group form, as built and transposed), with the
    inputs, float64 reference, measure and bound = MARGIN x the float32 formulation's error of the pair's own cases module
    (guarded_cases.boundary), the square entry and the *_rect entry with n_cols = m: training forward with every optional
    output, inference, backward with every optional output the case supports -- each output within its bound, and the
    binding's bits."""
    g, x, scal, ref, bounds, error_of, bo = gc.boundary(pair, case)
    m, nnz, (h, f) = g["m"], g["nnz"], x["grad_out"].shape[1:]
    assert gc.rc.lane_form(m, nnz) == case[1]
    unit = pair in gc.TAKES_VAL and bool((x["val"] == 1).all())
    what = f"{pair} boundary {case}"
    scal = dict(scal, **({"T": gc.BOUNDARY_T} if pair in ("typed", "tbias") else {}))
    ws = dict(typed=lambda L: L.dfgnn_gt_typed_bwd_ws_floats(gc.BOUNDARY_T, h, f) if not bo else 0,
              tbias=lambda L: L.dfgnn_gt_tbias_bwd_ws_floats(gc.BOUNDARY_T, h), gatv2=lambda L: L.dfgnn_gatv2_bwd_ws_floats(h, f),
              gatv2_edge=lambda L: L.dfgnn_gatv2_bwd_ws_floats(h, f), gatedgcn=lambda L: m * h * f).get(pair, lambda L: 0)(_lib())
    base = dict(m=m, n_cols=m, nnz=nnz, h=h, f=f, stream=_stream(), ws_numel=int(ws), **scal, **{k: g[k] for k in GRAPH_KEYS})
    base.update(x)
    if unit:
        base["val"] = None
    stats = gc.stats_of(pair)

    def check(name, got):
        return error_of(g, name, got.astype(np.float64), ref[name]), bounds[name]
    log, missed = _Log(), []
    for rect in (False, True):
        fwd, bwd = (e + ("_rect" if rect else "") for e in gc.PAIRS[pair])
        train = gc.Call(fwd, base, DEV)
        _run(train, log, missed, what, check)
        inf = gc.Call(fwd, base, DEV, omit=stats + ("W", "Z"))
        _run(inf, log, missed, what + " inference", check)
        if not torch.equal(inf.outputs["out"], train.outputs["out"]):
            missed.append((what, fwd, "inference differs from the training forward's out"))
        back = gc.Call(bwd, dict(base, **{k: v for k, v in train.numpy().items() if k in ("out",) + stats}), DEV, omit=bo)
        _run(back, log, missed, what, check)
        t = {k: _dev(v) for k, v in x.items()}
        if unit:
            t["val"] = None
        theirs = _pair_binding(pair, {k: _dev(g[k]) for k in GRAPH_KEYS}, t, scal, not bo)
        torch.cuda.synchronize()
        _same_bits(log, missed, what, fwd, train.outputs, theirs)
        _same_bits(log, missed, what, fwd, dict(inference=inf.outputs["out"]), theirs)
        _same_bits(log, missed, what, bwd, back.outputs, theirs)
    log.show(what)
    log.require_bits()
    assert not missed, missed


@pytest.mark.parametrize("kind", gc.SHIFT_KINDS)
@pytest.mark.parametrize("pair", sorted(gc.PAIRS))
def test_pair_one_float_off_alignment(pair, kind):
    """Every float array starts 4 bytes after a 16-byte boundary (the workspaces the header wants aligned stay aligned): the
    scalar lane layouts run where the float4 ones would, with the same guards and the same bound."""
    _pair_test(pair, kind, (gc.SHIFT_WIDTH,), 1, _Log())


def test_the_gpu_run_notices_an_unwritten_row_and_a_store_into_a_guard():
    """The run's own power on the device, without a kernel that misbehaves: dfgnn_gt_fwd_rowstats_rect is told one row
    fewer than its outputs have, so the last row of out / row_max / row_sum stays unwritten -- verify names `out` and the
    first unwritten offset; and one float stored behind `out` by the test itself is found in the guard."""
    g = gc.graph("tall")
    h, f = 2, 20
    x, scal, fo, bo, _, _ = _pair_case("rowstats", "tall", h, f, True, "full")
    case = dict(m=g["m"], n_cols=g["n_cols"], nnz=g["nnz"], h=h, f=f, stream=_stream(), **{k: g[k] for k in GRAPH_KEYS}, **x)
    m1 = g["m"] - 3                                          # rows 597 and 598 have edges, row 599 has none
    assert g["deg"][m1] > 0 and g["row_ptr"][m1] < g["nnz"]
    call = gc.Call("dfgnn_gt_fwd_rowstats_rect", case, DEV)
    args = list(call.args)
    args[0], args[2] = m1, int(g["row_ptr"][m1])             # a valid smaller problem: the first m1 rows and their edges
    assert _lib().dfgnn_gt_fwd_rowstats_rect(*args) == 0
    torch.cuda.synchronize()
    with pytest.raises(AssertionError, match=rf"^out: output element at offset {m1 * h * f} of {g['m'] * h * f} still carries"):
        call.arena.verify(outputs=["out"])
    with pytest.raises(AssertionError, match=rf"^row_sum: output element at offset {m1 * h} of "):
        call.arena.verify(outputs=["row_sum"])
    call.arena.verify(outputs=[])                            # guards and inputs are in order
    r = call.arena.records["out"]
    r.buf[r.lo + r.n + 7] = 0.0
    with pytest.raises(AssertionError, match=rf"^out: guard after the output written at offset {r.n + 7} "):
        call.arena.verify(outputs=[])


# ---- family B: the hyper path and the inference variants --------------------------------------------------------------------
GT_CASES = [(False, True, 128, 1, True), (True, True, 7, 2, False), (False, False, 32, 1, False), (True, False, 128, 1, True)]
GAT_CASES = [(False, True, 128, 1), (True, True, 7, 2), (False, False, 32, 1), (True, False, 128, 1)]


def _plan_for(g, f):
    """-> (BlockPlan | None, case entries): the plan of the graph at width f, built by the binding on plain tensors; the
    guarded calls read a copy of its buffer between guards."""
    from _binding_util import build_plan
    plan = build_plan(_dev(g["row_ptr"]), _dev(g["col_ind"]), f)
    torch.cuda.synchronize()
    return plan


def _pc_check(g, ref64, bounds, rename=None):
    rename = rename or {}

    def check(name, got):
        key = rename.get(name, name)
        if key in pc.STATS:                                  # (rows without an edge hold the sentinel; the reference 0)
            live = np.diff(g["row_ptr"]) > 0
            assert (got[~live] < -9e37).all() if key.endswith("max") else (got[~live] == 0).all(), key
            got = np.where(live[:, None], got, ref64[key])
        return pc.error_of(g, key, got.astype(np.float64), ref64[key]), bounds[key]
    return check


def _bar_check(ref):
    def check(name, got):
        err = np.abs(got.astype(np.float64) - ref[name])
        excess = err - (ATOL + RTOL * np.abs(ref[name]))
        at = int(excess.argmax()) if err.size else 0
        return (float(err.reshape(-1)[at]), float((ATOL + RTOL * np.abs(ref[name])).reshape(-1)[at])) if err.size else (0.0, 0.0)
    return check


def _grad_edge_ref(g, x, attn64):
    """dS[h, nnz] = P (dP - sum_row P dP), dP_e = <dO_i, V_j>, in float64 from the float64 attention: what dfgnn_gt_bwd_rows
    leaves in grad_edge (held to the absolute bar: the constructed cases have no fp32-level bound for it)."""
    rows = g["rows"].astype(np.int64)
    dP = (x["dO"].astype(np.float64)[rows] * x["V"].astype(np.float64)[g["col_ind"]]).sum(-1).T
    rowsum = np.zeros((dP.shape[0], g["m"]))
    for hd in range(dP.shape[0]):
        np.add.at(rowsum[hd], rows, (attn64 * dP)[hd])
    return attn64 * (dP - rowsum[:, rows])


def _gt_entries(g, x, check_rest, attn64, what, log, missed, plans):
    """Every entry of family `gt` on one graph and one set of inputs (numpy).  plans: the BlockPlans to run hyper under
    (None: the general kernels)."""
    import fused_gtconv as gt
    dS = _grad_edge_ref(g, x, attn64)
    check = lambda name, got: gc.error_and_bound(name, got, dS, None) if name == "grad_edge" else check_rest(name, got)  # noqa: E731
    m, nnz, (h, f) = g["m"], g["nnz"], x["Q"].shape[1:]
    unit = bool((x["val"] == 1).all())
    base = dict(m=m, nnz=nnz, h=h, f=f, stream=_stream(), **{k: g[k] for k in GRAPH_KEYS}, Q=x["Q"], K=x["K"], V=x["V"],
                grad_out=x["dO"], val=None if unit else x["val"])
    d = {k: _dev(g[k]) for k in GRAPH_KEYS}
    t = {k: _dev(x[k]) for k in ("val", "Q", "K", "V", "dO")}
    hyper_args = (d["row_ptr"], d["col_ind"], d["rows"], t["val"], d["col_ptr"], d["row_ind"], d["val_idx"], 1024, t["Q"], t["K"], t["V"])
    no_plan_bwd = None
    for plan in plans:
        tag = what + (" plan" if plan is not None else " no plan")
        pcase = dict(base, plan=plan.buf if plan is not None else None,
                     plan_meta=ctypes.addressof(plan._meta_c) if plan is not None else None)
        applies = plan is not None and _lib().dfgnn_plan_applies(m, nnz, h, f, pcase["plan_meta"]) == 1
        if plan is not None:
            assert applies and plan.num_fit > 0, (tag, plan.meta)
            print(f"guarded {tag}: fit {plan.num_fit}, spill {plan.num_spill}, edge-global {plan.num_edge_global}, "
                  f"dense {plan.num_dense}")
        fwd = gc.Call("dfgnn_gt_hyper_fwd", pcase, DEV, omit=("edge_ws",))
        _run(fwd, log, missed, tag, check)
        inf = gc.Call("dfgnn_gt_hyper_fwd", pcase, DEV, omit=("attn_edge",) + (() if plan is not None else ("edge_ws",)))
        _run(inf, log, missed, tag + " inference", check)
        bwd = gc.Call("dfgnn_gt_bwd", dict(pcase, attn_edge=fwd.numpy()["attn_edge"]), DEV)
        _run(bwd, log, missed, tag, check)
        gt.USE_BLOCK_PLAN = plan is not None
        try:
            out, attn = gt.gt_hyper_forward(*hyper_args)
            grads = gt.gt_backward(*hyper_args, attn, t["dO"])
            out_inf = gt.gt_hyper_inference(d["row_ptr"], d["col_ind"], d["rows"], t["val"], 1024, t["Q"], t["K"], t["V"])[0]
            used = d["row_ptr"].__dict__.get("_dfgnn_plans", {}).get(f)
            assert plan is None or (used is not None and used.meta == plan.meta), tag
        finally:
            gt.USE_BLOCK_PLAN = True
        torch.cuda.synchronize()
        _same_bits(log, missed, tag, "dfgnn_gt_hyper_fwd", fwd.outputs, dict(out=out, attn_edge=attn))
        if unit or plan is None or not gt.gt_stats_pair_applies(d["row_ptr"], d["col_ind"], t["val"], t["Q"]):
            _same_bits(log, missed, tag, "dfgnn_gt_hyper_fwd", dict(out=inf.outputs["out"]), dict(out=out_inf))
        _same_bits(log, missed, tag, "dfgnn_gt_bwd", bwd.outputs, dict(zip(("dQ", "dK", "dV"), grads)))
        if plan is None:
            no_plan_bwd, attn_np = bwd, fwd.numpy()["attn_edge"]
            if not gc.rc.lane_form(m, nnz):      # the general kernels: the rows pass leaves dS in the guarded scratch
                assert bool((bwd.arena["grad_edge"].view(torch.int32) != gc.guarded.FILL_BITS).all()), tag
    # the two passes of the plan-less backward on their own: grad_edge is the rows pass's output and the cols pass's input
    rows_pass = gc.Call("dfgnn_gt_bwd_rows", dict(base, attn_edge=attn_np), DEV, written=("grad_edge",))
    _run(rows_pass, log, missed, what, check)
    cols_pass = gc.Call("dfgnn_gt_bwd_cols", dict(base, attn_edge=attn_np, grad_edge=_np(rows_pass.outputs["grad_edge"])), DEV)
    _run(cols_pass, log, missed, what, check)
    if not gc.rc.lane_form(m, nnz):      # (below 8 edges per row dfgnn_gt_bwd takes the lane-group kernels: other bits)
        for call in (rows_pass, cols_pass):
            _same_bits(log, missed, what, call.entry, {k: v for k, v in call.outputs.items() if k != "grad_edge"},
                       no_plan_bwd.outputs)
    # the inference variants: tiling and the two-kernel forms multiply the values in as they are, the csr forms take NULL
    with_val, args = dict(base, val=x["val"]), (d["row_ptr"], d["col_ind"])
    for entry, case, theirs in (
            ("dfgnn_gt_tiling_fwd", with_val, lambda: gt.gt_tiling_inference(*args, t["val"], 128, t["Q"], t["K"], t["V"])[0]),
            ("dfgnn_gt_softmax_fwd", with_val, lambda: gt.gt_softmax_inference(*args, d["rows"], t["val"], 128, t["Q"], t["K"], t["V"])[0]),
            ("dfgnn_gt_softmax_gm_fwd", with_val, lambda: gt.gt_softmax_gm_inference(*args, d["rows"], t["val"], t["Q"], t["K"], t["V"])),
            ("dfgnn_gt_csr_fwd", base, lambda: gt.gt_csr_inference(*args, t["val"], 128, t["Q"], t["K"], t["V"])[0]),
            ("dfgnn_gt_csr_gm_fwd", base, lambda: gt.gt_csr_gm_inference(*args, t["val"], t["Q"], t["K"], t["V"])[0])):
        call = gc.Call(entry, case, DEV)
        _run(call, log, missed, what, check)
        got = theirs()
        torch.cuda.synchronize()
        _same_bits(log, missed, what, entry, call.outputs, dict(out=got))


@pytest.mark.parametrize("case", GT_CASES, ids=str)
def test_gt_family_on_boundary_cases(oracle_mod, case):
    """The lane-group and the wave form, with and without edge values, on the constructed boundary-degree graphs: every
    output within parity_cases' fp32-level bound.  Without a plan the general kernels run; the wave-form graphs also run
    under their plan."""
    g = pc.graph(case[0], case[1])
    x, ref64, _, bounds = pc.references("gt", *case)
    assert gc.rc.lane_form(g["m"], g["nnz"]) == case[1]
    plans = [None] if case[1] else [_plan_for(g, case[2]), None]
    if plans[0] is not None and (plans[0].num_fit == 0 or case[2] % 4):
        plans = [None]
    log, missed = _Log(), []
    _gt_entries(g, x, _pc_check(g, ref64, bounds), ref64["attn_edge"], f"gt {case}", log, missed, plans)
    log.show(f"gt {case}")
    assert set(log.rows) == set(gc.entries_of("gt")), sorted(log.rows)
    # (below 8 edges per row dfgnn_gt_bwd takes the lane-group kernels: the two passes have no counterpart to share bits with)
    log.require_bits(*(("dfgnn_gt_bwd_rows", "dfgnn_gt_bwd_cols") if case[1] else ()))
    assert not missed, missed


def _batch_inputs(g, h, f, unit, seed):
    rng = np.random.default_rng(seed)
    r = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    val = np.ones(g["nnz"], dtype=np.float32) if unit else rng.uniform(0.5, 1.5, g["nnz"]).astype(np.float32)
    return dict(val=val, Q=r(g["m"], h, f) * np.float32(f ** -0.25), K=r(g["m"], h, f) * np.float32(f ** -0.25), V=r(g["m"], h, f),
                dO=r(g["m"], h, f), attn_row=r(g["m"], h), attn_col=r(g["m"], h))


@pytest.mark.parametrize("f,unit", [(128, True), (256, False)])
def test_gt_family_on_a_mixed_batch(oracle_mod, f, unit):
    """A block-diagonal batch under its plan: ranges that run LDS-resident (gt_block*.hip -- at f = 128 the range with a
    duplicate edge and, with edge values, every fit range; at f = 256 every fit range: no matrix-core class), a range whose
    per-edge values live in the caller's scratch, and spilled ranges; then without a plan, the general kernels."""
    g = gc.batch_graph("mixed")
    x = _batch_inputs(g, 1, f, unit, 900 + f)
    plan = _plan_for(g, f)
    assert plan.num_fit > 0 and plan.num_spill > 0 and plan.num_dense < plan.num_fit and plan.num_edge_global > 0, plan.meta
    assert (plan.num_dense == 0) == (f == 256), plan.meta
    args = (g["row_ptr"], g["col_ind"], x["val"], x["Q"], x["K"], x["V"])
    out, attn = oracle_mod.gt_forward(*args, want_attn=True)
    dQ, dK, dV = oracle_mod.gt_backward(*args, x["dO"])
    ref = dict(out=out, attn_edge=attn, dQ=dQ, dK=dK, dV=dV)
    log, missed = _Log(), []
    _gt_entries(g, x, _bar_check(ref), attn, f"gt mixed batch f{f}", log, missed, [plan, None])
    log.show(f"gt mixed batch f{f}")
    assert set(log.rows) == set(gc.entries_of("gt")), sorted(log.rows)
    log.require_bits()
    assert not missed, missed


def test_ranked_pair_on_a_dense_batch(oracle_mod):
    """dfgnn_gt_hyper_fwd_ranked / dfgnn_gt_bwd_ranked (one head, unit values, every range dense): attn_ranked is attn_edge
    with each row's values by increasing column."""
    import fused_gtconv as gt
    g = gc.batch_graph("dense")
    h, f = 1, 64
    x = _batch_inputs(g, h, f, True, 964)
    plan = _plan_for(g, f)
    meta = ctypes.addressof(plan._meta_c)
    assert plan.num_dense == plan.num_fit > 0 and plan.num_spill == 0, plan.meta
    assert _lib().dfgnn_gt_stats_applies(g["m"], g["nnz"], h, f, meta) == 1
    args = (g["row_ptr"], g["col_ind"], x["val"], x["Q"], x["K"], x["V"])
    out, attn = oracle_mod.gt_forward(*args, want_attn=True)
    dQ, dK, dV = oracle_mod.gt_backward(*args, x["dO"])
    order = np.lexsort((g["col_ind"], g["rows"]))
    ref = dict(out=out, attn_ranked=attn[0][order], dQ=dQ, dK=dK, dV=dV)
    base = dict(m=g["m"], nnz=g["nnz"], h=h, f=f, stream=_stream(), row_ptr=g["row_ptr"], col_ind=g["col_ind"], Q=x["Q"],
                K=x["K"], V=x["V"], grad_out=x["dO"], plan=plan.buf, plan_meta=meta)
    log, missed = _Log(), []
    fwd = gc.Call("dfgnn_gt_hyper_fwd_ranked", base, DEV)
    _run(fwd, log, missed, "ranked", _bar_check(ref))
    bwd = gc.Call("dfgnn_gt_bwd_ranked", dict(base, attn_ranked=fwd.numpy()["attn_ranked"]), DEV)
    _run(bwd, log, missed, "ranked", _bar_check(ref))
    rp, ci, Q, K, V, dO = (_dev(a) for a in (g["row_ptr"], g["col_ind"], x["Q"], x["K"], x["V"], x["dO"]))
    o2, a2 = gt.gt_hyper_forward_ranked(rp, ci, Q, K, V)
    grads = gt.gt_backward_ranked(rp, ci, Q, K, V, a2, dO)
    torch.cuda.synchronize()
    _same_bits(log, missed, "ranked", fwd.entry, fwd.outputs, dict(out=o2, attn_ranked=a2.reshape(-1)))
    _same_bits(log, missed, "ranked", bwd.entry, bwd.outputs, dict(zip(("dQ", "dK", "dV"), grads)))
    log.show("ranked")
    log.require_bits()
    assert set(log.rows) == set(gc.entries_of("ranked"))
    assert not missed, missed


def _gat_entries(g, x, check, mask_check, what, log, missed, plans, monkeypatch, chunk_rows):
    import fused_gatconv as gat
    m, nnz, (h, f) = g["m"], g["nnz"], x["X"].shape[1:]
    base = dict(m=m, nnz=nnz, h=h, f=f, stream=_stream(), **{k: g[k] for k in GRAPH_KEYS}, permute=g["val_idx"],
                attn_row=x["attn_row"], attn_col=x["attn_col"], X=x["X"], grad_out=x["dO"], negative_slope=gc.SLOPE)
    d = {k: _dev(g[k]) for k in GRAPH_KEYS}
    ar, ac, X, dO = (_dev(x[k]) for k in ("attn_row", "attn_col", "X", "dO"))
    inference = lambda name, got: check("inference" if name == "out" else name, got)  # noqa: E731
    for plan in plans:
        tag = what + (" plan" if plan is not None else " no plan")
        pcase = dict(base, plan=plan.buf if plan is not None else None,
                     plan_meta=ctypes.addressof(plan._meta_c) if plan is not None else None)
        if plan is not None:
            print(f"guarded {tag}: fit {plan.num_fit}, spill {plan.num_spill}, edge-global {plan.num_edge_global}")
        call = gc.Call("dfgnn_gat_hyper_fwd", pcase, DEV, omit=() if plan is not None else ("edge_ws",))
        _run(call, log, missed, tag, inference)
        gat.USE_BLOCK_PLAN = plan is not None
        try:
            theirs = gat.gat_inference_hyper(1024, ar, ac, d["row_ptr"], d["col_ind"], d["rows"], gc.SLOPE, X)
        finally:
            gat.USE_BLOCK_PLAN = True
        torch.cuda.synchronize()
        _same_bits(log, missed, tag, call.entry, call.outputs, dict(out=theirs))
    rp, ci, rows = d["row_ptr"], d["col_ind"], d["rows"]
    for entry, theirs in (("dfgnn_gat_recompute_fwd", lambda: gat.gat_inference_hyper_recompute(ar, ac, rp, ci, gc.SLOPE, X)),
                          ("dfgnn_gat_softmax_fwd", lambda: gat.gat_inference_softmax(128, ar, ac, rp, ci, rows, gc.SLOPE, X)),
                          ("dfgnn_gat_softmax_gm_fwd", lambda: gat.gat_inference_softmax_gm(ar, ac, rp, ci, rows, gc.SLOPE, X)),
                          ("dfgnn_gat_tiling_fwd", lambda: gat.gat_inference_tiling(ar, ac, rp, ci, gc.SLOPE, X))):
        call = gc.Call(entry, base, DEV)
        _run(call, log, missed, what, inference)
        got = theirs()
        torch.cuda.synchronize()
        _same_bits(log, missed, what, entry, call.outputs, dict(out=got))
    # the chunked tiling: a chunk boundary inside the graph, the workspace exactly as large as the library asks
    assert 0 < chunk_rows < m
    seg_ptr, ccol = gat._tiling_chunks(rp, ci, chunk_rows)
    ws_bytes = int(_lib().dfgnn_gat_tiling_chunked_ws_bytes(m, h, f, chunk_rows))
    call = gc.Call("dfgnn_gat_tiling_chunked_fwd", dict(base, chunk_rows=chunk_rows, seg_ptr=seg_ptr, ccol=ccol, ws_numel=ws_bytes,
                                                        ws_bytes=ws_bytes), DEV)
    _run(call, log, missed, what + f" chunks of {chunk_rows}", inference)
    monkeypatch.setattr(gat, "TILING_CHUNK_ROWS", chunk_rows)
    monkeypatch.setattr(gat, "TILING_CHUNK_MIN_TABLE", 0)
    monkeypatch.setattr(gat, "TILING_CHUNK_MIN_DEGREE", 0)
    assert gat._use_chunked_tiling(m, nnz, h, f)
    theirs = gat.gat_inference_tiling(ar, ac, rp, ci, gc.SLOPE, X)
    monkeypatch.undo()
    torch.cuda.synchronize()
    _same_bits(log, missed, what, call.entry, call.outputs, dict(out=theirs))
    # the general training pair (no rows, no plan), without and with a dropout mask (the binding's randoms)
    gat.USE_BLOCK_PLAN = False
    try:
        for drop in (0.0, gc.ATTN_DROP):
            torch.manual_seed(5)
            out, emax, esum, mask = gat.gat_forward(ar, ac, rp, ci, gc.SLOPE, X, drop)
            grads = gat.gat_backward(gc.SLOPE, drop, rp, ci, d["col_ptr"], d["row_ind"], d["val_idx"], emax, esum, mask, X, ar, ac, dO)
            torch.cuda.synchronize()
            tcase = dict(base, rows=None, plan=None, plan_meta=None, attn_drop=drop, edge_mask=_np(mask) if drop else None)
            tcheck = mask_check(_np(mask)) if drop else check
            fwd = gc.Call("dfgnn_gat_fwd_train", tcase, DEV)
            _run(fwd, log, missed, what + f" dropout {drop}", tcheck)
            bwd = gc.Call("dfgnn_gat_bwd", dict(tcase, **{k: v for k, v in fwd.numpy().items() if k != "out"}), DEV)
            _run(bwd, log, missed, what + f" dropout {drop}", tcheck)
            _same_bits(log, missed, what, fwd.entry, fwd.outputs, dict(out=out, edge_max=emax, edge_sum=esum))
            _same_bits(log, missed, what, bwd.entry, bwd.outputs, dict(zip(("grad_feat", "grad_attn_row", "grad_attn_col"), grads)))
    finally:
        gat.USE_BLOCK_PLAN = True
    # the per-node scores of 'hyper_v2'
    rng = np.random.default_rng(11)
    a_l, a_r = (rng.standard_normal((h, f)).astype(np.float32) for _ in range(2))
    X64 = x["X"].astype(np.float64)
    sref = dict(attn_row=np.einsum("mhf,hf->mh", X64, a_l.astype(np.float64)), attn_col=np.einsum("mhf,hf->mh", X64, a_r.astype(np.float64)))
    call = gc.Call("dfgnn_gat_attn_scores", dict(base, a_l=a_l, a_r=a_r), DEV)
    _run(call, log, missed, what, lambda name, got: gc.error_and_bound("scores", got, sref[name], None))


@pytest.mark.parametrize("case", GAT_CASES, ids=str)
def test_gat_family_on_boundary_cases(oracle_mod, monkeypatch, case):
    """Every GAT inference variant, the chunked tiling with a chunk boundary inside the pool, the per-node scores and the
    general training pair with and without a dropout mask, on the constructed boundary-degree graphs under parity_cases'
    fp32-level bounds (with a mask: recomputed for the randoms the binding drew, as tests/test_gpu_edge_exact.py does)."""
    g = pc.graph(case[0], case[1])
    x, ref64, _, bounds = pc.references("gat", *case)

    def mask_check(mask):
        r64 = pc.gat_reference(g["row_ptr"], g["col_ind"], x, "f64", mask, gc.ATTN_DROP)
        r32 = pc.gat_reference(g["row_ptr"], g["col_ind"], x, "f32", mask, gc.ATTN_DROP)
        return _pc_check(g, r64, {k: pc.MARGIN * pc.error_of(g, k, r32[k], r64[k]) for k in r64})
    plans = [None] if case[1] or case[2] % 4 else [_plan_for(g, case[2]), None]
    if plans[0] is not None and plans[0].num_fit == 0:
        plans = [None]
    assert g["pool"][0] < 192 <= g["pool"][-1]
    log, missed = _Log(), []
    _gat_entries(g, x, _pc_check(g, ref64, bounds), mask_check, f"gat {case}", log, missed, plans, monkeypatch, 192)
    log.show(f"gat {case}")
    assert set(log.rows) == set(gc.entries_of("gat")), sorted(log.rows)
    log.require_bits("dfgnn_gat_attn_scores")               # (no operator returns the scores: 'hyper_v2' consumes them)
    assert not missed, missed


@pytest.mark.parametrize("f", [128, 256])
def test_gat_hyper_on_a_mixed_batch(oracle_mod, f):
    """dfgnn_gat_hyper_fwd under the plan of the mixed batch, at f = 128 (the range with a duplicate edge among the fit ones)
    and at f = 256: LDS-resident ranges (gat_block.hip), a range whose per-edge values live in the scratch of exactly h nnz
    floats, spilled ranges."""
    import fused_gatconv as gat
    g = gc.batch_graph("mixed")
    x = _batch_inputs(g, 1, f, True, 1000 + f)
    plan = _plan_for(g, f)
    assert plan.num_fit > 0 and plan.num_spill > 0 and plan.num_edge_global > 0, plan.meta
    print(f"guarded gat mixed batch f{f}: fit {plan.num_fit}, spill {plan.num_spill}, edge-global {plan.num_edge_global}")
    ref = dict(out=oracle_mod.gat_forward(g["row_ptr"], g["col_ind"], x["attn_row"], x["attn_col"], gc.SLOPE, x["V"]))
    case = dict(m=g["m"], nnz=g["nnz"], h=1, f=f, stream=_stream(), **{k: g[k] for k in GRAPH_KEYS}, attn_row=x["attn_row"],
                attn_col=x["attn_col"], X=x["V"], negative_slope=gc.SLOPE, plan=plan.buf, plan_meta=ctypes.addressof(plan._meta_c))
    log, missed = _Log(), []
    call = gc.Call("dfgnn_gat_hyper_fwd", case, DEV)
    _run(call, log, missed, "gat mixed batch", _bar_check(ref))
    d = {k: _dev(g[k]) for k in GRAPH_KEYS}
    theirs = gat.gat_inference_hyper(1024, _dev(x["attn_row"]), _dev(x["attn_col"]), d["row_ptr"], d["col_ind"], d["rows"],
                                     gc.SLOPE, _dev(x["V"]))
    torch.cuda.synchronize()
    _same_bits(log, missed, "gat mixed batch", call.entry, call.outputs, dict(out=theirs))
    log.show(f"gat mixed batch f{f}")
    log.require_bits()
    assert not missed, missed


# ---- family C: graph preparation --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("csc", [True, False], ids=["csc", "csr-only"])
@pytest.mark.parametrize("idx64", [0, 1], ids=["int32", "int64"])
@pytest.mark.parametrize("kind", ["sq_lane_odd", "tall", "wide", "block"])
def test_preprocessing(kind, idx64, csc):
    """dfgnn_preprocess_hyper (the square graph) / dfgnn_preprocess_hyper_rect on a shuffled COO list: integer outputs between
    guards of a fill no id equals, the workspace exactly as large as the library asks, bit-exact against numpy's stable
    sorts (rect_cases._finish) and against the binding."""
    import dfgnn_preprocess
    g = gc.graph(kind)
    m, n, nnz = g["m"], g["n_cols"], g["nnz"]
    perm = np.random.default_rng(4).permutation(nnz)
    dt = np.int64 if idx64 else np.int32
    src, dst = g["src"][perm].astype(dt), g["dst"][perm].astype(dt)
    want = gc.rc._finish(src, dst, m, n)
    want["edge_order"] = np.argsort(src, kind="stable").astype(np.int32)
    size = ctypes.c_size_t(0)
    if kind in gc.SQUARE_KINDS:
        entry, ws_bytes = "dfgnn_preprocess_hyper", int(_lib().dfgnn_preprocess_ws_bytes(m, nnz))
    else:
        assert _lib().dfgnn_preprocess_ws_bytes_rect(m, n, nnz, ctypes.addressof(size)) == 0
        entry, ws_bytes = "dfgnn_preprocess_hyper_rect", int(size.value)
    case = dict(m=m, n_cols=n, nnz=nnz, src=src, dst=dst, idx64=idx64, ws_numel=ws_bytes, ws_bytes=ws_bytes, stream=_stream())
    call = gc.Call(entry, case, DEV, omit=() if csc else ("col_ptr", "row_ind", "val_idx"))
    log, missed = _Log(), []
    exact = lambda name, got: (float((got != want[name]).sum()), 0.0)  # noqa: E731
    _run(call, log, missed, f"preprocess {kind}", exact)
    assert set(call.outputs) == {"row_ptr", "col_ind", "rows", "edge_order"} | ({"col_ptr", "row_ind", "val_idx"} if csc else set())
    theirs = dfgnn_preprocess.coo_to_hyper(_dev(src), _dev(dst), m if kind in gc.SQUARE_KINDS else (m, n), csc=csc)
    torch.cuda.synchronize()
    names = ("row_ptr", "col_ind", "rows", "edge_order", "col_ptr", "row_ind", "val_idx")
    _same_bits(log, missed, f"preprocess {kind}", entry, call.outputs, dict(zip(names, theirs)))
    log.show(f"preprocess {kind}")
    log.require_bits()
    assert not missed, missed


def test_plan_build_and_dense_weights(oracle_mod):
    """dfgnn_plan_build into a buffer of exactly dfgnn_plan_ints(m, nnz) int32 between guards -- the header words equal the
    binding's and a forward under that very plan gives the binding's bits -- and dfgnn_plan_dense_weights into exactly
    dfgnn_plan_dense_weights_floats(m) floats: W[256 i + (j - n0)] = val[e], zero elsewhere."""
    import fused_gtconv as gt
    L = _lib()
    log, missed = _Log(), []
    for kind, f in (("dense", 64), ("mixed", 128)):
        g = gc.batch_graph(kind)
        m, nnz = g["m"], g["nnz"]
        meta = (ctypes.c_int * 12)()
        case = dict(m=m, nnz=nnz, f=f, row_ptr=g["row_ptr"], col_ind=g["col_ind"], plan_numel=int(L.dfgnn_plan_ints(m, nnz)),
                    meta_host=ctypes.addressof(meta), stream=_stream())
        build = gc.Call("dfgnn_plan_build", case, DEV)
        _run(build, log, missed, f"plan {kind}")
        ref_plan = _plan_for(g, f)
        assert list(meta) == ref_plan.meta, (list(meta), ref_plan.meta)
        mine = build.arena["plan"]
        x = _batch_inputs(g, 1, f, True, 77)
        d = {k: _dev(g[k]) for k in GRAPH_KEYS}
        Q, K, V = (_dev(x[k]) for k in ("Q", "K", "V"))
        out, attn = torch.empty_like(Q), torch.empty(1, nnz, device=DEV)
        assert L.dfgnn_gt_hyper_fwd(m, nnz, 1, f, *(d[k].data_ptr() for k in ("row_ptr", "col_ind", "rows")), None, Q.data_ptr(),
                                    K.data_ptr(), V.data_ptr(), attn.data_ptr(), None, out.data_ptr(), mine.data_ptr(),
                                    ctypes.addressof(meta), _stream()) == 0
        theirs = gt.gt_hyper_forward(d["row_ptr"], d["col_ind"], d["rows"], _dev(x["val"]), d["col_ptr"], d["row_ind"],
                                     d["val_idx"], 1024, Q, K, V)
        torch.cuda.synchronize()
        assert torch.equal(out, theirs[0]) and torch.equal(attn, theirs[1]), kind
        build.arena.verify(outputs=[])                       # (the forward read the plan and wrote nothing around it)
        if kind == "dense":
            from _binding_util import plan_dense_weights
            val = np.random.default_rng(5).uniform(-1.0, 1.5, nnz).astype(np.float32)
            want = np.zeros((m, 256), np.float32)
            assert ref_plan.num_dense == ref_plan.num_fit > 0 and ref_plan.num_spill == 0, ref_plan.meta
            for n0, n1f in _np(ref_plan.buf)[12:12 + 2 * ref_plan.num_fit].reshape(-1, 2):
                for i in range(n0, n1f & ~((1 << 30) | (1 << 29))):
                    lo, hi = g["row_ptr"][i], g["row_ptr"][i + 1]
                    want[i, g["col_ind"][lo:hi] - n0] = val[lo:hi]
            wcase = dict(m=m, nnz=nnz, row_ptr=g["row_ptr"], val=val, plan=ref_plan.buf, plan_meta=ctypes.addressof(ref_plan._meta_c),
                         weights_numel=int(L.dfgnn_plan_dense_weights_floats(m)), stream=_stream())
            assert wcase["weights_numel"] == 256 * m
            call = gc.Call("dfgnn_plan_dense_weights", wcase, DEV)
            _run(call, log, missed, "dense weights", lambda name, got: (float((got.reshape(m, 256) != want).sum()), 0.0))
            theirs = plan_dense_weights(ref_plan, d["row_ptr"], _dev(val))
            torch.cuda.synchronize()
            _same_bits(log, missed, "dense weights", call.entry, call.outputs, dict(weights=theirs))
    log.show("plan")
    log.require_bits("dfgnn_plan_build")                     # (compared through the forward that ran under the guarded plan)
    assert set(log.rows) == {"dfgnn_plan_build", "dfgnn_plan_dense_weights"}
    assert not missed, missed
