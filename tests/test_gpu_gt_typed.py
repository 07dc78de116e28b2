"""GPU tests of the GT conv with typed edges (include/dfgnn.h: dfgnn_gt_fwd_typed / dfgnn_gt_bwd_typed;
csrc/gt_typed_train.hip): inference, the training pair that saves two floats per (row, head), the reduction of dR, the
autograd Function and the layer.  The reference is the float64 torch formulation of tests/gt_typed_cases.py on the CPU
(index ops on the materialised R[etype], dR by index_add); the bar is the project's own, max abs error <
1e-3 * max(1, max |ref|), all finite -- and, on the boundary-degree cases, the fp32-level bounds of the edge pair, whose
power tests/test_gt_edge_host.py proves, plus the bound of dR (tests/gt_typed_cases.py)."""
import functools

import numpy as np
import pytest
import torch

import gt_edge_cases as ec
import gt_typed_cases as tc
import parity_cases as pc
import rect_cases as rc
from conftest import csc_of

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-3
SENTINEL = np.float32(-1e38)
PAIR_OUTPUTS = ("out", "row_max", "row_sum", "dQ", "dK", "dV")     # what the edge pair has too


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _check(got, ref, what):
    """The parity bar; prints the measured figure first (pytest -s / a failing run shows it)."""
    got, ref = _np(got).astype(np.float64), _np(ref).astype(np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    bound = BAR * max(1.0, float(np.abs(ref).max()) if ref.size else 0.0)
    print(f"gt_typed {what}: max abs err {err:.3e} (bound {bound:.3e})")
    assert np.isfinite(got).all(), what
    assert err < bound, (what, err, bound)


# ---- graphs and inputs ------------------------------------------------------------------------------------------------
def _from_csr(row_ptr, col_ind, n_cols):
    """Host CSR arrays of an m x n_cols graph -> the dict the tests use: device int32 arrays (CSR, CSC, val_idx), host copies."""
    m = len(row_ptr) - 1
    rows = np.repeat(np.arange(m, dtype=np.int32), np.diff(row_ptr))
    col_ptr, row_ind, val_idx = csc_of(np.asarray(row_ptr), np.asarray(col_ind), rows, n_cols)
    g = dict(m=m, n_cols=n_cols, nnz=len(col_ind), row_ptr_np=np.asarray(row_ptr), col_ind_np=np.asarray(col_ind),
             val_idx_np=np.asarray(val_idx), rows_np=rows, empty_rows=np.diff(row_ptr) == 0, empty_cols=np.diff(col_ptr) == 0)
    for k, v in (("row_ptr", row_ptr), ("col_ind", col_ind), ("col_ptr", col_ptr), ("row_ind", row_ind), ("val_idx", val_idx)):
        g[k] = _dev(v, torch.int32)
    return g


@functools.lru_cache(maxsize=None)
def _graph(kind):
    """lane / wave: the graphs of tests/test_gpu_gatv2.py::_graph, as the edge tests use them (lane: m = 257, ~3 edges per row,
    one row above 64 edges, empty rows and columns, duplicates; wave: m = 96, ~40 edges per row, one row of 200 edges).
    w16: m = 16, one row of 70 edges, the others of 8..12, one duplicate -- nnz <= 256.  w4: m = 4, 16 edges per row.  Both
    wave form.  tall: 150 x 96 (a lane group per row, a wave per column); wide: 96 x 150 (the reverse)."""
    if kind in ("lane", "wave"):
        from test_gpu_gatv2 import _graph as base
        b = base(kind)
        g = _from_csr(_np(b["row_ptr"]), _np(b["col_ind"]), b["m"])
        assert torch.equal(g["row_ind"], b["row_ind"]) and torch.equal(g["col_ptr"], b["col_ptr"])
        return g
    if kind in ("w16", "w4"):
        rng = np.random.default_rng(16 if kind == "w16" else 4)
        m = 16 if kind == "w16" else 4
        deg = rng.integers(8, 13, m) if kind == "w16" else np.full(m, 16)
        if kind == "w16":
            deg[5] = 70
        row_ptr = np.r_[0, np.cumsum(deg)].astype(np.int32)
        col_ind = rng.integers(0, m, int(row_ptr[-1])).astype(np.int32)
        if kind == "w16":
            col_ind[row_ptr[2] + 1] = col_ind[row_ptr[2]]             # the duplicate
        g = _from_csr(row_ptr, col_ind, m)
        assert g["nnz"] >= 8 * m and g["nnz"] <= 256 and (kind == "w16" or g["nnz"] == 64)
        return g
    if kind == "tall":
        r = rc._random_rect(np.random.default_rng(15096), 150, 96, 6, empty_rows=(4, 149), empty_cols=(13,))
    else:
        r = rc._random_rect(np.random.default_rng(96150), 96, 150, 10, empty_rows=(11,), empty_cols=(77,), heavy_row=(3, 100))
    g = _from_csr(r["row_ptr"], r["col_ind"], r["n_cols"])
    assert rc.lane_form(g["m"], g["nnz"]) == (kind == "tall") and rc.lane_form(g["n_cols"], g["nnz"]) == (kind == "wide")
    return g


def _types(rng, nnz, T):
    """Random types in [0, T) of which T // 2 has no edge (T = 1: all zero)."""
    if T == 1:
        return np.zeros(nnz, dtype=np.int32)
    t = rng.integers(0, T - 1, nnz)
    t[t >= T // 2] += 1
    return t.astype(np.int32)


def _inputs(g, h, f, weighted, etype, T, seed=0):
    """float32 host inputs on graph g with the given types."""
    m, n, nnz = g["m"], g["n_cols"], g["nnz"]
    rng = np.random.default_rng(1000 * h + f + 7 * weighted + 13 * seed)
    val = rng.uniform(0.5, 1.5, nnz) if weighted else np.ones(nnz)
    Q, K = rng.standard_normal((m, h, f)) * f ** -0.25, rng.standard_normal((n, h, f)) * f ** -0.25
    V, dO = rng.standard_normal((n, h, f)), rng.standard_normal((m, h, f))
    R = rng.standard_normal((T, h, f)) * 0.5
    x = {k: np.ascontiguousarray(a, dtype=np.float32) for k, a in dict(val=val, R=R, Q=Q, K=K, V=V, dO=dO).items()}
    x["etype"] = np.ascontiguousarray(etype, dtype=np.int32)
    x["etype_csc"] = np.ascontiguousarray(x["etype"][g["val_idx_np"]])
    return x


def _reference(g, x):
    return tc.reference(g["row_ptr_np"], g["col_ind_np"], g["n_cols"], x["val"], x["etype"], x["R"], x["Q"], x["K"], x["V"],
                        x["dO"])


@functools.lru_cache(maxsize=None)
def _case(kind, h, f, weighted, T):
    """-> (host inputs dict, float64 reference dict); computed once per case and shared, nobody writes to it."""
    g = _graph(kind)
    x = _inputs(g, h, f, weighted, _types(np.random.default_rng(T), g["nnz"], T), T)
    return x, _reference(g, x)


def _on_device(x):
    return {k: _dev(a) for k, a in x.items()}


def _pair(g, d, need_dR=True):
    import fused_gtconv as gt
    out, mx, sm = gt.gt_forward_typed(g["row_ptr"], g["col_ind"], d["val"], d["etype"], d["R"], d["Q"], d["K"], d["V"])
    dQ, dK, dV, dR = gt.gt_backward_typed(g["row_ptr"], g["col_ind"], d["val"], d["etype"], g["col_ptr"], g["row_ind"],
                                          g["val_idx"], d["etype_csc"], d["R"], d["Q"], d["K"], d["V"], out, mx, sm, d["dO"],
                                          need_dR=need_dR)
    torch.cuda.synchronize()
    return dict(out=out, row_max=mx, row_sum=sm, dQ=dQ, dK=dK, dV=dV, dR=dR)


def _edge_pair(g, d, need_dE=False):
    """The edge pair on the materialised E = R[etype]."""
    import fused_gtconv as gt
    E = d["R"][d["etype"].long()].contiguous()
    out, mx, sm = gt.gt_forward_edge(g["row_ptr"], g["col_ind"], d["val"], E, d["Q"], d["K"], d["V"])
    dQ, dK, dV, dE = gt.gt_backward_edge(g["row_ptr"], g["col_ind"], d["val"], E, g["col_ptr"], g["row_ind"], g["val_idx"],
                                         d["Q"], d["K"], d["V"], out, mx, sm, d["dO"], need_dE=need_dE)
    torch.cuda.synchronize()
    return dict(out=out, row_max=mx, row_sum=sm, dQ=dQ, dK=dK, dV=dV, dE=dE)


def _against_reference(res, ref, what, names=("out", "row_sum", "dQ", "dK", "dV", "dR")):
    """Everything at the bar; row_max where the row has an edge, the sentinel exactly elsewhere."""
    live = ref["row_max"] != tc.SENTINEL_MAX
    for name in names:
        _check(res[name], ref[name], f"{what} {name}")
    mx = _np(res["row_max"])
    _check(mx[live], ref["row_max"][live], f"{what} row_max")
    assert (mx[~live] == SENTINEL).all(), what


def _exact_zeros(g, res):
    er, ecol = g["empty_rows"], g["empty_cols"]
    assert (_np(res["out"])[er] == 0).all() and (_np(res["dQ"])[er] == 0).all()
    assert (_np(res["dK"])[ecol] == 0).all() and (_np(res["dV"])[ecol] == 0).all()
    assert (_np(res["row_max"])[er] == SENTINEL).all() and (_np(res["row_sum"])[er] == 0).all()


# ---- 1. the pair against the reference --------------------------------------------------------------------------------
CASES = [("lane", 2, 20), ("lane", 3, 7), ("lane", 1, 128), ("wave", 1, 128), ("wave", 8, 16), ("wave", 2, 7)]


@pytest.mark.parametrize("T", [1, 5, 64])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind,h,f", CASES)
def test_pair_against_reference(kind, h, f, weighted, T):
    """Both forms, float4 and scalar lane layouts, several heads, a table of one row, of a few and of 64 (T f = 8192 at
    f = 128): every output at the bar; exact zeros and sentinels where a row / column has no edge; the dR row of the type
    without an edge is exactly 0; inference equals the training forward's out, two backward calls agree, need_dR=False
    leaves dQ, dK, dV as they are, and out, the statistics, dQ, dK, dV equal the edge pair's on E = R[etype] -- all bit for
    bit."""
    import fused_gtconv as gt
    g = _graph(kind)
    x, ref = _case(kind, h, f, weighted, T)
    d = _on_device(x)
    assert gt.gt_typed_dR_supported(T, h, f)
    res = _pair(g, d)
    _against_reference(res, ref, f"{kind} h{h} f{f} val={weighted} T={T}")
    _exact_zeros(g, res)
    assert res["dR"].shape == (T, h, f)
    if T > 1:
        assert (x["etype"] != T // 2).all() and (_np(res["dR"])[T // 2] == 0).all() and (ref["dR"][T // 2] == 0).all()
    plain = gt.gt_inference_typed(g["row_ptr"], g["col_ind"], d["val"], d["etype"], d["R"], d["Q"], d["K"], d["V"])
    assert torch.equal(plain, res["out"])
    again, without = _pair(g, d), _pair(g, d, need_dR=False)
    assert without["dR"] is None
    for name in ("dQ", "dK", "dV"):
        assert torch.equal(res[name], again[name]) and torch.equal(res[name], without[name]), name
    assert torch.equal(res["dR"], again["dR"])
    edge = _edge_pair(g, d)
    for name in PAIR_OUTPUTS:
        assert torch.equal(res[name], edge[name]), name


# ---- 2. boundary degrees at fp32 level --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.case_ids("gt"), ids=str)
def test_boundary_degrees(case):
    """The 32 cases of the edge pair's power test with R = K'[:304], etype = col_ind (R[etype] == E exactly, checked in
    tests/test_gt_typed_host.py): out, row_max (rows with edges), row_sum, dQ, dK, dV within the edge pair's bounds; dR within
    MARGIN x the float32 formulation's error wherever the table is supported with dR (T f = 304 f <= 8192: the eight (7, 2)
    cases), the other cases run with need_dR=False.  Prints measured error / fp32 reference error per output (pytest -s).
    Worst ratios on the MI355X: row_max 5.08 (the degree-1 row at f = 7), dK 3.77 at (260, 1), dQ 2.03, out 0.70, dV 0.62,
    row_sum 0.59 -- the edge pair's figures, as the bits are the edge pair's -- and dR 0.46 (the lane-group form at (7, 2))."""
    import fused_gtconv as gt
    g = pc.graph(case[0], case[1])
    x, ref64, bounds = tc.boundary_references(case)
    f, h = case[2], case[3]
    need_dR = gt.gt_typed_dR_supported(tc.BOUNDARY_T, h, f)
    assert need_dR == ((f, h) == (7, 2))
    dg = {k: _dev(g[k], torch.int32) for k in ("row_ptr", "col_ind", "col_ptr", "row_ind", "val_idx")}
    d = _on_device({k: x[k] for k in ("val", "R", "Q", "K", "V", "dO", "etype")})
    d["etype_csc"] = _dev(x["etype"][g["val_idx"].astype(np.int64)])
    res = _pair(dg, d, need_dR=need_dR)
    assert (res["dR"] is not None) == need_dR
    missed = []
    for name in tc.OUTPUTS if need_dR else PAIR_OUTPUTS:
        got = _np(res[name]).astype(np.float64)
        assert np.isfinite(got).all(), (case, name)
        err, at = tc.error_of(g, name, got, ref64[name], where=True)
        fp32 = bounds[name] / pc.MARGIN / (ec.DK_FACTOR if name == "dK" else 1.0)
        print(f"gt_typed boundary {case} {name}: measured {err:.3e} at (node, head) {at}, fp32 reference {fp32:.3e}, "
              f"ratio {err / fp32 if fp32 > 0 else float('nan'):.2f}, bound {bounds[name]:.3e}")
        if not err <= bounds[name]:
            missed.append((name, err, bounds[name]))
    er, ecol = np.diff(g["row_ptr"]) == 0, np.diff(g["col_ptr"]) == 0
    assert (_np(res["out"])[er] == 0).all() and (_np(res["dQ"])[er] == 0).all()
    assert (_np(res["dK"])[ecol] == 0).all() and (_np(res["dV"])[ecol] == 0).all()
    assert (_np(res["row_max"])[er] == SENTINEL).all() and (_np(res["row_sum"])[er] == 0).all()
    assert not missed, (case, missed)


# ---- 3. one type per edge ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f", [("lane", 3, 7), ("w16", 2, 32), ("w16", 8, 16), ("w4", 1, 128)])
def test_one_type_per_edge(kind, h, f):
    """etype = arange(nnz), T = nnz: every row of dR receives exactly one edge's contribution, so dR must equal the edge
    pair's dE bit for bit -- a contribution that is lost, misrouted or added twice cannot hide.  The same inputs with all
    types 0 (T = 1: every contribution meets every other) are at the bar against the reference."""
    import fused_gtconv as gt
    g = _graph(kind)
    nnz = g["nnz"]
    assert gt.gt_typed_dR_supported(nnz, h, f) and (kind != "w4" or nnz * f == 8192)
    x = _inputs(g, h, f, True, np.arange(nnz), nnz)
    d = _on_device(x)
    res, edge = _pair(g, d), _edge_pair(g, d, need_dE=True)
    assert res["dR"].shape == edge["dE"].shape == (nnz, h, f)
    assert torch.equal(res["dR"], edge["dE"])
    for name in PAIR_OUTPUTS:
        assert torch.equal(res[name], edge[name]), name
    one = _inputs(g, h, f, True, np.zeros(nnz), 1)
    _against_reference(_pair(g, _on_device(one)), _reference(g, one), f"one type {kind} h{h} f{f}")


# ---- 4. head offset ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f", [("lane", 3, 7), ("wave", 8, 16)])
def test_single_slot_touches_one_head(kind, h, f):
    """R is non-zero in one (type, head) slot only: the outputs of every other head equal the R = 0 run bit for bit.  With
    R = 0 the pair equals the row-statistics pair bit for bit, and dR -- sum over a type's edges of dS_e val_e Q_i + P_e
    dO_i -- is at the bar (a table row read from a wrong slot that happens to cancel cannot hide there)."""
    import fused_gtconv as gt
    g, T = _graph(kind), 5
    x = dict(_case(kind, h, f, True, T)[0])
    zero = dict(x, R=np.zeros_like(x["R"]))
    one = dict(x, R=np.zeros_like(x["R"]))
    head = h - 2
    one["R"][3, head] = np.linspace(1.0, 2.0, f, dtype=np.float32)
    dz = _on_device(zero)
    base, res = _pair(g, dz), _pair(g, _on_device(one))
    others = [hd for hd in range(h) if hd != head]
    for name in tc.OUTPUTS:
        assert torch.equal(res[name][:, others], base[name][:, others]), name
        assert name == "row_max" or not torch.equal(res[name][:, head], base[name][:, head]), name
    _against_reference(res, _reference(g, one), f"single slot {kind}")
    out, mx, sm = gt.gt_forward_rowstats(g["row_ptr"], g["col_ind"], dz["val"], dz["Q"], dz["K"], dz["V"])
    dQ, dK, dV = gt.gt_backward_rowstats(g["row_ptr"], g["col_ind"], dz["val"], g["col_ptr"], g["row_ind"], g["val_idx"],
                                         dz["Q"], dz["K"], dz["V"], out, mx, sm, dz["dO"])
    for name, want in (("out", out), ("row_max", mx), ("row_sum", sm), ("dQ", dQ), ("dK", dK), ("dV", dV)):
        assert torch.equal(base[name], want), name
    ref = _reference(g, zero)
    _check(base["dR"], ref["dR"], f"R = 0 {kind} dR")
    assert np.abs(ref["dR"]).max() > 0.1


# ---- 5. rectangular graphs --------------------------------------------------------------------------------------------
def _raw(g, d, T, h, f, rect):
    """The C entries through ctypes: the square ones, or the _rect ones with n_cols given."""
    from _binding_util import call
    m, nnz = g["m"], g["nnz"]
    E = lambda *s: torch.empty(s, dtype=torch.float32, device=DEV)  # noqa: E731
    import dfgnn_native
    ws = E(int(dfgnn_native.lib().dfgnn_gt_typed_bwd_ws_floats(T, h, f)))
    out, mx, sm, delta = E(m, h, f), E(m, h), E(m, h), E(m, h)
    dQ, dK, dV, dR = E(m, h, f), E(g["n_cols"], h, f), E(g["n_cols"], h, f), E(T, h, f)
    dims = (m, g["n_cols"], nnz, h, f, T) if rect else (m, nnz, h, f, T)
    sfx = "_rect" if rect else ""
    call("dfgnn_gt_fwd_typed" + sfx, "fwd", d["Q"].device, *dims, g["row_ptr"], g["col_ind"], d["val"], d["etype"], d["R"],
         d["Q"], d["K"], d["V"], mx, sm, out)
    call("dfgnn_gt_bwd_typed" + sfx, "bwd", d["Q"].device, *dims, g["row_ptr"], g["col_ind"], d["val"], d["etype"],
         g["col_ptr"], g["row_ind"], g["val_idx"], d["etype_csc"], d["R"], d["Q"], d["K"], d["V"], out, mx, sm, d["dO"], delta,
         ws, dQ, dK, dV, dR)
    torch.cuda.synchronize()
    return dict(out=out, row_max=mx, row_sum=sm, dQ=dQ, dK=dK, dV=dV, dR=dR)


@pytest.mark.parametrize("kind,h,f", [("tall", 2, 20), ("wide", 1, 128), ("wide", 3, 7)])
def test_rectangular(kind, h, f):
    """150 x 96 (a lane group per row, a wave per column) and 96 x 150 (the reverse), empty rows and columns: every output
    at the bar against the rect-capable reference, exact zeros where nothing arrives, and the edge pair's bits."""
    g, T = _graph(kind), 5
    x = _inputs(g, h, f, True, _types(np.random.default_rng(5), g["nnz"], T), T)
    d = _on_device(x)
    res = _pair(g, d)
    assert res["out"].shape == res["dQ"].shape == (g["m"], h, f) and res["dK"].shape == res["dV"].shape == (g["n_cols"], h, f)
    _against_reference(res, _reference(g, x), f"rect {kind} h{h} f{f}")
    _exact_zeros(g, res)
    edge = _edge_pair(g, d)
    for name in PAIR_OUTPUTS:
        assert torch.equal(res[name], edge[name]), name


def test_square_entry_is_the_rect_entry():
    """dfgnn_gt_*_typed and dfgnn_gt_*_typed_rect with n_cols = m: the same bits; and without rows (m = 0, n_cols > 0) the
    backward writes dK = dV = dR = 0 in full."""
    import fused_gtconv as gt
    h, f, T = 2, 20, 5
    g = _graph("lane")
    d = _on_device(_case("lane", h, f, True, T)[0])
    sq, rect = _raw(g, d, T, h, f, False), _raw(g, d, T, h, f, True)
    for name in tc.OUTPUTS:
        assert torch.equal(sq[name], rect[name]), name
    i32 = dict(dtype=torch.int32, device=DEV)
    none, n = torch.zeros(0, **i32), 7
    Q, KV, R = torch.zeros(0, h, f, device=DEV), torch.randn(n, h, f, device=DEV), torch.randn(T, h, f, device=DEV)
    out, mx, sm = gt.gt_forward_typed(torch.zeros(1, **i32), none, None, none, R, Q, KV, KV)
    dQ, dK, dV, dR = gt.gt_backward_typed(torch.zeros(1, **i32), none, None, none, torch.zeros(n + 1, **i32), none, none, none,
                                          R, Q, KV, KV, out, mx, sm, Q)
    torch.cuda.synchronize()
    assert dK.shape == dV.shape == (n, h, f) and dR.shape == (T, h, f) and dQ.shape == (0, h, f)
    assert (dK == 0).all() and (dV == 0).all() and (dR == 0).all()


# ---- 6. operator ------------------------------------------------------------------------------------------------------
def _op(g, d, q, k, v, r):
    from DFGNN.operators.fused_gtconv import GTConvFuse_typed
    return GTConvFuse_typed(None, g["row_ptr"], g["col_ind"], d["val"], g["col_ptr"], g["row_ind"], g["val_idx"], 0, q, k, v, r,
                            d["etype"], d["etype_csc"])


@pytest.mark.parametrize("kind,h,f,weighted", [("lane", 2, 20, True), ("wave", 8, 16, False)])
def test_operator_equals_raw_calls(kind, h, f, weighted):
    """GTConvFuse_typed + autograd.grad equals the raw binding calls bit for bit; `val` is saved only when it is not all
    ones; with R.requires_grad == False its gradient is None and the others are the same bits."""
    from DFGNN.operators.fused_gtconv import GTConvFuse_inference_typed
    g = _graph(kind)
    d = _on_device(_case(kind, h, f, weighted, 5)[0])
    raw = _pair(g, d)
    q, k, v, r = (d[n].clone().requires_grad_(True) for n in ("Q", "K", "V", "R"))
    out = _op(g, d, q, k, v, r)
    assert any(t.data_ptr() == d["val"].data_ptr() for t in out.grad_fn.saved_tensors) == weighted
    grads = torch.autograd.grad(out, (q, k, v, r), d["dO"])
    assert torch.equal(out, raw["out"])
    for got, name in zip(grads, ("dQ", "dK", "dV", "dR")):
        assert torch.equal(got, raw[name]), name
    assert torch.equal(GTConvFuse_inference_typed(g["row_ptr"], g["col_ind"], d["val"], d["Q"], d["K"], d["V"], d["R"],
                                                  d["etype"]), raw["out"])
    out = _op(g, d, q, k, v, d["R"])
    out.backward(d["dO"])
    assert d["R"].grad is None
    for t, name in zip((q, k, v), ("dQ", "dK", "dV")):
        assert torch.equal(t.grad, raw[name]), name


def test_operator_falls_back_above_the_limit():
    """The wave graph with one type per edge at f = 16: T f is far above 8192.  The raw backward with need_dR raises the
    library's "unsupported" RuntimeError (and runs without dR); the operator still returns every gradient at the bar, through
    GTConvFuse_edge on R[etype]."""
    import fused_gtconv as gt
    g, h, f = _graph("wave"), 8, 16
    nnz = g["nnz"]
    assert nnz * f > 8192 and not gt.gt_typed_dR_supported(nnz, h, f)
    x = _inputs(g, h, f, True, np.arange(nnz), nnz)
    d, ref = _on_device(x), _reference(g, x)
    with pytest.raises(RuntimeError, match="unsupported"):
        _pair(g, d)
    res = _pair(g, d, need_dR=False)
    _against_reference(res, ref, "above the limit, raw without dR", names=("out", "row_sum", "dQ", "dK", "dV"))
    q, k, v, r = (d[n].clone().requires_grad_(True) for n in ("Q", "K", "V", "R"))
    out = _op(g, d, q, k, v, r)
    grads = torch.autograd.grad(out, (q, k, v, r), d["dO"])
    _check(out, ref["out"], "fallback out")
    for got, name in zip(grads, ("dQ", "dK", "dV", "dR")):
        _check(got, ref[name], f"fallback {name}")


# ---- 7. memory --------------------------------------------------------------------------------------------------------
def test_memory_of_one_step():
    """The wave graph at h = 2, f = 16, T = 16.  The fused step allocates out, dQ, dK, dV (4 bytes(Q)), the three [m, h]
    arrays, the partials ws, dR and autograd's handful of small blocks -- nothing of size nnz h f: its peak over the inputs
    is at most 8 bytes(Q) + 4 ws_floats + 2 bytes(R) + 64 KB.  The edge-pair step on the materialised R[etype] is above
    bytes(E)."""
    import dfgnn_native
    from DFGNN.operators.fused_gtconv import GTConvFuse_edge
    g, h, f, T = _graph("wave"), 2, 16, 16
    d = _on_device(_case("wave", h, f, True, T)[0])
    bytes_q, bytes_e, bytes_r = 4 * g["m"] * h * f, 4 * g["nnz"] * h * f, 4 * T * h * f
    ws_floats = int(dfgnn_native.lib().dfgnn_gt_typed_bwd_ws_floats(T, h, f))
    assert bytes_e > 16 * bytes_q and ws_floats > 0

    def peak(fused):
        q, k, v, r = (d[n].clone().requires_grad_(True) for n in ("Q", "K", "V", "R"))

        def step():
            if fused:
                o = _op(g, d, q, k, v, r)
            else:
                o = GTConvFuse_edge(None, g["row_ptr"], g["col_ind"], d["val"], g["col_ptr"], g["row_ind"], g["val_idx"], 0,
                                    q, k, v, r[d["etype"].long()])
            return torch.autograd.grad(o, (q, k, v, r), d["dO"])

        step()                                                   # (the all-ones test of `val` is cached here)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res = step()
        torch.cuda.synchronize()
        assert len(res) == 4
        return torch.cuda.max_memory_allocated() - base

    p_typed, p_edge = peak(True), peak(False)
    print(f"gt_typed peak of one fwd+bwd: typed {p_typed} B (of which ws {4 * ws_floats} B), edge pair on R[etype] {p_edge} B; "
          f"bytes(E) = {bytes_e} B, bytes(Q) = {bytes_q} B, bytes(R) = {bytes_r} B")
    assert p_typed <= 8 * bytes_q + 4 * ws_floats + 2 * bytes_r + 65536
    assert p_typed - 4 * ws_floats < bytes_e                    # nothing of size nnz h f
    assert p_edge > bytes_e


# ---- 8. layer ---------------------------------------------------------------------------------------------------------
def test_layer_against_its_torch_branch():
    """SparseMHA_typed(fuse=True) in training mode at two heads against its own fuse=False branch on the cora-like graph: the
    output and the gradients of the q / k / v projection weights and of rel; in .eval() the inference operator gives the same
    output; --conv gt --format forward_typed runs."""
    import argparse

    from DFGNN.layers import SparseMHA_typed, load_graphconv_layer, preprocess_Hyper_fw_bw, preprocess_types
    from DFGNN.utils import synthetic as S
    torch.manual_seed(1)
    g = S.cora_like().to(DEV)
    params = preprocess_Hyper_fw_bw(g)
    nnz, T = params[3].numel(), 9
    types = preprocess_types(params, torch.randint(0, T, (nnz,), device=DEV), T)
    assert torch.equal(types[1], types[0][params[7].long()])
    layer = SparseMHA_typed(64, 64, 2, T).to(DEV).train()
    x = torch.randn(g.num_nodes(), 64, device=DEV)
    weights = (layer.q_proj.weight, layer.k_proj.weight, layer.v_proj.weight, layer.rel)
    outs, grads = [], []
    for fuse in (False, True):
        layer.zero_grad()
        out = layer(params, x, types, fuse=fuse)
        (out * torch.linspace(-1, 1, out.numel(), device=DEV).reshape(out.shape)).sum().backward()
        outs.append(out.detach())
        grads.append([p.grad.clone() for p in weights])
    _check(outs[1], outs[0], "layer out")
    for name, a, b in zip(("q_proj.weight", "k_proj.weight", "v_proj.weight", "rel"), *grads):
        _check(b, a, f"layer d{name}")
    assert float(grads[0][3].abs().max()) > 0
    with torch.no_grad():
        _check(layer.eval()(params, x, types, fuse=True), outs[0], "layer eval out")
    args = argparse.Namespace(conv="gt", format="forward_typed", dim=64, heads=2)
    out, ms = load_graphconv_layer(args).to(DEV).train()(params, x, fuse=True)
    assert out.shape == (g.num_nodes(), 64) and ms > 0


# ---- 9. empty problems and the two transports -------------------------------------------------------------------------
def _empty_problem(m):
    import fused_gtconv as gt
    h, f, T = 2, 12, 3
    i32 = dict(dtype=torch.int32, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(m)
    row_ptr, none = torch.zeros(m + 1, **i32), torch.zeros(0, **i32)
    x, dO = torch.randn(m, h, f, device=DEV, generator=gen), torch.randn(m, h, f, device=DEV, generator=gen)
    R = torch.randn(T, h, f, device=DEV, generator=gen)
    out, mx, sm = gt.gt_forward_typed(row_ptr, none, None, none, R, x, x, x)
    dQ, dK, dV, dR = gt.gt_backward_typed(row_ptr, none, None, none, row_ptr, none, none, none, R, x, x, x, out, mx, sm, dO)
    torch.cuda.synchronize()
    assert out.shape == dQ.shape == dK.shape == dV.shape == (m, h, f) and mx.shape == sm.shape == (m, h)
    assert dR.shape == (T, h, f) and (dR == 0).all()
    if m:      # (m == 0 launches nothing but the reduction)
        for t in (out, dQ, dK, dV, sm):
            assert (t == 0).all()
        assert (mx == -1e38).all()
    return [out, mx, sm, dQ, dK, dV, dR]


def test_bindings_agree_and_empty_problems():
    """The torch C++ extension and the ctypes transport give bit-identical results for gt_inference_typed, gt_forward_typed
    and gt_backward_typed (with and without dR), also on empty problems (m == 0, and m == 5 without an edge: zero outputs,
    sentinels, dR = 0), and the same RuntimeError words for a bad argument."""
    import dfgnn_native
    import fused_gtconv as gt
    assert dfgnn_native.ext() is not None and hasattr(dfgnn_native.ext(), "gt_bwd_typed")
    cases = [(_graph(kind), _on_device(_case(kind, h, f, w, T)[0])) for kind, h, f, w, T in
             (("lane", 2, 20, True, 5), ("wave", 8, 16, False, 64), ("wave", 2, 7, True, 1))]

    def run():
        res = []
        for g, d in cases:
            both = _pair(g, d)
            res += [both[k] for k in tc.OUTPUTS]
            res += [_pair(g, d, need_dR=False)[k] for k in ("dQ", "dK", "dV")]
            res.append(gt.gt_inference_typed(g["row_ptr"], g["col_ind"], d["val"], d["etype"], d["R"], d["Q"], d["K"], d["V"]))
        res += _empty_problem(0) + _empty_problem(5)
        g, d = cases[0]
        first = _pair(g, d)
        errs = []
        for bad in (dict(row_ptr=g["row_ptr"].long()), dict(etype=d["etype"][:-1].contiguous()),
                    dict(R=d["R"].transpose(1, 2).contiguous()), dict(R=d["R"].reshape(5, -1)), dict(R=d["R"][:0])):
            a = dict(row_ptr=g["row_ptr"], etype=d["etype"], R=d["R"])
            a.update(bad)
            try:
                gt.gt_forward_typed(a["row_ptr"], g["col_ind"], d["val"], a["etype"], a["R"], d["Q"], d["K"], d["V"])
                errs.append(None)
            except RuntimeError as e:
                errs.append(str(e))
        try:
            gt.gt_backward_typed(g["row_ptr"], g["col_ind"], d["val"], d["etype"], g["col_ptr"], g["row_ind"], g["val_idx"],
                                 d["etype_csc"][:-1].contiguous(), d["R"], d["Q"], d["K"], d["V"], first["out"], first["row_max"],
                                 first["row_sum"], d["dO"])
            errs.append(None)
        except RuntimeError as e:
            errs.append(str(e))
        return res, errs

    via_ext, err_ext = run()
    saved = dfgnn_native._ext
    dfgnn_native._ext = None                      # force the ctypes path
    try:
        via_ctypes, err_ctypes = run()
    finally:
        dfgnn_native._ext = saved
    assert len(via_ext) == len(via_ctypes) == 3 * 11 + 14
    for a, b in zip(via_ext, via_ctypes):
        assert torch.equal(a, b)
    words = ("int32", "etype must have", "R must have", "R must have", "R must have", "etype_csc must have")
    for e1, e2, word in zip(err_ext, err_ctypes, words):
        assert e1 and e2 and word in e1 and word in e2, (e1, e2)


# ---- 10. HIP graph ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f,T", [("lane", 2, 20, 5), ("wave", 1, 128, 5), ("wave", 1, 128, 64)])
def test_hipgraph_capture(kind, h, f, T):
    """fwd + bwd (with dR: CSR pass, CSC pass, reduction) recorded into a HIP graph (one stream, no parallel branches)
    replays bit-identically, also after Q and R were overwritten in place.  T = 64 at f = 128: tables of 128 KB, above the
    default limit of dynamic LDS, which the library raises once per kernel on its first launch -- GraphedStep's warm-up
    calls, outside the capture (include/dfgnn.h says that a first call must precede a capture)."""
    import fused_gtconv as gt
    from DFGNN.utils import GraphedStep
    g = _graph(kind)
    d = _on_device(_case(kind, h, f, True, T)[0])

    def step():
        out, mx, sm = gt.gt_forward_typed(g["row_ptr"], g["col_ind"], d["val"], d["etype"], d["R"], d["Q"], d["K"], d["V"])
        return [out] + list(gt.gt_backward_typed(g["row_ptr"], g["col_ind"], d["val"], d["etype"], g["col_ptr"], g["row_ind"],
                                                 g["val_idx"], d["etype_csc"], d["R"], d["Q"], d["K"], d["V"], out, mx, sm,
                                                 d["dO"]))

    eager = [t.clone() for t in step()]
    graphed = GraphedStep(step)
    for a, b in zip(eager, graphed.replay()):
        assert torch.equal(a, b)
    d["Q"].mul_(0.5)                                       # next "batch" of features, same structure
    d["R"].add_(0.25)
    again = [t.clone() for t in graphed.replay()]
    for a, b in zip(step(), again):
        assert torch.equal(a, b)
    assert not torch.equal(again[0], eager[0])
