"""GPU tests of the GatedGCN conv (include/dfgnn.h: dfgnn_gatedgcn_fwd / dfgnn_gatedgcn_bwd and their _rect forms;
csrc/gatedgcn_train.hip): inference, the training pair that saves out and den and takes a second gradient stream G =
d loss / d Z, the autograd Function and the layer.  The reference is the float64 torch formulation of
tests/gatedgcn_cases.py on the CPU (index ops over the edge list, gradients from torch.autograd.grad of (out, Z) with
(dO, G)); the bar is the project's own, max abs error < 1e-3 * max(1, max |ref|), all finite -- and, on the boundary-degree
cases, the fp32-level bounds whose power tests/test_gatedgcn_host.py proves."""
import functools

import numpy as np
import pytest
import torch

import gatedgcn_cases as gc
import parity_cases as pc
import rect_cases as rc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-3
EPS = gc.EPS
MAIN = ("out", "den", "dX_row", "dX_col", "dV")        # everything but the two per-edge outputs


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
    print(f"gatedgcn {what}: max abs err {err:.3e} (bound {bound:.3e})")
    assert np.isfinite(got).all(), what
    assert err < bound, (what, err, bound)


# ---- graphs and inputs ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _graph(kind):
    """The graphs of tests/test_gpu_gatv2.py::_graph plus val_idx and the host copies the reference needs.
    lane: m = 257, ~3 edges per row, one row above 64 edges, empty rows and columns, duplicates (lane-group form, COOP).
    wave: m = 96, ~40 edges per row, one row of 200 edges (wave form)."""
    from test_gpu_gatv2 import _graph as base
    g = dict(base(kind))
    order = torch.argsort(g["cols"], stable=True)                      # conftest.csc_of's val_idx
    g["val_idx"] = order.to(torch.int32).to(DEV)
    g["row_ptr_np"], g["col_ind_np"] = _np(g["row_ptr"]), _np(g["col_ind"])
    assert torch.equal(g["rows"][order].to(torch.int32), g["row_ind"].cpu())
    return g


@functools.lru_cache(maxsize=None)
def _inputs(kind, h, f):
    g = _graph(kind)
    m, nnz = g["m"], g["nnz"]
    rng = np.random.default_rng(1000 * h + f + 47)
    X_row, X_col, V, dO = (rng.standard_normal((m, h, f)) for _ in range(4))
    E = rng.standard_normal((nnz, h, f))
    G = 0.25 * rng.standard_normal((nnz, h, f))
    return {k: np.ascontiguousarray(a, dtype=np.float32) for k, a in
            dict(E=E, G=G, X_row=X_row, X_col=X_col, V=V, dO=dO).items()}


def _reference(g, x, normalize, with_E=True, with_G=True):
    rp, ci = (g["row_ptr_np"], g["col_ind_np"]) if "row_ptr_np" in g else (g["row_ptr"], g["col_ind"])
    return gc.reference(rp, ci, x["E"] if with_E else None, x["G"] if with_G else None, x["X_row"], x["X_col"], x["V"],
                        x["dO"], normalize, EPS)


@functools.lru_cache(maxsize=None)
def _case(kind, h, f, normalize, with_E, with_G):
    """-> (host inputs dict, float64 reference dict); computed once per case and shared, nobody writes to it."""
    x = _inputs(kind, h, f)
    return x, _reference(_graph(kind), x, normalize, with_E, with_G)


def _on_device(x):
    return {k: _dev(a) for k, a in x.items()}


def _pair(g, d, normalize=1, with_E=True, with_G=True, need_Z=True, need_dE=True):
    import fused_gtconv as gt
    E = d["E"] if with_E else None
    out, den, Z = gt.gatedgcn_forward(g["row_ptr"], g["col_ind"], d["X_row"], d["X_col"], d["V"], E, normalize, EPS,
                                      need_Z=need_Z)
    dXr, dXc, dV, dE = gt.gatedgcn_backward(g["row_ptr"], g["col_ind"], g["col_ptr"], g["row_ind"], g["val_idx"], d["X_row"],
                                            d["X_col"], d["V"], E, out, den, d["dO"], G=d["G"] if with_G else None,
                                            normalize=normalize, eps=EPS, need_dE=need_dE)
    torch.cuda.synchronize()
    return dict(out=out, den=den, Z=Z, dX_row=dXr, dX_col=dXc, dV=dV, dE=dE)


# ---- 1. the pair against the reference --------------------------------------------------------------------------------
CASES = [("lane", 2, 20), ("lane", 3, 7), ("lane", 1, 128), ("wave", 1, 128), ("wave", 8, 16), ("wave", 2, 7)]


@pytest.mark.parametrize("with_G", [True, False], ids=["G", "noG"])
@pytest.mark.parametrize("with_E", [True, False], ids=["E", "noE"])
@pytest.mark.parametrize("normalize", gc.MODES, ids=["norm", "plain"])
@pytest.mark.parametrize("kind,h,f", CASES)
def test_pair_against_reference(kind, h, f, normalize, with_E, with_G):
    """Both forms, float4 and scalar lane layouts, several heads (a wrong [nnz, h, f] offset shows there): every output at
    the bar; exact zeros where a row / column has no edge; inference equals the training forward's out and Z, two backward
    calls agree, need_Z=False / need_dE=False leave every other output as it is, G = zeros is G = None and E = zeros is
    E = None -- all bit for bit."""
    import fused_gtconv as gt
    g = _graph(kind)
    x, ref = _case(kind, h, f, normalize, with_E, with_G)
    d = _on_device(x)
    res = _pair(g, d, normalize, with_E, with_G)
    for name in gc.OUTPUTS:
        _check(res[name], ref[name], f"{kind} h{h} f{f} normalize={normalize} E={with_E} G={with_G} {name}")
    er, ecol = g["empty_rows"], g["empty_cols"]
    for name in ("out", "den", "dX_row"):
        assert (_np(res[name])[er] == 0).all(), name
    assert (_np(res["dX_col"])[ecol] == 0).all() and (_np(res["dV"])[ecol] == 0).all()
    args = (g["row_ptr"], g["col_ind"], d["X_row"], d["X_col"], d["V"], d["E"] if with_E else None, normalize, EPS)
    assert torch.equal(gt.gatedgcn_inference(*args), res["out"])
    o2, z2 = gt.gatedgcn_inference(*args, need_Z=True)
    assert torch.equal(o2, res["out"]) and torch.equal(z2, res["Z"])
    again = _pair(g, d, normalize, with_E, with_G)
    without = _pair(g, d, normalize, with_E, with_G, need_Z=False, need_dE=False)
    assert without["dE"] is None and without["Z"] is None and res["dE"].shape == res["Z"].shape == (g["nnz"], h, f)
    for name in MAIN:
        assert torch.equal(res[name], again[name]) and torch.equal(res[name], without[name]), name
    assert torch.equal(res["dE"], again["dE"]) and torch.equal(res["Z"], again["Z"])
    if not with_G:
        zeros = _pair(g, dict(d, G=torch.zeros_like(d["G"])), normalize, with_E, True)
        for name in gc.OUTPUTS:
            assert torch.equal(res[name], zeros[name]), name
    if not with_E:
        zeros = _pair(g, dict(d, E=torch.zeros_like(d["E"])), normalize, True, with_G)
        for name in gc.OUTPUTS:
            assert torch.equal(res[name], zeros[name]), name


# ---- 2. boundary degrees at fp32 level --------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", gc.MODES, ids=["norm", "plain"])
@pytest.mark.parametrize("case", pc.case_ids("gt"), ids=str)
def test_boundary_degrees(case, normalize):
    """The 32 cases of the host power test, same inputs and bounds, in both modes: every output within MARGIN x the float32
    formulation's error.  Prints measured error / fp32 reference error per output (pytest -s).  Worst ratios on the MI355X
    (normalize = 1 / 0): dE 1.66 / 2.74, dX_col 1.37 / 1.00, dX_row 1.19 / 0.97, dV 1.18 / 0.79, Z 1.00 / 1.00,
    out 0.71 / 0.82, den 0.65 / 0.65."""
    g = pc.graph(case[0], case[1])
    x, ref64, bounds = gc.boundary_references(case, normalize)
    dg = {k: _dev(g[k], torch.int32) for k in ("row_ptr", "col_ind", "col_ptr", "row_ind", "val_idx")}
    res = _pair(dg, _on_device(x), normalize)
    missed = []
    for name in gc.OUTPUTS:
        got = _np(res[name]).astype(np.float64)
        assert np.isfinite(got).all(), (case, name)
        err, at = gc.error_of(g, name, got, ref64[name], where=True)
        fp32 = bounds[name] / pc.MARGIN
        print(f"gatedgcn boundary {case} normalize={normalize} {name}: measured {err:.3e} at (node, head) {at}, fp32 reference "
              f"{fp32:.3e}, ratio {err / fp32 if fp32 > 0 else float('nan'):.2f}, bound {bounds[name]:.3e}")
        if not err <= bounds[name]:
            missed.append((name, err, bounds[name]))
    er, ecol = np.diff(g["row_ptr"]) == 0, np.diff(g["col_ptr"]) == 0
    for name in ("out", "den", "dX_row"):
        assert (_np(res[name])[er] == 0).all(), name
    assert (_np(res["dX_col"])[ecol] == 0).all() and (_np(res["dV"])[ecol] == 0).all()
    assert not missed, (case, normalize, missed)


# ---- 3. extremes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", gc.MODES, ids=["norm", "plain"])
@pytest.mark.parametrize("kind,h,f", [("lane", 2, 20), ("wave", 1, 128)])
def test_saturated_gates(kind, h, f, normalize):
    """X_row shifted by +60 in every third dimension and by -60 in the next: the sigmoid saturates at 1 and at e^-60 (exp
    of +60 and of -60; beyond |z| = 88.7 the exponential overflows to inf and the gate is an exact 0).  Everything stays
    finite and at the bar; one row is shifted by -60 (and one by -120) in ALL dimensions: its gates are all ~e^-60 (0), den is
    far below eps, and out is ~0 through eps, not NaN."""
    g = _graph(kind)
    x = dict(_inputs(kind, h, f))
    shift = np.zeros(f, dtype=np.float32)
    shift[0::3], shift[1::3] = 60.0, -60.0
    X_row = x["X_row"] + shift
    deg = np.diff(g["row_ptr_np"])
    r60, r120 = (int(r) for r in np.nonzero(deg >= 3)[0][:2])
    X_row[r60], X_row[r120] = x["X_row"][r60] - 60.0, x["X_row"][r120] - 120.0
    x["X_row"] = np.ascontiguousarray(X_row, dtype=np.float32)
    ref = _reference(g, x, normalize)
    res = _pair(g, _on_device(x), normalize)
    for name in gc.OUTPUTS:
        _check(res[name], ref[name], f"saturated {kind} normalize={normalize} {name}")
    for r in (r60, r120):
        assert np.abs(_np(res["out"])[r]).max() < 1e-15 and np.abs(_np(res["den"])[r]).max() < 1e-20, r
    assert (_np(res["den"])[r120] == 0).all()


# ---- 4. head offset and edge order ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f", [("lane", 3, 7), ("wave", 8, 16)])
def test_single_slot_touches_one_head(kind, h, f):
    """E differs from the base in one (edge, head) slot, G in one other slot of the same head, in another row.  The outputs
    of every other head equal the base run bit for bit; on the row side out and den move in the E slot's row only and dX_row
    in the two rows only; Z moves in the E slot only; dX_col, which the G slot reaches through val_idx, moves in that slot's
    column; the whole result is at the bar."""
    g = _graph(kind)
    x = _inputs(kind, h, f)
    deg = np.diff(g["row_ptr_np"])
    row_e, row_g = (int(r) for r in np.nonzero(deg >= 3)[0][1:3])
    slot_e, slot_g, head = int(g["row_ptr_np"][row_e]) + 1, int(g["row_ptr_np"][row_g]) + 2, h - 2
    one = dict(x, E=x["E"].copy(), G=x["G"].copy())
    one["E"][slot_e, head] += np.linspace(0.5, 1.5, f, dtype=np.float32)
    one["G"][slot_g, head] += np.linspace(-1.0, 1.0, f, dtype=np.float32) + np.float32(0.25)
    base, res = _pair(g, _on_device(x)), _pair(g, _on_device(one))
    others = [hd for hd in range(h) if hd != head]
    for name in gc.OUTPUTS:
        assert torch.equal(res[name][:, others], base[name][:, others]), name
        assert not torch.equal(res[name][:, head], base[name][:, head]), name
    rest = ~np.isin(np.arange(g["m"]), (row_e, row_g))
    for name in ("out", "den", "dX_row"):                             # the row side: only the two rows move ...
        assert torch.equal(res[name][rest], base[name][rest]), name
    for name in ("out", "den"):                                       # ... and G does not reach the forward
        assert torch.equal(res[name][row_g], base[name][row_g]), name
    assert not torch.equal(res["dX_row"][row_g], base["dX_row"][row_g])
    assert not torch.equal(res["dX_row"][row_e], base["dX_row"][row_e])
    other_slots = np.arange(g["nnz"]) != slot_e
    assert torch.equal(res["Z"][other_slots], base["Z"][other_slots])
    assert not torch.equal(res["Z"][slot_e, head], base["Z"][slot_e, head])
    col_g = int(g["col_ind_np"][slot_g])
    assert not torch.equal(res["dX_col"][col_g, head], base["dX_col"][col_g, head])
    outside = ~np.isin(np.arange(g["nnz"]), np.r_[np.arange(g["row_ptr_np"][row_e], g["row_ptr_np"][row_e + 1]), slot_g])
    assert torch.equal(res["dE"][outside], base["dE"][outside])
    ref = _reference(g, one, 1)
    for name in gc.OUTPUTS:
        _check(res[name], ref[name], f"single slot {kind} {name}")


# ---- 5. rectangular graphs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", gc.MODES, ids=["norm", "plain"])
@pytest.mark.parametrize("kind,h,f", [("tall", 2, 20), ("wide", 1, 128), ("wide", 3, 7)])
def test_rectangular(kind, h, f, normalize):
    """tall 600 x 40: a lane group per row, a wave per column; wide 40 x 600: a wave per row, a lane group per column
    (tests/rect_cases.py).  Every output at the bar against the float64 reference on the m x n_cols graph."""
    g = rc.graph(kind)
    y = rc.inputs("edge", g, h, f, unit_val=True)
    rng = np.random.default_rng(5 + h + f)
    x = dict(X_row=y["Q"] * np.float32(f ** 0.25), X_col=y["K"] * np.float32(f ** 0.25), V=y["V"], dO=y["dO"], E=y["E"],
             G=(0.25 * rng.standard_normal(y["E"].shape)).astype(np.float32))
    ref = _reference(g, x, normalize)
    dg = {k: _dev(g[k], torch.int32) for k in ("row_ptr", "col_ind", "col_ptr", "row_ind", "val_idx")}
    res = _pair(dg, _on_device(x), normalize)
    assert res["out"].shape == res["den"].shape == res["dX_row"].shape == (g["m"], h, f)
    assert res["dX_col"].shape == res["dV"].shape == (g["n_cols"], h, f) and res["Z"].shape == res["dE"].shape == (g["nnz"], h, f)
    for name in gc.OUTPUTS:
        _check(res[name], ref[name], f"rect {kind} h{h} f{f} normalize={normalize} {name}")
    assert (_np(res["out"])[g["deg"] == 0] == 0).all() and (_np(res["dX_col"])[g["indeg"] == 0] == 0).all()
    assert (_np(res["dV"])[g["indeg"] == 0] == 0).all()


@pytest.mark.parametrize("normalize", gc.MODES, ids=["norm", "plain"])
@pytest.mark.parametrize("kind,h,f", [("lane", 2, 20), ("wave", 1, 128)])
def test_square_entry_is_the_rect_entry(kind, h, f, normalize):
    """dfgnn_gatedgcn_fwd / dfgnn_gatedgcn_bwd called through the C ABI equal the _rect entries with n_cols = m (which the
    bindings call) bit for bit; normalize = 0 takes NULL for out, den and the scratch."""
    from _binding_util import call
    g = _graph(kind)
    d = _on_device(_inputs(kind, h, f))
    res = _pair(g, d, normalize)
    m, nnz = g["m"], g["nnz"]
    e = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
    out, den, Z = e(m, h, f), e(m, h, f), e(nnz, h, f)
    call("dfgnn_gatedgcn_fwd", "gatedgcn_forward", DEV, m, nnz, h, f, g["row_ptr"], g["col_ind"], d["X_row"], d["X_col"],
         d["V"], d["E"], normalize, EPS, den, out, Z)
    dXr, dXc, dV, dE, ws = e(m, h, f), e(m, h, f), e(m, h, f), e(nnz, h, f), e(m, h, f)
    saved = (out, den, d["dO"], d["G"], dXr, dXc, dV, dE, ws) if normalize else (None, None, d["dO"], d["G"], dXr, dXc, dV, dE, None)
    call("dfgnn_gatedgcn_bwd", "gatedgcn_backward", DEV, m, nnz, h, f, g["row_ptr"], g["col_ind"], g["col_ptr"], g["row_ind"],
         g["val_idx"], d["X_row"], d["X_col"], d["V"], d["E"], normalize, EPS, *saved)
    torch.cuda.synchronize()
    for name, got in dict(out=out, den=den, Z=Z, dX_row=dXr, dX_col=dXc, dV=dV, dE=dE).items():
        assert torch.equal(got, res[name]), name


# ---- 6. operator ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", gc.MODES, ids=["norm", "plain"])
@pytest.mark.parametrize("kind,h,f", [("lane", 2, 20), ("wave", 8, 16)])
def test_operator_equals_raw_calls(kind, h, f, normalize):
    """GatedGCNConvFuse + autograd.grad of (out, Z) with (dO, G) equals the raw binding calls bit for bit; Z is not among the
    saved tensors; edge_out=False, E.requires_grad == False and a Z that is returned but not used (its gradient arrives as
    None -> NULL) each give the bits of the matching raw call; so does E = None."""
    from DFGNN.operators.fused_gtconv import GatedGCNConvFuse, GatedGCNConvFuse_inference
    g = _graph(kind)
    d = _on_device(_inputs(kind, h, f))
    raw, raw_nog = _pair(g, d, normalize), _pair(g, d, normalize, with_G=False)
    graph_args = (g["row_ptr"], g["col_ind"], g["col_ptr"], g["row_ind"], g["val_idx"])
    names = ("dX_row", "dX_col", "dV", "dE")
    xr, xc, v, e = (d[n].clone().requires_grad_(True) for n in ("X_row", "X_col", "V", "E"))
    out, Z = GatedGCNConvFuse(*graph_args, xr, xc, v, e, normalize, EPS)
    saved = out.grad_fn.saved_tensors
    assert not any(t.data_ptr() == Z.data_ptr() for t in saved)                             # Z is recomputed, not saved
    assert not any(t.dim() == 3 and t.size(0) == g["nnz"] and t.data_ptr() != e.data_ptr() for t in saved)
    assert any(t.data_ptr() == out.data_ptr() for t in saved) == bool(normalize)            # out and den: normalize only
    grads = torch.autograd.grad((out, Z), (xr, xc, v, e), (d["dO"], d["G"]), retain_graph=True)
    assert torch.equal(out, raw["out"]) and torch.equal(Z, raw["Z"])
    for got, name in zip(grads, names):
        assert torch.equal(got, raw[name]), name
    grads = torch.autograd.grad(out, (xr, xc, v, e), d["dO"])                                # Z returned but unused
    for got, name in zip(grads, names):
        assert torch.equal(got, raw_nog[name]), name
    inf_args = (g["row_ptr"], g["col_ind"], d["X_row"], d["X_col"], d["V"], d["E"], normalize, EPS)
    o_inf, z_inf = GatedGCNConvFuse_inference(*inf_args, edge_out=True)
    assert torch.equal(o_inf, raw["out"]) and torch.equal(z_inf, raw["Z"])
    assert torch.equal(GatedGCNConvFuse_inference(*inf_args), raw["out"])
    only = GatedGCNConvFuse(*graph_args, xr, xc, v, e, normalize, EPS, edge_out=False)        # no edge output
    assert isinstance(only, torch.Tensor) and torch.equal(only, raw["out"])
    grads = torch.autograd.grad(only, (xr, xc, v, e), d["dO"])
    for got, name in zip(grads, names):
        assert torch.equal(got, raw_nog[name]), name
    xr, xc, v = (d[n].clone().requires_grad_(True) for n in ("X_row", "X_col", "V"))        # a frozen E
    out, Z = GatedGCNConvFuse(*graph_args, xr, xc, v, d["E"], normalize, EPS)
    torch.autograd.backward((out, Z), (d["dO"], d["G"]))
    assert d["E"].grad is None
    for t, name in zip((xr, xc, v), names):
        assert torch.equal(t.grad, raw[name]), name
    raw_noe = _pair(g, d, normalize, with_E=False)                                          # no edge term
    xr, xc, v = (d[n].clone().requires_grad_(True) for n in ("X_row", "X_col", "V"))
    out, Z = GatedGCNConvFuse(*graph_args, xr, xc, v, None, normalize, EPS)
    grads = torch.autograd.grad((out, Z), (xr, xc, v), (d["dO"], d["G"]))
    assert torch.equal(out, raw_noe["out"]) and torch.equal(Z, raw_noe["Z"])
    for got, name in zip(grads, names):
        assert torch.equal(got, raw_noe[name]), name


# ---- 7. memory --------------------------------------------------------------------------------------------------------
def test_memory_of_one_step():
    """The wave graph at h = 2, f = 16.  The fused step allocates out, den, dX_row, dX_col, dV and the row-sized scratch
    (6 bytes(X_row)), autograd's handful of small blocks, and Z and dE when they are wanted -- nothing else of size nnz h f:
    its peak over the inputs (G among them) is at most bytes(Z) + bytes(dE) + 8 bytes(X_row) + 64 KB with both, 8
    bytes(X_row) + 64 KB with neither.  The index-op formulation keeps X_row[rows], X_col[cols], z, sg, sg (.) V[cols] and
    their gradients."""
    from DFGNN.layers import index_ops_gatedgcn
    from DFGNN.operators.fused_gtconv import GatedGCNConvFuse
    g, h, f = _graph("wave"), 2, 16
    d = _on_device(_inputs("wave", h, f))
    rows = g["rows"].to(DEV)
    bytes_x, bytes_e = 4 * g["m"] * h * f, 4 * g["nnz"] * h * f
    assert bytes_e > 16 * bytes_x

    def peak(fused, edge):
        xr, xc, v = (d[n].clone().requires_grad_(True) for n in ("X_row", "X_col", "V"))
        e = d["E"].clone().requires_grad_(True) if edge else None

        def step():
            if fused:
                res = GatedGCNConvFuse(g["row_ptr"], g["col_ind"], g["col_ptr"], g["row_ind"], g["val_idx"], xr, xc, v, e,
                                       True, EPS, edge_out=edge)
                o, z = res if edge else (res, None)
            else:
                o, z = index_ops_gatedgcn(rows, g["col_ind"], xr, xc, v, e, True, EPS)
            if edge:
                return torch.autograd.grad((o, z), (xr, xc, v, e), (d["dO"], d["G"]))
            return torch.autograd.grad(o, (xr, xc, v), d["dO"])

        step()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res = step()
        torch.cuda.synchronize()
        assert len(res) == (4 if edge else 3)
        return torch.cuda.max_memory_allocated() - base

    p_with, p_without, p_torch = peak(True, True), peak(True, False), peak(False, True)
    print(f"gatedgcn peak of one fwd+bwd: fused with Z and dE {p_with} B, with neither {p_without} B, index ops {p_torch} B; "
          f"bytes(E) = {bytes_e} B, bytes(X_row) = {bytes_x} B")
    assert p_with <= 2 * bytes_e + 8 * bytes_x + 65536
    assert p_without <= 8 * bytes_x + 65536
    assert p_torch > p_with


# ---- 8. layer ---------------------------------------------------------------------------------------------------------
def test_layer_against_its_torch_branch():
    """GatedGCNConv(fuse=True) in training mode at two heads against its own fuse=False branch on the cora-like graph:
    h_out, e_out and the gradients of all five projection weights under a loss that uses both outputs; in .eval() the
    inference operator gives the same outputs; both --conv gatedgcn formats run."""
    import argparse

    from DFGNN.layers import GatedGCNConv, load_graphconv_layer, load_prepfunc
    from DFGNN.utils import synthetic as S
    torch.manual_seed(1)
    g = S.cora_like().to(DEV)
    args = argparse.Namespace(conv="gatedgcn", format="forward", dim=64, heads=2)
    params = load_prepfunc(args)(g)
    nnz = params[3].numel()
    layer = GatedGCNConv(64, 64, 2, edge_dim=8).to(DEV).train()
    x = torch.randn(g.num_nodes(), 64, device=DEV)
    edge_attr = torch.randn(nnz, 8, device=DEV)
    names = ("lin_self", "lin_msg", "lin_row", "lin_col", "lin_edge")
    weights = [getattr(layer, n).weight for n in names]
    outs, grads = [], []
    for fuse in (False, True):
        layer.zero_grad()
        out, e_out = layer(params, x, edge_attr, fuse=fuse)
        assert out.shape == (g.num_nodes(), 64) and e_out.shape == (nnz, 64)
        loss = (out * torch.linspace(-1, 1, out.numel(), device=DEV).reshape(out.shape)).sum()
        loss = loss + (e_out * torch.linspace(1, -1, e_out.numel(), device=DEV).reshape(e_out.shape)).sum()
        loss.backward()
        outs.append((out.detach(), e_out.detach()))
        grads.append([p.grad.clone() for p in weights])
    _check(outs[1][0], outs[0][0], "layer h_out")
    _check(outs[1][1], outs[0][1], "layer e_out")
    for name, a, b in zip(names, *grads):
        _check(b, a, f"layer d{name}.weight")
    with torch.no_grad():
        out, e_out = layer.eval()(params, x, edge_attr, fuse=True)
        _check(out, outs[0][0], "layer eval h_out")
        _check(e_out, outs[0][1], "layer eval e_out")
    for fmt in ("forward", "forward_plain"):
        args = argparse.Namespace(conv="gatedgcn", format=fmt, dim=64, heads=2)
        timing = load_graphconv_layer(args).to(DEV).train()
        fused, ms = timing(load_prepfunc(args)(g), x, fuse=True)
        plain, _ = timing(params, x, fuse=False)
        assert fused.shape == (g.num_nodes(), 64) and ms > 0
        _check(fused, plain, f"--format {fmt}")


# ---- 9. empty problems ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", gc.MODES, ids=["norm", "plain"])
@pytest.mark.parametrize("m", [0, 5])
def test_empty_problems(m, normalize):
    """m == 0, and m == 5 without an edge (E, G [0, h, f]): zero outputs, no error."""
    import fused_gtconv as gt
    h, f = 2, 12
    i32 = dict(dtype=torch.int32, device=DEV)
    row_ptr, none = torch.zeros(m + 1, **i32), torch.zeros(0, **i32)
    x, dO, E = torch.randn(m, h, f, device=DEV), torch.randn(m, h, f, device=DEV), torch.zeros(0, h, f, device=DEV)
    out, den, Z = gt.gatedgcn_forward(row_ptr, none, x, x, x, E, normalize, EPS, need_Z=True)
    res = gt.gatedgcn_backward(row_ptr, none, row_ptr, none, none, x, x, x, E, out, den, dO, G=E, normalize=normalize, eps=EPS)
    torch.cuda.synchronize()
    assert out.shape == den.shape == (m, h, f) and all(t.shape == (m, h, f) for t in res[:3])
    assert res[3].shape == Z.shape == (0, h, f)
    if m:      # (m == 0 launches nothing)
        for t in (out, den) + tuple(res[:3]):
            assert (t == 0).all()


# ---- 10. the two transports agree -------------------------------------------------------------------------------------
def test_bindings_agree():
    """The torch C++ extension and the ctypes transport give bit-identical results for gatedgcn_inference, gatedgcn_forward
    and gatedgcn_backward (both modes; with and without E, G, Z, dE), and the same RuntimeError for a bad argument ([nnz, h,
    f] shapes included)."""
    import dfgnn_native
    import fused_gtconv as gt
    assert dfgnn_native.ext() is not None and hasattr(dfgnn_native.ext(), "gatedgcn_bwd")
    cases = [(_graph(kind), _on_device(_inputs(kind, h, f)), nz) for kind, h, f, nz in
             (("lane", 2, 20, 1), ("wave", 8, 16, 0), ("wave", 2, 7, 1))]

    def run():
        res = []
        for g, d, nz in cases:
            both = _pair(g, d, nz)
            res += [both[k] for k in gc.OUTPUTS]
            res += [_pair(g, d, nz, with_E=False, with_G=False, need_Z=False, need_dE=False)[k] for k in MAIN]
            res.append(gt.gatedgcn_inference(g["row_ptr"], g["col_ind"], d["X_row"], d["X_col"], d["V"], d["E"], nz, EPS))
        g, d, nz = cases[0]
        both = _pair(g, d, nz)
        errs = []
        for bad in (dict(row_ptr=g["row_ptr"].long()), dict(E=d["E"].transpose(0, 1).contiguous()),
                    dict(E=d["E"].reshape(g["nnz"], -1)), dict(E=d["E"].double()), dict(E=d["E"][1:]), dict(G=d["G"][1:]),
                    dict(G=d["G"].reshape(g["nnz"], -1)), dict(G=d["G"].double())):
            a = dict(row_ptr=g["row_ptr"], E=d["E"], G=d["G"])
            a.update(bad)
            try:
                if "G" in bad:
                    gt.gatedgcn_backward(g["row_ptr"], g["col_ind"], g["col_ptr"], g["row_ind"], g["val_idx"], d["X_row"],
                                         d["X_col"], d["V"], d["E"], both["out"], both["den"], d["dO"], G=a["G"])
                else:
                    gt.gatedgcn_forward(a["row_ptr"], g["col_ind"], d["X_row"], d["X_col"], d["V"], a["E"])
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
    assert len(via_ext) == len(via_ctypes) == 3 * (7 + 5 + 1)
    for a, b in zip(via_ext, via_ctypes):
        assert torch.equal(a, b)
    words = ("int32",) + ("E must have",) * 4 + ("G must have",) * 3
    for e1, e2, word in zip(err_ext, err_ctypes, words):
        assert e1 and e2 and word in e1 and word in e2, (e1, e2)
        if word != "int32":
            assert e1.splitlines()[0] == e2.splitlines()[0], (e1, e2)          # the same text on both transports


# ---- 11. HIP graph ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f", [("lane", 2, 20), ("wave", 1, 128)])
def test_hipgraph_capture(kind, h, f):
    """fwd + bwd recorded into a HIP graph (one stream, no parallel branches) replays bit-identically, also after X_row, E
    and G were overwritten in place."""
    import fused_gtconv as gt
    from DFGNN.utils import GraphedStep
    g = _graph(kind)
    d = _on_device(_inputs(kind, h, f))

    def step():
        out, den, Z = gt.gatedgcn_forward(g["row_ptr"], g["col_ind"], d["X_row"], d["X_col"], d["V"], d["E"], need_Z=True)
        return [out, Z] + list(gt.gatedgcn_backward(g["row_ptr"], g["col_ind"], g["col_ptr"], g["row_ind"], g["val_idx"],
                                                    d["X_row"], d["X_col"], d["V"], d["E"], out, den, d["dO"], G=d["G"]))

    eager = [t.clone() for t in step()]
    graphed = GraphedStep(step)
    for a, b in zip(eager, graphed.replay()):
        assert torch.equal(a, b)
    d["X_row"].mul_(0.5)                                   # next "batch" of features, same structure
    d["E"].add_(0.25)
    d["G"].mul_(-2.0)
    again = [t.clone() for t in graphed.replay()]
    for a, b in zip(step(), again):
        assert torch.equal(a, b)
    assert not torch.equal(again[0], eager[0]) and not torch.equal(again[5], eager[5])
