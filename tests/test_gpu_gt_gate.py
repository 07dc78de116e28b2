"""GPU tests of the GT conv with a per-edge multiplicative gate on the keys and an edge output (include/dfgnn.h:
dfgnn_gt_fwd_gate / dfgnn_gt_bwd_gate and their _rect forms; csrc/gt_gate_train.hip): inference, the training pair that
saves two floats per (row, head) and takes a second gradient stream G = d loss / d W, the autograd Function and the layer.
The reference is the float64 torch formulation of tests/gt_gate_cases.py on the CPU (index ops over the edge list,
gradients from torch.autograd.grad of (out, W) with (dO, G)); the bar is the project's own, max abs error <
1e-3 * max(1, max |ref|), all finite -- and, on the boundary-degree cases, the fp32-level bounds whose power
tests/test_gt_gate_host.py proves."""
import functools

import numpy as np
import pytest
import torch

import gt_gate_cases as gc
import parity_cases as pc
import rect_cases as rc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-3
SENTINEL = np.float32(-1e38)
MAIN = ("out", "row_max", "row_sum", "dQ", "dK", "dV")        # what the pair shares with the row-statistics pair


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
    print(f"gt_gate {what}: max abs err {err:.3e} (bound {bound:.3e})")
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
    g["rows_np"] = g["rows"].numpy()
    assert torch.equal(g["rows"][order].to(torch.int32), g["row_ind"].cpu())
    return g


@functools.lru_cache(maxsize=None)
def _inputs(kind, h, f, weighted):
    g = _graph(kind)
    m, nnz = g["m"], g["nnz"]
    rng = np.random.default_rng(1000 * h + f + 7 * weighted + 31)
    val = rng.uniform(0.5, 1.5, nnz) if weighted else np.ones(nnz)
    Q, K = (rng.standard_normal((m, h, f)) * f ** -0.25 for _ in range(2))
    V, dO = (rng.standard_normal((m, h, f)) for _ in range(2))
    E = 1.0 + 0.5 * rng.standard_normal((nnz, h, f))                   # a gate around 1, both signs occur
    G = 0.25 * rng.standard_normal((nnz, h, f))
    return {k: np.ascontiguousarray(a, dtype=np.float32) for k, a in dict(val=val, E=E, G=G, Q=Q, K=K, V=V, dO=dO).items()}


@functools.lru_cache(maxsize=None)
def _case(kind, h, f, weighted, with_G=True):
    """-> (host inputs dict, float64 reference dict); computed once per case and shared, nobody writes to it."""
    g, x = _graph(kind), _inputs(kind, h, f, weighted)
    return x, _reference(g, x, with_G)


def _reference(g, x, with_G=True):
    return gc.reference(g["row_ptr_np"], g["col_ind_np"], x["val"], x["E"], x["G"] if with_G else None, x["Q"], x["K"],
                        x["V"], x["dO"])


def _on_device(x):
    return {k: _dev(a) for k, a in x.items()}


def _pair(g, d, with_G=True, need_W=True, need_dE=True):
    import fused_gtconv as gt
    out, mx, sm, W = gt.gt_forward_gate(g["row_ptr"], g["col_ind"], d["val"], d["E"], d["Q"], d["K"], d["V"], need_W=need_W)
    dQ, dK, dV, dE = gt.gt_backward_gate(g["row_ptr"], g["col_ind"], d["val"], d["E"], g["col_ptr"], g["row_ind"],
                                         g["val_idx"], d["Q"], d["K"], d["V"], out, mx, sm, d["dO"],
                                         G=d["G"] if with_G else None, need_dE=need_dE)
    torch.cuda.synchronize()
    return dict(out=out, W=W, row_max=mx, row_sum=sm, dQ=dQ, dK=dK, dV=dV, dE=dE)


def _against_reference(res, ref, what, names=("out", "W", "row_sum", "dQ", "dK", "dV", "dE")):
    """Everything at the bar; row_max where the row has an edge, the sentinel exactly elsewhere."""
    live = ref["row_max"] != gc.SENTINEL_MAX
    for name in names:
        _check(res[name], ref[name], f"{what} {name}")
    mx = _np(res["row_max"])
    _check(mx[live], ref["row_max"][live], f"{what} row_max")
    assert (mx[~live] == SENTINEL).all(), what


# ---- 1. the pair against the reference --------------------------------------------------------------------------------
CASES = [("lane", 2, 20), ("lane", 3, 7), ("lane", 1, 128), ("wave", 1, 128), ("wave", 8, 16), ("wave", 2, 7)]


@pytest.mark.parametrize("with_G", [True, False], ids=["G", "noG"])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind,h,f", CASES)
def test_pair_against_reference(kind, h, f, weighted, with_G):
    """Both forms, float4 and scalar lane layouts, several heads (a wrong [nnz, h, f] offset shows there): every output at
    the bar; exact zeros and sentinels where a row / column has no edge; inference equals the training forward's out, two
    backward calls agree, need_W=False / need_dE=False leave every other output as it is, and G = zeros is G = None -- all
    bit for bit."""
    import fused_gtconv as gt
    g = _graph(kind)
    x, ref = _case(kind, h, f, weighted, with_G)
    d = _on_device(x)
    res = _pair(g, d, with_G)
    _against_reference(res, ref, f"{kind} h{h} f{f} val={weighted} G={with_G}")
    er, ecol = g["empty_rows"], g["empty_cols"]
    assert (_np(res["out"])[er] == 0).all() and (_np(res["dQ"])[er] == 0).all()
    assert (_np(res["dK"])[ecol] == 0).all() and (_np(res["dV"])[ecol] == 0).all()
    assert (_np(res["row_max"])[er] == SENTINEL).all() and (_np(res["row_sum"])[er] == 0).all()
    args = (g["row_ptr"], g["col_ind"], d["val"], d["E"], d["Q"], d["K"], d["V"])
    assert torch.equal(gt.gt_inference_gate(*args), res["out"])
    o2, w2 = gt.gt_inference_gate(*args, need_W=True)
    assert torch.equal(o2, res["out"]) and torch.equal(w2, res["W"])
    again, without = _pair(g, d, with_G), _pair(g, d, with_G, need_W=False, need_dE=False)
    assert without["dE"] is None and without["W"] is None and res["dE"].shape == res["W"].shape == (g["nnz"], h, f)
    for name in MAIN:
        assert torch.equal(res[name], again[name]) and torch.equal(res[name], without[name]), name
    assert torch.equal(res["dE"], again["dE"]) and torch.equal(res["W"], again["W"])
    if not with_G:
        zeros = _pair(g, dict(d, G=torch.zeros_like(d["G"])), True)
        for name in MAIN + ("W", "dE"):
            assert torch.equal(res[name], zeros[name]), name


# ---- 2. boundary degrees at fp32 level --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.case_ids("gt"), ids=str)
def test_boundary_degrees(case):
    """The 32 cases of the host power test, same inputs and bounds: every output within MARGIN x the float32 formulation's
    error (dK: MARGIN x DK_FACTOR, derived in tests/gt_bias_cases.py); row_max on rows with edges only.  Prints measured
    error / fp32 reference error per output (pytest -s).  Worst ratios on the MI355X: dK 5.05 at
    (32, 1) in the wave form with edge values, dE 3.47 at (7, 2) in the lane-group form, row_max 2.77, dQ 1.75, W 1.00, everything else below 1."""
    g = pc.graph(case[0], case[1])
    x, ref64, bounds = gc.boundary_references(case)
    dg = {k: _dev(g[k], torch.int32) for k in ("row_ptr", "col_ind", "col_ptr", "row_ind", "val_idx")}
    res = _pair(dg, _on_device(x))
    missed = []
    for name in gc.OUTPUTS:
        got = _np(res[name]).astype(np.float64)
        assert np.isfinite(got).all(), (case, name)
        err, at = gc.error_of(g, name, got, ref64[name], where=True)
        fp32 = bounds[name] / pc.MARGIN / (gc.DK_FACTOR if name == "dK" else 1.0)
        print(f"gt_gate boundary {case} {name}: measured {err:.3e} at (node, head) {at}, fp32 reference {fp32:.3e}, "
              f"ratio {err / fp32 if fp32 > 0 else float('nan'):.2f}, bound {bounds[name]:.3e}")
        if not err <= bounds[name]:
            missed.append((name, err, bounds[name]))
    er, ecol = np.diff(g["row_ptr"]) == 0, np.diff(g["col_ptr"]) == 0
    assert (_np(res["out"])[er] == 0).all() and (_np(res["dQ"])[er] == 0).all()
    assert (_np(res["dK"])[ecol] == 0).all() and (_np(res["dV"])[ecol] == 0).all()
    assert (_np(res["row_max"])[er] == SENTINEL).all() and (_np(res["row_sum"])[er] == 0).all()
    assert not missed, (case, missed)


# ---- 3. E = 1 is the row-statistics pair ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f,weighted", [("lane", 2, 20, True), ("wave", 1, 128, False), ("lane", 3, 7, False),
                                               ("wave", 8, 16, True)])
def test_unit_gate_reproduces_rowstats(kind, h, f, weighted):
    """E = 1, no W, no G: out, the statistics, dQ, dK, dV equal gt_forward_rowstats / gt_backward_rowstats bit for bit, and
    dE equals val_e dS_e Q_i (.) K_j of the reference."""
    import fused_gtconv as gt
    g = _graph(kind)
    x = dict(_inputs(kind, h, f, weighted))
    x["E"] = np.ones_like(x["E"])
    d = _on_device(x)
    res = _pair(g, d, with_G=False, need_W=False)
    out, mx, sm = gt.gt_forward_rowstats(g["row_ptr"], g["col_ind"], d["val"], d["Q"], d["K"], d["V"])
    dQ, dK, dV = gt.gt_backward_rowstats(g["row_ptr"], g["col_ind"], d["val"], g["col_ptr"], g["row_ind"], g["val_idx"],
                                         d["Q"], d["K"], d["V"], out, mx, sm, d["dO"])
    for name, want in (("out", out), ("row_max", mx), ("row_sum", sm), ("dQ", dQ), ("dK", dK), ("dV", dV)):
        assert torch.equal(res[name], want), name
    ref = _reference(g, x, with_G=False)
    _check(res["dE"], ref["dE"], f"E = 1 {kind} dE")
    assert np.abs(ref["dE"]).max() > 0.1


# ---- 4. head offset and edge order ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f", [("lane", 3, 7), ("wave", 8, 16)])
def test_single_slot_touches_one_head(kind, h, f):
    """E differs from 1 in one (edge, head) slot, G from 0 in one other slot of the same head, in another row.  The outputs
    of every other head equal the base run (E = 1, G = 0) bit for bit; on the row side out and the statistics move in the
    gated edge's row only and dQ in the two rows only; W moves in the gated slot only; dK, which the G slot reaches through
    val_idx, moves in that head; the whole result is at the bar."""
    g = _graph(kind)
    x = dict(_inputs(kind, h, f, True))
    base_x = dict(x, E=np.ones_like(x["E"]), G=np.zeros_like(x["G"]))
    deg = np.diff(g["row_ptr_np"])
    row_e, row_g = (int(r) for r in np.nonzero(deg >= 3)[0][1:3])
    slot_e, slot_g, head = int(g["row_ptr_np"][row_e]) + 1, int(g["row_ptr_np"][row_g]) + 2, h - 2
    one = dict(x, E=np.ones_like(x["E"]), G=np.zeros_like(x["G"]))
    one["E"][slot_e, head] = np.linspace(1.5, 2.5, f, dtype=np.float32)
    one["G"][slot_g, head] = np.linspace(-1.0, 1.0, f, dtype=np.float32) + np.float32(0.25)
    base, res = _pair(g, _on_device(base_x)), _pair(g, _on_device(one))
    others = [hd for hd in range(h) if hd != head]
    for name in MAIN + ("W", "dE"):
        assert torch.equal(res[name][:, others], base[name][:, others]), name
        assert name == "row_max" or not torch.equal(res[name][:, head], base[name][:, head]), name
    rest = ~np.isin(np.arange(g["m"]), (row_e, row_g))
    for name in ("out", "row_max", "row_sum", "dQ"):                  # the row side: only the two rows move ...
        assert torch.equal(res[name][rest], base[name][rest]), name
    for name in ("out", "row_max", "row_sum"):                        # ... and G does not reach the forward
        assert torch.equal(res[name][row_g], base[name][row_g]), name
    assert not torch.equal(res["dQ"][row_g], base["dQ"][row_g]) and not torch.equal(res["dQ"][row_e], base["dQ"][row_e])
    other_slots = np.arange(g["nnz"]) != slot_e
    assert torch.equal(res["W"][other_slots], base["W"][other_slots])
    col_g = int(g["col_ind_np"][slot_g])
    assert not torch.equal(res["dK"][col_g, head], base["dK"][col_g, head])
    outside = ~np.isin(np.arange(g["nnz"]), np.r_[np.arange(g["row_ptr_np"][row_e], g["row_ptr_np"][row_e + 1]), slot_g])
    assert torch.equal(res["dE"][outside], base["dE"][outside])
    ref = _reference(g, one)
    for name in ("out", "W", "dQ", "dK", "dV", "dE"):
        _check(res[name], ref[name], f"single slot {kind} {name}")


# ---- 5. rectangular graphs --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f", [("tall", 2, 20), ("wide", 1, 128), ("wide", 3, 7)])
def test_rectangular(kind, h, f):
    """tall 600 x 40: a lane group per row, a wave per column; wide 40 x 600: a wave per row, a lane group per column
    (tests/rect_cases.py).  Every output at the bar against the float64 reference on the m x n_cols graph."""
    g = rc.graph(kind)
    x = dict(rc.inputs("edge", g, h, f, unit_val=False))
    rng = np.random.default_rng(5 + h + f)
    x["E"] = (1.0 + x["E"]).astype(np.float32)
    x["G"] = (0.25 * rng.standard_normal(x["E"].shape)).astype(np.float32)
    ref = gc.reference(g["row_ptr"], g["col_ind"], x["val"], x["E"], x["G"], x["Q"], x["K"], x["V"], x["dO"])
    dg = {k: _dev(g[k], torch.int32) for k in ("row_ptr", "col_ind", "col_ptr", "row_ind", "val_idx")}
    res = _pair(dg, _on_device(x))
    assert res["out"].shape == res["dQ"].shape == (g["m"], h, f) and res["dK"].shape == res["dV"].shape == (g["n_cols"], h, f)
    _against_reference(res, ref, f"rect {kind} h{h} f{f}")
    assert (_np(res["out"])[g["deg"] == 0] == 0).all() and (_np(res["dK"])[g["indeg"] == 0] == 0).all()


@pytest.mark.parametrize("kind,h,f", [("lane", 2, 20), ("wave", 1, 128)])
def test_square_entry_is_the_rect_entry(kind, h, f):
    """dfgnn_gt_fwd_gate / dfgnn_gt_bwd_gate called through the C ABI equal the _rect entries with n_cols = m (which the
    bindings call) bit for bit."""
    from _binding_util import call
    g = _graph(kind)
    d = _on_device(_inputs(kind, h, f, True))
    res = _pair(g, d)
    m, nnz = g["m"], g["nnz"]
    e = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
    out, W, mx, sm = e(m, h, f), e(nnz, h, f), e(m, h), e(m, h)
    call("dfgnn_gt_fwd_gate", "gt_forward_gate", d["Q"].device, m, nnz, h, f, g["row_ptr"], g["col_ind"], d["val"], d["E"],
         d["Q"], d["K"], d["V"], mx, sm, out, W)
    delta, dQ, dK, dV, dE = e(m, h), e(m, h, f), e(m, h, f), e(m, h, f), e(nnz, h, f)
    call("dfgnn_gt_bwd_gate", "gt_backward_gate", d["Q"].device, m, nnz, h, f, g["row_ptr"], g["col_ind"], d["val"], d["E"],
         g["col_ptr"], g["row_ind"], g["val_idx"], d["Q"], d["K"], d["V"], out, mx, sm, d["dO"], d["G"], delta, dQ, dK, dV, dE)
    torch.cuda.synchronize()
    for name, got in dict(out=out, W=W, row_max=mx, row_sum=sm, dQ=dQ, dK=dK, dV=dV, dE=dE).items():
        assert torch.equal(got, res[name]), name


# ---- 6. operator ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f,weighted", [("lane", 2, 20, True), ("wave", 8, 16, False)])
def test_operator_equals_raw_calls(kind, h, f, weighted):
    """GTConvFuse_gate + autograd.grad of (out, W) with (dO, G) equals the raw binding calls bit for bit; `val` is saved only
    when it is not all ones; edge_out=False, E.requires_grad == False and a W that is returned but not used (its gradient
    arrives as None -> NULL) each give the bits of the matching raw call."""
    from DFGNN.operators.fused_gtconv import GTConvFuse_gate, GTConvFuse_inference_gate
    g = _graph(kind)
    d = _on_device(_inputs(kind, h, f, weighted))
    raw, raw_nog = _pair(g, d), _pair(g, d, with_G=False)
    graph_args = (None, g["row_ptr"], g["col_ind"], d["val"], g["col_ptr"], g["row_ind"], g["val_idx"], 0)
    q, k, v, e = (d[n].clone().requires_grad_(True) for n in ("Q", "K", "V", "E"))
    out, W = GTConvFuse_gate(*graph_args, q, k, v, e)
    assert any(t.data_ptr() == d["val"].data_ptr() for t in out.grad_fn.saved_tensors) == weighted
    assert not any(t.data_ptr() == W.data_ptr() for t in out.grad_fn.saved_tensors)       # W is recomputed, not saved
    grads = torch.autograd.grad((out, W), (q, k, v, e), (d["dO"], d["G"]), retain_graph=True)
    assert torch.equal(out, raw["out"]) and torch.equal(W, raw["W"])
    for got, name in zip(grads, ("dQ", "dK", "dV", "dE")):
        assert torch.equal(got, raw[name]), name
    grads = torch.autograd.grad(out, (q, k, v, e), d["dO"])                                # W returned but unused
    for got, name in zip(grads, ("dQ", "dK", "dV", "dE")):
        assert torch.equal(got, raw_nog[name]), name
    o_inf, w_inf = GTConvFuse_inference_gate(g["row_ptr"], g["col_ind"], d["val"], d["Q"], d["K"], d["V"], d["E"])
    assert torch.equal(o_inf, raw["out"]) and torch.equal(w_inf, raw["W"])
    only = GTConvFuse_gate(*graph_args, q, k, v, e, edge_out=False)                        # no edge output
    assert isinstance(only, torch.Tensor) and torch.equal(only, raw["out"])
    grads = torch.autograd.grad(only, (q, k, v, e), d["dO"])
    for got, name in zip(grads, ("dQ", "dK", "dV", "dE")):
        assert torch.equal(got, raw_nog[name]), name
    assert torch.equal(GTConvFuse_inference_gate(g["row_ptr"], g["col_ind"], d["val"], d["Q"], d["K"], d["V"], d["E"],
                                                 edge_out=False), raw["out"])
    q, k, v = (d[n].clone().requires_grad_(True) for n in ("Q", "K", "V"))                 # a frozen E
    out, W = GTConvFuse_gate(*graph_args, q, k, v, d["E"])
    torch.autograd.backward((out, W), (d["dO"], d["G"]))
    assert d["E"].grad is None
    for t, name in zip((q, k, v), ("dQ", "dK", "dV")):
        assert torch.equal(t.grad, raw[name]), name


# ---- 7. memory --------------------------------------------------------------------------------------------------------
def test_memory_of_one_step():
    """The wave graph at h = 2, f = 16.  The fused step allocates out, dQ, dK, dV (4 bytes(Q)), the three [m, h] arrays
    row_max, row_sum, delta, autograd's handful of small blocks, and W and dE when they are wanted -- nothing else of size
    nnz h f: its peak over the inputs (G among them) is at most bytes(W) + bytes(dE) + 8 bytes(Q) + 64 KB with both,
    8 bytes(Q) + 64 KB with neither.  The index-op formulation keeps Q[rows], K[cols] E, W and their gradients."""
    from DFGNN.layers.GT.gtconv_layer_gate import index_ops_mha_gate
    from DFGNN.operators.fused_gtconv import GTConvFuse_gate
    g, h, f = _graph("wave"), 2, 16
    d = _on_device(_inputs("wave", h, f, True))
    rows = g["rows"].to(DEV)
    bytes_q, bytes_e = 4 * g["m"] * h * f, 4 * g["nnz"] * h * f
    assert bytes_e > 16 * bytes_q

    def peak(fused, edge):
        q, k, v = (d[n].clone().requires_grad_(True) for n in ("Q", "K", "V"))
        e = d["E"].clone().requires_grad_(edge)

        def step():
            if fused:
                res = GTConvFuse_gate(None, g["row_ptr"], g["col_ind"], d["val"], g["col_ptr"], g["row_ind"], g["val_idx"],
                                      0, q, k, v, e, edge_out=edge)
                o, w = res if edge else (res, None)
            else:
                o, w = index_ops_mha_gate(rows, g["col_ind"], d["val"], q, k, v, e)
            if edge:
                return torch.autograd.grad((o, w), (q, k, v, e), (d["dO"], d["G"]))
            return torch.autograd.grad(o, (q, k, v), d["dO"])

        step()                                                   # (the all-ones test of `val` is cached here)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res = step()
        torch.cuda.synchronize()
        assert len(res) == (4 if edge else 3)
        return torch.cuda.max_memory_allocated() - base

    p_with, p_without, p_torch = peak(True, True), peak(True, False), peak(False, True)
    print(f"gt_gate peak of one fwd+bwd: fused with W and dE {p_with} B, with neither {p_without} B, index ops {p_torch} B; "
          f"bytes(E) = {bytes_e} B, bytes(Q) = {bytes_q} B")
    assert p_with <= 2 * bytes_e + 8 * bytes_q + 65536
    assert p_without <= 8 * bytes_q + 65536
    assert p_torch > p_with


# ---- 8. layer ---------------------------------------------------------------------------------------------------------
def test_layer_against_its_torch_branch():
    """SparseMHA_gate(fuse=True) in training mode at two heads against its own fuse=False branch on the cora-like graph:
    h_out, e_out and the gradients of the q / k / v / edge projection weights under a loss that uses both outputs; in
    .eval() the inference operator gives the same outputs; --conv gt --format forward_gate runs."""
    import argparse

    from DFGNN.layers import SparseMHA_gate, load_graphconv_layer, preprocess_Hyper_fw_bw
    from DFGNN.utils import synthetic as S
    torch.manual_seed(1)
    g = S.cora_like().to(DEV)
    params = preprocess_Hyper_fw_bw(g)
    nnz = params[3].numel()
    layer = SparseMHA_gate(64, 64, 2, edge_dim=8).to(DEV).train()
    x = torch.randn(g.num_nodes(), 64, device=DEV)
    edge_attr = torch.randn(nnz, 8, device=DEV)
    weights = (layer.q_proj.weight, layer.k_proj.weight, layer.v_proj.weight, layer.lin_edge.weight)
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
    for name, a, b in zip(("q_proj.weight", "k_proj.weight", "v_proj.weight", "lin_edge.weight"), *grads):
        _check(b, a, f"layer d{name}")
    with torch.no_grad():
        out, e_out = layer.eval()(params, x, edge_attr, fuse=True)
        _check(out, outs[0][0], "layer eval h_out")
        _check(e_out, outs[0][1], "layer eval e_out")
    args = argparse.Namespace(conv="gt", format="forward_gate", dim=64, heads=2)
    out, ms = load_graphconv_layer(args).to(DEV).train()(params, x, fuse=True)
    assert out.shape == (g.num_nodes(), 64) and ms > 0


# ---- 9. empty problems ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [0, 5])
def test_empty_problems(m):
    """m == 0, and m == 5 without an edge (E, G [0, h, f]): zero outputs, sentinels, no error."""
    import fused_gtconv as gt
    h, f = 2, 12
    i32 = dict(dtype=torch.int32, device=DEV)
    row_ptr, none = torch.zeros(m + 1, **i32), torch.zeros(0, **i32)
    x, dO, E = torch.randn(m, h, f, device=DEV), torch.randn(m, h, f, device=DEV), torch.zeros(0, h, f, device=DEV)
    out, mx, sm, W = gt.gt_forward_gate(row_ptr, none, None, E, x, x, x)
    dQ, dK, dV, dE = gt.gt_backward_gate(row_ptr, none, None, E, row_ptr, none, none, x, x, x, out, mx, sm, dO, G=E)
    torch.cuda.synchronize()
    assert out.shape == dQ.shape == dK.shape == dV.shape == (m, h, f) and mx.shape == sm.shape == (m, h)
    assert dE.shape == W.shape == (0, h, f)
    if m:      # (m == 0 launches nothing)
        for t in (out, dQ, dK, dV, sm):
            assert (t == 0).all()
        assert (mx == -1e38).all()


# ---- 10. the two transports agree -------------------------------------------------------------------------------------
def test_bindings_agree():
    """The torch C++ extension and the ctypes transport give bit-identical results for gt_inference_gate, gt_forward_gate and
    gt_backward_gate (with and without W, G, dE), and the same RuntimeError for a bad argument ([nnz, h, f] shapes
    included)."""
    import dfgnn_native
    import fused_gtconv as gt
    assert dfgnn_native.ext() is not None and hasattr(dfgnn_native.ext(), "gt_bwd_gate")
    cases = [(_graph(kind), _on_device(_inputs(kind, h, f, w))) for kind, h, f, w in
             (("lane", 2, 20, True), ("wave", 8, 16, False), ("wave", 2, 7, True))]

    def run():
        res = []
        for g, d in cases:
            both = _pair(g, d)
            res += [both[k] for k in gc.OUTPUTS]
            res += [_pair(g, d, with_G=False, need_W=False, need_dE=False)[k] for k in MAIN]
            res.append(gt.gt_inference_gate(g["row_ptr"], g["col_ind"], d["val"], d["E"], d["Q"], d["K"], d["V"]))
        g, d = cases[0]
        both = _pair(g, d)
        errs = []
        for bad in (dict(row_ptr=g["row_ptr"].long()), dict(E=d["E"].transpose(0, 1).contiguous()),
                    dict(E=d["E"].reshape(g["nnz"], -1)), dict(E=d["E"].double()), dict(G=d["G"][1:]),
                    dict(G=d["G"].reshape(g["nnz"], -1))):
            a = dict(row_ptr=g["row_ptr"], E=d["E"], G=d["G"])
            a.update(bad)
            try:
                if "G" in bad:
                    gt.gt_backward_gate(g["row_ptr"], g["col_ind"], d["val"], d["E"], g["col_ptr"], g["row_ind"], g["val_idx"],
                                        d["Q"], d["K"], d["V"], both["out"], both["row_max"], both["row_sum"], d["dO"], G=a["G"])
                else:
                    gt.gt_forward_gate(a["row_ptr"], g["col_ind"], d["val"], a["E"], d["Q"], d["K"], d["V"])
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
    assert len(via_ext) == len(via_ctypes) == 3 * (8 + 6 + 1)
    for a, b in zip(via_ext, via_ctypes):
        assert torch.equal(a, b)
    words = ("int32", "E must have", "E must have", "E must have", "G must have", "G must have")
    for e1, e2, word in zip(err_ext, err_ctypes, words):
        assert e1 and e2 and word in e1 and word in e2, (e1, e2)


# ---- 11. HIP graph ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f", [("lane", 2, 20), ("wave", 1, 128)])
def test_hipgraph_capture(kind, h, f):
    """fwd + bwd recorded into a HIP graph (one stream, no parallel branches) replays bit-identically, also after Q, E and G
    were overwritten in place."""
    import fused_gtconv as gt
    from DFGNN.utils import GraphedStep
    g = _graph(kind)
    d = _on_device(_inputs(kind, h, f, True))

    def step():
        out, mx, sm, W = gt.gt_forward_gate(g["row_ptr"], g["col_ind"], d["val"], d["E"], d["Q"], d["K"], d["V"])
        return [out, W] + list(gt.gt_backward_gate(g["row_ptr"], g["col_ind"], d["val"], d["E"], g["col_ptr"], g["row_ind"],
                                                   g["val_idx"], d["Q"], d["K"], d["V"], out, mx, sm, d["dO"], G=d["G"]))

    eager = [t.clone() for t in step()]
    graphed = GraphedStep(step)
    for a, b in zip(eager, graphed.replay()):
        assert torch.equal(a, b)
    d["Q"].mul_(0.5)                                       # next "batch" of features, same structure
    d["E"].add_(0.25)
    d["G"].mul_(-2.0)
    again = [t.clone() for t in graphed.replay()]
    for a, b in zip(step(), again):
        assert torch.equal(a, b)
    assert not torch.equal(again[0], eager[0]) and not torch.equal(again[5], eager[5])
