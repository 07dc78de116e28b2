"""GPU tests of the GT conv with per-edge feature vectors in keys and values (include/dfgnn.h: dfgnn_gt_fwd_edge /
dfgnn_gt_bwd_edge; csrc/gt_edge_train.hip): inference, the training pair that saves two floats per (row, head), the
autograd Function and the layer.  The reference is the float64 torch formulation of tests/gt_edge_cases.py on the CPU
(index ops over the edge list, gradients from torch.autograd.grad); the bar is the project's own, max abs error <
1e-3 * max(1, max |ref|), all finite -- and, on the boundary-degree cases, the fp32-level bounds whose power
tests/test_gt_edge_host.py proves."""
import functools

import numpy as np
import pytest
import torch

import gt_edge_cases as ec
import parity_cases as pc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-3
SENTINEL = np.float32(-1e38)


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
    print(f"gt_edge {what}: max abs err {err:.3e} (bound {bound:.3e})")
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
def _case(kind, h, f, weighted):
    """-> (host inputs dict, float64 reference dict); computed once per case and shared, nobody writes to it."""
    g = _graph(kind)
    m, nnz = g["m"], g["nnz"]
    rng = np.random.default_rng(1000 * h + f + 7 * weighted)
    val = rng.uniform(0.5, 1.5, nnz) if weighted else np.ones(nnz)
    Q, K = (rng.standard_normal((m, h, f)) * f ** -0.25 for _ in range(2))
    V, dO = (rng.standard_normal((m, h, f)) for _ in range(2))
    E = rng.standard_normal((nnz, h, f)) * 0.5
    x = {k: np.ascontiguousarray(a, dtype=np.float32) for k, a in dict(val=val, E=E, Q=Q, K=K, V=V, dO=dO).items()}
    ref = ec.reference(g["row_ptr_np"], g["col_ind_np"], x["val"], x["E"], x["Q"], x["K"], x["V"], x["dO"])
    return x, ref


def _on_device(x):
    return {k: _dev(a) for k, a in x.items()}


def _pair(g, d, need_dE=True):
    import fused_gtconv as gt
    out, mx, sm = gt.gt_forward_edge(g["row_ptr"], g["col_ind"], d["val"], d["E"], d["Q"], d["K"], d["V"])
    dQ, dK, dV, dE = gt.gt_backward_edge(g["row_ptr"], g["col_ind"], d["val"], d["E"], g["col_ptr"], g["row_ind"],
                                         g["val_idx"], d["Q"], d["K"], d["V"], out, mx, sm, d["dO"], need_dE=need_dE)
    torch.cuda.synchronize()
    return dict(out=out, row_max=mx, row_sum=sm, dQ=dQ, dK=dK, dV=dV, dE=dE)


def _against_reference(res, ref, what):
    """Everything at the bar; row_max where the row has an edge, the sentinel exactly elsewhere."""
    live = ref["row_max"] != ec.SENTINEL_MAX
    for name in ("out", "row_sum", "dQ", "dK", "dV", "dE"):
        _check(res[name], ref[name], f"{what} {name}")
    mx = _np(res["row_max"])
    _check(mx[live], ref["row_max"][live], f"{what} row_max")
    assert (mx[~live] == SENTINEL).all(), what


# ---- 1. the pair against the reference --------------------------------------------------------------------------------
CASES = [("lane", 2, 20), ("lane", 3, 7), ("lane", 1, 128), ("wave", 1, 128), ("wave", 8, 16), ("wave", 2, 7)]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind,h,f", CASES)
def test_pair_against_reference(kind, h, f, weighted):
    """Both forms, float4 and scalar lane layouts, several heads (a wrong [nnz, h, f] offset shows there): every output at
    the bar; exact zeros and sentinels where a row / column has no edge; inference equals the training forward's out, two
    backward calls agree, and need_dE=False leaves dQ, dK, dV as they are -- all bit for bit."""
    import fused_gtconv as gt
    g = _graph(kind)
    x, ref = _case(kind, h, f, weighted)
    d = _on_device(x)
    res = _pair(g, d)
    _against_reference(res, ref, f"{kind} h{h} f{f} val={weighted}")
    er, ecol = g["empty_rows"], g["empty_cols"]
    assert (_np(res["out"])[er] == 0).all() and (_np(res["dQ"])[er] == 0).all()
    assert (_np(res["dK"])[ecol] == 0).all() and (_np(res["dV"])[ecol] == 0).all()
    assert (_np(res["row_max"])[er] == SENTINEL).all() and (_np(res["row_sum"])[er] == 0).all()
    plain = gt.gt_inference_edge(g["row_ptr"], g["col_ind"], d["val"], d["E"], d["Q"], d["K"], d["V"])
    assert torch.equal(plain, res["out"])
    again, without = _pair(g, d), _pair(g, d, need_dE=False)
    assert without["dE"] is None and res["dE"].shape == (g["nnz"], h, f)
    for name in ("dQ", "dK", "dV"):
        assert torch.equal(res[name], again[name]) and torch.equal(res[name], without[name]), name
    assert torch.equal(res["dE"], again["dE"])


# ---- 2. boundary degrees at fp32 level --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.case_ids("gt"), ids=str)
def test_boundary_degrees(case):
    """The 32 cases of the host power test, same inputs and bounds: every output within MARGIN x the float32 formulation's
    error (dK: MARGIN x DK_FACTOR, derived in tests/gt_bias_cases.py); row_max on rows with edges only.  Prints measured
    error / fp32 reference error per output (pytest -s).  Worst ratios on the MI355X: row_max 5.08 (the degree-1 row at
    f = 7), dK 3.77 at (260, 1) in the lane-group form with unit values, dQ 2.03, dE 1.00, everything else below 1."""
    g = pc.graph(case[0], case[1])
    x, ref64, bounds = ec.boundary_references(case)
    dg = {k: _dev(g[k], torch.int32) for k in ("row_ptr", "col_ind", "col_ptr", "row_ind", "val_idx")}
    res = _pair(dg, _on_device(x))
    missed = []
    for name in ec.OUTPUTS:
        got = _np(res[name]).astype(np.float64)
        assert np.isfinite(got).all(), (case, name)
        err, at = ec.error_of(g, name, got, ref64[name], where=True)
        fp32 = bounds[name] / pc.MARGIN / (ec.DK_FACTOR if name == "dK" else 1.0)
        print(f"gt_edge boundary {case} {name}: measured {err:.3e} at (node, head) {at}, fp32 reference {fp32:.3e}, "
              f"ratio {err / fp32 if fp32 > 0 else float('nan'):.2f}, bound {bounds[name]:.3e}")
        if not err <= bounds[name]:
            missed.append((name, err, bounds[name]))
    er, ecol = np.diff(g["row_ptr"]) == 0, np.diff(g["col_ptr"]) == 0
    assert (_np(res["out"])[er] == 0).all() and (_np(res["dQ"])[er] == 0).all()
    assert (_np(res["dK"])[ecol] == 0).all() and (_np(res["dV"])[ecol] == 0).all()
    assert (_np(res["row_max"])[er] == SENTINEL).all() and (_np(res["row_sum"])[er] == 0).all()
    assert not missed, (case, missed)


# ---- 3. E = 0 is the row-statistics pair ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f,weighted", [("lane", 2, 20, True), ("wave", 1, 128, False)])
def test_zero_edge_features_reproduce_rowstats(kind, h, f, weighted):
    """E = 0: out, the statistics, dQ, dK, dV equal gt_forward_rowstats / gt_backward_rowstats bit for bit, and dE equals
    dS_e val_e Q_i + P_e dO_i of the reference -- an E read from a wrong slot that happens to cancel cannot hide here."""
    import fused_gtconv as gt
    g = _graph(kind)
    x = dict(_case(kind, h, f, weighted)[0])
    x["E"] = np.zeros_like(x["E"])
    d = _on_device(x)
    res = _pair(g, d)
    out, mx, sm = gt.gt_forward_rowstats(g["row_ptr"], g["col_ind"], d["val"], d["Q"], d["K"], d["V"])
    dQ, dK, dV = gt.gt_backward_rowstats(g["row_ptr"], g["col_ind"], d["val"], g["col_ptr"], g["row_ind"], g["val_idx"],
                                         d["Q"], d["K"], d["V"], out, mx, sm, d["dO"])
    for name, want in (("out", out), ("row_max", mx), ("row_sum", sm), ("dQ", dQ), ("dK", dK), ("dV", dV)):
        assert torch.equal(res[name], want), name
    ref = ec.reference(g["row_ptr_np"], g["col_ind_np"], x["val"], x["E"], x["Q"], x["K"], x["V"], x["dO"])
    _check(res["dE"], ref["dE"], f"E = 0 {kind} dE")
    assert np.abs(ref["dE"]).max() > 0.1


# ---- 4. head offset and edge order ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f", [("lane", 3, 7), ("wave", 8, 16)])
def test_single_slot_touches_one_head(kind, h, f):
    """E is non-zero in one (edge, head) slot only: the outputs of every other head equal the E = 0 run bit for bit; in
    that head the row side (out, the statistics, dQ) moves in the edge's row only; the whole result is at the bar."""
    g = _graph(kind)
    x = dict(_case(kind, h, f, True)[0])
    zero = dict(x, E=np.zeros_like(x["E"]))
    deg = np.diff(g["row_ptr_np"])
    row = int(np.nonzero(deg >= 3)[0][1])
    slot, head = int(g["row_ptr_np"][row]) + 1, h - 2
    one = dict(x, E=np.zeros_like(x["E"]))
    one["E"][slot, head] = np.linspace(1.0, 2.0, f, dtype=np.float32)
    base, res = _pair(g, _on_device(zero)), _pair(g, _on_device(one))
    others = [hd for hd in range(h) if hd != head]
    for name in ("out", "row_max", "row_sum", "dQ", "dK", "dV"):
        assert torch.equal(res[name][:, others], base[name][:, others]), name
        assert name == "row_max" or not torch.equal(res[name][:, head], base[name][:, head]), name
    assert torch.equal(res["dE"][:, others], base["dE"][:, others])
    rest = np.arange(g["m"]) != row
    for name in ("out", "row_max", "row_sum", "dQ"):                  # the row side: only the edge's row moves
        assert torch.equal(res[name][rest], base[name][rest]), name
    ref = ec.reference(g["row_ptr_np"], g["col_ind_np"], one["val"], one["E"], one["Q"], one["K"], one["V"], one["dO"])
    for name in ("out", "dQ", "dK", "dV", "dE"):
        _check(res[name], ref[name], f"single slot {kind} {name}")


# ---- 5. operator ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f,weighted", [("lane", 2, 20, True), ("wave", 8, 16, False)])
def test_operator_equals_raw_calls(kind, h, f, weighted):
    """GTConvFuse_edge + autograd.grad equals the raw binding calls bit for bit; `val` is saved only when it is not all
    ones; with E.requires_grad == False its gradient is None and the others are the same bits."""
    from DFGNN.operators.fused_gtconv import GTConvFuse_edge, GTConvFuse_inference_edge
    g = _graph(kind)
    d = _on_device(_case(kind, h, f, weighted)[0])
    raw = _pair(g, d)
    q, k, v, e = (d[n].clone().requires_grad_(True) for n in ("Q", "K", "V", "E"))
    out = GTConvFuse_edge(None, g["row_ptr"], g["col_ind"], d["val"], g["col_ptr"], g["row_ind"], g["val_idx"], 0, q, k, v, e)
    assert any(t.data_ptr() == d["val"].data_ptr() for t in out.grad_fn.saved_tensors) == weighted
    grads = torch.autograd.grad(out, (q, k, v, e), d["dO"])
    assert torch.equal(out, raw["out"])
    for got, name in zip(grads, ("dQ", "dK", "dV", "dE")):
        assert torch.equal(got, raw[name]), name
    assert torch.equal(GTConvFuse_inference_edge(g["row_ptr"], g["col_ind"], d["val"], d["Q"], d["K"], d["V"], d["E"]),
                       raw["out"])
    out = GTConvFuse_edge(None, g["row_ptr"], g["col_ind"], d["val"], g["col_ptr"], g["row_ind"], g["val_idx"], 0, q, k, v,
                          d["E"])
    out.backward(d["dO"])
    assert d["E"].grad is None
    for t, name in zip((q, k, v), ("dQ", "dK", "dV")):
        assert torch.equal(t.grad, raw[name]), name


# ---- 6. memory --------------------------------------------------------------------------------------------------------
def test_memory_of_one_step():
    """The wave graph at h = 2, f = 16.  The fused step allocates out, dQ, dK, dV (4 bytes(Q)), the three [m, h] arrays
    row_max, row_sum, delta, autograd's handful of small blocks, and dE when it is wanted -- nothing else of size nnz h f:
    its peak over the inputs is at most bytes(dE) + 8 bytes(Q) + 64 KB with dE, 8 bytes(Q) + 64 KB without.  The index-op
    formulation keeps K[cols] + E, V[cols] + E, Q[rows] and their products: more than 3 bytes(E)."""
    from DFGNN.layers.GT.gtconv_layer_edge import index_ops_mha_edge
    from DFGNN.operators.fused_gtconv import GTConvFuse_edge
    g, h, f = _graph("wave"), 2, 16
    d = _on_device(_case("wave", h, f, True)[0])
    rows = g["rows"].to(DEV)
    bytes_q, bytes_e = 4 * g["m"] * h * f, 4 * g["nnz"] * h * f
    assert bytes_e > 16 * bytes_q

    def peak(fused, e_grad):
        q, k, v = (d[n].clone().requires_grad_(True) for n in ("Q", "K", "V"))
        e = d["E"].clone().requires_grad_(e_grad)

        def step():
            if fused:
                o = GTConvFuse_edge(None, g["row_ptr"], g["col_ind"], d["val"], g["col_ptr"], g["row_ind"], g["val_idx"], 0,
                                    q, k, v, e)
            else:
                o = index_ops_mha_edge(rows, g["col_ind"], d["val"], q, k, v, e)
            return torch.autograd.grad(o, (q, k, v, e) if e_grad else (q, k, v), d["dO"])

        step()                                                   # (the all-ones test of `val` is cached here)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res = step()
        torch.cuda.synchronize()
        assert len(res) == (4 if e_grad else 3)
        return torch.cuda.max_memory_allocated() - base

    p_with, p_without, p_torch = peak(True, True), peak(True, False), peak(False, True)
    print(f"gt_edge peak of one fwd+bwd: fused with dE {p_with} B, without {p_without} B, index ops {p_torch} B; "
          f"bytes(E) = {bytes_e} B, bytes(Q) = {bytes_q} B")
    assert p_with <= bytes_e + 8 * bytes_q + 65536
    assert p_without <= 8 * bytes_q + 65536
    assert p_torch > 3 * bytes_e


# ---- 7. layer ---------------------------------------------------------------------------------------------------------
def test_layer_against_its_torch_branch():
    """SparseMHA_edge(fuse=True) in training mode at two heads against its own fuse=False branch on the cora-like graph: the
    output and the gradients of the q / k / v / edge projection weights; in .eval() the inference operator gives the same
    output; --conv gt --format forward_edge runs."""
    import argparse

    from DFGNN.layers import SparseMHA_edge, load_graphconv_layer, preprocess_Hyper_fw_bw
    from DFGNN.utils import synthetic as S
    torch.manual_seed(1)
    g = S.cora_like().to(DEV)
    params = preprocess_Hyper_fw_bw(g)
    nnz = params[3].numel()
    layer = SparseMHA_edge(64, 64, 2, edge_dim=8).to(DEV).train()
    x = torch.randn(g.num_nodes(), 64, device=DEV)
    edge_attr = torch.randn(nnz, 8, device=DEV)
    weights = (layer.q_proj.weight, layer.k_proj.weight, layer.v_proj.weight, layer.lin_edge.weight)
    outs, grads = [], []
    for fuse in (False, True):
        layer.zero_grad()
        out = layer(params, x, edge_attr, fuse=fuse)
        (out * torch.linspace(-1, 1, out.numel(), device=DEV).reshape(out.shape)).sum().backward()
        outs.append(out.detach())
        grads.append([p.grad.clone() for p in weights])
    _check(outs[1], outs[0], "layer out")
    for name, a, b in zip(("q_proj.weight", "k_proj.weight", "v_proj.weight", "lin_edge.weight"), *grads):
        _check(b, a, f"layer d{name}")
    with torch.no_grad():
        _check(layer.eval()(params, x, edge_attr, fuse=True), outs[0], "layer eval out")
    args = argparse.Namespace(conv="gt", format="forward_edge", dim=64, heads=2)
    out, ms = load_graphconv_layer(args).to(DEV).train()(params, x, fuse=True)
    assert out.shape == (g.num_nodes(), 64) and ms > 0


# ---- 8. empty problems ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [0, 5])
def test_empty_problems(m):
    """m == 0, and m == 5 without an edge (E [0, h, f]): zero outputs, sentinels, no error."""
    import fused_gtconv as gt
    h, f = 2, 12
    i32 = dict(dtype=torch.int32, device=DEV)
    row_ptr, none = torch.zeros(m + 1, **i32), torch.zeros(0, **i32)
    x, dO, E = torch.randn(m, h, f, device=DEV), torch.randn(m, h, f, device=DEV), torch.zeros(0, h, f, device=DEV)
    out, mx, sm = gt.gt_forward_edge(row_ptr, none, None, E, x, x, x)
    dQ, dK, dV, dE = gt.gt_backward_edge(row_ptr, none, None, E, row_ptr, none, none, x, x, x, out, mx, sm, dO)
    torch.cuda.synchronize()
    assert out.shape == dQ.shape == dK.shape == dV.shape == (m, h, f) and mx.shape == sm.shape == (m, h)
    assert dE.shape == (0, h, f)
    if m:      # (m == 0 launches nothing)
        for t in (out, dQ, dK, dV, sm):
            assert (t == 0).all()
        assert (mx == -1e38).all()


# ---- 9. the two transports agree --------------------------------------------------------------------------------------
def test_bindings_agree():
    """The torch C++ extension and the ctypes transport give bit-identical results for gt_inference_edge, gt_forward_edge and
    gt_backward_edge (with and without dE), and the same RuntimeError for a bad argument ([nnz, h, f] shape included)."""
    import dfgnn_native
    import fused_gtconv as gt
    assert dfgnn_native.ext() is not None and hasattr(dfgnn_native.ext(), "gt_bwd_edge")
    cases = [(_graph(kind), _on_device(_case(kind, h, f, w)[0])) for kind, h, f, w in
             (("lane", 2, 20, True), ("wave", 8, 16, False), ("wave", 2, 7, True))]

    def run():
        res = []
        for g, d in cases:
            both = _pair(g, d)
            res += [both[k] for k in ec.OUTPUTS]
            res += [_pair(g, d, need_dE=False)[k] for k in ("dQ", "dK", "dV")]
            res.append(gt.gt_inference_edge(g["row_ptr"], g["col_ind"], d["val"], d["E"], d["Q"], d["K"], d["V"]))
        g, d = cases[0]
        errs = []
        for bad in (dict(row_ptr=g["row_ptr"].long()), dict(E=d["E"].transpose(0, 1).contiguous()),
                    dict(E=d["E"].reshape(g["nnz"], -1)), dict(E=d["E"].double())):
            a = dict(row_ptr=g["row_ptr"], E=d["E"])
            a.update(bad)
            try:
                gt.gt_forward_edge(a["row_ptr"], g["col_ind"], d["val"], a["E"], d["Q"], d["K"], d["V"])
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
    assert len(via_ext) == len(via_ctypes) == 3 * 11
    for a, b in zip(via_ext, via_ctypes):
        assert torch.equal(a, b)
    for e1, e2, word in zip(err_ext, err_ctypes, ("int32", "E must have", "E must have", "E must have")):
        assert e1 and e2 and word in e1 and word in e2, (e1, e2)


# ---- 10. HIP graph ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f", [("lane", 2, 20), ("wave", 1, 128)])
def test_hipgraph_capture(kind, h, f):
    """fwd + bwd recorded into a HIP graph (one stream, no parallel branches) replays bit-identically, also after Q and E
    were overwritten in place."""
    import fused_gtconv as gt
    from DFGNN.utils import GraphedStep
    g = _graph(kind)
    d = _on_device(_case(kind, h, f, True)[0])

    def step():
        out, mx, sm = gt.gt_forward_edge(g["row_ptr"], g["col_ind"], d["val"], d["E"], d["Q"], d["K"], d["V"])
        return [out] + list(gt.gt_backward_edge(g["row_ptr"], g["col_ind"], d["val"], d["E"], g["col_ptr"], g["row_ind"],
                                                g["val_idx"], d["Q"], d["K"], d["V"], out, mx, sm, d["dO"]))

    eager = [t.clone() for t in step()]
    graphed = GraphedStep(step)
    for a, b in zip(eager, graphed.replay()):
        assert torch.equal(a, b)
    d["Q"].mul_(0.5)                                       # next "batch" of features, same structure
    d["E"].add_(0.25)
    again = [t.clone() for t in graphed.replay()]
    for a, b in zip(step(), again):
        assert torch.equal(a, b)
    assert not torch.equal(again[0], eager[0])
