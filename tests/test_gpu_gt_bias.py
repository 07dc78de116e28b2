"""GPU tests of the GT conv with a per-edge, per-head additive attention bias (include/dfgnn.h: dfgnn_gt_fwd_bias /
dfgnn_gt_bwd_bias; csrc/gt_bias_train.hip): inference, the training pair that saves two floats per (row, head), masks
(bias = -inf), the autograd Function and the layer.  The reference is the float64 torch formulation of
tests/gt_bias_cases.py on the CPU (index ops over the edge list, gradients from torch.autograd.grad, masked edges removed
from the graph per head); the bar is the project's own, max abs error < 1e-3 * max(1, max |ref|), all finite -- and, on the
boundary-degree cases, the fp32-level bounds whose power tests/test_gt_bias_host.py proves."""
import functools

import numpy as np
import pytest
import torch

import gt_bias_cases as bc
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
    print(f"gt_bias {what}: max abs err {err:.3e} (bound {bound:.3e})")
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


def _mask(g, h, rng):
    """[h, nnz] bool, about 30 % set: random entries, every edge of three rows in all heads, every edge of three other rows
    in head 0 only, every entry into three columns."""
    nnz, rp = g["nnz"], g["row_ptr_np"]
    mask = rng.random((h, nnz)) < 0.25
    with_edges = np.nonzero(np.diff(rp) > 1)[0]
    picked = rng.choice(with_edges, 6, replace=False)
    for i in picked[:3]:
        mask[:, rp[i]:rp[i + 1]] = True
    for i in picked[3:]:
        mask[0, rp[i]:rp[i + 1]] = True
    indeg = np.bincount(g["col_ind_np"], minlength=g["m"])
    for j in rng.choice(np.nonzero(indeg > 1)[0], 3, replace=False):
        mask[:, g["col_ind_np"] == j] = True
    return mask


@functools.lru_cache(maxsize=None)
def _case(kind, h, f, weighted, variant="plain"):
    """-> (host inputs dict, float64 reference dict); computed once per case and shared, nobody writes to it.
    variant: plain (bias ~ N(0, 1)), mask (plain with -inf entries, _mask), large (bias in {-40, +40})."""
    g = _graph(kind)
    m, nnz = g["m"], g["nnz"]
    rng = np.random.default_rng(1000 * h + f + 7 * weighted + len(variant))
    val = rng.uniform(0.5, 1.5, nnz) if weighted else np.ones(nnz)
    Q, K = (rng.standard_normal((m, h, f)) * f ** -0.25 for _ in range(2))
    V, dO = (rng.standard_normal((m, h, f)) for _ in range(2))
    bias = rng.standard_normal((h, nnz))
    if variant == "large":
        bias = rng.choice([-40.0, 40.0], (h, nnz))
    if variant == "mask":
        bias[_mask(g, h, rng)] = -np.inf
    x = {k: np.ascontiguousarray(a, dtype=np.float32) for k, a in
         dict(val=val, bias=bias, Q=Q, K=K, V=V, dO=dO).items()}
    ref = bc.reference(g["row_ptr_np"], g["col_ind_np"], x["val"], x["bias"], x["Q"], x["K"], x["V"], x["dO"])
    return x, ref


def _on_device(x):
    return {k: _dev(a) for k, a in x.items()}


def _pair(g, d, need_dbias=True):
    import fused_gtconv as gt
    out, mx, sm = gt.gt_forward_bias(g["row_ptr"], g["col_ind"], d["val"], d["bias"], d["Q"], d["K"], d["V"])
    dQ, dK, dV, db = gt.gt_backward_bias(g["row_ptr"], g["col_ind"], d["val"], d["bias"], g["col_ptr"], g["row_ind"],
                                         g["val_idx"], d["Q"], d["K"], d["V"], out, mx, sm, d["dO"], need_dbias=need_dbias)
    torch.cuda.synchronize()
    return dict(out=out, row_max=mx, row_sum=sm, dQ=dQ, dK=dK, dV=dV, dbias=db)


def _against_reference(res, ref, what):
    """Everything at the bar; row_max where the reference has a live edge, the sentinel exactly elsewhere."""
    live = ref["row_max"] != bc.SENTINEL_MAX
    for name in ("out", "row_sum", "dQ", "dK", "dV", "dbias"):
        _check(res[name], ref[name], f"{what} {name}")
    mx = _np(res["row_max"])
    _check(mx[live], ref["row_max"][live], f"{what} row_max")
    assert (mx[~live] == SENTINEL).all(), what
    return live


# ---- 1. the pair against the reference --------------------------------------------------------------------------------
CASES = [("lane", 2, 20), ("lane", 3, 7), ("lane", 1, 128), ("wave", 1, 128), ("wave", 8, 16), ("wave", 2, 7)]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind,h,f", CASES)
def test_pair_against_reference(kind, h, f, weighted):
    """Both forms, float4 and scalar lane layouts, several heads (a wrong [h, nnz] offset shows there): every output at the
    bar; exact zeros and sentinels where a row / column has no edge; inference equals the training forward's out, two
    backward calls agree, and need_dbias=False leaves dQ, dK, dV as they are -- all bit for bit."""
    import fused_gtconv as gt
    g = _graph(kind)
    x, ref = _case(kind, h, f, weighted)
    d = _on_device(x)
    res = _pair(g, d)
    _against_reference(res, ref, f"{kind} h{h} f{f} val={weighted}")
    er, ec = g["empty_rows"], g["empty_cols"]
    assert (_np(res["out"])[er] == 0).all() and (_np(res["dQ"])[er] == 0).all()
    assert (_np(res["dK"])[ec] == 0).all() and (_np(res["dV"])[ec] == 0).all()
    assert (_np(res["row_max"])[er] == SENTINEL).all() and (_np(res["row_sum"])[er] == 0).all()
    plain = gt.gt_inference_bias(g["row_ptr"], g["col_ind"], d["val"], d["bias"], d["Q"], d["K"], d["V"])
    assert torch.equal(plain, res["out"])
    again, without = _pair(g, d), _pair(g, d, need_dbias=False)
    assert without["dbias"] is None and res["dbias"].shape == (h, g["nnz"])
    for name in ("dQ", "dK", "dV"):
        assert torch.equal(res[name], again[name]) and torch.equal(res[name], without[name]), name
    assert torch.equal(res["dbias"], again["dbias"])


# ---- 2. masks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,f,weighted", [("lane", 20, True), ("wave", 16, False)])
def test_masks(kind, f, weighted):
    """About 30 % of the bias is -inf, with fully masked rows (both heads / head 0 only) and fully masked columns: everything
    finite, dbias exactly 0 at masked slots, a fully masked (row, head) exactly an empty row, a fully masked column exactly
    zero in dK and dV, the rest at the bar against the reference on the reduced graph."""
    h = 2
    g = _graph(kind)
    x, ref = _case(kind, h, f, weighted, "mask")
    masked = ~np.isfinite(x["bias"])
    assert 0.2 < masked.mean() < 0.45
    res = _pair(g, _on_device(x))
    for name, t in res.items():
        assert np.isfinite(_np(t)).all(), name
    live = _against_reference(res, ref, f"masks {kind}")
    assert (_np(res["dbias"])[masked] == 0).all()
    deg = np.diff(g["row_ptr_np"])
    rows, cols = g["rows_np"], g["col_ind_np"]
    unmasked_out = np.stack([np.bincount(rows[~masked[hd]], minlength=g["m"]) for hd in range(h)], axis=1)
    unmasked_in = np.stack([np.bincount(cols[~masked[hd]], minlength=g["m"]) for hd in range(h)], axis=1)
    dead_rows = (unmasked_out == 0) & (deg > 0)[:, None]                # (row, head) with edges, all masked
    dead_cols = (unmasked_in == 0) & (np.bincount(cols, minlength=g["m"]) > 0)[:, None]
    assert dead_rows[:, 0].sum() >= 6 and dead_rows[:, 1].sum() >= 3 and dead_cols.all(axis=1).sum() >= 3
    assert (live == (unmasked_out > 0)).all()
    assert (_np(res["out"])[dead_rows] == 0).all() and (_np(res["dQ"])[dead_rows] == 0).all()
    assert (_np(res["row_max"])[dead_rows] == SENTINEL).all() and (_np(res["row_sum"])[dead_rows] == 0).all()
    assert (_np(res["dK"])[dead_cols] == 0).all() and (_np(res["dV"])[dead_cols] == 0).all()


# ---- 3. large bias ----------------------------------------------------------------------------------------------------
def test_large_bias():
    """bias in {-40, +40}: a maximum taken before the bias is added would overflow or lose the -40 edges' rows; out, dV and
    dbias at the bar, dQ and dK (which cancel on near-one-hot rows) at the absolute bar 1e-3 max(1, max |ref|)."""
    g = _graph("wave")
    x, ref = _case("wave", 2, 16, True, "large")
    res = _pair(g, _on_device(x))
    for name, t in res.items():
        assert np.isfinite(_np(t)).all(), name
    _against_reference(res, ref, "large bias")


# ---- 4. boundary degrees at fp32 level --------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.case_ids("gt"), ids=str)
def test_boundary_degrees(case):
    """The 32 cases of the host power test, same inputs and bounds: every output within MARGIN x the float32 formulation's
    error (dK: MARGIN x DK_FACTOR, derived in tests/gt_bias_cases.py); row_max on rows with edges only.  Prints measured
    error / fp32 reference error per output (pytest -s).  Worst ratios on the MI355X: dK 13.7 at (260, 1) with edge values
    in the wave form (2.6 elsewhere), row_max 6.1, dbias 1.6, dQ 1.5, everything else below 1."""
    g = pc.graph(case[0], case[1])
    x, ref64, bounds = bc.boundary_references(case)
    dg = {k: _dev(g[k], torch.int32) for k in ("row_ptr", "col_ind", "col_ptr", "row_ind", "val_idx")}
    res = _pair(dg, _on_device(x))
    missed = []
    for name in bc.OUTPUTS:
        got = _np(res[name]).astype(np.float64)
        assert np.isfinite(got).all(), (case, name)
        err, at = bc.error_of(g, name, got, ref64[name], where=True)
        fp32 = bounds[name] / pc.MARGIN / (bc.DK_FACTOR if name == "dK" else 1.0)
        print(f"gt_bias boundary {case} {name}: measured {err:.3e} at (node, head) {at}, fp32 reference {fp32:.3e}, "
              f"ratio {err / fp32 if fp32 > 0 else float('nan'):.2f}, bound {bounds[name]:.3e}")
        if not err <= bounds[name]:
            missed.append((name, err, bounds[name]))
    er, ec = np.diff(g["row_ptr"]) == 0, np.diff(g["col_ptr"]) == 0
    assert (_np(res["out"])[er] == 0).all() and (_np(res["dQ"])[er] == 0).all()
    assert (_np(res["dK"])[ec] == 0).all() and (_np(res["dV"])[ec] == 0).all()
    assert (_np(res["row_max"])[er] == SENTINEL).all() and (_np(res["row_sum"])[er] == 0).all()
    assert not missed, (case, missed)


# ---- 5. operator and layer --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f,weighted", [("lane", 2, 20, True), ("wave", 8, 16, False)])
def test_operator_equals_raw_calls(kind, h, f, weighted):
    """GTConvFuse_bias + autograd.grad equals the raw binding calls bit for bit; `val` is saved only when it is not all ones."""
    from DFGNN.operators.fused_gtconv import GTConvFuse_bias, GTConvFuse_inference_bias
    g = _graph(kind)
    d = _on_device(_case(kind, h, f, weighted)[0])
    raw = _pair(g, d)
    q, k, v, b = (d[n].clone().requires_grad_(True) for n in ("Q", "K", "V", "bias"))
    out = GTConvFuse_bias(None, g["row_ptr"], g["col_ind"], d["val"], g["col_ptr"], g["row_ind"], g["val_idx"], 0, q, k, v, b)
    assert any(t.data_ptr() == d["val"].data_ptr() for t in out.grad_fn.saved_tensors) == weighted
    grads = torch.autograd.grad(out, (q, k, v, b), d["dO"])
    assert torch.equal(out, raw["out"])
    for got, name in zip(grads, ("dQ", "dK", "dV", "dbias")):
        assert torch.equal(got, raw[name]), name
    assert torch.equal(GTConvFuse_inference_bias(g["row_ptr"], g["col_ind"], d["val"], d["Q"], d["K"], d["V"], d["bias"]),
                       raw["out"])


def test_no_bias_gradient_allocates_nothing_per_edge():
    """m = 64, ~200 edges per row, h = 2, f = 8: every feature-sized tensor is 4 KB and h nnz floats are ~100 KB.  With
    bias.requires_grad == False one forward + backward peaks below 4 h nnz bytes above its start (bias itself is
    allocated before): no h nnz float buffer exists.  With a gradient wanted the same measure sees dbias."""
    from conftest import csc_of, random_graph
    from DFGNN.operators.fused_gtconv import GTConvFuse_bias
    rng = np.random.default_rng(64)
    m, h, f = 64, 2, 8
    row_ptr, col_ind, rows = random_graph(rng, m, 200)
    nnz = len(col_ind)
    col_ptr, row_ind, val_idx = csc_of(row_ptr, col_ind, rows, m)
    graph = [_dev(a, torch.int32) for a in (row_ptr, col_ind, col_ptr, row_ind, val_idx)]
    gen = torch.Generator().manual_seed(1)
    Q, K, V, dO = (torch.randn(m, h, f, generator=gen).to(DEV) for _ in range(4))
    bias, val = torch.randn(h, nnz, generator=gen).to(DEV), torch.ones(nnz, device=DEV)
    assert 4 * h * nnz > 8 * 4 * m * h * f

    def peak(bias_grad):
        q, k, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
        b = bias.clone().requires_grad_(bias_grad)

        def step():
            o = GTConvFuse_bias(None, graph[0], graph[1], val, graph[2], graph[3], graph[4], 0, q, k, v, b)
            return torch.autograd.grad(o, (q, k, v, b) if bias_grad else (q, k, v), dO)

        step()                                                   # (the all-ones test of `val` is cached here)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res = step()
        torch.cuda.synchronize()
        assert len(res) == (4 if bias_grad else 3)
        return torch.cuda.max_memory_allocated() - base

    p_without, p_with = peak(False), peak(True)
    print(f"gt_bias peak of one fwd+bwd: without dbias {p_without} B, with {p_with} B, 4 h nnz = {4 * h * nnz} B")
    assert p_without < 4 * h * nnz <= p_with


def test_layer_against_its_torch_branch():
    """SparseMHA_bias(fuse=True) in training mode at one head against its own fuse=False branch on the cora-like graph: the
    output, the projection-weight gradients and the edge_bias gradient; in .eval() the inference operator gives the same
    output; --conv gt --format forward_bias runs."""
    import argparse

    from DFGNN.layers import SparseMHA_bias, load_graphconv_layer, preprocess_Hyper_fw_bw
    from DFGNN.utils import synthetic as S
    torch.manual_seed(1)
    g = S.cora_like().to(DEV)
    params = preprocess_Hyper_fw_bw(g)
    nnz = params[3].numel()
    layer = SparseMHA_bias(64, 64, 1).to(DEV).train()
    x = torch.randn(g.num_nodes(), 64, device=DEV)
    edge_bias = torch.randn(nnz, 1, device=DEV, requires_grad=True)
    outs, grads = [], []
    for fuse in (False, True):
        layer.zero_grad()
        edge_bias.grad = None
        out = layer(params, x, edge_bias, fuse=fuse)
        (out * torch.linspace(-1, 1, out.numel(), device=DEV).reshape(out.shape)).sum().backward()
        outs.append(out.detach())
        grads.append([p.grad.clone() for p in (layer.q_proj.weight, layer.k_proj.weight, layer.v_proj.weight, edge_bias)])
    _check(outs[1], outs[0], "layer out")
    for name, a, b in zip(("q_proj.weight", "k_proj.weight", "v_proj.weight", "edge_bias"), *grads):
        _check(b, a, f"layer d{name}")
    with torch.no_grad():
        _check(layer.eval()(params, x, edge_bias, fuse=True), outs[0], "layer eval out")
    args = argparse.Namespace(conv="gt", format="forward_bias", dim=64, heads=2)
    out, ms = load_graphconv_layer(args).to(DEV).train()(params, x, fuse=True)
    assert out.shape == (g.num_nodes(), 64) and ms > 0


@pytest.mark.parametrize("m", [0, 5])
def test_empty_problems(m):
    """m == 0, and m == 5 without an edge (bias [h, 0]): zero outputs, sentinels, no error."""
    import fused_gtconv as gt
    h, f = 2, 12
    i32 = dict(dtype=torch.int32, device=DEV)
    row_ptr, none = torch.zeros(m + 1, **i32), torch.zeros(0, **i32)
    x, dO, bias = torch.randn(m, h, f, device=DEV), torch.randn(m, h, f, device=DEV), torch.zeros(h, 0, device=DEV)
    out, mx, sm = gt.gt_forward_bias(row_ptr, none, None, bias, x, x, x)
    dQ, dK, dV, db = gt.gt_backward_bias(row_ptr, none, None, bias, row_ptr, none, none, x, x, x, out, mx, sm, dO)
    torch.cuda.synchronize()
    assert out.shape == dQ.shape == dK.shape == dV.shape == (m, h, f) and mx.shape == sm.shape == (m, h) and db.shape == (h, 0)
    if m:      # (m == 0 launches nothing)
        for t in (out, dQ, dK, dV, sm):
            assert (t == 0).all()
        assert (mx == -1e38).all()


# ---- 6. the two transports agree --------------------------------------------------------------------------------------
def test_bindings_agree():
    """The torch C++ extension and the ctypes transport give bit-identical results for gt_inference_bias, gt_forward_bias and
    gt_backward_bias (with and without dbias), and the same RuntimeError for a bad argument."""
    import dfgnn_native
    import fused_gtconv as gt
    assert dfgnn_native.ext() is not None and hasattr(dfgnn_native.ext(), "gt_bwd_bias")
    cases = [(_graph(kind), _on_device(_case(kind, h, f, w, variant)[0])) for kind, h, f, w, variant in
             (("lane", 2, 20, True, "plain"), ("wave", 8, 16, False, "plain"), ("wave", 2, 16, False, "mask"))]

    def run():
        res = []
        for g, d in cases:
            both = _pair(g, d)
            res += [both[k] for k in bc.OUTPUTS]
            res += [_pair(g, d, need_dbias=False)[k] for k in ("dQ", "dK", "dV")]
            res.append(gt.gt_inference_bias(g["row_ptr"], g["col_ind"], d["val"], d["bias"], d["Q"], d["K"], d["V"]))
        g, d = cases[0]
        errs = []
        for bad in (dict(row_ptr=g["row_ptr"].long()), dict(bias=d["bias"].t().contiguous()), dict(bias=d["bias"].double())):
            a = dict(row_ptr=g["row_ptr"], bias=d["bias"])
            a.update(bad)
            try:
                gt.gt_forward_bias(a["row_ptr"], g["col_ind"], d["val"], a["bias"], d["Q"], d["K"], d["V"])
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
    for e1, e2, word in zip(err_ext, err_ctypes, ("int32", "bias", "bias")):
        assert e1 and e2 and word in e1 and word in e2, (e1, e2)
