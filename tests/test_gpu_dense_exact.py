"""GPU tests of the matrix-core ("dense") kernels at fp32-level bounds (run with `-m gpu` on an MI355X): gt_dense.hip,
gt_dense_stats.hip, gt_dense_stats_w.hip and the dfgnn_dense*.hpp bodies, on the two batches of tests/dense_cases.py -- one
range of every size next to a 16-row strip, a 32 / 64-column boundary and a size-class boundary, with an edge at every tile
corner -- at ten widths, through every call path: the CSR attn_edge pair, inference, the rank-ordered pair, the statistics
pair, the weighted statistics pair and inference, the autograd function, and the GAT dense pair with and without dropout.
Which body runs is decided by the batch and the width alone (no environment switch is set); that every intended range is a
dense range of its own, and that `narrow` holds no wide range, is asserted from the plan first.  Every output is held to
MARGIN x (error of the plain-fp32 reference against the float64 one on the same inputs) in the per-row measure of
parity_cases; tests/test_dense_cases_host.py proves that one lost probe edge moves every such output by at least POWER x
that bound.  Each check prints measured error, fp32-reference error and bound (pytest -s)."""
import numpy as np
import pytest
import torch

import dense_cases as dc
import parity_cases as pc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SLOPE = pc.SLOPE
DENSE, EDGE_GLOBAL = 1 << 29, 1 << 30
CASES = [(name, h, f) for name in dc.BATCHES for h, f in dc.WIDTHS]
_DEVICE = {}


@pytest.fixture(scope="module", autouse=True)
def _leave_no_device_memory_behind():
    """The batches stay on the device for the whole module; afterwards they are dropped -- also from the bindings' LRU caches
    (_binding_util: plans, dense weights of 1 KB per node, COO rows), which keep the tensors of their keys alive -- and the
    caching allocator's free blocks are released.  tests/test_gpu_gt_typed.py::test_memory_of_one_step measures a peak in
    allocated bytes: with this module's megabyte-sized tensors still pinned inside the allocator's 20 MiB segments, its 2 MiB
    workspace was served from a hole 135 KiB larger, which is not split and counts in full."""
    yield
    import gc
    import _binding_util as bu
    _DEVICE.clear()
    for cache in (bu._unit_cache, bu._plan_cache, bu._rows_cache, bu._weights_cache):
        cache.d.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


class _Checker:
    """One case's float64 reference and bounds; check() prints measured error, fp32-reference error and bound and notes a
    miss, done() asserts."""

    def __init__(self, g, ref64, bounds, what):
        self.g, self.ref64, self.bounds, self.what, self.missed = g, ref64, bounds, what, []

    def check(self, entry, name, got, ref_name=None):
        ref_name = ref_name or name
        got = _np(got).astype(np.float64)
        assert np.isfinite(got).all(), (self.what, entry, name)
        err, at = pc.error_of(self.g, ref_name, got, self.ref64[ref_name], where=True)
        bound = self.bounds[ref_name]
        print(f"dense-exact {self.what} | {entry} | {name}: measured {err:.3e} at (node, head) {at}, fp32 reference "
              f"{bound / pc.MARGIN:.3e}, bound {bound:.3e}, ratio {err / (bound / pc.MARGIN):.2f}")
        if not err <= bound:
            self.missed.append((entry, name, err, bound))

    def done(self):
        assert not self.missed, (self.what, self.missed)


def _on_device(g, key):
    """The batch through the public preprocessing (member graphs -> batch -> preprocess_Hyper_fw_bw), once per session; the
    arrays must be the ones the references were computed on."""
    if key not in _DEVICE:
        from DFGNN.layers import preprocess_Hyper_fw_bw
        from DFGNN.utils import Graph, batch
        b = batch([Graph(s, d, n) for s, d, n in g["members"]]).to(DEV)
        A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem = preprocess_Hyper_fw_bw(b)
        d = dict(rows=rows, row_ptr=row_ptr, col_ind=col_ind, val=val, col_ptr=col_ptr, row_ind=row_ind, val_idx=val_idx,
                 smem=smem)
        for k in ("rows", "row_ptr", "col_ind", "col_ptr", "row_ind", "val_idx"):
            assert np.array_equal(_np(d[k]), g[k]), k
        _DEVICE[key] = d
    return _DEVICE[key]


def _fit_ranges(plan):
    raw = _np(plan.buf)[12:12 + 2 * plan.num_fit].reshape(-1, 2)
    return {int(n0): (int(n1f & ~(DENSE | EDGE_GLOBAL)), bool(n1f & DENSE)) for n0, n1f in raw}


def _assert_plan(plan, g):
    """Every intended range is a fit range of its own with the dense flag; nothing else is in the plan."""
    assert plan is not None and plan.num_spill == 0
    fit = _fit_ranges(plan)
    for r in g["ranges"]:
        assert fit.get(r["n0"]) == (r["n0"] + r["n"], True), (r["n0"], r["n"], fit.get(r["n0"]))
    assert plan.num_fit == len(g["ranges"]) == plan.num_dense
    wide = sum(r["n"] > 128 for r in g["ranges"])
    assert plan.num_dense_wide == wide and (wide == 0) == (g["name"] == "narrow")


def _empties(g):
    return np.diff(g["row_ptr"]) == 0, np.diff(g["col_ptr"]) == 0


def _exact_zeros(g, what, out=None, dQ=None, dK=None, dV=None, row_max=None, row_sum=None):
    """Rows without out-edges, columns without in-edges (the isolated nodes of the hole copies are both): bit for bit."""
    er, ec = _empties(g)
    iso = [r["isolated"] for r in g["ranges"] if r["hole"]]
    assert er[iso].all() and ec[iso].all()
    for name, t, rows in (("out", out, er), ("dQ", dQ, er), ("dK", dK, ec), ("dV", dV, ec), ("row_sum", row_sum, er)):
        if t is not None:
            assert (_np(t)[rows] == 0).all(), (what, name)
    if row_max is not None:
        assert (_np(row_max)[er] == np.float32(-1e38)).all(), (what, "row_max")


def _hole_copies(g, ref64, bounds, what, dQ, dK, dV):
    """Node n - 1 of a hole copy has one out-edge: a softmax over one edge has no gradient, its dQ row is the oracle's zero
    (to the bound's floor); dK and dV of its partner hold its term."""
    floor = pc.floor_of(ref64["dQ"])
    for r in g["ranges"]:
        if r["hole"]:
            last, partner = r["last"], r["partner"]
            assert np.abs(ref64["dQ"][last]).max() <= 1e-12
            assert np.abs(_np(dQ)[last]).max() <= bounds["dQ"] * floor, (what, r["n"], "dQ")
            for name, t in (("dK", dK), ("dV", dV)):
                assert np.abs(_np(t)[partner]).max() > 0 and np.abs(ref64[name][partner]).max() > 0, (what, r["n"], name)
                e = pc.row_errors(_np(t), ref64[name])[partner]
                assert (e <= bounds[name]).all(), (what, r["n"], name, e)


def _csr_order(g, attn_ranked):
    """Rank-ordered attention values (row i's k-th edge by increasing column at row_ptr[i] + k) back in CSR order."""
    ci = g["col_ind"].astype(np.int64)
    order = np.lexsort((ci, g["rows"].astype(np.int64)))
    assert (order != np.arange(g["nnz"])).any()
    got = np.empty_like(_np(attn_ranked))
    got[:, order] = _np(attn_ranked)
    return got


# ---- GT ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,h,f", CASES)
def test_gt_dense_unit_values(oracle_mod, name, h, f):
    """CSR attn_edge pair, inference, rank-ordered pair, statistics pair and -- at one head -- the autograd function."""
    import fused_gtconv as gt
    from DFGNN.operators.fused_gtconv import GTConvFuse_hyper
    g = dc.graph(name)
    d = _on_device(g, name)
    x, ref64, _, bounds = dc.gt_references(name, h, f, True)
    Q, K, V, dO = (_dev(x[k]) for k in ("Q", "K", "V", "dO"))
    rp, ci, val = d["row_ptr"], d["col_ind"], d["val"]
    plan = gt.gt_stats_pair_applies(rp, ci, val, Q)
    _assert_plan(plan, g)
    what = f"gt {name} h={h} f={f}"
    c = _Checker(g, ref64, bounds, what)
    args = (rp, ci, d["rows"], val, d["col_ptr"], d["row_ind"], d["val_idx"], d["smem"], Q, K, V)
    res = {}
    out, attn = gt.gt_hyper_forward(*args)
    dQ, dK, dV = gt.gt_backward(*args, attn, dO)
    res["attn_edge"] = (out, dQ, dK, dV)
    for nm, t in (("out", out), ("attn_edge", attn), ("dQ", dQ), ("dK", dK), ("dV", dV)):
        c.check("attn_edge pair", nm, t)
    _exact_zeros(g, what, out, dQ, dK, dV)
    _hole_copies(g, ref64, bounds, what, dQ, dK, dV)
    (inf,) = gt.gt_hyper_inference(rp, ci, d["rows"], val, d["smem"], Q, K, V)
    c.check("inference", "out", inf)
    _exact_zeros(g, what, inf)
    assert gt.gt_ranked_pair_applies(rp, ci, val, Q) is plan
    out, attn_r = gt.gt_hyper_forward_ranked(rp, ci, Q, K, V, plan=plan)
    dQ, dK, dV = gt.gt_backward_ranked(rp, ci, Q, K, V, attn_r, dO, plan=plan)
    res["ranked"] = (out, dQ, dK, dV)
    for nm, t in (("out", out), ("attn_edge", _csr_order(g, attn_r)), ("dQ", dQ), ("dK", dK), ("dV", dV)):
        c.check("ranked pair", nm, t)
    _exact_zeros(g, what, out, dQ, dK, dV)
    _hole_copies(g, ref64, bounds, what, dQ, dK, dV)
    out, mx, sm = gt.gt_hyper_forward_stats(rp, ci, Q, K, V, plan=plan)
    dQ, dK, dV = gt.gt_backward_stats(rp, ci, Q, K, V, mx, sm, dO, plan=plan)
    res["stats"] = (out, dQ, dK, dV)
    for nm, t in (("out", out), ("row_max", mx), ("row_sum", sm), ("dQ", dQ), ("dK", dK), ("dV", dV)):
        c.check("stats pair", nm, t)
    _exact_zeros(g, what, out, dQ, dK, dV, mx, sm)
    _hole_copies(g, ref64, bounds, what, dQ, dK, dV)
    if h == 1:                    # the autograd function: bit-equal to the pair it chooses
        pair, _ = gt.gt_training_pair(rp, ci, val, Q)
        Qg, Kg, Vg = (t.clone().requires_grad_(True) for t in (Q, K, V))
        o = GTConvFuse_hyper(d["rows"], rp, ci, val, d["col_ptr"], d["row_ind"], d["val_idx"], d["smem"], Qg, Kg, Vg)
        o.backward(dO)
        print(f"dense-exact {what} | autograd takes the {pair} pair")
        for a, b in zip((o.detach(), Qg.grad, Kg.grad, Vg.grad), res[pair]):
            assert torch.equal(a, b), (what, pair)
    c.done()


@pytest.mark.parametrize("name,h,f", CASES)
def test_gt_dense_edge_values(oracle_mod, name, h, f):
    """Edge values in [0.5, 1.5): the statistics pair and inference read them in the plan's dense form."""
    import fused_gtconv as gt
    g = dc.graph(name)
    d = _on_device(g, name)
    x, ref64, _, bounds = dc.gt_references(name, h, f, False)
    val, Q, K, V, dO = (_dev(x[k]) for k in ("val", "Q", "K", "V", "dO"))
    rp, ci = d["row_ptr"], d["col_ind"]
    plan = gt.gt_stats_pair_applies(rp, ci, val, Q)
    _assert_plan(plan, g)
    assert gt.gt_stats_pair_chosen(rp, ci, val, Q) is plan and gt.gt_ranked_pair_applies(rp, ci, val, Q) is None
    what = f"gt {name} h={h} f={f} edge values"
    c = _Checker(g, ref64, bounds, what)
    out, mx, sm = gt.gt_hyper_forward_stats(rp, ci, Q, K, V, plan=plan, val=val)
    dQ, dK, dV = gt.gt_backward_stats(rp, ci, Q, K, V, mx, sm, dO, plan=plan, val=val)
    for nm, t in (("out", out), ("row_max", mx), ("row_sum", sm), ("dQ", dQ), ("dK", dK), ("dV", dV)):
        c.check("weighted stats pair", nm, t)
    _exact_zeros(g, what, out, dQ, dK, dV, mx, sm)
    _hole_copies(g, ref64, bounds, what, dQ, dK, dV)
    (inf,) = gt.gt_hyper_inference(rp, ci, d["rows"], val, d["smem"], Q, K, V)
    c.check("weighted inference", "out", inf)
    _exact_zeros(g, what, inf)
    c.done()


# ---- GAT --------------------------------------------------------------------------------------------------------------
def _gat_training(c, g, d, x, ar, ac, X, dO, attn_drop):
    """gat_forward / gat_backward; with dropout the references are recomputed with the randoms the forward drew."""
    import fused_gatconv as gat
    rp, ci = d["row_ptr"], d["col_ind"]
    torch.manual_seed(5)
    out, emax, esum, mask = gat.gat_forward(ar, ac, rp, ci, SLOPE, X, attn_drop)
    gf, gr, gc = gat.gat_backward(SLOPE, attn_drop, rp, ci, d["col_ptr"], d["row_ind"], d["val_idx"], emax, esum, mask, X, ar,
                                  ac, dO)
    tag = "gat pair" if attn_drop == 0 else f"gat pair, dropout {attn_drop}"
    if attn_drop > 0:
        mask_np = _np(mask)
        assert mask_np.shape == (g["nnz"], X.size(1))
        ref64 = pc.gat_reference(g["row_ptr"], g["col_ind"], x, "f64", mask_np, attn_drop)
        ref32 = pc.gat_reference(g["row_ptr"], g["col_ind"], x, "f32", mask_np, attn_drop)
        c = _Checker(g, ref64, dc.bounds_of(g, ref32, ref64), c.what)
    for nm, t in (("out", out), ("edge_max", emax), ("edge_sum", esum), ("grad_feat", gf), ("grad_attn_row", gr),
                  ("grad_attn_col", gc)):
        c.check(tag, nm, t)
    er, ec = _empties(g)
    assert (_np(out)[er] == 0).all() and (_np(gr)[er] == 0).all() and (_np(emax)[er] < -9e37).all(), (c.what, tag)
    assert (_np(gf)[ec] == 0).all() and (_np(gc)[ec] == 0).all(), (c.what, tag)
    return c


@pytest.mark.parametrize("name,h,f", CASES)
def test_gat_dense(oracle_mod, name, h, f):
    """gat_inference_hyper and the training pair at attn_drop 0 and 0.25 on the matrix-core kernels."""
    import fused_gatconv as gat
    from _binding_util import get_plan_obj
    g = dc.graph(name)
    d = _on_device(g, name)
    x, ref64, _, bounds = dc.gat_references(name, h, f)
    ar, ac, X, dO = (_dev(x[k]) for k in ("attn_row", "attn_col", "X", "dO"))
    _assert_plan(get_plan_obj(d["row_ptr"], d["col_ind"], X, True), g)
    c = _Checker(g, ref64, bounds, f"gat {name} h={h} f={f}")
    inf = gat.gat_inference_hyper(d["smem"], ar, ac, d["row_ptr"], d["col_ind"], d["rows"], SLOPE, X)
    inf = inf[0] if isinstance(inf, (list, tuple)) else inf
    c.check("gat_inference_hyper", "out", inf, "inference")
    assert (_np(inf)[_empties(g)[0]] == 0).all()
    _gat_training(c, g, d, x, ar, ac, X, dO, 0.0)
    c2 = _gat_training(c, g, d, x, ar, ac, X, dO, 0.25)
    c2.done()
    c.done()


# ---- the density threshold ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", dc.THRESHOLD_SIZES)
def test_density_threshold(oracle_mod, n):
    """A range with exactly ceil(n^2 / 32) edges runs on the matrix cores, the same range without its last edge on the
    edge-walking kernels: the plan's flag is the rule computed here, and both results stay inside their bounds."""
    import fused_gtconv as gt
    h, f = 1, 64
    for short in (0, 1):
        g = dc.threshold_graph(n, short)
        d = _on_device(g, ("threshold", n, short))
        x, ref64, _, bounds = dc.threshold_references(n, short, h, f)
        Q, K, V, dO = (_dev(x[k]) for k in ("Q", "K", "V", "dO"))
        args = (d["row_ptr"], d["col_ind"], d["rows"], d["val"], d["col_ptr"], d["row_ind"], d["val_idx"], d["smem"], Q, K, V)
        out, attn = gt.gt_hyper_forward(*args)
        plan = d["row_ptr"]._dfgnn_plans[f]
        n0, _, edges = g["test"]
        rule = dc.dense_rule(n, edges)
        assert rule == (short == 0)
        assert _fit_ranges(plan).get(n0) == (n0 + n, rule), (n, short, _fit_ranges(plan))
        assert plan.num_fit == 3 and plan.num_dense == 2 + rule and plan.num_spill == 0
        dQ, dK, dV = gt.gt_backward(*args, attn, dO)
        c = _Checker(g, ref64, bounds, f"threshold n={n} edges={edges} dense={rule}")
        for nm, t in (("out", out), ("attn_edge", attn), ("dQ", dQ), ("dK", dK), ("dV", dV)):
            c.check("attn_edge pair", nm, t)
        c.check("inference", "out", gt.gt_hyper_inference(d["row_ptr"], d["col_ind"], d["rows"], d["val"], d["smem"], Q, K, V)[0])
        er, ec = _empties(g)
        assert (_np(out)[er] == 0).all() and (_np(dQ)[er] == 0).all() and (_np(dK)[ec] == 0).all() and (_np(dV)[ec] == 0).all()
        c.done()
