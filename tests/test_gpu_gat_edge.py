"""GPU: the any-graph GAT pair with a per-edge attention term (dfgnn_gat_fwd_edge / dfgnn_gat_bwd_edge, csrc/gat_edge_train.hip)
against the float64 torch reference of tests/gat_edge_cases.py -- square and rectangular graphs, both kernel forms on
either side, with and without score, with and without dropout (the reference is given the same randoms), both transports --
plus the bit-for-bit properties of include/dfgnn.h, -inf scores, dropped rows, the fp32-level boundary cases whose power
tests/test_gat_edge_host.py proves, agreement with the existing general GAT pair, the absence of any per-edge allocation,
and autograd through the operator and the layers."""
import functools
import os
import re

import numpy as np
import pytest
import torch

import gat_edge_cases as ge
import parity_cases as pc
import rect_cases as rc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-3
SLOPE = pc.SLOPE
DROP = 0.4
MAIN = ("out", "edge_max", "edge_sum", "grad_feat", "grad_attn_row", "grad_attn_col")    # everything but grad_score
INT_KEYS = ("row_ptr", "col_ind", "col_ptr", "row_ind", "val_idx")
SQUARE = ("lane", "wave")
RECT = ("tall", "wide", "block", "line_row", "line_col", "no_rows", "no_cols")


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
    print(f"gat_edge {what}: max abs err {err:.3e} (bound {bound:.3e})")
    assert np.isfinite(got).all(), what
    assert err < bound, (what, err, bound)


class _Ctypes:
    """Inside: the ctypes transport (the torch extension hidden)."""

    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        import dfgnn_native
        self.saved = dfgnn_native._ext
        assert self.saved is not None and hasattr(self.saved, "gat_bwd_edge")
        if self.on:
            dfgnn_native._ext = None

    def __exit__(self, *exc):
        import dfgnn_native
        dfgnn_native._ext = self.saved


# ---- graphs and inputs ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _threshold():
    text = open(os.path.join(rc.CSRC, "gat_edge_train.hip")).read()
    hits = re.findall(r"constexpr\s+int\s+kGatEdgeGroupMaxDegree\s*=\s*(\d+)\s*;", text)
    assert len(hits) == 1
    return int(hits[0])


@functools.lru_cache(maxsize=None)
def _graph(kind):
    """lane (m = 257) / wave (m = 96, one 200-edge row) of tests/test_gpu_gatv2.py::_graph, or a graph of rect_cases.graph:
    host CSR / CSC arrays and their int32 device copies.  Asserts the side of the new file's thresholds each pass is on."""
    if kind in SQUARE:
        from test_gpu_gatv2 import _graph as base
        b = base(kind)
        rows, cols, m = _np(b["rows"]), _np(b["cols"]), b["m"]
        g = rc._finish(rows, cols, m, m)
        assert np.array_equal(g["row_ptr"], _np(b["row_ptr"])) and np.array_equal(g["col_ind"], _np(b["col_ind"]))
    else:
        g = dict(rc.graph(kind))
    m, n, nnz, cap = g["m"], g["n_cols"], g["nnz"], _threshold()
    rows_lane, cols_lane = rc.lane_form(m, nnz), rc.lane_form(n, nnz)
    want = dict(lane=(True, True), wave=(False, False), tall=(True, False), wide=(False, True), block=(False, True))
    if kind in want:
        assert (rows_lane, cols_lane) == want[kind], (kind, rows_lane, cols_lane)
    if kind == "lane":        # the cooperative switch inside the lane form, on either side
        assert g["deg"].max() > max(cap, 64) and 0 < g["indeg"].max() and (g["deg"] == 0).any() and (g["indeg"] == 0).any()
    if kind == "wave":
        assert g["deg"].max() == 200
    if kind == "wide":
        assert g["indeg"].max() > cap
    g["dev"] = {k: _dev(g[k], torch.int32) for k in INT_KEYS}
    return g


@functools.lru_cache(maxsize=None)
def _inputs(kind, h, f):
    g = _graph(kind)
    m, n, nnz = g["m"], g["n_cols"], g["nnz"]
    rng = np.random.default_rng(1000 * h + f + 53)
    r = lambda *s: np.ascontiguousarray(rng.standard_normal(s), dtype=np.float32)  # noqa: E731
    x = dict(attn_row=r(m, h), attn_col=r(n, h), X=r(n, h, f), dO=r(m, h, f), score=r(h, nnz) * np.float32(0.5))
    x["mask"] = np.ascontiguousarray(rng.uniform(0.01, 1.0, (nnz, h)), dtype=np.float32)
    return x


@functools.lru_cache(maxsize=None)
def _case(kind, h, f, with_score, with_drop):
    """-> (host inputs, float64 reference); computed once per case and shared, nobody writes to it."""
    g, x = _graph(kind), _inputs(kind, h, f)
    ref = ge.reference(g["row_ptr"], g["col_ind"], x["attn_row"], x["attn_col"], x["score"] if with_score else None, x["X"],
                       x["dO"], SLOPE, x["mask"] if with_drop else None, DROP if with_drop else 0.0)
    return x, ref


def _on_device(x):
    return {k: _dev(a) for k, a in x.items()}


def _pair(g, d, with_score=True, with_drop=False, want_grad_score=True, drop=DROP):
    import fused_gatconv as gat
    dg = g["dev"] if "dev" in g else g
    score = d["score"] if with_score else None
    mask, drop = (d["mask"], drop) if with_drop else (None, 0.0)
    out, emax, esum, used = gat.gat_forward_edge(d["attn_row"], d["attn_col"], dg["row_ptr"], dg["col_ind"], SLOPE, d["X"], score,
                                                 drop, mask)
    assert used is mask
    gf, gr, gc, gs = gat.gat_backward_edge(SLOPE, drop, dg["row_ptr"], dg["col_ind"], dg["col_ptr"], dg["row_ind"], dg["val_idx"],
                                           d["attn_row"], d["attn_col"], d["X"], emax, esum, d["dO"], score=score,
                                           edge_mask=mask, want_grad_score=want_grad_score)
    torch.cuda.synchronize()
    return dict(out=out, edge_max=emax, edge_sum=esum, grad_feat=gf, grad_attn_row=gr, grad_attn_col=gc, grad_score=gs)


def _same(a, b, names=ge.OUTPUTS):
    for name in names:
        assert torch.equal(a[name], b[name]), name


# ---- 1. + 2. the pair against the reference, and what holds bit for bit -----------------------------------------------------
@pytest.mark.parametrize("h,f", rc.WIDTHS)
@pytest.mark.parametrize("kind", SQUARE + RECT)
def test_pair_against_reference(kind, h, f):
    """Every output at the bar with and without score, with and without dropout, on both transports (which agree bit for
    bit); the conventions of empty rows and columns; and on the extension's transport: inference equals the training
    forward's out, score = None is score = zeros, want_grad_score = False leaves the other outputs alone, two backward calls
    agree."""
    import fused_gatconv as gat
    g = _graph(kind)
    d = _on_device(_inputs(kind, h, f))
    er, ecol = g["deg"] == 0, g["indeg"] == 0
    for with_score in (True, False):
        for with_drop in (False, True):
            x, ref = _case(kind, h, f, with_score, with_drop)
            res = _pair(g, d, with_score, with_drop)
            with _Ctypes():
                _same(res, _pair(g, d, with_score, with_drop))
            for name in ge.OUTPUTS:
                _check(res[name], ref[name], f"{kind} h{h} f{f} score={with_score} drop={with_drop} {name}")
            assert res["grad_score"].shape == (h, g["nnz"]) and res["grad_feat"].shape == (g["n_cols"], h, f)
            for name, fill in (("out", 0), ("edge_sum", 0), ("grad_attn_row", 0), ("edge_max", np.float32(-1e38))):
                assert (_np(res[name])[er] == fill).all(), name
            assert (_np(res["grad_feat"])[ecol] == 0).all() and (_np(res["grad_attn_col"])[ecol] == 0).all()
            score = d["score"] if with_score else None
            mask, drop = (d["mask"], DROP) if with_drop else (None, 0.0)
            inf = gat.gat_inference_edge(d["attn_row"], d["attn_col"], g["dev"]["row_ptr"], g["dev"]["col_ind"], SLOPE, d["X"],
                                         score, drop, mask)
            assert torch.equal(inf, res["out"])
            _same(res, _pair(g, d, with_score, with_drop))
            without = _pair(g, d, with_score, with_drop, want_grad_score=False)
            assert without["grad_score"] is None
            _same(res, without, MAIN)
            if not with_score:
                _same(res, _pair(g, dict(d, score=torch.zeros_like(d["score"])), True, with_drop))


def _raw(g, d, rect, score, mask, drop):
    """One forward and backward through the C entry points themselves: the square ones, or the _rect ones."""
    from _binding_util import call
    dg, (m, n, nnz), (h, f) = g["dev"], (g["m"], g["n_cols"], g["nnz"]), d["X"].shape[1:]
    e = lambda *s: torch.empty(s, dtype=torch.float32, device=DEV)  # noqa: E731
    r = dict(out=e(m, h, f), edge_max=e(m, h), edge_sum=e(m, h), grad_feat=e(n, h, f), grad_attn_row=e(m, h),
             grad_attn_col=e(n, h), grad_score=e(h, nnz))
    dims = (m, n, nnz, h, f) if rect else (m, nnz, h, f)
    sfx = "_rect" if rect else ""
    call("dfgnn_gat_fwd_edge" + sfx, "fwd", d["X"].device, *dims, dg["row_ptr"], dg["col_ind"], d["attn_row"], d["attn_col"], SLOPE,
         score, d["X"], mask, drop, r["edge_max"], r["edge_sum"], r["out"])
    call("dfgnn_gat_bwd_edge" + sfx, "bwd", d["X"].device, *dims, dg["row_ptr"], dg["col_ind"], dg["col_ptr"], dg["row_ind"],
         dg["val_idx"], d["attn_row"], d["attn_col"], SLOPE, score, d["X"], mask, drop, r["edge_max"], r["edge_sum"],
         d["dO"], e(m, h), r["grad_feat"], r["grad_attn_row"], r["grad_attn_col"], r["grad_score"])
    torch.cuda.synchronize()
    return r


@pytest.mark.parametrize("kind,h,f", [("lane", 2, 20), ("wave", 8, 16), ("wave", 3, 7)])
def test_square_entry_is_the_rect_entry(kind, h, f):
    g = _graph(kind)
    d = _on_device(_inputs(kind, h, f))
    for score, mask, drop in ((d["score"], d["mask"], DROP), (None, None, 0.0)):
        sq, rect = _raw(g, d, False, score, mask, drop), _raw(g, d, True, score, mask, drop)
        _same(sq, rect)
        _same(sq, _pair(g, d, score is not None, mask is not None))


@pytest.mark.parametrize("kind,h,f", [("lane", 2, 20), ("lane", 3, 7), ("wave", 1, 128), ("wave", 8, 16)])
def test_square_case_embedded_in_a_rectangle(kind, h, f):
    """Columns shifted by 3, two empty columns and four empty rows appended: the same bits inside the image, exact zeros
    (edge_max: the sentinel) outside, whatever the padding rows of the inputs hold."""
    g = _graph(kind)
    x = _inputs(kind, h, f)
    shift, cpad, rpad = 3, 2, 4
    eg = rc.embed_graph(g["row_ptr"], g["col_ind"], shift, cpad, rpad)
    assert rc.lane_form(eg["m"], eg["nnz"]) == rc.lane_form(g["m"], g["nnz"])
    assert rc.lane_form(eg["n_cols"], eg["nnz"]) == rc.lane_form(g["n_cols"], g["nnz"])
    eg["dev"] = {k: _dev(eg[k], torch.int32) for k in INT_KEYS}
    # (CSC order inside a column is by row id on both sides, so val_idx maps entry for entry)
    ex = dict(attn_row=rc.embed_rows(x["attn_row"], rpad), dO=rc.embed_rows(x["dO"], rpad),
              attn_col=rc.embed_cols(x["attn_col"], shift, cpad), X=rc.embed_cols(x["X"], shift, cpad), score=x["score"],
              mask=x["mask"])
    for with_score, with_drop in ((True, True), (False, False)):
        sq = _pair(g, _on_device(x), with_score, with_drop)
        em = _pair(eg, _on_device(ex), with_score, with_drop)
        for name in ("out", "edge_sum", "grad_attn_row", "edge_max"):
            inside, clean = rc.restrict_rows(_np(em[name]), g["m"], rc.SENTINEL_MAX if name == "edge_max" else 0.0)
            assert clean and np.array_equal(inside, _np(sq[name])), name
        for name in ("grad_feat", "grad_attn_col"):
            inside, clean = rc.restrict_cols(_np(em[name]), g["m"], shift)
            assert clean and np.array_equal(inside, _np(sq[name])), name
        assert torch.equal(em["grad_score"], sq["grad_score"])


# ---- 3. -inf scores ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_drop", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("kind,h,f", [("lane", 2, 20), ("wave", 8, 16), ("wide", 3, 7), ("tall", 1, 128)])
def test_masked_edges(kind, h, f, with_drop):
    """score = -inf on one edge of a row, and on every edge of a (row, head) -- among them the longest row: everything
    stays finite and at the bar, the masked slots of grad_score are exact zeros and the fully masked (row, head) follows the
    empty-row conventions while its other heads go on."""
    g = _graph(kind)
    x = dict(_inputs(kind, h, f))
    rp, deg = g["row_ptr"], g["deg"]
    full = [int(deg.argmax()), int(np.nonzero(deg >= 2)[0][0])]
    one = [int(i) for i in np.nonzero(deg >= 2)[0] if i not in full][:3]
    score = x["score"].copy()
    for i in full:
        score[0, rp[i]:rp[i + 1]] = -np.inf
    for i in one:
        score[h - 1, rp[i] + 1] = -np.inf
    x["score"] = score
    ref = ge.reference(g["row_ptr"], g["col_ind"], x["attn_row"], x["attn_col"], score, x["X"], x["dO"], SLOPE,
                       x["mask"] if with_drop else None, DROP if with_drop else 0.0)
    res = _pair(g, _on_device(x), True, with_drop)
    for name in ge.OUTPUTS:
        _check(res[name], ref[name], f"masked {kind} h{h} f{f} drop={with_drop} {name}")
    got = {k: _np(v) for k, v in res.items()}
    for i in full:
        assert (got["out"][i, 0] == 0).all() and got["edge_sum"][i, 0] == 0 and got["edge_max"][i, 0] == np.float32(-1e38)
        assert got["grad_attn_row"][i, 0] == 0 and (got["grad_score"][0, rp[i]:rp[i + 1]] == 0).all()
        if h > 1:
            assert got["edge_sum"][i, 1] > 0
    for i in one:
        assert got["grad_score"][h - 1, rp[i] + 1] == 0 and got["edge_sum"][i, h - 1] > 0


# ---- 4. dropout corners -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f", [("lane", 2, 20), ("wave", 8, 16), ("wide", 3, 7)])
def test_dropped_rows_and_zero_rate(kind, h, f):
    """Every edge of a row dropped (its longest row among them): out = 0, the statistics are those of the row without
    dropout, the gradients are finite and at the bar.  attn_drop = 0 with a mask given keeps every edge: the bits of no mask."""
    g = _graph(kind)
    x = dict(_inputs(kind, h, f))
    rp, deg = g["row_ptr"], g["deg"]
    rows = [int(deg.argmax()), int(np.nonzero(deg >= 1)[0][0])]
    mask = x["mask"].copy()
    for i in rows:
        mask[rp[i]:rp[i + 1]] = 0.25 * DROP    # below the rate: dropped
    x["mask"] = mask
    ref = ge.reference(g["row_ptr"], g["col_ind"], x["attn_row"], x["attn_col"], x["score"], x["X"], x["dO"], SLOPE, mask, DROP)
    d = _on_device(x)
    res = _pair(g, d, True, True)
    for name in ge.OUTPUTS:
        _check(res[name], ref[name], f"dropped {kind} h{h} f{f} {name}")
    plain = _pair(g, d, True, False)
    for i in rows:
        assert (_np(res["out"])[i] == 0).all() and (_np(res["grad_attn_row"])[i] == 0).all()
        assert (_np(res["grad_score"])[:, rp[i]:rp[i + 1]] == 0).all()
    _same(res, plain, ("edge_max", "edge_sum"))
    _same(_pair(g, d, True, True, drop=0.0), plain)


# ---- 5. boundary degrees at fp32 level ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.case_ids("gat"), ids=str)
def test_boundary_degrees(case):
    """The 16 cases of the host power test, same inputs and bounds: every output within MARGIN x the float32 formulation's
    error.  Prints measured error / fp32 reference error per output (pytest -s); DESIGN.md 3.2m records the worst ratios."""
    g = pc.graph(case[0], case[1])
    x, ref64, bounds = ge.boundary_references(case)
    dg = {k: _dev(g[k], torch.int32) for k in INT_KEYS}
    res = _pair(dg, _on_device(x))
    missed = []
    for name in ge.OUTPUTS:
        got = _np(res[name]).astype(np.float64)
        assert np.isfinite(got).all(), (case, name)
        err, at = ge.error_of(g, name, got, ref64[name], where=True)
        fp32 = bounds[name] / pc.MARGIN
        print(f"gat_edge boundary {case} {name}: measured {err:.3e} at (node, head) {at}, fp32 reference {fp32:.3e}, "
              f"ratio {err / fp32 if fp32 > 0 else float('nan'):.2f}, bound {bounds[name]:.3e}")
        if not err <= bounds[name]:
            missed.append((name, err, bounds[name]))
    assert not missed, (case, missed)


# ---- 6. the existing general pair -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_drop", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("case", [(False, False, 32, 1), (False, True, 7, 2), (True, False, 128, 1), (True, True, 32, 1)], ids=str)
def test_agrees_with_the_existing_general_pair(case, with_drop):
    """gat_forward / gat_backward with USE_BLOCK_PLAN = False on the same inputs and the same randoms, no score: every common
    output within the sum of the two pairs' fp32-level bounds (the same function: twice MARGIN x the float32 formulation's
    error with that mask), in parity_cases' measure with the float64 reference's row norms.  Not bit equality: the two
    backward passes sum in different orders, and the column pass here recomputes what the other reads from grad_edge."""
    import fused_gatconv as gat
    g = pc.graph(case[0], case[1])
    x = pc.gat_inputs(*case)
    m, nnz, h = g["m"], g["nnz"], case[3]
    dg = {k: _dev(g[k], torch.int32) for k in INT_KEYS}
    d = _on_device(dict(x))
    drop = 0.3 if with_drop else 0.0
    saved = gat.USE_BLOCK_PLAN
    gat.USE_BLOCK_PLAN = False
    try:
        torch.manual_seed(11)
        out, emax, esum, mask = gat.gat_forward(d["attn_row"], d["attn_col"], dg["row_ptr"], dg["col_ind"], SLOPE, d["X"], drop)
        gf, gr, gc = gat.gat_backward(SLOPE, drop, dg["row_ptr"], dg["col_ind"], dg["col_ptr"], dg["row_ind"], dg["val_idx"], emax,
                                      esum, mask, d["X"], d["attn_row"], d["attn_col"], d["dO"])
    finally:
        gat.USE_BLOCK_PLAN = saved
    old = dict(out=out, edge_max=emax, edge_sum=esum, grad_feat=gf, grad_attn_row=gr, grad_attn_col=gc)
    mask = mask.contiguous() if with_drop else None
    assert mask is None or mask.shape == (nnz, h)
    new = _pair(dg, dict(d, mask=mask), False, with_drop, want_grad_score=False, drop=drop)
    args = (g["row_ptr"], g["col_ind"], x["attn_row"], x["attn_col"], None, x["X"], x["dO"], SLOPE, _np(mask) if with_drop else None,
            drop)
    ref64, ref32 = ge.reference(*args), ge.reference(*args, acc="f32")
    valid = (np.diff(g["row_ptr"]) > 0)[:, None]
    for name in MAIN:
        bound = pc.MARGIN * ge.error_of(g, name, ref32[name], ref64[name])
        diff = pc._row_norms(_np(new[name]).astype(np.float64) - _np(old[name]).astype(np.float64))
        e = diff / np.maximum(pc._row_norms(ref64[name]), pc.floor_of(ref64[name]))
        if name in pc.STATS:
            e = np.where(valid, e, 0.0)
        print(f"gat_edge against the general pair {case} drop={drop} {name}: {e.max():.3e} (sum of bounds {2 * bound:.3e})")
        assert e.max() <= 2 * bound, (name, float(e.max()), 2 * bound)


# ---- 7. no per-edge allocation ----------------------------------------------------------------------------------------------
def test_backward_allocates_nothing_of_size_nnz():
    """The wave graph at 8 x 16, no dropout, want_grad_score = False: over the backward, max_memory_allocated rises by less
    than its node-sized outputs and delta plus 2 h nnz bytes -- half of one [h, nnz] float tensor."""
    import fused_gatconv as gat
    g, h, f = _graph("wave"), 8, 16
    m, n, nnz, dg = g["m"], g["n_cols"], g["nnz"], g["dev"]
    d = _on_device(_inputs("wave", h, f))
    node_bytes = 4 * (n * h * f + m * h + n * h + m * h)          # grad_feat, grad_attn_row, grad_attn_col, delta
    assert 4 * h * nnz > 2 * node_bytes

    def bwd(score):
        out, emax, esum, _ = gat.gat_forward_edge(d["attn_row"], d["attn_col"], dg["row_ptr"], dg["col_ind"], SLOPE, d["X"], score)
        del out                                 # (the backward does not take it)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res = gat.gat_backward_edge(SLOPE, 0.0, dg["row_ptr"], dg["col_ind"], dg["col_ptr"], dg["row_ind"], dg["val_idx"],
                                    d["attn_row"], d["attn_col"], d["X"], emax, esum, d["dO"], score=score,
                                    want_grad_score=False)
        torch.cuda.synchronize()
        assert res[3] is None
        return torch.cuda.max_memory_allocated() - base

    for transport in (False, True):
        with _Ctypes(transport):
            for score in (None, d["score"]):
                bwd(score)
                rise = bwd(score)
                print(f"gat_edge backward peak rise {rise} B (node arrays {node_bytes} B, one [h, nnz] tensor {4 * h * nnz} B)")
                assert rise < node_bytes + 2 * h * nnz, (rise, node_bytes, 2 * h * nnz)


# ---- 8. autograd, layers, argument errors -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f", [("lane", 2, 20), ("wave", 8, 16), ("block", 3, 7), ("tall", 1, 128)])
def test_autograd_through_the_operator(kind, h, f):
    """GATConvFuse_edge under torch.autograd: the gradients are gat_backward_edge's; grad_score exists only when score
    requires one; the inference operator gives the forward's bits."""
    from DFGNN.operators.fused_gatconv import GATConvFuse_edge, GATConvFuse_inference_edge
    g = _graph(kind)
    dg = g["dev"]
    d = _on_device(_inputs(kind, h, f))
    raw = _pair(g, d)
    leaves = {k: d[k].clone().requires_grad_(True) for k in ("attn_row", "attn_col", "X", "score")}

    def run(score):
        return GATConvFuse_edge(leaves["attn_row"], leaves["attn_col"], dg["row_ptr"], dg["col_ind"], dg["col_ptr"], dg["row_ind"],
                                dg["val_idx"], SLOPE, leaves["X"], 0.0, score)
    out = run(leaves["score"])
    assert torch.equal(out, raw["out"])
    grads = torch.autograd.grad(out, list(leaves.values()), d["dO"])
    for got, name in zip(grads, ("grad_attn_row", "grad_attn_col", "grad_feat", "grad_score")):
        assert torch.equal(got, raw[name]), name
    out = run(d["score"])                                           # a score that needs no gradient
    grads = torch.autograd.grad(out, [leaves[k] for k in ("attn_row", "attn_col", "X")], d["dO"])
    for got, name in zip(grads, ("grad_attn_row", "grad_attn_col", "grad_feat")):
        assert torch.equal(got, raw[name]), name
    plain = _pair(g, d, with_score=False)
    out = run(None)
    assert torch.equal(out, plain["out"])
    assert torch.equal(torch.autograd.grad(out, leaves["X"], d["dO"])[0], plain["grad_feat"])
    with torch.no_grad():
        assert torch.equal(GATConvFuse_inference_edge(d["attn_row"], d["attn_col"], dg["row_ptr"], dg["col_ind"], SLOPE, d["X"],
                                                      d["score"]), raw["out"])
    torch.manual_seed(3)                                            # dropout: the randoms are drawn in the forward and kept
    out = GATConvFuse_edge(leaves["attn_row"], leaves["attn_col"], dg["row_ptr"], dg["col_ind"], dg["col_ptr"], dg["row_ind"],
                           dg["val_idx"], SLOPE, leaves["X"], 0.5, leaves["score"])
    torch.manual_seed(3)
    mask = torch.rand((g["nnz"], h), dtype=torch.float32, device=DEV)
    want = _pair(g, dict(d, mask=mask), True, True, drop=0.5)
    assert torch.equal(out, want["out"])
    grads = torch.autograd.grad(out, list(leaves.values()), d["dO"])
    for got, name in zip(grads, ("grad_attn_row", "grad_attn_col", "grad_feat", "grad_score")):
        assert torch.equal(got, want[name]), name


def _layer_grads(layer, run, weights):
    outs, grads = [], []
    for fuse in (False, True):
        layer.zero_grad()
        out = run(fuse)
        (out * torch.linspace(-1, 1, out.numel(), device=DEV).reshape(out.shape)).sum().backward()
        outs.append(out.detach())
        grads.append([p.grad.clone() for p in weights])
    return outs, grads


def test_layers_against_their_torch_branches():
    """GATConv_edge fused against its non-fused branch on the cora-like graph at two heads, the gradients of W, a_l, a_r,
    lin_edge and att_edge included, and in .eval() through the inference operator; GATConv_forward on `block` with
    (h_cols, h_rows); both --conv gat training formats run."""
    import argparse

    from DFGNN.layers import GATConv_edge, GATConv_forward, load_graphconv_layer, load_prepfunc, preprocess_block
    from DFGNN.utils import synthetic as S
    from DFGNN.utils.graph import Block
    torch.manual_seed(1)
    cora = S.cora_like().to(DEV)
    args = argparse.Namespace(conv="gat", format="forward", dim=64, heads=2)
    params = load_prepfunc(args)(cora)
    nnz = params[3].numel()
    layer = GATConv_edge(64, 32, 2, edge_dim=8).to(DEV).train()
    x = torch.randn(cora.num_nodes(), 64, device=DEV)
    edge_attr = torch.randn(nnz, 8, device=DEV)
    names = ("W.weight", "a_l", "a_r", "lin_edge.weight", "att_edge")
    weights = [layer.W.weight, layer.a_l, layer.a_r, layer.lin_edge.weight, layer.att_edge]
    outs, grads = _layer_grads(layer, lambda fuse: layer(params, x, edge_attr, fuse=fuse), weights)
    assert outs[1].shape == (cora.num_nodes(), 64)
    _check(outs[1], outs[0], "GATConv_edge out")
    for name, a, b in zip(names, *grads):
        _check(b, a, f"GATConv_edge d{name}")
    with torch.no_grad():
        _check(layer.eval()(params, x, edge_attr, fuse=True), outs[0], "GATConv_edge eval out")
    g = rc.graph("block")
    bparams = preprocess_block(Block(g["src"], g["dst"], g["m"], g["n_cols"]).to(DEV))
    h_cols = torch.randn(g["n_cols"], 16, device=DEV)
    h_rows = h_cols[:g["m"]].contiguous()
    layer = GATConv_forward(16, 8, 3).to(DEV).train()
    weights = [layer.W.weight, layer.a_l, layer.a_r]
    outs, grads = _layer_grads(layer, lambda fuse: layer(bparams, (h_cols, h_rows), fuse=fuse), weights)
    assert outs[1].shape == (g["m"], 24)
    _check(outs[1], outs[0], "GATConv_forward block out")
    for name, a, b in zip(names, *grads):
        _check(b, a, f"GATConv_forward block d{name}")
    for fmt in ("forward", "forward_edge"):
        args = argparse.Namespace(conv="gat", format=fmt, dim=64, heads=2)
        timing = load_graphconv_layer(args).to(DEV).eval()
        with torch.no_grad():
            fused, plain = timing(params, x, fuse=True), timing(params, x, fuse=False)
        if fmt == "forward_edge":
            assert fused[1] > 0
            fused, plain = fused[0], plain[0]
        assert fused.shape == (cora.num_nodes(), 128)
        _check(fused, plain, f"--conv gat --format {fmt}")


def test_argument_errors_agree_between_transports():
    """A bad argument raises the same RuntimeError text on the torch extension and on the ctypes transport."""
    import fused_gatconv as gat
    g = _graph("lane")
    dg = g["dev"]
    d = _on_device(_inputs("lane", 2, 20))
    good = _pair(g, d)

    def run():
        errs = []
        for bad in (dict(score=d["score"].t().contiguous()), dict(score=d["score"][:, 1:].contiguous()), dict(score=d["score"].double()),
                    dict(attn_col=d["attn_col"][1:]), dict(attn_row=d["attn_row"].reshape(-1)), dict(mask=d["mask"][1:]),
                    dict(drop=1.5), dict(grad=d["dO"][1:]), dict(edge_max=good["edge_max"].t().contiguous())):
            a = dict(score=d["score"], attn_col=d["attn_col"], attn_row=d["attn_row"], mask=d["mask"], drop=DROP, grad=d["dO"],
                     edge_max=good["edge_max"])
            a.update(bad)
            try:
                if set(bad) & {"grad", "edge_max"}:
                    gat.gat_backward_edge(SLOPE, a["drop"], dg["row_ptr"], dg["col_ind"], dg["col_ptr"], dg["row_ind"], dg["val_idx"],
                                          a["attn_row"], a["attn_col"], d["X"], a["edge_max"], good["edge_sum"], a["grad"],
                                          score=a["score"], edge_mask=a["mask"])
                else:
                    gat.gat_forward_edge(a["attn_row"], a["attn_col"], dg["row_ptr"], dg["col_ind"], SLOPE, d["X"], a["score"],
                                         a["drop"], a["mask"])
                errs.append(None)
            except RuntimeError as e:
                errs.append(str(e).splitlines()[0])
        return errs

    err_ext = run()
    with _Ctypes():
        err_ctypes = run()
    words = ("score must have shape",) * 2 + ("score must have dtype", "attn_col must have shape", "attn_row must have shape",
                                               "edge_mask must have shape", "attn_drop must be in", "grad must have shape",
                                               "edge_max must have shape")
    assert len(err_ext) == len(err_ctypes) == len(words)
    for e1, e2, word in zip(err_ext, err_ctypes, words):
        assert e1 and e2 and word in e1 and word in e2, (e1, e2)
        assert e1 == e2, (e1, e2)                                   # the same text on both transports
