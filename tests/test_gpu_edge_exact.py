"""GPU tests at fp32-level bounds (run with `-m gpu` on an MI355X): every general-kernel entry point of GT, GAT and GATv2
on the boundary-degree cases of tests/parity_cases.py -- rows (transposed: columns) of degree cap - 1, cap, cap + 1 around
every tile, unroll and LDS-cap boundary of the row loops, two aligned 16-row blocks at the workgroup cap, four lane
layouts, both forms (wave per row / lane groups), with and without edge values.  Every output is held to
MARGIN x (error of the plain-fp32 reference against the float64 one on the same inputs), in the per-row measure of
parity_cases; tests/test_parity_cases_host.py proves that one lost boundary edge moves every such output by at least
POWER x that bound.  Each check prints measured error, fp32-reference error and bound (pytest -s)."""
import numpy as np
import pytest
import torch

import parity_cases as pc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SLOPE = pc.SLOPE


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _one(x):
    return x[0] if isinstance(x, (list, tuple)) else x


class _Checker:
    """Holds one case's float64 reference and bounds; check() prints the triple and notes a miss, done() asserts.
    Outputs named in `loose` are held to the suite's absolute bar 1e-3 max(1, max |ref|) instead (peaked rows only)."""

    def __init__(self, g, ref64, bounds, what, loose=()):
        self.g, self.ref64, self.bounds, self.what, self.loose = g, ref64, bounds, what, loose
        self.missed, self.outputs = [], {}

    def check(self, entry, name, got, ref_name=None):
        ref_name = ref_name or name
        self.outputs[(entry, name)] = _np(got)
        got = _np(got).astype(np.float64)
        assert np.isfinite(got).all(), (self.what, entry, name)
        if ref_name in self.loose:
            ref = self.ref64[ref_name]
            err, bar = float(np.abs(got - ref).max()), 1e-3 * max(1.0, float(np.abs(ref).max()))
            print(f"edge-exact {self.what} | {entry} {name}: max abs err {err:.3e} (absolute bar {bar:.3e})")
            if not err < bar:
                self.missed.append((entry, name, err, bar))
            return
        err, at = pc.error_of(self.g, ref_name, got, self.ref64[ref_name], where=True)
        bound = self.bounds[ref_name]
        print(f"edge-exact {self.what} | {entry} {name}: measured {err:.3e} at (node, head) {at}, fp32 reference "
              f"{bound / pc.MARGIN:.3e}, bound {bound:.3e}")
        if not err <= bound:
            self.missed.append((entry, name, err, bound))

    def done(self):
        assert not self.missed, (self.what, self.missed)


def _graph_on_device(g):
    return {k: _dev(g[k], torch.int32) for k in ("row_ptr", "col_ind", "rows", "col_ptr", "row_ind", "val_idx")}


def _empties(g):
    return np.diff(g["row_ptr"]) == 0, np.diff(g["col_ptr"]) == 0


def _block_plan(module, on):
    class _Ctx:
        def __enter__(self):
            self.saved = module.USE_BLOCK_PLAN
            module.USE_BLOCK_PLAN = on

        def __exit__(self, *exc):
            module.USE_BLOCK_PLAN = self.saved
    return _Ctx()


# ---- GT -------------------------------------------------------------------------------------------------------------------
def _gt_entry_points(c, d, val, Q, K, V, dO, er, ec):
    """Every GT entry point on one set of device inputs, checked through checker c."""
    import dfgnn_native
    import fused_gtconv as gt
    from _binding_util import stream_ptr
    ip, idx, rows, cp, ri, vi = (d[k] for k in ("row_ptr", "col_ind", "rows", "col_ptr", "row_ind", "val_idx"))
    for plan in (True, False):
        with _block_plan(gt, plan):
            tag = "plan" if plan else "no plan"
            c.check(f"hyper ({tag})", "out", gt.gt_hyper_inference(ip, idx, rows, val, 1024, Q, K, V)[0])
            out, attn = gt.gt_hyper_forward(ip, idx, rows, val, cp, ri, vi, 1024, Q, K, V)
            c.check(f"gt_hyper_forward ({tag})", "out", out)
            c.check(f"gt_hyper_forward ({tag})", "attn_edge", attn)
            dQ, dK, dV = gt.gt_backward(ip, idx, rows, val, cp, ri, vi, 1024, Q, K, V, attn, dO)
            for name, t in (("dQ", dQ), ("dK", dK), ("dV", dV)):
                c.check(f"gt_backward ({tag})", name, t)
            assert (_np(out)[er] == 0).all() and (_np(dQ)[er] == 0).all()
            assert (_np(dK)[ec] == 0).all() and (_np(dV)[ec] == 0).all()
    c.check("tiling", "out", gt.gt_tiling_inference(ip, idx, val, 128, Q, K, V)[0])
    c.check("softmax", "out", gt.gt_softmax_inference(ip, idx, rows, val, 128, Q, K, V)[0])
    c.check("softmax_gm", "out", _one(gt.gt_softmax_gm_inference(ip, idx, rows, val, Q, K, V)))
    c.check("csr", "out", gt.gt_csr_inference(ip, idx, val, 128, Q, K, V)[0])
    c.check("csr_gm", "out", gt.gt_csr_gm_inference(ip, idx, val, Q, K, V)[0])
    out, mx, sm = gt.gt_forward_rowstats(ip, idx, val, Q, K, V)
    dQ, dK, dV = gt.gt_backward_rowstats(ip, idx, val, cp, ri, vi, Q, K, V, out, mx, sm, dO)
    for name, t in (("out", out), ("row_max", mx), ("row_sum", sm), ("dQ", dQ), ("dK", dK), ("dV", dV)):
        c.check("rowstats pair", name, t)
    assert (_np(out)[er] == 0).all() and (_np(dQ)[er] == 0).all() and (_np(dK)[ec] == 0).all() and (_np(dV)[ec] == 0).all()
    assert (_np(mx)[er] == np.float32(-1e38)).all() and (_np(sm)[er] == 0).all()
    m, h, f = Q.shape
    plain = torch.full_like(Q, float("nan"))                    # the C ABI's forward without statistics: inference
    rc = dfgnn_native.lib().dfgnn_gt_fwd_rowstats(m, idx.numel(), h, f, ip.data_ptr(), idx.data_ptr(), val.data_ptr(),
                                                  Q.data_ptr(), K.data_ptr(), V.data_ptr(), None, None, plain.data_ptr(),
                                                  stream_ptr(Q.device))
    torch.cuda.synchronize()
    assert rc == 0
    c.check("rowstats inference", "out", plain)


@pytest.mark.parametrize("case", pc.case_ids("gt"), ids=str)
def test_gt_boundary_degrees(oracle_mod, case):
    """GT inference (hyper with and without the block plan, tiling, softmax, softmax_gm, csr, csr_gm, rowstats inference)
    and both training pairs: out, attn_edge, row statistics, dQ, dK, dV."""
    g = pc.graph(case[0], case[1])
    x, ref64, _, bounds = pc.references("gt", *case)
    d = _graph_on_device(g)
    val, Q, K, V, dO = (_dev(x[k]) for k in ("val", "Q", "K", "V", "dO"))
    c = _Checker(g, ref64, bounds, f"gt {case}")
    _gt_entry_points(c, d, val, Q, K, V, dO, *_empties(g))
    c.done()


# ---- GAT ------------------------------------------------------------------------------------------------------------------
def _gat_inference_entry_points(c, d, ar, ac, X, monkeypatch, chunk_rows):
    import fused_gatconv as gat
    ip, idx, rows = d["row_ptr"], d["col_ind"], d["rows"]
    for plan in (True, False):
        with _block_plan(gat, plan):
            c.check(f"hyper ({'plan' if plan else 'no plan'})", "out",
                    _one(gat.gat_inference_hyper(1024, ar, ac, ip, idx, rows, SLOPE, X)), "inference")
    c.check("softmax", "out", _one(gat.gat_inference_softmax(128, ar, ac, ip, idx, rows, SLOPE, X)), "inference")
    c.check("softmax_gm", "out", _one(gat.gat_inference_softmax_gm(ar, ac, ip, idx, rows, SLOPE, X)), "inference")
    c.check("tiling", "out", _one(gat.gat_inference_tiling(ar, ac, ip, idx, SLOPE, X)), "inference")
    c.check("csr", "out", _one(gat.gat_inference(ar, ac, ip, idx, SLOPE, X)), "inference")
    c.check("recompute", "out", _one(gat.gat_inference_hyper_recompute(ar, ac, ip, idx, SLOPE, X)), "inference")
    monkeypatch.setattr(gat, "TILING_CHUNK_ROWS", chunk_rows)
    monkeypatch.setattr(gat, "TILING_CHUNK_MIN_TABLE", 0)
    monkeypatch.setattr(gat, "TILING_CHUNK_MIN_DEGREE", 0)
    assert gat._use_chunked_tiling(X.size(0), idx.numel(), X.size(1), X.size(2))
    c.check(f"tiling chunked ({chunk_rows} rows)", "out", _one(gat.gat_inference_tiling(ar, ac, ip, idx, SLOPE, X)),
            "inference")
    monkeypatch.undo()


def _gat_training(c, g, d, x, ar, ac, X, dO, attn_drop, er, ec):
    """gat_forward / gat_backward; with dropout the references are recomputed with the randoms the forward drew."""
    import fused_gatconv as gat
    ip, idx, cp, ri, vi = (d[k] for k in ("row_ptr", "col_ind", "col_ptr", "row_ind", "val_idx"))
    torch.manual_seed(5)
    out, emax, esum, mask = gat.gat_forward(ar, ac, ip, idx, SLOPE, X, attn_drop)
    gf, gr, gc = gat.gat_backward(SLOPE, attn_drop, ip, idx, cp, ri, vi, emax, esum, mask, X, ar, ac, dO)
    tag = "training" if attn_drop == 0 else f"training, dropout {attn_drop}"
    if attn_drop > 0:
        mask_np = _np(mask)
        assert mask_np.shape == (g["nnz"], X.size(1))
        ref64 = pc.gat_reference(g["row_ptr"], g["col_ind"], x, "f64", mask_np, attn_drop)
        ref32 = pc.gat_reference(g["row_ptr"], g["col_ind"], x, "f32", mask_np, attn_drop)
        c = _Checker(g, ref64, {k: pc.MARGIN * pc.error_of(g, k, ref32[k], ref64[k]) for k in ref64}, c.what, c.loose)
    for name, t in (("out", out), ("edge_max", emax), ("edge_sum", esum), ("grad_feat", gf), ("grad_attn_row", gr),
                    ("grad_attn_col", gc)):
        c.check(tag, name, t)
    assert (_np(out)[er] == 0).all() and (_np(gr)[er] == 0).all() and (_np(emax)[er] < -9e37).all()
    assert (_np(gf)[ec] == 0).all() and (_np(gc)[ec] == 0).all()
    return c


@pytest.mark.parametrize("case", pc.case_ids("gat"), ids=str)
def test_gat_boundary_degrees(oracle_mod, monkeypatch, case):
    """GAT inference (hyper with and without the block plan, softmax, softmax_gm, tiling, csr, recompute, chunked tiling
    with a chunk boundary inside the pool) and the training pair with and without a dropout mask."""
    g = pc.graph(case[0], case[1])
    x, ref64, _, bounds = pc.references("gat", *case)
    d = _graph_on_device(g)
    ar, ac, X, dO = (_dev(x[k]) for k in ("attn_row", "attn_col", "X", "dO"))
    er, ec = _empties(g)
    c = _Checker(g, ref64, bounds, f"gat {case}")
    assert g["pool"][0] < 192 <= g["pool"][-1]
    _gat_inference_entry_points(c, d, ar, ac, X, monkeypatch, 192)
    _gat_training(c, g, d, x, ar, ac, X, dO, 0.0, er, ec)
    c2 = _gat_training(c, g, d, x, ar, ac, X, dO, 0.25, er, ec)
    c2.done()
    c.done()


# ---- GATv2 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.case_ids("gatv2"), ids=str)
def test_gatv2_boundary_degrees(case):
    """gatv2_forward / gatv2_backward (out, row statistics, dX_row, dX_col, dattn) and gatv2_inference."""
    import fused_gatconv as gat
    g = pc.graph(case[0], case[1])
    x, ref64, _, bounds = pc.references("gatv2", *case)
    d = _graph_on_device(g)
    attn, xr, xc, dO = (_dev(x[k]) for k in ("attn", "X_row", "X_col", "dO"))
    er, ec = _empties(g)
    c = _Checker(g, ref64, bounds, f"gatv2 {case}")
    out, mx, sm = gat.gatv2_forward(attn, d["row_ptr"], d["col_ind"], SLOPE, xr, xc)
    dxr, dxc, da = gat.gatv2_backward(SLOPE, d["row_ptr"], d["col_ind"], d["col_ptr"], d["row_ind"], attn, xr, xc, out, mx, sm,
                                      dO)
    torch.cuda.synchronize()
    for name, t in (("out", out), ("row_max", mx), ("row_sum", sm), ("dX_row", dxr), ("dX_col", dxc), ("dattn", da[None])):
        c.check("training pair", name, t)
    c.check("gatv2_inference", "out", gat.gatv2_inference(attn, d["row_ptr"], d["col_ind"], SLOPE, xr, xc))
    assert (_np(out)[er] == 0).all() and (_np(dxr)[er] == 0).all() and (_np(dxc)[ec] == 0).all()
    assert (_np(mx)[er] == np.float32(-1e38)).all() and (_np(sm)[er] == 0).all()
    c.done()


# ---- peaked and ordered softmax in the general kernels -------------------------------------------------------------------
PEAKED = [(wave, f) for wave in (False, True) for f in pc.PEAKED_WIDTHS]


def _constant_rows_sum_to_degree(g, row_sum, what):
    """Rows whose logits are all equal: every exponential is exp(0) = 1 exactly, so the sum is the degree bit for bit."""
    rows = np.nonzero(g["pattern"] == "constant")[0]
    assert len(rows) == len(pc.PEAKED_DEGREES)
    got = _np(row_sum)[rows, 0]
    print(f"edge-exact {what}: row_sum of the constant rows {got.tolist()} (degrees {g['deg'][rows].tolist()})")
    assert (got == g["deg"][rows].astype(np.float32)).all(), (what, got)


@pytest.mark.parametrize("wave,f", PEAKED)
def test_gt_peaked_softmax(oracle_mod, wave, f):
    """Ascending / descending ladders (rescale factor 0 between 64-edge tiles), constant rows, logits of +-60: out,
    attn_edge, the row statistics and dV at the fp32-level bound; dQ, dK finite and at the absolute bar."""
    g = pc.peaked_graph(wave)
    x, ref64, _, bounds = pc.peaked_references("gt", wave, f)
    d = _graph_on_device(g)
    val, Q, K, V, dO = (_dev(x[k]) for k in ("val", "Q", "K", "V", "dO"))
    c = _Checker(g, ref64, bounds, f"gt peaked wave={wave} f={f}", loose=pc.PEAKED_LOOSE["gt"])
    _gt_entry_points(c, d, val, Q, K, V, dO, *_empties(g))
    _constant_rows_sum_to_degree(g, c.outputs[("rowstats pair", "row_sum")], c.what)
    c.done()


@pytest.mark.parametrize("wave,f", PEAKED)
def test_gat_peaked_softmax(oracle_mod, monkeypatch, wave, f):
    g = pc.peaked_graph(wave)
    x, ref64, _, bounds = pc.peaked_references("gat", wave, f)
    d = _graph_on_device(g)
    ar, ac, X, dO = (_dev(x[k]) for k in ("attn_row", "attn_col", "X", "dO"))
    c = _Checker(g, ref64, bounds, f"gat peaked wave={wave} f={f}", loose=pc.PEAKED_LOOSE["gat"])
    _gat_inference_entry_points(c, d, ar, ac, X, monkeypatch, 512)        # (a chunk boundary inside the ladder)
    _gat_training(c, g, d, x, ar, ac, X, dO, 0.0, *_empties(g))
    _constant_rows_sum_to_degree(g, c.outputs[("training", "edge_sum")], c.what)
    c.done()


@pytest.mark.parametrize("wave,f", PEAKED)
def test_gatv2_peaked_softmax(wave, f):
    import fused_gatconv as gat
    g = pc.peaked_graph(wave)
    x, ref64, _, bounds = pc.peaked_references("gatv2", wave, f)
    d = _graph_on_device(g)
    attn, xr, xc, dO = (_dev(x[k]) for k in ("attn", "X_row", "X_col", "dO"))
    c = _Checker(g, ref64, bounds, f"gatv2 peaked wave={wave} f={f}", loose=pc.PEAKED_LOOSE["gatv2"])
    out, mx, sm = gat.gatv2_forward(attn, d["row_ptr"], d["col_ind"], SLOPE, xr, xc)
    dxr, dxc, da = gat.gatv2_backward(SLOPE, d["row_ptr"], d["col_ind"], d["col_ptr"], d["row_ind"], attn, xr, xc, out, mx, sm,
                                      dO)
    torch.cuda.synchronize()
    for name, t in (("out", out), ("row_max", mx), ("row_sum", sm), ("dX_row", dxr), ("dX_col", dxc), ("dattn", da[None])):
        c.check("training pair", name, t)
    c.check("gatv2_inference", "out", gat.gatv2_inference(attn, d["row_ptr"], d["col_ind"], SLOPE, xr, xc))
    _constant_rows_sum_to_degree(g, sm, c.what)
    c.done()
