"""GPU tests of RECTANGULAR graphs (m rows x n_cols columns) in the four any-graph pairs -- GT row statistics, GT with an
attention bias, GT with edge features, GATv2 (include/dfgnn.h: dfgnn_*_rect) -- and of the rectangular preprocessing.
Cases, reference and the embedding of square cases: tests/rect_cases.py.  The bar of groups 1 and 5 is the project's own,
max abs error < 1e-3 * max(1, max |ref|) with every value finite; group 3 holds the embedded boundary-degree cases of
tests/parity_cases.py to those cases' own fp32-level bounds.

Measured on an MI355X: the worst ratio of the measured error to the fp32 reference's own over all cases of group 3, both
embeddings (the bound is parity_cases.MARGIN = 8 x; dK: 8 x gt_bias_cases.DK_FACTOR):
    row-statistics pair   out 0.62   row_sum 0.51   row_max 2.61   dQ 4.38   dK 5.05 (0.16 of its bound)   dV 0.87
    GATv2 (shifted)       out 0.43   row_sum 0.10   row_max 3.41   dX_row 0.62   dX_col 0.89   dattn 1.54
The worst of all is dQ of (transposed, low, f 7, h 2, weighted) under col_shift: 0.55 of its bound."""
import numpy as np
import pytest
import torch

import parity_cases as pc
import rect_cases as rc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-3
TRANSPORTS = ("ext", "ctypes")


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _check(got, ref, what):
    got, ref = _np(got).astype(np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    bound = BAR * max(1.0, float(np.abs(ref).max()) if ref.size else 0.0)
    print(f"rect {what}: max abs err {err:.3e} (bound {bound:.3e})")
    assert np.isfinite(got).all(), what
    assert err < bound, (what, err, bound)


def _graph_on_device(g):
    return {k: _dev(g[k], torch.int32) for k in ("row_ptr", "col_ind", "rows", "col_ptr", "row_ind", "val_idx")}


def _poison(nbytes):
    """Best effort against an unwritten output slot: fill and free a NaN tensor of the outputs' total size, so that the
    allocations of the next call tend to land on NaN.  The caching allocator gives no guarantee that they do."""
    torch.full((max(1, nbytes // 4),), float("nan"), device=DEV)


def _run(pair, d, x, poison=0):
    """Forward, inference and backward of `pair` on device inputs x -> dict of outputs (out, row_max, row_sum, inference,
    gradients named as rect_cases.reference names them)."""
    import fused_gatconv as gat
    import fused_gtconv as gt
    rp, ci, cp, ri, vi = (d[k] for k in ("row_ptr", "col_ind", "col_ptr", "row_ind", "val_idx"))
    _poison(poison)
    if pair == "gatv2":
        out, mx, sm = gat.gatv2_forward(x["attn"], rp, ci, rc.SLOPE, x["X_row"], x["X_col"])
        inf = gat.gatv2_inference(x["attn"], rp, ci, rc.SLOPE, x["X_row"], x["X_col"])
        _poison(poison)
        dxr, dxc, da = gat.gatv2_backward(rc.SLOPE, rp, ci, cp, ri, x["attn"], x["X_row"], x["X_col"], out, mx, sm, x["dO"])
        res = dict(out=out, row_max=mx, row_sum=sm, inference=inf, dX_row=dxr, dX_col=dxc, dattn=da)
    elif pair == "rowstats":
        out, mx, sm = gt.gt_forward_rowstats(rp, ci, x["val"], x["Q"], x["K"], x["V"])
        _poison(poison)
        dQ, dK, dV = gt.gt_backward_rowstats(rp, ci, x["val"], cp, ri, vi, x["Q"], x["K"], x["V"], out, mx, sm, x["dO"])
        res = dict(out=out, row_max=mx, row_sum=sm, dQ=dQ, dK=dK, dV=dV)
    elif pair == "bias":
        out, mx, sm = gt.gt_forward_bias(rp, ci, x["val"], x["bias"], x["Q"], x["K"], x["V"])
        inf = gt.gt_inference_bias(rp, ci, x["val"], x["bias"], x["Q"], x["K"], x["V"])
        _poison(poison)
        dQ, dK, dV, db = gt.gt_backward_bias(rp, ci, x["val"], x["bias"], cp, ri, vi, x["Q"], x["K"], x["V"], out, mx, sm, x["dO"])
        res = dict(out=out, row_max=mx, row_sum=sm, inference=inf, dQ=dQ, dK=dK, dV=dV, dbias=db)
    else:
        out, mx, sm = gt.gt_forward_edge(rp, ci, x["val"], x["E"], x["Q"], x["K"], x["V"])
        inf = gt.gt_inference_edge(rp, ci, x["val"], x["E"], x["Q"], x["K"], x["V"])
        _poison(poison)
        dQ, dK, dV, dE = gt.gt_backward_edge(rp, ci, x["val"], x["E"], cp, ri, vi, x["Q"], x["K"], x["V"], out, mx, sm, x["dO"])
        res = dict(out=out, row_max=mx, row_sum=sm, inference=inf, dQ=dQ, dK=dK, dV=dV, dE=dE)
    torch.cuda.synchronize()
    return res


class _Transport:
    """Run the block with the torch extension (`ext`) or with the ctypes transport alone."""

    def __init__(self, which):
        self.which = which

    def __enter__(self):
        import dfgnn_native
        self.saved = dfgnn_native.ext
        if self.which == "ctypes":
            dfgnn_native.ext = lambda: None
        else:
            assert dfgnn_native.ext() is not None, "the torch extension is not built"

    def __exit__(self, *exc):
        import dfgnn_native
        dfgnn_native.ext = self.saved


# ---- 1. every output of every pair against the float64 reference ----------------------------------------------------------
@pytest.mark.parametrize("h,f", rc.WIDTHS)
@pytest.mark.parametrize("kind", ["tall", "wide", "block", "line_row", "line_col"])
def test_pairs_against_reference(kind, h, f):
    """All four pairs, unit and weighted val: every output at the bar; exact zeros at empty rows and columns, the sentinel
    at empty rows; inference equals the training forward's out bit for bit; a second backward agrees bit for bit.  Before
    each call a NaN tensor of the outputs' size is filled and freed (_poison: best effort, the allocator decides)."""
    g = rc.graph(kind)
    d = _graph_on_device(g)
    er, ec = g["deg"] == 0, g["indeg"] == 0
    for pair in rc.PAIRS:
        for unit in ((True,) if pair == "gatv2" else (True, False)):
            xn = rc.inputs(pair, g, h, f, unit)
            ref = rc.reference_on(pair, g, xn)
            x = {k: _dev(v) for k, v in xn.items()}
            nbytes = 4 * sum(v.size for v in ref.values())
            got = _run(pair, d, x, poison=nbytes)
            what = f"{kind} {pair} h{h} f{f} {'unit' if unit else 'weighted'}"
            for name, want in ref.items():
                _check(got[name], want, f"{what} {name}")
            if "inference" in got:
                assert torch.equal(got["inference"], got["out"]), what
            for name in rc.ROW_OUTPUTS[pair]:
                assert (_np(got[name])[er] == 0).all(), (what, name)
            for name in rc.COL_OUTPUTS[pair]:
                assert (_np(got[name])[ec] == 0).all(), (what, name)
            assert (_np(got["row_max"])[er] == np.float32(rc.SENTINEL_MAX)).all() and (_np(got["row_sum"])[er] == 0).all()
            again = _run(pair, d, x, poison=nbytes)
            for name in got:
                assert torch.equal(got[name], again[name]), (what, name)


@pytest.mark.parametrize("transport", TRANSPORTS)
@pytest.mark.parametrize("kind", ["no_rows", "no_cols"])
def test_degenerate_extents(kind, transport):
    """0 x 5 and 5 x 0, nnz = 0: nothing raises; the outputs that exist are zeros or sentinels in full (they are allocated
    over NaN where the allocator obliges)."""
    g = rc.graph(kind)
    d = _graph_on_device(g)
    with _Transport(transport):
        for pair in rc.PAIRS:
            xn = rc.inputs(pair, g, 2, 20, True)
            ref = rc.reference_on(pair, g, xn)
            got = _run(pair, d, {k: _dev(v) for k, v in xn.items()}, poison=4 * 5 * 2 * 20 * 4)
            for name, want in ref.items():
                assert _np(got[name]).shape == want.shape, (pair, name)
                assert np.array_equal(_np(got[name]).astype(np.float64), want.astype(np.float32).astype(np.float64)), (pair, name)


# ---- 2. square is untouched ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["lane", "wave"])
def test_square_entries_are_the_rect_entries(kind):
    """On the lane and wave graphs of test_gpu_gatv2._graph: the square C entry, the *_rect entry with n_cols == m and the
    Python function give torch.equal results, for every output of every pair."""
    import dfgnn_native
    from _binding_util import stream_ptr
    from test_gpu_gatv2 import _graph
    sq = _graph(kind)
    m, nnz, h, f = sq["m"], sq["nnz"], 2, 20
    rows = _np(sq["rows"]).astype(np.int32)
    _, _, val_idx = rc.csc_of(_np(sq["row_ptr"]), _np(sq["col_ind"]), rows, m)
    d = dict(row_ptr=sq["row_ptr"], col_ind=sq["col_ind"], col_ptr=sq["col_ptr"], row_ind=sq["row_ind"], val_idx=_dev(val_idx))
    g = dict(m=m, n_cols=m, nnz=nnz)
    lib, st = dfgnn_native.lib(), stream_ptr(torch.device(DEV))
    p = lambda t: t.data_ptr()  # noqa: E731
    E = lambda *s: torch.full(s, float("nan"), device=DEV)  # noqa: E731
    for pair in rc.PAIRS:
        x = {k: _dev(v) for k, v in rc.inputs(pair, g, h, f, False).items()}
        py = _run(pair, d, x)
        for rect in (False, True):
            ext = (m,) if rect else ()
            sfx = "_rect" if rect else ""
            out, mx, sm, dr = E(m, h, f), E(m, h), E(m, h), E(m, h, f)
            dc, dc2, delta = E(m, h, f), E(m, h, f), E(m, h)
            gp = (p(d["row_ptr"]), p(d["col_ind"]))
            csc = (p(d["col_ptr"]), p(d["row_ind"]), p(d["val_idx"]))
            if pair == "gatv2":
                ws, da = E(lib.dfgnn_gatv2_bwd_ws_floats(h, f)), E(h, f)
                feats = (p(x["attn"]), rc.SLOPE, p(x["X_row"]), p(x["X_col"]))
                assert getattr(lib, "dfgnn_gatv2_fwd" + sfx)(m, *ext, nnz, h, f, *gp, *feats, p(mx), p(sm), p(out), st) == 0
                assert getattr(lib, "dfgnn_gatv2_bwd" + sfx)(m, *ext, nnz, h, f, *gp, *csc[:2], *feats, p(out), p(mx), p(sm),
                                                             p(x["dO"]), p(delta), p(ws), p(dr), p(dc), p(da), st) == 0
                c = dict(out=out, row_max=mx, row_sum=sm, dX_row=dr, dX_col=dc, dattn=da)
            else:
                name = {"rowstats": "rowstats", "bias": "bias", "edge": "edge"}[pair]
                extra_in = () if pair == "rowstats" else (p(x["bias"]),) if pair == "bias" else (p(x["E"]),)
                gextra = E(h, nnz) if pair == "bias" else E(nnz, h, f) if pair == "edge" else None
                qkv = (p(x["Q"]), p(x["K"]), p(x["V"]))
                assert getattr(lib, f"dfgnn_gt_fwd_{name}{sfx}")(m, *ext, nnz, h, f, *gp, p(x["val"]), *extra_in, *qkv, p(mx), p(sm),
                                                                p(out), st) == 0
                tail = () if gextra is None else (p(gextra),)
                assert getattr(lib, f"dfgnn_gt_bwd_{name}{sfx}")(m, *ext, nnz, h, f, *gp, p(x["val"]), *extra_in, *csc, *qkv, p(out),
                                                                p(mx), p(sm), p(x["dO"]), p(delta), p(dr), p(dc), p(dc2), *tail,
                                                                st) == 0
                c = dict(out=out, row_max=mx, row_sum=sm, dQ=dr, dK=dc, dV=dc2)
                if gextra is not None:
                    c["dbias" if pair == "bias" else "dE"] = gextra
            torch.cuda.synchronize()
            for k, v in c.items():
                assert torch.equal(v, py[k]), (kind, pair, "rect" if rect else "square", k)


# ---- 3. boundary degrees at fp32 level ------------------------------------------------------------------------------------
def _embedded(g0, x, shift, cpad, rpad):
    g = rc.embed_graph(g0["row_ptr"], g0["col_ind"], shift, cpad, rpad)
    y = dict(val=x["val"], Q=rc.embed_rows(x["Q"], rpad), dO=rc.embed_rows(x["dO"], rpad),
             K=rc.embed_cols(x["K"], shift, cpad), V=rc.embed_cols(x["V"], shift, cpad))
    got = _run("rowstats", _graph_on_device(g), {k: _dev(v) for k, v in y.items()})
    back = {}
    for name in ("out", "dQ", "row_sum", "row_max"):
        back[name], clean = rc.restrict_rows(_np(got[name]), g0["m"], np.float32(rc.SENTINEL_MAX) if name == "row_max" else 0.0)
        assert clean, name
    for name in ("dK", "dV"):
        back[name], clean = rc.restrict_cols(_np(got[name]), g0["m"], shift)
        assert clean, name
    return g, back


@pytest.mark.parametrize("case", pc.case_ids("gt"), ids=str)
def test_gt_boundary_degrees_embedded(oracle_mod, case):
    """Every parity_cases GT case of the row-statistics pair in three rectangles.  Trailing padding (3 empty rows, 5 empty
    columns; neither pass changes its form, asserted): torch.equal to the square entry's result on the original case.
    col_shift = m (every column with an edge lies beyond the row extent) and row_pad = m (more rows than columns): every
    output within the case's own fp32-level bounds (dK: x gt_bias_cases.DK_FACTOR, the row-statistics pair's delta, as
    tests/test_gpu_gt_bias.py holds it)."""
    from gt_bias_cases import DK_FACTOR
    g0 = pc.graph(case[0], case[1])
    x, ref64, _, bounds = pc.references("gt", *case)
    m0, nnz = g0["m"], g0["nnz"]
    sq = _run("rowstats", _graph_on_device(g0), {k: _dev(x[k]) for k in ("val", "Q", "K", "V", "dO")})
    assert rc.lane_form(m0 + 3, nnz) == rc.lane_form(m0, nnz) == rc.lane_form(m0 + 5, nnz)
    _, back = _embedded(g0, x, 0, 5, 3)
    for name, a in back.items():
        assert np.array_equal(a, _np(sq[name])), ("padding", name)
    missed = []
    for tag, emb in (("col_shift", (m0, 0, 0)), ("row_pad", (0, 0, m0))):
        _, back = _embedded(g0, x, *emb)
        for name, a in back.items():
            if name == "row_max":                # (the square reference holds 0 at empty rows, the kernels the sentinel)
                a = np.where(np.diff(g0["row_ptr"])[:, None] > 0, a, 0)
            err = pc.error_of(g0, name, a.astype(np.float64), ref64[name])
            bound = bounds[name] * (DK_FACTOR if name == "dK" else 1.0)
            print(f"rect boundary {case} {tag} {name}: measured {err:.3e}, fp32 reference {bounds[name] / pc.MARGIN:.3e}, "
                  f"bound {bound:.3e}")
            assert np.isfinite(a).all()
            if not err <= bound:
                missed.append((tag, name, err, bound))
    assert not missed, (case, missed)


@pytest.mark.parametrize("case", [c for c in pc.case_ids("gatv2") if not c[1]], ids=str)
def test_gatv2_boundary_degrees_shifted(case):
    """GATv2: one as-built and one transposed case per width, col_shift = m, within parity_cases' bounds."""
    g0 = pc.graph(case[0], case[1])
    x, ref64, _, bounds = pc.references("gatv2", *case)
    m0 = g0["m"]
    g = rc.embed_graph(g0["row_ptr"], g0["col_ind"], m0, 0, 0)
    y = dict(attn=x["attn"], X_row=x["X_row"], dO=x["dO"], X_col=rc.embed_cols(x["X_col"], m0, 0))
    got = _run("gatv2", _graph_on_device(g), {k: _dev(v) for k, v in y.items()})
    dxc, clean = rc.restrict_cols(_np(got["dX_col"]), m0, m0)
    assert clean
    mx = np.where(np.diff(g0["row_ptr"])[:, None] > 0, _np(got["row_max"]), 0)
    missed = []
    for name, a in (("out", _np(got["out"])), ("row_max", mx), ("row_sum", _np(got["row_sum"])), ("dX_row", _np(got["dX_row"])),
                    ("dX_col", dxc), ("dattn", _np(got["dattn"])[None])):
        err = pc.error_of(g0, name, a.astype(np.float64), ref64[name])
        print(f"rect boundary gatv2 {case} col_shift {name}: measured {err:.3e}, bound {bounds[name]:.3e}")
        if not err <= bounds[name]:
            missed.append((name, err, bounds[name]))
    assert not missed, (case, missed)


# one as-built case (wave form, unit val) and one transposed case (lane-group form, weighted val) per width
SHIFTED_CASES = [c for f, h in pc.WIDTHS for c in ((False, False, f, h, True), (True, True, f, h, False))]


@pytest.mark.parametrize("case", SHIFTED_CASES, ids=str)
@pytest.mark.parametrize("pair", ["bias", "edge"])
def test_bias_edge_boundary_degrees_shifted(pair, case):
    """The bias pair on gt_bias_cases' inputs and the edge pair on gt_edge_cases.boundary_inputs, col_shift = m: every
    output within that module's own bounds (dK: its DK_FACTOR included); the per-edge gradients dbias [h, nnz] / dE
    [nnz, h, f] keep their CSR order, so they are compared as they are, grouped by CSR row."""
    import gt_bias_cases as bc
    import gt_edge_cases as ec
    mod, extra, gextra = (bc, "bias", "dbias") if pair == "bias" else (ec, "E", "dE")
    assert case in pc.case_ids("gt")
    g0 = pc.graph(case[0], case[1])
    x, ref64, bounds = mod.boundary_references(case)
    m0 = g0["m"]
    g = rc.embed_graph(g0["row_ptr"], g0["col_ind"], m0, 0, 0)
    assert np.array_equal(g["rows"], g0["rows"]) and g["n_cols"] == 2 * m0 and int(g["col_ind"].min()) >= m0
    y = {"val": x["val"], extra: x[extra], "Q": x["Q"], "dO": x["dO"], "K": rc.embed_cols(x["K"], m0, 0),
         "V": rc.embed_cols(x["V"], m0, 0)}
    got = _run(pair, _graph_on_device(g), {k: _dev(v) for k, v in y.items()})
    assert torch.equal(got["inference"], got["out"])
    back = {k: _np(got[k]) for k in ("out", "row_max", "row_sum", "dQ", gextra)}
    for name in ("dK", "dV"):
        back[name], clean = rc.restrict_cols(_np(got[name]), m0, m0)
        assert clean, name
    er = np.diff(g0["row_ptr"]) == 0
    assert (back["row_max"][er] == np.float32(rc.SENTINEL_MAX)).all() and (back["out"][er] == 0).all()
    missed = []
    for name in mod.OUTPUTS:
        a = back[name].astype(np.float64)
        assert np.isfinite(a).all(), name
        err = mod.error_of(g0, name, a, ref64[name])
        print(f"rect boundary {pair} {case} col_shift {name}: measured {err:.3e}, bound {bounds[name]:.3e}")
        if not err <= bounds[name]:
            missed.append((name, err, bounds[name]))
    assert not missed, (pair, case, missed)


# ---- 4. preprocessing -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transport", TRANSPORTS)
@pytest.mark.parametrize("idtype", [torch.int32, torch.int64])
def test_rect_preprocessing(idtype, transport):
    """coo_to_hyper with a (rows, cols) pair against the CPU restatement (preprocess_block on the CPU) and numpy's stable sorts, bit-exact, on the tall, wide and block edge
    lists and on one with out-of-range ids (clamped per side); the square call gives what it gave."""
    import dfgnn_preprocess
    from DFGNN.layers import preprocess_block
    from DFGNN.utils.graph import Block
    names = ("row_ptr", "col_ind", "rows", None, "col_ptr", "row_ind", "val_idx")
    with _Transport(transport):
        for kind in ("tall", "wide", "block", "clamped", "square"):
            g = rc.graph("tall" if kind in ("clamped", "square") else kind)
            perm = np.random.default_rng(4).permutation(g["nnz"])
            src, dst = g["src"][perm].copy(), g["dst"][perm].copy()
            shape = (g["m"], g["n_cols"])
            want_src, want_dst = src, dst
            if kind == "clamped":
                src[:4], dst[:4] = (-3, 600, 10 ** 6, 7), (40, -1, 39, 10 ** 6)
                want_src, want_dst = np.clip(src, 0, 599), np.clip(dst, 0, 39)
            if kind == "square":
                shape = (600, 600)
            want = rc._finish(want_src, want_dst, *shape)
            if kind != "square":                # ... and the CPU restatement itself (DFGNN/utils/sparse.py through preprocess_block)
                cpu = preprocess_block(Block(want_src, want_dst, *shape))
                for name, t in zip(("rows", "row_ptr", "col_ind", None, "col_ptr", "row_ind", "val_idx"), cpu[1:8]):
                    if name is not None:
                        assert np.array_equal(_np(t), want[name]), (kind, name, "cpu")
            got = dfgnn_preprocess.coo_to_hyper(_dev(src, idtype), _dev(dst, idtype), 600 if kind == "square" else shape)
            torch.cuda.synchronize()
            for name, t in zip(names, got):
                if name is not None:
                    assert t.dtype == torch.int32 and np.array_equal(_np(t), want[name]), (kind, name)
            assert np.array_equal(want_src[_np(got[3])], want["rows"])          # edge_order: COO position of each CSR slot


# ---- 5. autograd and layers -----------------------------------------------------------------------------------------------
def test_autograd_on_a_block():
    """GTConvFuse_rowstats / _bias / _edge and GATv2ConvFuse on `block`: the gradient of every input that requires one."""
    from DFGNN.operators.fused_gatconv import GATv2ConvFuse
    from DFGNN.operators.fused_gtconv import GTConvFuse_bias, GTConvFuse_edge, GTConvFuse_rowstats
    g = rc.graph("block")
    d = _graph_on_device(g)
    graph_args = (d["rows"], d["row_ptr"], d["col_ind"])
    csc = (d["col_ptr"], d["row_ind"], d["val_idx"])
    for pair in rc.PAIRS:
        xn = rc.inputs(pair, g, 2, 20, False)
        ref = rc.reference_on(pair, g, xn)
        x = {k: _dev(v) for k, v in xn.items()}
        leaves = {"rowstats": ("Q", "K", "V"), "bias": ("Q", "K", "V", "bias"), "edge": ("Q", "K", "V", "E"),
                  "gatv2": ("X_row", "X_col", "attn")}[pair]
        for k in leaves:
            x[k].requires_grad_(True)
        if pair == "gatv2":
            out = GATv2ConvFuse(x["attn"], d["row_ptr"], d["col_ind"], d["col_ptr"], d["row_ind"], rc.SLOPE, x["X_row"], x["X_col"])
        else:
            extra = () if pair == "rowstats" else (x["bias"],) if pair == "bias" else (x["E"],)
            fn = {"rowstats": GTConvFuse_rowstats, "bias": GTConvFuse_bias, "edge": GTConvFuse_edge}[pair]
            out = fn(*graph_args, x["val"], *csc, 1024, x["Q"], x["K"], x["V"], *extra)
        out.backward(x["dO"])
        torch.cuda.synchronize()
        _check(out, ref["out"], f"autograd {pair} out")
        for k in leaves:
            name = {"Q": "dQ", "K": "dK", "V": "dV", "bias": "dbias", "E": "dE", "X_row": "dX_row", "X_col": "dX_col",
                    "attn": "dattn"}[k]
            _check(x[k].grad, ref[name], f"autograd {pair} {name}")


def test_layers_with_a_pair_input():
    """Each layer on `block` with (h_cols, h_rows): [m, heads * dim]; the fused branch agrees with the non-fused one."""
    from DFGNN.layers import GATv2Conv_forward, SparseMHA_bias, SparseMHA_edge, SparseMHA_rowstats, preprocess_block
    from DFGNN.utils.graph import Block
    g = rc.graph("block")
    params = preprocess_block(Block(g["src"], g["dst"], g["m"], g["n_cols"]).to(DEV))
    assert np.array_equal(_np(params[2]), g["row_ptr"]) and np.array_equal(_np(params[5]), g["col_ptr"])
    torch.manual_seed(0)
    h_cols = torch.randn(g["n_cols"], 16, device=DEV)
    h_rows = h_cols[:g["m"]].contiguous()
    # (SparseMHA_rowstats' two branches lay the heads out differently and agree at one head, as SparseMHA_forward's)
    for heads, make in ((1, lambda: SparseMHA_rowstats(16, 24, 1)), (3, lambda: SparseMHA_bias(16, 24, 3)),
                        (3, lambda: SparseMHA_edge(16, 24, 3)), (3, lambda: GATv2Conv_forward(16, 8, 3))):
        layer = make().to(DEV).train()
        extra = ()
        if isinstance(layer, SparseMHA_bias):
            extra = (torch.randn(g["nnz"], heads, device=DEV),)
        if isinstance(layer, SparseMHA_edge):
            extra = (torch.randn(g["nnz"], 16, device=DEV),)
        fused = layer(params, (h_cols, h_rows), *extra, fuse=True)
        plain = layer(params, (h_cols, h_rows), *extra, fuse=False)
        assert fused.shape == (g["m"], 24)
        _check(fused, _np(plain), f"layer {type(layer).__name__} fused against non-fused")
        fused.sum().backward()                                      # the fused backward runs on the pair input
        torch.cuda.synchronize()
        assert all(p.grad is None or bool(torch.isfinite(p.grad).all()) for p in layer.parameters())


# ---- 6. rejections --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("transport", TRANSPORTS)
def test_square_only_operators_and_mismatches_raise(transport):
    """On `tall` (600 x 40: every column id is also a valid row id, and its average degree keeps the block plan away, so a
    check that did not fire could not send a kernel out of bounds): the square-only operators raise on Q and K / V of
    different extents; a col_ptr or statistics tensor of the wrong extent and K / V that disagree raise in both transports."""
    import fused_gatconv as gat
    import fused_gtconv as gt
    g = rc.graph("tall")
    assert g["n_cols"] <= g["m"] and rc.lane_form(g["m"], g["nnz"])
    d = _graph_on_device(g)
    rp, ci, rows, cp, ri, vi = (d[k] for k in ("row_ptr", "col_ind", "rows", "col_ptr", "row_ind", "val_idx"))
    x = {k: _dev(v) for k, v in rc.inputs("rowstats", g, 2, 20, True).items()}
    Q, K, V, val, dO = x["Q"], x["K"], x["V"], x["val"], x["dO"]
    m, n = g["m"], g["n_cols"]
    with _Transport(transport):
        with pytest.raises(RuntimeError):
            gt.gt_hyper_forward(rp, ci, rows, val, cp, ri, vi, 1024, Q, K, V)
        with pytest.raises(RuntimeError):
            gt.gt_hyper_forward_stats(rp, ci, Q, K, V)
        with pytest.raises(RuntimeError):
            gt.gt_tiling_inference(rp, ci, val, 128, Q, K, V)
        with pytest.raises(RuntimeError):
            gat.gat_forward(torch.randn(m, 2, device=DEV), torch.randn(n, 2, device=DEV), rp, ci, 0.2, Q, 0.0)
        out, mx, sm = gt.gt_forward_rowstats(rp, ci, val, Q, K, V)
        with pytest.raises(RuntimeError, match="col_ptr must have shape"):
            gt.gt_backward_rowstats(rp, ci, val, rp, ri, vi, Q, K, V, out, mx, sm, dO)                 # (m + 1,) for n_cols columns
        with pytest.raises(RuntimeError, match="row_max"):
            gt.gt_backward_rowstats(rp, ci, val, cp, ri, vi, Q, K, V, out, torch.zeros(n, 2, device=DEV), sm, dO)
        with pytest.raises(RuntimeError, match="V must have shape"):
            gt.gt_forward_rowstats(rp, ci, val, Q, K, V[:-1].contiguous())
        with pytest.raises(RuntimeError, match="the heads and features of Q"):
            gt.gt_forward_rowstats(rp, ci, val, Q, K[:, :1].contiguous(), V[:, :1].contiguous())
        xg = {k: _dev(v) for k, v in rc.inputs("gatv2", g, 2, 20, True).items()}
        o2, mx2, sm2 = gat.gatv2_forward(xg["attn"], rp, ci, rc.SLOPE, xg["X_row"], xg["X_col"])
        with pytest.raises(RuntimeError, match="col_ptr must have shape"):
            gat.gatv2_backward(rc.SLOPE, rp, ci, rp, ri, xg["attn"], xg["X_row"], xg["X_col"], o2, mx2, sm2, xg["dO"])
        torch.cuda.synchronize()


def test_c_abi_return_codes():
    """dfgnn_*_rect: BADARG for a negative extent and for nnz > 0 with n_cols == 0 or m == 0 (no launch: the pointers are never
    read); dfgnn_preprocess_ws_bytes_rect is the larger of the two square sizes."""
    import ctypes
    import dfgnn_native
    lib = dfgnn_native.lib()
    one = torch.zeros(64, device=DEV)
    p = one.data_ptr()
    assert lib.dfgnn_gt_fwd_rowstats_rect(4, -1, 0, 1, 4, p, p, None, p, p, p, p, p, p, None) == -1
    assert lib.dfgnn_gt_fwd_rowstats_rect(-1, 4, 0, 1, 4, p, p, None, p, p, p, p, p, p, None) == -1
    assert lib.dfgnn_gt_fwd_rowstats_rect(4, 0, 3, 1, 4, p, p, None, p, p, p, p, p, p, None) == -1
    assert lib.dfgnn_gatv2_fwd_rect(4, 0, 3, 1, 4, p, p, p, 0.2, p, p, p, p, p, None) == -1
    assert lib.dfgnn_gt_bwd_rowstats_rect(0, 4, 3, 1, 4, None, p, None, p, p, p, p, p, p, p, p, p, p, p, p, p, p, None) == -1  # an edge needs a row
    nbytes = ctypes.c_size_t(0)
    assert lib.dfgnn_preprocess_ws_bytes_rect(600, 40, 1800, ctypes.addressof(nbytes)) == 0
    assert nbytes.value == max(lib.dfgnn_preprocess_ws_bytes(600, 1800), lib.dfgnn_preprocess_ws_bytes(40, 1800)) > 0
    assert lib.dfgnn_preprocess_ws_bytes_rect(600, -1, 1800, ctypes.addressof(nbytes)) == -1
    assert lib.dfgnn_gt_fwd_rowstats_rect(4, 4, 0, 1, 2000, p, p, None, p, p, p, p, p, p, None) == -2     # f beyond the range
