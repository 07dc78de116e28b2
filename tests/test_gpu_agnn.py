"""GPU tests of the fused AGNN / dot-product convolution with tied keys and values (include/dfgnn.h: dfgnn_agnn_fwd /
dfgnn_agnn_bwd; csrc/agnn_train.hip): inference, the training pair that saves two floats per (row, head), the autograd
Function and the layers, on square and rectangular graphs.  The reference is a float64 torch formulation on the CPU (index ops
over the edge list, F.normalize(eps=1e-12), gradients from torch.autograd.grad); the bar is tests/test_gpu_gatv2.py::_check:
max abs error < 1e-3 * max(1, max |ref|), all finite."""
import functools

import numpy as np
import pytest
import torch

from conftest import csc_of, random_graph

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-3
WIDTHS = [(2, 20), (3, 7), (1, 128), (8, 16)]            # (h, f): float4 / scalar lanes / float4 two chunks / many heads
MODES = [True, False]                                    # cosine (AGNN) / dot product


def _np(t):
    return t.detach().cpu().numpy()


def _check(got, ref, what):
    """The parity bar; prints the measured figure first (pytest -s / a failing run shows it)."""
    got = _np(got).astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    ref = _np(ref).astype(np.float64) if isinstance(ref, torch.Tensor) else np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    bound = BAR * max(1.0, float(np.abs(ref).max()) if ref.size else 0.0)
    print(f"agnn {what}: max abs err {err:.3e} (bound {bound:.3e})")
    assert np.isfinite(got).all(), what
    assert err < bound, (what, err, bound)
    return err


# ---- graphs ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _graph(kind):
    """lane: the lane-group form (nnz < 8 m) with a row above 64 edges (cooperative branch), empty rows, empty columns,
    duplicates.  wave: the wave form (nnz >= 8 m); its 200-edge row is three full 64-edge tiles and a partial one.
    rect: 96 rows x 257 columns -- a wave per row, a lane group per column."""
    rng = np.random.default_rng({"lane": 257, "wave": 96, "rect": 96257}[kind])
    if kind == "lane":
        m = n_cols = 257
        indptr, indices, rows = random_graph(rng, m, 3, empty_frac=0.2, dup_frac=0.1, max_deg=70)
    elif kind == "wave":
        m = n_cols = 96
        indptr, indices, rows = random_graph(rng, m, 40, max_deg=200)
    else:
        m, n_cols = 96, 257
        indptr, _, rows = random_graph(rng, m, 10, max_deg=70)
        indices = rng.integers(0, n_cols, len(rows)).astype(np.int32)
    nnz = len(indices)
    deg, indeg = np.diff(indptr), np.bincount(indices, minlength=n_cols)
    if kind == "lane":
        assert nnz < 8 * m and deg.max() > 64 and (deg == 0).any() and (indeg == 0).any()
        assert (np.diff(indices)[np.diff(rows) == 0] == 0).any()                          # a duplicate edge
    elif kind == "wave":
        assert nnz >= 8 * m and deg.max() == 200
    else:
        assert nnz >= 8 * m and nnz < 8 * n_cols and deg.max() == 70 and indices.max() >= m and (indeg == 0).any()
    col_ptr, row_ind, val_idx = csc_of(indptr, indices, rows, n_cols)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to(torch.int32).to(DEV)
           for k, v in (("row_ptr", indptr), ("col_ind", indices), ("col_ptr", col_ptr), ("row_ind", row_ind),
                        ("val_idx", val_idx))}
    return dict(m=m, n_cols=n_cols, nnz=nnz, rows=torch.from_numpy(rows.astype(np.int64)),
                cols=torch.from_numpy(indices.astype(np.int64)), deg=deg, indeg=indeg, empty_rows=deg == 0,
                empty_cols=indeg == 0, **dev)


# ---- float64 reference ----------------------------------------------------------------------------------------------------
from agnn_cases import ref_conv as _ref_conv  # noqa: E402  (shared with tests/test_gpu_guarded.py)


def _inputs(kind, h, f, cosine, zero=None):
    """beta in [0.5, 4.5) (times f^-1/2 in dot mode), features and dO ~ N(0, 1); zero = (row, column): that row of X_row
    and that row of X_col are zeros."""
    g = _graph(kind)
    gen = torch.Generator().manual_seed(1000 * h + f + (0 if cosine else 1))
    beta = (torch.rand(h, generator=gen) * 4 + 0.5) * (1.0 if cosine else f ** -0.5)
    x_row, x_col, dO = (torch.randn(n, h, f, generator=gen) for n in (g["m"], g["n_cols"], g["m"]))
    if zero is not None:
        x_row[zero[0]] = 0
        x_col[zero[1]] = 0
    return g, beta, x_row, x_col, dO


@functools.lru_cache(maxsize=None)
def _reference(kind, h, f, cosine, shared=False, zero=None):
    """float64 CPU: out, row_max, row_sum and torch.autograd.grad's (dX_row, dX_col, dbeta) -- for `shared` (one tensor as
    both operands) (dX, dbeta).  Computed once per case and shared by the tests; nobody writes to it."""
    g, beta, x_row, x_col, dO = _inputs(kind, h, f, cosine, zero)
    b = beta.double().requires_grad_(True)
    xr = x_row.double().requires_grad_(True)
    xc = xr if shared else x_col.double().requires_grad_(True)
    out, mx, den = _ref_conv(g["rows"], g["cols"], g["m"], b, xr, xc, cosine)
    grads = torch.autograd.grad(out, (xr, b) if shared else (xr, xc, b), dO.double())
    return dict(out=out.detach(), row_max=mx, row_sum=den.detach(), grads=[t.detach() for t in grads])


def _dev(items):
    return [t.to(DEV) if isinstance(t, torch.Tensor) else t for t in items]


def _pair(g, beta, x_row, x_col, dO, cosine, need_dbeta=True):
    import fused_gtconv as gt
    out, mx, sm = gt.agnn_forward(g["row_ptr"], g["col_ind"], beta, x_row, x_col, cosine)
    dxr, dxc, db = gt.agnn_backward(g["row_ptr"], g["col_ind"], g["col_ptr"], g["row_ind"], beta, x_row, x_col, out, mx, sm, dO,
                                    cosine, need_dbeta=need_dbeta)
    torch.cuda.synchronize()
    return out, mx, sm, dxr, dxc, db


@pytest.mark.parametrize("cosine", MODES)
@pytest.mark.parametrize("h,f", WIDTHS)
@pytest.mark.parametrize("kind", ["lane", "wave", "rect"])
def test_pair_against_reference(kind, h, f, cosine):
    """Every form, float4 and scalar lane layouts, both modes: out, the row statistics, dX_row, dX_col, dbeta at the bar; exact
    zeros and sentinels where a row / column has no edge; inference equals the training forward's out bit for bit."""
    import fused_gtconv as gt
    g, beta, x_row, x_col, dO = _dev(_inputs(kind, h, f, cosine))
    ref = _reference(kind, h, f, cosine)
    out, mx, sm, dxr, dxc, db = _pair(g, beta, x_row, x_col, dO, cosine)
    what = f"{kind} h{h} f{f} {'cos' if cosine else 'dot'}"
    er, ec = g["empty_rows"], g["empty_cols"]
    assert dxr.shape == x_row.shape and dxc.shape == x_col.shape and db.shape == beta.shape
    _check(out, ref["out"], f"{what} out")
    _check(_np(mx)[~er], _np(ref["row_max"])[~er], f"{what} row_max")
    _check(sm, ref["row_sum"], f"{what} row_sum")
    for got, want, name in zip((dxr, dxc, db), ref["grads"], ("dX_row", "dX_col", "dbeta")):
        _check(got, want, f"{what} {name}")
    assert (_np(out)[er] == 0).all() and (_np(dxr)[er] == 0).all() and (_np(dxc)[ec] == 0).all()
    assert (_np(mx)[er] == np.float32(-1e38)).all() and (_np(sm)[er] == 0).all()
    plain = gt.agnn_inference(g["row_ptr"], g["col_ind"], beta, x_row, x_col, cosine)
    assert torch.equal(plain, out)


@pytest.mark.parametrize("cosine", MODES)
@pytest.mark.parametrize("kind,h,f", [("lane", 2, 20), ("wave", 8, 16)])
def test_shared_operand_and_determinism(kind, h, f, cosine):
    """X_row is X_col (one pointer for both operands) runs and matches: out, and dX_row + dX_col against the reference's
    single gradient.  Two backward calls on the same inputs agree bit for bit (no atomics)."""
    import fused_gtconv as gt
    g, beta, x, _, dO = _dev(_inputs(kind, h, f, cosine))
    ref = _reference(kind, h, f, cosine, shared=True)
    out, mx, sm, dxr, dxc, db = _pair(g, beta, x, x, dO, cosine)
    assert torch.equal(out, gt.agnn_inference(g["row_ptr"], g["col_ind"], beta, x, x, cosine))
    _check(out, ref["out"], f"shared {kind} out")
    _check(dxr + dxc, ref["grads"][0], f"shared {kind} dX")
    _check(db, ref["grads"][1], f"shared {kind} dbeta")
    again = gt.agnn_backward(g["row_ptr"], g["col_ind"], g["col_ptr"], g["row_ind"], beta, x, x, out, mx, sm, dO, cosine)
    for a, b in zip((dxr, dxc, db), again):
        assert torch.equal(a, b)


def _raw(g, beta, x_row, x_col, dO, cosine, rect, want_dbeta=True):
    """The C entry points through the ctypes transport: the square ones, or the *_rect ones with n_cols = m -> every output,
    the rows' shares of dbeta included."""
    from _binding_util import call
    m, nnz, (h, f) = g["m"], g["nnz"], x_row.shape[1:]
    ext = (m, m) if rect else (m,)
    sfx = "_rect" if rect else ""
    e = lambda *s: torch.empty(s, dtype=torch.float32, device=DEV)  # noqa: E731
    out, mx, sm, delta, dbr = e(m, h, f), e(m, h), e(m, h), e(m, h), e(m, h)
    dxr, dxc = torch.empty_like(x_row), torch.empty_like(x_col)
    call("dfgnn_agnn_fwd" + sfx, "agnn_forward", x_row.device, *ext, nnz, h, f, g["row_ptr"], g["col_ind"], beta, int(cosine),
         x_row, x_col, mx, sm, out)
    call("dfgnn_agnn_bwd" + sfx, "agnn_backward", x_row.device, *ext, nnz, h, f, g["row_ptr"], g["col_ind"], g["col_ptr"],
         g["row_ind"], beta, int(cosine), x_row, x_col, out, mx, sm, dO, delta, dxr, dxc, dbr if want_dbeta else None)
    torch.cuda.synchronize()
    return [out, mx, sm, delta, dxr, dxc] + ([dbr] if want_dbeta else [])


@pytest.mark.parametrize("cosine", MODES)
@pytest.mark.parametrize("kind,h,f", [("lane", 3, 7), ("wave", 1, 128)])
def test_square_entry_is_rect_entry_and_bindings_agree(kind, h, f, cosine):
    """The square entry and the *_rect entry with n_cols = m give the same bits on every output; so does the torch C++
    extension, whose dbeta is the column sum of the rows' shares.  Without dbeta_rows everything else is bit-identical."""
    import dfgnn_native
    args = _dev(_inputs(kind, h, f, cosine))
    square, rect = _raw(*args, cosine, rect=False), _raw(*args, cosine, rect=True)
    assert len(square) == len(rect) == 7
    for a, b in zip(square, rect):
        assert torch.equal(a, b)
    assert dfgnn_native.ext() is not None and hasattr(dfgnn_native.ext(), "agnn_bwd")
    out, mx, sm, dxr, dxc, db = _pair(*args, cosine)
    for a, b in zip((out, mx, sm, dxr, dxc, db), square[:3] + square[4:6] + [square[6].sum(0)]):
        assert torch.equal(a, b)
    without = _raw(*args, cosine, rect=False, want_dbeta=False)
    for a, b in zip(without, square[:6]):
        assert torch.equal(a, b)
    nodb = _pair(*args, cosine, need_dbeta=False)
    assert nodb[5] is None and all(torch.equal(a, b) for a, b in zip(nodb[:5], (out, mx, sm, dxr, dxc)))


@pytest.mark.parametrize("kind,h,f", [("lane", 2, 20), ("wave", 1, 128), ("rect", 8, 16)])
def test_dot_mode_against_rowstats_pair(kind, h, f):
    """Dot mode is the GT row-statistics pair on (beta X_row, X_col, X_col): out, dX_row = beta dQ, dX_col = dK + dV."""
    import fused_gtconv as gt
    g, beta, x_row, x_col, dO = _dev(_inputs(kind, h, f, False))
    out, _, _, dxr, dxc, _ = _pair(g, beta, x_row, x_col, dO, False)
    q = (x_row * beta[None, :, None]).contiguous()
    o2, mx2, sm2 = gt.gt_forward_rowstats(g["row_ptr"], g["col_ind"], None, q, x_col, x_col)
    dq, dk, dv = gt.gt_backward_rowstats(g["row_ptr"], g["col_ind"], None, g["col_ptr"], g["row_ind"], g["val_idx"], q, x_col,
                                         x_col, o2, mx2, sm2, dO)
    _check(out, o2, f"dot vs rowstats {kind} out")
    _check(dxr, dq * beta[None, :, None], f"dot vs rowstats {kind} dX_row")
    _check(dxc, dk + dv, f"dot vs rowstats {kind} dX_col")


@pytest.mark.parametrize("cosine", MODES)
def test_autograd_function(cosine):
    """AGNNConvFuse under torch.autograd.grad gives the raw pair's bits for beta, X_row, X_col; a beta that needs no gradient
    gets none; one leaf passed as both operands receives the reference's single summed gradient."""
    from DFGNN.operators.fused_gtconv import AGNNConvFuse
    g, beta, x_row, x_col, dO = _dev(_inputs("lane", 2, 20, cosine))
    graph = (g["row_ptr"], g["col_ind"], g["col_ptr"], g["row_ind"])
    out0, _, _, dxr, dxc, db = _pair(g, beta, x_row, x_col, dO, cosine)
    b, xr, xc = (t.clone().requires_grad_(True) for t in (beta, x_row, x_col))
    out = AGNNConvFuse(*graph, b, xr, xc, cosine)
    grads = torch.autograd.grad(out, (xr, xc, b), dO)
    for a, want in zip((out,) + grads, (out0, dxr, dxc, db)):
        assert torch.equal(a, want)
    xr, xc = (t.clone().requires_grad_(True) for t in (x_row, x_col))
    grads = torch.autograd.grad(AGNNConvFuse(*graph, beta, xr, xc, cosine), (xr, xc), dO)
    assert torch.equal(grads[0], dxr) and torch.equal(grads[1], dxc)
    b, x = (t.clone().requires_grad_(True) for t in (beta, x_row))
    AGNNConvFuse(*graph, b, x, x, cosine).backward(dO)
    ref = _reference("lane", 2, 20, cosine, shared=True)
    _check(x.grad, ref["grads"][0], "autograd shared X.grad")
    _check(b.grad, ref["grads"][1], "autograd shared beta.grad")


def test_zero_feature_row():
    """Cosine mode, one row of zeros on each side (norm 0: F.normalize's eps decides).  The forward is finite and at the bar
    everywhere.  The gradient of a zero row is of order beta / 1e-12 by definition and only has to be finite; the backward
    is compared on the rows that are neither a zero row nor adjacent to one -- a condition, checked to leave over 90 % of
    the rows, not a tolerance."""
    g = _graph("lane")
    m, rows, cols = g["m"], g["rows"].numpy(), g["cols"].numpy()
    zr = int(np.nonzero(g["deg"] == 3)[0][0])                      # the zero row of X_row: a row with three edges
    zc = int(np.nonzero(g["indeg"] == 3)[0][0])                    # the zero row of X_col: a column with three entries
    skip_rows = np.zeros(m, dtype=bool)
    skip_rows[zr] = True
    skip_rows[rows[cols == zc]] = True                             # rows with an edge into the zero column
    skip_cols = np.zeros(m, dtype=bool)
    skip_cols[zc] = True
    skip_cols[cols[rows == zr]] = True                             # columns the zero row has an edge to
    assert skip_rows.sum() < 0.1 * m and skip_cols.sum() < 0.1 * m
    h, f = 2, 20
    _, beta, x_row, x_col, dO = _dev(_inputs("lane", h, f, True, zero=(zr, zc)))
    ref = _reference("lane", h, f, True, zero=(zr, zc))
    out, mx, sm, dxr, dxc, db = _pair(g, beta, x_row, x_col, dO, True)
    _check(out, ref["out"], "zero row out")
    _check(sm, ref["row_sum"], "zero row row_sum")
    for t in (dxr, dxc, db):
        assert torch.isfinite(t).all()
    _check(_np(dxr)[~skip_rows], _np(ref["grads"][0])[~skip_rows], "zero row dX_row (other rows)")
    _check(_np(dxc)[~skip_cols], _np(ref["grads"][1])[~skip_cols], "zero row dX_col (other rows)")
    print(f"zero row: |dX_row[zero row]| max {float(dxr[zr].abs().max()):.3e}, |dX_col[zero row]| max "
          f"{float(dxc[zc].abs().max()):.3e}")


@pytest.mark.parametrize("m", [0, 5])
def test_empty_problems(m):
    """m == 0, and m == 5 without an edge: zero outputs, sentinels, a zero dbeta, no error."""
    import fused_gtconv as gt
    h, f = 2, 12
    i32 = dict(dtype=torch.int32, device=DEV)
    row_ptr, col_ind = torch.zeros(m + 1, **i32), torch.zeros(0, **i32)
    beta, x, dO = torch.ones(h, device=DEV), torch.randn(m, h, f, device=DEV), torch.randn(m, h, f, device=DEV)
    out, mx, sm = gt.agnn_forward(row_ptr, col_ind, beta, x, x)
    dxr, dxc, db = gt.agnn_backward(row_ptr, col_ind, row_ptr, col_ind, beta, x, x, out, mx, sm, dO)
    torch.cuda.synchronize()
    assert out.shape == dxr.shape == dxc.shape == (m, h, f) and mx.shape == sm.shape == (m, h) and db.shape == (h,)
    for t in (out, dxr, dxc, db, sm):
        assert (t == 0).all()
    assert (mx == -1e38).all()


# ---- layers ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _layer_graph(name):
    from DFGNN.utils import synthetic as S
    return (S.cora_like() if name == "cora" else S.pattern_like(batch_size=16, seed=3)).to(DEV)


def _fuse_against_nofuse(layer, params, feat, n_out, what, n_params):
    """out and the gradient of every parameter, fused branch against the layer's own torch branch, for a random dO."""
    gen = torch.Generator().manual_seed(11)
    dO = torch.randn(n_out, layer.num_heads * layer.out_size, generator=gen).to(DEV)
    outs, grads = [], []
    for fuse in (False, True):
        layer.zero_grad()
        out = layer(params, feat, fuse=fuse)
        (out * dO).sum().backward()
        outs.append(out.detach())
        grads.append({n: p.grad.clone() for n, p in layer.named_parameters()})
    assert sorted(grads[0]) == sorted(n_params)
    err = float((outs[1] - outs[0]).abs().max())
    print(f"{what} out: max abs diff {err:.3e}")
    assert torch.allclose(outs[1], outs[0], atol=1e-4, rtol=1e-3), (what, err)
    for n in grads[0]:
        err = float((grads[1][n] - grads[0][n]).abs().max())
        print(f"{what} d{n}: max abs diff {err:.3e} (max |ref| {float(grads[0][n].abs().max()):.3e})")
        assert torch.allclose(grads[1][n], grads[0][n], atol=1e-4, rtol=1e-3), (what, n, err)


@pytest.mark.parametrize("name,heads", [("cora", 1), ("cora", 4), ("pattern", 2)])
def test_agnn_layer(name, heads):
    """AGNNConv_beta in .train(): fuse=True against fuse=False on the output and on the gradients of proj and beta."""
    from DFGNN.layers import AGNNConv_beta, preprocess_Hyper_fw_bw
    g = _layer_graph(name)
    torch.manual_seed(3)
    layer = AGNNConv_beta(32, 16, heads).to(DEV).train()
    with torch.no_grad():
        layer.beta.copy_(torch.rand(heads) * 4 + 0.5)
    feat = torch.randn(g.num_nodes(), 32, device=DEV)
    _fuse_against_nofuse(layer, preprocess_Hyper_fw_bw(g), feat, g.num_nodes(), f"AGNNConv_beta {name} heads {heads}",
                         ("beta", "proj.bias", "proj.weight"))


@pytest.mark.parametrize("name,heads", [("cora", 1), ("pattern", 4)])
def test_dotgat_layer(name, heads):
    """DOTGATConv_forward in .train(): fuse=True against fuse=False (DotGatConv) on the output and the gradient of fc."""
    from DFGNN.layers import DOTGATConv_forward, preprocess_Hyper_fw_bw
    g = _layer_graph(name)
    torch.manual_seed(4)
    layer = DOTGATConv_forward(32, 16, heads).to(DEV).train()
    feat = torch.randn(g.num_nodes(), 32, device=DEV)
    _fuse_against_nofuse(layer, (g,) + tuple(preprocess_Hyper_fw_bw(g)), feat, g.num_nodes(),
                         f"DOTGATConv_forward {name} heads {heads}", ("conv_nofuse.fc.weight",))


def test_agnn_layer_rectangular():
    """AGNNConv_beta on the 96 x 257 graph through preprocess_block, feat = (h_cols, h_rows)."""
    from DFGNN.layers import AGNNConv_beta, preprocess_block
    from DFGNN.utils.graph import Block
    g = _graph("rect")
    params = preprocess_block(Block(g["rows"], g["cols"], g["m"], g["n_cols"]).to(DEV))
    torch.manual_seed(5)
    layer = AGNNConv_beta(24, 20, 2).to(DEV).train()
    with torch.no_grad():
        layer.beta.copy_(torch.rand(2) * 4 + 0.5)
    feat = (torch.randn(g["n_cols"], 24, device=DEV), torch.randn(g["m"], 24, device=DEV))
    _fuse_against_nofuse(layer, params, feat, g["m"], "AGNNConv_beta rect", ("beta", "proj.bias", "proj.weight"))
