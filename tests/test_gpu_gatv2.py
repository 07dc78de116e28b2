"""GPU tests of the fused GATv2 convolution (include/dfgnn.h: dfgnn_gatv2_fwd / dfgnn_gatv2_bwd; csrc/gatv2_train.hip):
inference, the training pair that saves two floats per (row, head), the autograd Function and the layers.  The reference
is a float64 torch formulation on the CPU (index ops over the edge list, gradients from torch.autograd.grad); the bar is
the project's own, as tests/test_gpu_rowstats_pair.py::_check: max abs error < 1e-3 * max(1, max |ref|), all finite."""
import functools

import numpy as np
import pytest
import torch

from conftest import csc_of, random_graph

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-3
SLOPE = 0.2


def _np(t):
    return t.detach().cpu().numpy()


def _check(got, ref, what):
    """The parity bar; prints the measured figure first (pytest -s / a failing run shows it)."""
    got = _np(got).astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    ref = _np(ref).astype(np.float64) if isinstance(ref, torch.Tensor) else np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    bound = BAR * max(1.0, float(np.abs(ref).max()) if ref.size else 0.0)
    print(f"gatv2 {what}: max abs err {err:.3e} (bound {bound:.3e})")
    assert np.isfinite(got).all(), what
    assert err < bound, (what, err, bound)
    return err


# ---- graphs ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _graph(kind):
    """lane: the lane-group form (nnz < 8 m) with a row above 64 edges (COOP), empty rows, empty columns, duplicates.
    wave: the wave form (nnz >= 8 m); its 200-edge row is three full 64-edge tiles and a partial one.
    saved: m h f < nnz, for the saved-state test."""
    rng = np.random.default_rng({"lane": 257, "wave": 96, "saved": 64}[kind])
    if kind == "lane":
        m = 257
        indptr, indices, rows = random_graph(rng, m, 3, empty_frac=0.2, dup_frac=0.1, max_deg=70)
    elif kind == "wave":
        m = 96
        indptr, indices, rows = random_graph(rng, m, 40, max_deg=200)
    else:
        m = 64
        indptr, indices, rows = random_graph(rng, m, 60)
    nnz = len(indices)
    deg, indeg = np.diff(indptr), np.bincount(indices, minlength=m)
    if kind == "lane":
        assert nnz < 8 * m and deg.max() > 64 and (deg == 0).any() and (indeg == 0).any()
    elif kind == "wave":
        assert nnz >= 8 * m and deg.max() == 200
    col_ptr, row_ind, _ = csc_of(indptr, indices, rows, m)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v)).to(torch.int32).to(DEV)
           for k, v in (("row_ptr", indptr), ("col_ind", indices), ("col_ptr", col_ptr), ("row_ind", row_ind))}
    return dict(m=m, nnz=nnz, rows=torch.from_numpy(rows.astype(np.int64)), cols=torch.from_numpy(indices.astype(np.int64)),
                empty_rows=deg == 0, empty_cols=indeg == 0, **dev)


# ---- float64 reference ----------------------------------------------------------------------------------------------------
def _ref_conv(rows, cols, n, attn, x_row, x_col):
    """-> out, row_max, row_sum in the dtype of the inputs; differentiable."""
    z = x_row[rows] + x_col[cols]
    s = (torch.nn.functional.leaky_relu(z, SLOPE) * attn).sum(-1)                         # [E, h]
    mx = torch.full((n, s.size(1)), float("-inf"), dtype=s.dtype)
    mx = mx.scatter_reduce(0, rows[:, None].expand_as(s), s.detach(), reduce="amax", include_self=True)
    p = torch.exp(s - mx[rows])
    den = torch.zeros_like(mx).index_add_(0, rows, p)
    out = torch.zeros_like(x_row).index_add_(0, rows, x_col[cols] * (p / den[rows])[:, :, None])
    return out, mx, den


def _inputs(kind, h, f, seed=0):
    g = _graph(kind)
    gen = torch.Generator().manual_seed(1000 * h + f + seed)
    attn = torch.randn(h, f, generator=gen) * f ** -0.5
    x_row, x_col, dO = (torch.randn(g["m"], h, f, generator=gen) for _ in range(3))
    return g, attn, x_row, x_col, dO


@functools.lru_cache(maxsize=None)
def _reference(kind, h, f, shared=False):
    """float64 CPU: out, row_max, row_sum and torch.autograd.grad's (dX_row, dX_col, dattn) -- for `shared` (one tensor as
    both operands) (dX, dattn).  Computed once per case and shared by the tests; nobody writes to it."""
    g, attn, x_row, x_col, dO = _inputs(kind, h, f)
    a = attn.double().requires_grad_(True)
    xr = x_row.double().requires_grad_(True)
    xc = xr if shared else x_col.double().requires_grad_(True)
    out, mx, den = _ref_conv(g["rows"], g["cols"], g["m"], a, xr, xc)
    grads = torch.autograd.grad(out, (xr, a) if shared else (xr, xc, a), dO.double())
    return dict(out=out.detach(), row_max=mx, row_sum=den.detach(), grads=[t.detach() for t in grads])


def _pair(g, attn, x_row, x_col, dO):
    import fused_gatconv as gat
    out, mx, sm = gat.gatv2_forward(attn, g["row_ptr"], g["col_ind"], SLOPE, x_row, x_col)
    dxr, dxc, da = gat.gatv2_backward(SLOPE, g["row_ptr"], g["col_ind"], g["col_ptr"], g["row_ind"], attn, x_row, x_col, out, mx,
                                      sm, dO)
    torch.cuda.synchronize()
    return out, mx, sm, dxr, dxc, da


CASES = [("lane", 2, 20), ("lane", 3, 7), ("lane", 1, 128), ("wave", 1, 128), ("wave", 8, 16), ("wave", 2, 7)]


@pytest.mark.parametrize("kind,h,f", CASES)
def test_pair_against_reference(kind, h, f):
    """Both forms, float4 and scalar lane layouts: out, the row statistics, dX_row, dX_col, dattn at the bar; exact zeros and
    sentinels where a row / column has no edge; inference equals the training forward's out bit for bit."""
    import fused_gatconv as gat
    g, attn, x_row, x_col, dO = (t.to(DEV) if isinstance(t, torch.Tensor) else t for t in _inputs(kind, h, f))
    ref = _reference(kind, h, f)
    out, mx, sm, dxr, dxc, da = _pair(g, attn, x_row, x_col, dO)
    what = f"{kind} h{h} f{f}"
    er, ec = g["empty_rows"], g["empty_cols"]
    _check(out, ref["out"], f"{what} out")
    _check(_np(mx)[~er], _np(ref["row_max"])[~er], f"{what} row_max")
    _check(sm, ref["row_sum"], f"{what} row_sum")
    for got, want, name in zip((dxr, dxc, da), ref["grads"], ("dX_row", "dX_col", "dattn")):
        _check(got, want, f"{what} {name}")
    assert (_np(out)[er] == 0).all() and (_np(dxr)[er] == 0).all() and (_np(dxc)[ec] == 0).all()
    assert (_np(mx)[er] == np.float32(-1e38)).all() and (_np(sm)[er] == 0).all()
    plain = gat.gatv2_inference(attn, g["row_ptr"], g["col_ind"], SLOPE, x_row, x_col)
    assert torch.equal(plain, out)


@pytest.mark.parametrize("kind,h,f", [("lane", 2, 20), ("wave", 8, 16)])
def test_shared_weights_and_determinism(kind, h, f):
    """X_row is X_col (one pointer for both operands) runs and matches: out, and dX_row + dX_col against the reference's
    single gradient.  Two backward calls on the same inputs agree bit for bit (no atomics)."""
    import fused_gatconv as gat
    g, attn, x, _, dO = (t.to(DEV) if isinstance(t, torch.Tensor) else t for t in _inputs(kind, h, f))
    ref = _reference(kind, h, f, shared=True)
    out, mx, sm, dxr, dxc, da = _pair(g, attn, x, x, dO)
    assert torch.equal(out, gat.gatv2_inference(attn, g["row_ptr"], g["col_ind"], SLOPE, x, x))
    _check(out, ref["out"], f"shared {kind} out")
    _check(dxr + dxc, ref["grads"][0], f"shared {kind} dX")
    _check(da, ref["grads"][1], f"shared {kind} dattn")
    again = gat.gatv2_backward(SLOPE, g["row_ptr"], g["col_ind"], g["col_ptr"], g["row_ind"], attn, x, x, out, mx, sm, dO)
    for a, b in zip((dxr, dxc, da), again):
        assert torch.equal(a, b)


def test_autograd_function():
    """GATv2ConvFuse + .backward() on the lane-group graph at (2, 20): the reference's gradients for attn, X_row, X_col; one
    leaf passed as both operands receives the reference's single summed gradient."""
    from DFGNN.operators.fused_gatconv import GATv2ConvFuse
    g, attn, x_row, x_col, dO = (t.to(DEV) if isinstance(t, torch.Tensor) else t for t in _inputs("lane", 2, 20))
    graph = (g["row_ptr"], g["col_ind"], g["col_ptr"], g["row_ind"])
    a, xr, xc = (t.clone().requires_grad_(True) for t in (attn, x_row, x_col))
    out = GATv2ConvFuse(a, *graph, SLOPE, xr, xc)
    out.backward(dO)
    ref = _reference("lane", 2, 20)
    _check(out, ref["out"], "autograd out")
    for got, want, name in zip((xr.grad, xc.grad, a.grad), ref["grads"], ("X_row.grad", "X_col.grad", "attn.grad")):
        _check(got, want, f"autograd {name}")
    a, x = (t.clone().requires_grad_(True) for t in (attn, x_row))
    GATv2ConvFuse(a, *graph, SLOPE, x, x).backward(dO)
    ref = _reference("lane", 2, 20, shared=True)
    _check(x.grad, ref["grads"][0], "autograd shared X.grad")
    _check(a.grad, ref["grads"][1], "autograd shared attn.grad")


def test_saved_state_has_nothing_per_edge():
    """m = 64, average degree 60, h = 1, f = 8: m h f = 512 < nnz, so any floating-point tensor of nnz elements or more among
    what autograd keeps between forward and backward would be per-edge state."""
    from DFGNN.operators.fused_gatconv import GATv2ConvFuse
    g, attn, x_row, x_col, dO = (t.to(DEV) if isinstance(t, torch.Tensor) else t for t in _inputs("saved", 1, 8))
    assert g["m"] * 1 * 8 < g["nnz"]
    saved = []

    def pack(t):
        saved.append(t)
        return t

    a, xr, xc = (t.clone().requires_grad_(True) for t in (attn, x_row, x_col))
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = GATv2ConvFuse(a, g["row_ptr"], g["col_ind"], g["col_ptr"], g["row_ind"], SLOPE, xr, xc)
    floating = [t for t in saved if t.is_floating_point()]
    assert len(floating) >= 5                                         # attn, X_row, X_col, out and the statistics
    assert all(t.numel() < g["nnz"] for t in floating), [tuple(t.shape) for t in floating]
    out.backward(dO)
    _check(xr.grad, _reference("saved", 1, 8)["grads"][0], "saved-state case X_row.grad")


@pytest.mark.parametrize("m", [0, 5])
def test_empty_problems(m):
    """m == 0, and m == 5 without an edge: zero outputs, sentinels, a zero dattn, no error."""
    import fused_gatconv as gat
    h, f = 2, 12
    i32 = dict(dtype=torch.int32, device=DEV)
    row_ptr, col_ind = torch.zeros(m + 1, **i32), torch.zeros(0, **i32)
    attn, x, dO = torch.randn(h, f, device=DEV), torch.randn(m, h, f, device=DEV), torch.randn(m, h, f, device=DEV)
    out, mx, sm = gat.gatv2_forward(attn, row_ptr, col_ind, SLOPE, x, x)
    dxr, dxc, da = gat.gatv2_backward(SLOPE, row_ptr, col_ind, row_ptr, col_ind, attn, x, x, out, mx, sm, dO)
    torch.cuda.synchronize()
    assert out.shape == dxr.shape == dxc.shape == (m, h, f) and mx.shape == sm.shape == (m, h) and da.shape == (h, f)
    assert gat.gatv2_inference(attn, row_ptr, col_ind, SLOPE, x, x).shape == (m, h, f)
    for t in (out, dxr, dxc, da, sm):
        assert (t == 0).all()
    assert (mx == -1e38).all()


def test_bindings_agree():
    """The torch C++ extension and the ctypes transport give bit-identical results and the same RuntimeError for a bad
    argument."""
    import dfgnn_native
    import fused_gatconv as gat
    assert dfgnn_native.ext() is not None and hasattr(dfgnn_native.ext(), "gatv2_bwd")
    cases = [[t.to(DEV) if isinstance(t, torch.Tensor) else t for t in _inputs(kind, h, f)] for kind, h, f in
             (("lane", 2, 20), ("wave", 8, 16))]

    def run():
        res = []
        for c in cases:
            res += list(_pair(*c))
        g, attn, x_row, x_col, _ = cases[0]
        try:
            gat.gatv2_forward(attn, g["row_ptr"].long(), g["col_ind"], SLOPE, x_row, x_col)
            err = None
        except RuntimeError as e:
            err = str(e)
        try:
            gat.gatv2_inference(attn[:, :-1].contiguous(), g["row_ptr"], g["col_ind"], SLOPE, x_row, x_col)
            err2 = None
        except RuntimeError as e:
            err2 = str(e)
        return res, err, err2

    via_ext, err_ext, shape_ext = run()
    saved = dfgnn_native._ext
    dfgnn_native._ext = None                      # force the ctypes path
    try:
        via_ctypes, err_ctypes, shape_ctypes = run()
    finally:
        dfgnn_native._ext = saved
    assert len(via_ext) == len(via_ctypes) == 12
    for a, b in zip(via_ext, via_ctypes):
        assert torch.equal(a, b)
    assert err_ext and err_ctypes and "int32" in err_ext and "int32" in err_ctypes
    assert shape_ext and shape_ctypes and "attn" in shape_ext and "attn" in shape_ctypes


# ---- layers ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _cora():
    from DFGNN.utils import synthetic as S
    return S.cora_like().to(DEV)


@pytest.mark.parametrize("heads", [1, 4])
def test_inference_layer(heads):
    """GATv2Conv_tiling on the cora-like graph: the fused operator against the layer's own torch branch."""
    from DFGNN.layers import GATv2Conv_tiling, preprocess_CSR
    from DFGNN.utils import preprocess_dglsp
    g = _cora()
    torch.manual_seed(2)
    layer = GATv2Conv_tiling(32, 16, heads).to(DEV).eval()
    feat = torch.randn(g.num_nodes(), 32, device=DEV)
    want, ms0 = layer(preprocess_dglsp(g), feat, fuse=False)
    got, ms1 = layer(preprocess_CSR(g), feat, fuse=True)
    assert got.shape == (g.num_nodes(), heads * 16) and ms0 > 0 and ms1 > 0
    _check(got, want, f"GATv2Conv_tiling heads {heads}")


@pytest.mark.parametrize("heads,share", [(1, False), (4, False), (2, True)])
def test_training_layer(heads, share):
    """GATv2Conv_forward in .train(): after out.sum().backward() the gradient of every parameter agrees between the fused
    branch and the torch branch."""
    from DFGNN.layers import GATv2Conv_forward, preprocess_Hyper_fw_bw
    g = _cora()
    torch.manual_seed(3)
    layer = GATv2Conv_forward(32, 16, heads, share_weights=share).to(DEV).train()
    feat = torch.randn(g.num_nodes(), 32, device=DEV)
    params = preprocess_Hyper_fw_bw(g)
    outs, grads = [], []
    for fuse in (False, True):
        layer.zero_grad()
        out = layer(params, feat, fuse=fuse)
        out.sum().backward()
        outs.append(out.detach())
        grads.append({n: p.grad.clone() for n, p in layer.named_parameters()})
    assert len(grads[0]) == (3 if share else 5)
    _check(outs[1], outs[0], f"GATv2Conv_forward heads {heads} out")
    for n in grads[0]:
        _check(grads[1][n], grads[0][n], f"GATv2Conv_forward heads {heads} d{n}")
