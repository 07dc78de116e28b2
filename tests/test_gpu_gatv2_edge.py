"""GPU tests of the fused GATv2 convolution with per-edge feature vectors inside the LeakyReLU (include/dfgnn.h:
dfgnn_gatv2_fwd_edge / dfgnn_gatv2_bwd_edge and their *_rect forms; csrc/gatv2_edge_train.hip): inference, the training pair,
the autograd Function and the layers.  The reference is a float64 torch formulation on the CPU (index ops over the edge
list, gradients from torch.autograd.grad); the bar is the project's own, as tests/test_gpu_gatv2.py::_check: max abs error
< 1e-3 * max(1, max |ref|), all finite.  The graphs are the small ones of tests/test_gpu_gatv2.py, rebuilt here with
val_idx.  Where the arithmetic allows it the checks are exact (torch.equal): E = 0 against the plain GATv2 pair, and the
boundary-degree cases of tests/parity_cases.py with X_row moved into E."""
import functools

import numpy as np
import pytest
import torch

import parity_cases as pc
import rect_cases as rc
from conftest import csc_of, random_graph

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-3
SLOPE = 0.2


def _np(t):
    return t.detach().cpu().numpy()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _check(got, ref, what):
    """The parity bar; prints the measured figure first (pytest -s / a failing run shows it)."""
    got = _np(got).astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    ref = _np(ref).astype(np.float64) if isinstance(ref, torch.Tensor) else np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    bound = BAR * max(1.0, float(np.abs(ref).max()) if ref.size else 0.0)
    print(f"gatv2_edge {what}: max abs err {err:.3e} (bound {bound:.3e})")
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
        assert any(len(set(indices[indptr[i]:indptr[i + 1]])) < deg[i] for i in range(m))      # duplicates
    elif kind == "wave":
        assert nnz >= 8 * m and deg.max() == 200
    col_ptr, row_ind, val_idx = csc_of(indptr, indices, rows, m)
    assert not np.array_equal(val_idx, np.arange(nnz))                 # (the CSC order is not the CSR order)
    dev = {k: _dev(v, torch.int32) for k, v in (("row_ptr", indptr), ("col_ind", indices), ("col_ptr", col_ptr),
                                                ("row_ind", row_ind), ("val_idx", val_idx))}
    return dict(m=m, n_cols=m, nnz=nnz, rows=torch.from_numpy(rows.astype(np.int64)),
                cols=torch.from_numpy(indices.astype(np.int64)), empty_rows=deg == 0, empty_cols=indeg == 0, **dev)


# ---- float64 reference ----------------------------------------------------------------------------------------------------
from gatv2_edge_cases import ref_all as _ref_all, ref_conv as _ref_conv  # noqa: E402, F401  (shared with tests/test_gpu_guarded.py)


def _inputs(kind, h, f, seed=0):
    """-> g, attn, x_row, x_col, E ~ N(0, 1), dO on the CPU."""
    g = _graph(kind)
    gen = torch.Generator().manual_seed(1000 * h + f + seed)
    attn = torch.randn(h, f, generator=gen) * f ** -0.5
    x_row, x_col, dO = (torch.randn(g["m"], h, f, generator=gen) for _ in range(3))
    E = torch.randn(g["nnz"], h, f, generator=gen)
    return g, attn, x_row, x_col, E, dO


def _on_device(case):
    return [t.to(DEV) if isinstance(t, torch.Tensor) else t for t in case]


@functools.lru_cache(maxsize=None)
def _reference(kind, h, f, shared=False, zero_e=False):
    """Computed once per case and shared by the tests; nobody writes to it."""
    g, attn, x_row, x_col, E, dO = _inputs(kind, h, f)
    return _ref_all(g["rows"], g["cols"], g["m"], attn, x_row, x_col, torch.zeros_like(E) if zero_e else E, dO, shared)


def _pair(g, attn, x_row, x_col, E, dO, want_dE=True):
    import fused_gatconv as gat
    out, mx, sm = gat.gatv2_forward_edge(attn, g["row_ptr"], g["col_ind"], SLOPE, x_row, x_col, E)
    dxr, dxc, da, dE = gat.gatv2_backward_edge(SLOPE, g["row_ptr"], g["col_ind"], g["col_ptr"], g["row_ind"], g["val_idx"], attn,
                                               x_row, x_col, E, out, mx, sm, dO, want_dE=want_dE)
    torch.cuda.synchronize()
    return out, mx, sm, dxr, dxc, da, dE


def _plain_pair(g, attn, x_row, x_col, dO):
    import fused_gatconv as gat
    out, mx, sm = gat.gatv2_forward(attn, g["row_ptr"], g["col_ind"], SLOPE, x_row, x_col)
    dxr, dxc, da = gat.gatv2_backward(SLOPE, g["row_ptr"], g["col_ind"], g["col_ptr"], g["row_ind"], attn, x_row, x_col, out, mx,
                                      sm, dO)
    torch.cuda.synchronize()
    return out, mx, sm, dxr, dxc, da


# ---- 1. against the float64 reference -------------------------------------------------------------------------------------
CASES = [("lane", 2, 20), ("lane", 3, 7), ("lane", 1, 128), ("wave", 1, 128), ("wave", 8, 16), ("wave", 2, 7),
         ("lane", 1, 260)]                                             # (the last: f > 256, one edge in flight)


@pytest.mark.parametrize("kind,h,f", CASES)
def test_pair_against_reference(kind, h, f):
    """Both forms, float4 and scalar lane layouts, random E: out, the row statistics, dX_row, dX_col, dattn, dE at the bar;
    exact zeros and sentinels where a row / column has no edge; inference equals the training forward's out bit for bit.  A
    mis-indexed slot of E in any pass -- the val_idx gather of the CSC pass included -- moves a logit by O(1)."""
    import fused_gatconv as gat
    g, attn, x_row, x_col, E, dO = _on_device(_inputs(kind, h, f))
    ref = _reference(kind, h, f)
    out, mx, sm, dxr, dxc, da, dE = _pair(g, attn, x_row, x_col, E, dO)
    what = f"{kind} h{h} f{f}"
    er, ec = g["empty_rows"], g["empty_cols"]
    _check(out, ref["out"], f"{what} out")
    _check(_np(mx)[~er], _np(ref["row_max"])[~er], f"{what} row_max")
    _check(sm, ref["row_sum"], f"{what} row_sum")
    for got, want, name in zip((dxr, dxc, da, dE), ref["grads"], ("dX_row", "dX_col", "dattn", "dE")):
        _check(got, want, f"{what} {name}")
    assert (_np(out)[er] == 0).all() and (_np(dxr)[er] == 0).all() and (_np(dxc)[ec] == 0).all()
    assert (_np(mx)[er] == np.float32(-1e38)).all() and (_np(sm)[er] == 0).all()
    plain = gat.gatv2_inference_edge(attn, g["row_ptr"], g["col_ind"], SLOPE, x_row, x_col, E)
    assert torch.equal(plain, out)


# ---- 2. E = 0 is the plain pair -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f", [("lane", 2, 20), ("lane", 3, 7), ("wave", 1, 128), ("wave", 8, 16)])
def test_zero_edge_features_reproduce_the_plain_pair(kind, h, f):
    g, attn, x_row, x_col, E, dO = _on_device(_inputs(kind, h, f))
    got = _pair(g, attn, x_row, x_col, torch.zeros_like(E), dO)
    want = _plain_pair(g, attn, x_row, x_col, dO)
    for a, b, name in zip(got, want, ("out", "row_max", "row_sum", "dX_row", "dX_col", "dattn")):
        assert torch.equal(a, b), (kind, h, f, name)
    _check(got[6], _reference(kind, h, f, zero_e=True)["grads"][3], f"E = 0 {kind} h{h} f{f} dE")


# ---- 3. no edge is lost: the boundary-degree cases, exactly -----------------------------------------------------------------
@pytest.mark.parametrize("case", pc.case_ids("gatv2"), ids=str)
def test_boundary_degrees_exact(case):
    """X_row' = 0 and E_e = X_row[row(e)]: 0 + x = x and x + y = y + x are exact in fp32, so z_e has the plain pair's bits
    and every output must be torch.equal to gatv2_forward / gatv2_backward on the original inputs (which
    tests/test_gpu_edge_exact.py holds to the fp32-level bounds there).  Every reduction of the new file has the plain
    file's order, so no output is excepted.  sum_{e of row i} dE_e is the plain pair's dX_row_i at the bar."""
    pg = pc.graph(case[0], case[1])
    x = pc.gatv2_inputs(*case)
    g = {k: _dev(pg[k], torch.int32) for k in ("row_ptr", "col_ind", "col_ptr", "row_ind", "val_idx")}
    attn, x_row, x_col, dO = (_dev(x[k]) for k in ("attn", "X_row", "X_col", "dO"))
    rows = _dev(pg["rows"], torch.int64)
    want = _plain_pair(g, attn, x_row, x_col, dO)
    got = _pair(g, attn, torch.zeros_like(x_row), x_col, x_row[rows].contiguous(), dO)
    for a, b, name in zip(got, want, ("out", "row_max", "row_sum", "dX_row", "dX_col", "dattn")):
        assert torch.equal(a, b), (case, name, float((a - b).abs().max()))
    summed = torch.zeros_like(x_row, dtype=torch.float64).index_add_(0, rows, got[6].double())
    _check(summed, want[3], f"boundary {case} sum of dE over a row")


# ---- 4. dE == NULL ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f", [("lane", 2, 20), ("wave", 8, 16)])
def test_without_dE(kind, h, f):
    from DFGNN.operators.fused_gatconv import GATv2ConvFuse_edge
    g, attn, x_row, x_col, E, dO = _on_device(_inputs(kind, h, f))
    with_dE = _pair(g, attn, x_row, x_col, E, dO)
    without = _pair(g, attn, x_row, x_col, E, dO, want_dE=False)
    assert without[6] is None
    for a, b in zip(with_dE[:6], without[:6]):
        assert torch.equal(a, b)
    graph = (g["row_ptr"], g["col_ind"], g["col_ptr"], g["row_ind"], g["val_idx"])
    a, xr, xc = (t.clone().requires_grad_(True) for t in (attn, x_row, x_col))
    e = E.clone()
    GATv2ConvFuse_edge(a, *graph, SLOPE, xr, xc, e).backward(dO)
    assert e.grad is None
    for got, want in zip((xr.grad, xc.grad, a.grad), with_dE[3:6]):
        assert torch.equal(got, want)


# ---- 5. shared weights, determinism -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f", [("lane", 2, 20), ("wave", 8, 16)])
def test_shared_weights_and_determinism(kind, h, f):
    """X_row is X_col (one pointer for both operands) runs and matches: out, and dX_row + dX_col against the reference's
    single gradient.  Two backward calls on the same inputs agree bit for bit in all four gradients (no atomics)."""
    import fused_gatconv as gat
    g, attn, x, _, E, dO = _on_device(_inputs(kind, h, f))
    ref = _reference(kind, h, f, shared=True)
    out, mx, sm, dxr, dxc, da, dE = _pair(g, attn, x, x, E, dO)
    assert torch.equal(out, gat.gatv2_inference_edge(attn, g["row_ptr"], g["col_ind"], SLOPE, x, x, E))
    _check(out, ref["out"], f"shared {kind} out")
    _check(dxr + dxc, ref["grads"][0], f"shared {kind} dX")
    _check(da, ref["grads"][1], f"shared {kind} dattn")
    _check(dE, ref["grads"][2], f"shared {kind} dE")
    again = gat.gatv2_backward_edge(SLOPE, g["row_ptr"], g["col_ind"], g["col_ptr"], g["row_ind"], g["val_idx"], attn, x, x, E,
                                    out, mx, sm, dO)
    for a, b in zip((dxr, dxc, da, dE), again):
        assert torch.equal(a, b)


# ---- 6. rectangular -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f", [("tall", 2, 20), ("wide", 1, 128), ("block", 8, 16)])
def test_rectangular_against_reference(kind, h, f):
    """m != n_cols.  tall: a lane group per row, a wave per column; wide and block: a wave per row, a lane group per
    column."""
    rg = rc.graph(kind)
    assert rg["m"] != rg["n_cols"]
    g = {k: _dev(rg[k], torch.int32) for k in ("row_ptr", "col_ind", "col_ptr", "row_ind", "val_idx")}
    gen = torch.Generator().manual_seed(7 + h + f)
    attn = torch.randn(h, f, generator=gen) * f ** -0.5
    x_row, dO = (torch.randn(rg["m"], h, f, generator=gen) for _ in range(2))
    x_col = torch.randn(rg["n_cols"], h, f, generator=gen)
    E = torch.randn(rg["nnz"], h, f, generator=gen)
    rows, cols = (torch.from_numpy(rg[k].astype(np.int64)) for k in ("rows", "col_ind"))
    ref = _ref_all(rows, cols, rg["m"], attn, x_row, x_col, E, dO)
    out, mx, sm, dxr, dxc, da, dE = _pair(g, *(t.to(DEV) for t in (attn, x_row, x_col, E, dO)))
    er, ec = rg["deg"] == 0, rg["indeg"] == 0
    what = f"rect {kind} h{h} f{f}"
    assert dxc.shape == x_col.shape
    _check(out, ref["out"], f"{what} out")
    _check(_np(mx)[~er], _np(ref["row_max"])[~er], f"{what} row_max")
    _check(sm, ref["row_sum"], f"{what} row_sum")
    for got, want, name in zip((dxr, dxc, da, dE), ref["grads"], ("dX_row", "dX_col", "dattn", "dE")):
        _check(got, want, f"{what} {name}")
    assert (_np(out)[er] == 0).all() and (_np(dxr)[er] == 0).all() and (_np(dxc)[ec] == 0).all()
    assert (_np(mx)[er] == np.float32(-1e38)).all() and (_np(sm)[er] == 0).all()


@pytest.mark.parametrize("kind,h,f", [("lane", 2, 20), ("wave", 8, 16)])
def test_square_entries_are_the_rect_entries(kind, h, f):
    """dfgnn_gatv2_fwd_edge / _bwd_edge through the C ABI against the *_rect entries at n_cols = m: equal bits."""
    import dfgnn_native
    from _binding_util import call
    g, attn, x_row, x_col, E, dO = _on_device(_inputs(kind, h, f))
    m, nnz = g["m"], g["nnz"]
    want = _pair(g, attn, x_row, x_col, E, dO)                                         # (the bindings call the _rect entries)
    new = lambda *shape: torch.full(shape, float("nan"), device=DEV)  # noqa: E731
    out, mx, sm, delta = new(m, h, f), new(m, h), new(m, h), new(m, h)
    ws = new(int(dfgnn_native.lib().dfgnn_gatv2_bwd_ws_floats(h, f)))
    dxr, dxc, da, dE = new(m, h, f), new(m, h, f), new(h, f), new(nnz, h, f)
    call("dfgnn_gatv2_fwd_edge", "gatv2_forward_edge", DEV, m, nnz, h, f, g["row_ptr"], g["col_ind"], attn, SLOPE, x_row, x_col, E,
         mx, sm, out)
    call("dfgnn_gatv2_bwd_edge", "gatv2_backward_edge", DEV, m, nnz, h, f, g["row_ptr"], g["col_ind"], g["col_ptr"], g["row_ind"],
         g["val_idx"], attn, SLOPE, x_row, x_col, E, out, mx, sm, dO, delta, ws, dxr, dxc, da, dE)
    torch.cuda.synchronize()
    for a, b, name in zip((out, mx, sm, dxr, dxc, da, dE), want, ("out", "row_max", "row_sum", "dX_row", "dX_col", "dattn", "dE")):
        assert torch.equal(a, b), name


# ---- 7. autograd Function and layers ----------------------------------------------------------------------------------------
def test_autograd_function():
    """GATv2ConvFuse_edge + .backward() on the lane-group graph at (2, 20): the reference's gradients for attn, X_row, X_col,
    E; one leaf passed as both operands receives the reference's single summed gradient."""
    from DFGNN.operators.fused_gatconv import GATv2ConvFuse_edge
    g, attn, x_row, x_col, E, dO = _on_device(_inputs("lane", 2, 20))
    graph = (g["row_ptr"], g["col_ind"], g["col_ptr"], g["row_ind"], g["val_idx"])
    a, xr, xc, e = (t.clone().requires_grad_(True) for t in (attn, x_row, x_col, E))
    out = GATv2ConvFuse_edge(a, *graph, SLOPE, xr, xc, e)
    out.backward(dO)
    ref = _reference("lane", 2, 20)
    _check(out, ref["out"], "autograd out")
    for got, want, name in zip((xr.grad, xc.grad, a.grad, e.grad), ref["grads"], ("X_row.grad", "X_col.grad", "attn.grad", "E.grad")):
        _check(got, want, f"autograd {name}")
    a, x, e = (t.clone().requires_grad_(True) for t in (attn, x_row, E))
    GATv2ConvFuse_edge(a, *graph, SLOPE, x, x, e).backward(dO)
    ref = _reference("lane", 2, 20, shared=True)
    for got, want, name in zip((x.grad, a.grad, e.grad), ref["grads"], ("X.grad", "attn.grad", "E.grad")):
        _check(got, want, f"autograd shared {name}")


@functools.lru_cache(maxsize=None)
def _cora():
    from DFGNN.layers import preprocess_Hyper_fw_bw
    from DFGNN.utils import synthetic as S
    g = S.cora_like().to(DEV)
    return g.num_nodes(), preprocess_Hyper_fw_bw(g)


def _layer_both_branches(layer, params, feat, edge_attr, what, n_params):
    outs, grads = [], []
    for fuse in (False, True):
        layer.zero_grad()
        out = layer(params, feat, edge_attr, fuse=fuse)
        out.sum().backward()
        outs.append(out.detach())
        grads.append({n: p.grad.clone() for n, p in layer.named_parameters()})
    assert len(grads[0]) == n_params and "lin_edge.weight" in grads[0]
    _check(outs[1], outs[0], f"{what} out")
    for n in grads[0]:
        _check(grads[1][n], grads[0][n], f"{what} d{n}")
    with torch.no_grad():
        _check(layer.eval()(params, feat, edge_attr, fuse=True), outs[0], f"{what} eval out")
    layer.train()
    return outs[0]


@pytest.mark.parametrize("heads,share", [(1, False), (4, False), (2, True)])
def test_layer_against_its_index_op_branch(heads, share):
    """GATv2Conv_edge on the cora-like graph.  .train(): after out.sum().backward() the gradient of every parameter,
    lin_edge.weight included, agrees between the fused branch and the index-op branch; .eval(): the fused branch (the
    inference operator) gives the same output."""
    from DFGNN.layers import GATv2Conv_edge
    n, params = _cora()
    torch.manual_seed(3)
    layer = GATv2Conv_edge(32, 16, heads, share_weights=share, edge_dim=6).to(DEV).train()
    feat = torch.randn(n, 32, device=DEV)
    edge_attr = torch.randn(params[3].numel(), 6, device=DEV)
    out = _layer_both_branches(layer, params, feat, edge_attr, f"GATv2Conv_edge heads {heads}", 4 if share else 6)
    assert out.shape == (n, heads * 16)


def test_layer_on_a_sampled_block_and_the_harness_format():
    """feat = (feat_cols, feat_rows) on a sample_block block (96 x 257); --conv gatv2 --format forward_edge runs."""
    import argparse

    from DFGNN.layers import GATv2Conv_edge, load_graphconv_layer, preprocess_block
    from DFGNN.utils.graph import Block
    rg = rc.graph("block")
    params = preprocess_block(Block(rg["src"], rg["dst"], rg["m"], rg["n_cols"]).to(DEV))
    torch.manual_seed(4)
    layer = GATv2Conv_edge(16, 8, 3, edge_dim=5).to(DEV).train()
    h_cols = torch.randn(rg["n_cols"], 16, device=DEV)
    h_rows = h_cols[:rg["m"]].contiguous()
    edge_attr = torch.randn(rg["nnz"], 5, device=DEV)
    out = _layer_both_branches(layer, params, (h_cols, h_rows), edge_attr, "GATv2Conv_edge on a block", 6)
    assert out.shape == (rg["m"], 24)
    n, cora = _cora()
    args = argparse.Namespace(conv="gatv2", format="forward_edge", dim=32, heads=2)
    out, ms = load_graphconv_layer(args).to(DEV).train()(cora, torch.randn(n, 32, device=DEV), fuse=True)
    assert out.shape == (n, 64) and ms > 0


# ---- 8. saved state -------------------------------------------------------------------------------------------------------------
def test_saved_state_is_E_and_nothing_else_per_edge():
    """m = 64, average degree 60, h = 1, f = 8: m h f = 512 < nnz.  Among the floating-point tensors autograd keeps between
    forward and backward exactly one has nnz h f elements, and it is E itself; no other has nnz elements or more."""
    from DFGNN.operators.fused_gatconv import GATv2ConvFuse_edge
    g, attn, x_row, x_col, E, dO = _on_device(_inputs("saved", 1, 8))
    assert g["m"] * 1 * 8 < g["nnz"]
    saved = []

    def pack(t):
        saved.append(t)
        return t

    a, xr, xc, e = (t.clone().requires_grad_(True) for t in (attn, x_row, x_col, E))
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        out = GATv2ConvFuse_edge(a, g["row_ptr"], g["col_ind"], g["col_ptr"], g["row_ind"], g["val_idx"], SLOPE, xr, xc, e)
    floating = [t for t in saved if t.is_floating_point()]
    big = [t for t in floating if t.numel() >= g["nnz"]]
    assert len(floating) >= 6                                         # attn, X_row, X_col, E, out and the statistics
    assert len(big) == 1 and big[0].numel() == g["nnz"] * 8 and big[0].data_ptr() == e.data_ptr(), [tuple(t.shape) for t in big]
    out.backward(dO)
    ref = _reference("saved", 1, 8)
    _check(xr.grad, ref["grads"][0], "saved-state case X_row.grad")
    _check(e.grad, ref["grads"][3], "saved-state case E.grad")


# ---- 9. peak memory -------------------------------------------------------------------------------------------------------------
def test_memory_of_one_step():
    """The wave graph at h = 2, f = 16, through the operator with dE wanted.  The step allocates out, dX_row, dX_col (and
    at most one more feature-sized tensor: 4 bytes(X)), row_max, row_sum, delta (3 [m, h] arrays), the partials ws, dattn and
    dE.  Its peak above the step's start stays below bytes(dE) + bytes(ws) + 4 bytes(X) + 3 bytes([m, h]) + 8 KB (16
    allocations rounded up to the caching allocator's 512-byte blocks).  The slack, the spare feature tensor included, is far
    below bytes(E): a second array of nnz h f floats cannot hide in it."""
    import dfgnn_native
    from DFGNN.operators.fused_gatconv import GATv2ConvFuse_edge
    h, f = 2, 16
    g, attn, x_row, x_col, E, dO = _on_device(_inputs("wave", h, f))
    bytes_x, bytes_mh, bytes_e = 4 * g["m"] * h * f, 4 * g["m"] * h, 4 * g["nnz"] * h * f
    bytes_ws = 4 * int(dfgnn_native.lib().dfgnn_gatv2_bwd_ws_floats(h, f))
    slack = 16 * 512
    assert bytes_ws == 4 * 2048 * h * f and slack + bytes_x < bytes_e // 4
    graph = (g["row_ptr"], g["col_ind"], g["col_ptr"], g["row_ind"], g["val_idx"])

    def peak(e_grad):
        a, xr, xc = (t.clone().requires_grad_(True) for t in (attn, x_row, x_col))
        e = E.clone().requires_grad_(e_grad)

        def step():
            o = GATv2ConvFuse_edge(a, *graph, SLOPE, xr, xc, e)
            return torch.autograd.grad(o, (a, xr, xc, e) if e_grad else (a, xr, xc), dO)

        step()
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res = step()
        torch.cuda.synchronize()
        assert len(res) == (4 if e_grad else 3)
        return torch.cuda.max_memory_allocated() - base

    p_with, p_without = peak(True), peak(False)
    bound = bytes_ws + 4 * bytes_x + 3 * bytes_mh + slack
    print(f"gatv2_edge peak of one fwd+bwd: with dE {p_with} B (bound {bytes_e + bound} B), without {p_without} B (bound {bound} B); "
          f"bytes(E) = {bytes_e} B, bytes(ws) = {bytes_ws} B, bytes(X) = {bytes_x} B")
    assert p_with <= bytes_e + bound
    assert p_without <= bound


# ---- 10. plumbing -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [0, 5])
def test_empty_problems(m):
    """m == 0, and m == 5 without an edge (E [0, h, f]): zero outputs, sentinels, a zero dattn, no error."""
    import fused_gatconv as gat
    h, f = 2, 12
    i32 = dict(dtype=torch.int32, device=DEV)
    row_ptr, none = torch.zeros(m + 1, **i32), torch.zeros(0, **i32)
    attn, x, dO = torch.randn(h, f, device=DEV), torch.randn(m, h, f, device=DEV), torch.randn(m, h, f, device=DEV)
    E = torch.zeros(0, h, f, device=DEV)
    out, mx, sm = gat.gatv2_forward_edge(attn, row_ptr, none, SLOPE, x, x, E)
    dxr, dxc, da, dE = gat.gatv2_backward_edge(SLOPE, row_ptr, none, row_ptr, none, none, attn, x, x, E, out, mx, sm, dO)
    torch.cuda.synchronize()
    assert out.shape == dxr.shape == dxc.shape == (m, h, f) and mx.shape == sm.shape == (m, h) and da.shape == (h, f)
    assert dE.shape == (0, h, f)
    assert gat.gatv2_inference_edge(attn, row_ptr, none, SLOPE, x, x, E).shape == (m, h, f)
    for t in (out, dxr, dxc, da, sm):
        assert (t == 0).all()
    assert (mx == -1e38).all()


def test_bindings_agree():
    """The torch C++ extension and the ctypes transport give bit-identical results (with and without dE, inference) and the
    same RuntimeError text for an int64 row_ptr, a wrong-shaped E and a missing val_idx."""
    import dfgnn_native
    import fused_gatconv as gat
    assert dfgnn_native.ext() is not None and hasattr(dfgnn_native.ext(), "gatv2_bwd_edge")
    cases = [_on_device(_inputs(kind, h, f)) for kind, h, f in (("lane", 2, 20), ("wave", 8, 16), ("wave", 2, 7))]

    def run():
        res = []
        for c in cases:
            res += list(_pair(*c))
            res += list(_pair(*c, want_dE=False)[3:6])
            g, attn, x_row, x_col, E, _ = c
            res.append(gat.gatv2_inference_edge(attn, g["row_ptr"], g["col_ind"], SLOPE, x_row, x_col, E))
        g, attn, x_row, x_col, E, dO = cases[0]
        out, mx, sm = res[:3]
        errs = []
        for bad in (dict(row_ptr=g["row_ptr"].long()), dict(E=E.transpose(0, 1).contiguous()), dict(E=E.reshape(g["nnz"], -1)),
                    dict(E=E.double())):
            a = dict(row_ptr=g["row_ptr"], E=E)
            a.update(bad)
            try:
                gat.gatv2_forward_edge(attn, a["row_ptr"], g["col_ind"], SLOPE, x_row, x_col, a["E"])
                errs.append(None)
            except RuntimeError as e:
                errs.append(str(e))
        for bad in (dict(val_idx=None), dict(val_idx=g["val_idx"][:-1].contiguous()), dict(E=E[:-1].contiguous())):
            a = dict(val_idx=g["val_idx"], E=E)
            a.update(bad)
            try:
                gat.gatv2_backward_edge(SLOPE, g["row_ptr"], g["col_ind"], g["col_ptr"], g["row_ind"], a["val_idx"], attn, x_row,
                                        x_col, a["E"], out, mx, sm, dO)
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
    words = ("int32", "E must have shape", "E must have shape", "E must have dtype", "val_idx is required", "val_idx", "E must have shape")
    for e1, e2, word in zip(err_ext, err_ctypes, words):
        assert e1 and e2 and word in e1 and word in e2, (e1, e2)
    for k in (0, 1, 2, 4, 6):                     # the same text: the int64 row_ptr, the wrong-shaped E, the missing val_idx
        assert err_ext[k] == err_ctypes[k], (err_ext[k], err_ctypes[k])


def test_hipgraph_capture_without_warmup():
    """One forward + backward step (with dE: forward, CSR pass, CSC pass, reduction -- a linear chain of launches) recorded
    into a HIP graph with no warm-up and no earlier eager run of its shape (only a step of ANOTHER shape runs first, so that
    the library and its code object are loaded); the eager step it is compared with runs after the capture.  The replay
    equals the eager result bit for bit, also after X_row and E were overwritten in place."""
    from DFGNN.utils import GraphedStep
    _pair(*_on_device(_inputs("lane", 2, 20)))
    g, attn, x_row, x_col, E, dO = _on_device(_inputs("wave", 1, 64, seed=5))

    def step():
        return [t for t in _pair_nosync(g, attn, x_row, x_col, E, dO)]

    graphed = GraphedStep(step, warmup=0)
    first = [t.clone() for t in graphed.replay()]
    for a, b in zip(step(), first):
        assert torch.equal(a, b)
    x_row.mul_(0.5)                                        # next "batch" of features, same structure
    E.add_(0.25)
    again = [t.clone() for t in graphed.replay()]
    for a, b in zip(step(), again):
        assert torch.equal(a, b)
    assert not torch.equal(again[0], first[0])
    ref = _ref_all(g["rows"], g["cols"], g["m"], *(t.cpu() for t in (attn, x_row, x_col, E, dO)))
    _check(again[0], ref["out"], "graphed out")
    _check(again[6], ref["grads"][3], "graphed dE")


def _pair_nosync(g, attn, x_row, x_col, E, dO):
    import fused_gatconv as gat
    out, mx, sm = gat.gatv2_forward_edge(attn, g["row_ptr"], g["col_ind"], SLOPE, x_row, x_col, E)
    return [out, mx, sm] + list(gat.gatv2_backward_edge(SLOPE, g["row_ptr"], g["col_ind"], g["col_ptr"], g["row_ind"], g["val_idx"],
                                                        attn, x_row, x_col, E, out, mx, sm, dO))
