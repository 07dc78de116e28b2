"""CPU: the GT pair with typed edges (dfgnn_gt_fwd_typed / dfgnn_gt_bwd_typed, their _rect forms and
dfgnn_gt_typed_bwd_ws_floats) is declared, exported, bound and validates its arguments before any GPU call; the operators
and layers import; preprocess_types orders and validates the types; the layer's torch branch and
tests/gt_typed_cases.reference agree with the closed-form backward; and the fp32-level inputs of
tests/test_gpu_gt_typed.py are those of the edge pair (R[etype] == E exactly), so that the power condition proven in
tests/test_gt_edge_host.py carries over."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gt_edge_cases as ec
import gt_typed_cases as tc
import parity_cases as pc
from conftest import ROOT, csc_of, random_graph

NAMES = ("dfgnn_gt_typed_bwd_ws_floats", "dfgnn_gt_fwd_typed", "dfgnn_gt_bwd_typed", "dfgnn_gt_fwd_typed_rect",
         "dfgnn_gt_bwd_typed_rect")


def test_symbols_declared_exported_and_bound():
    import dfgnn_native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfgnn.h")).read(), flags=re.S)
    raw = ctypes.CDLL(dfgnn_native.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), n
        assert hasattr(raw, n), n
        assert n in dfgnn_native.SIGNATURES
    sig = dfgnn_native.SIGNATURES
    assert len(sig["dfgnn_gt_typed_bwd_ws_floats"]) == 3
    assert len(sig["dfgnn_gt_fwd_typed"]) == 17 and len(sig["dfgnn_gt_fwd_typed_rect"]) == 18
    assert len(sig["dfgnn_gt_bwd_typed"]) == 28 and len(sig["dfgnn_gt_bwd_typed_rect"]) == 29
    assert dfgnn_native.lib().dfgnn_abi_version() == 11
    ext_src = open(os.path.join(ROOT, "df-gnn_amd", "csrc", "torch_ext.cpp")).read()
    for n in ("gt_fwd_typed", "gt_bwd_typed"):                         # the torch-extension transport binds both
        assert re.search(r'm\.def\("' + n + r'",\s*&' + n + r"\b", ext_src), n


def test_argument_checks_need_no_gpu():
    """Every check of the four entry points is answered before any launch."""
    import dfgnn_native
    L = dfgnn_native.lib()
    buf = (ctypes.c_float * 64)()
    idx = (ctypes.c_int * 8)(0, 1, 2, 2, 0, 0, 0, 0)
    p, i = ctypes.addressof(buf), ctypes.addressof(idx)

    def fwd(rect, m=3, nnz=2, h=1, T=2, row_ptr=i, col_ind=i, etype=i, R=p, Q=p, K=p, V=p, mx=p, sm=p, out=p):
        tail = (row_ptr, col_ind, None, etype, R, Q, K, V, mx, sm, out, None)
        if rect:
            return L.dfgnn_gt_fwd_typed_rect(m, 3, nnz, h, 4, T, *tail)
        return L.dfgnn_gt_fwd_typed(m, nnz, h, 4, T, *tail)

    def bwd(rect, m=3, nnz=2, h=1, T=2, row_ptr=i, col_ind=i, etype=i, col_ptr=i, row_ind=i, val_idx=None, etype_csc=i, R=p,
            Q=p, K=p, V=p, out=p, mx=p, sm=p, grad=p, delta=p, ws=p, dQ=p, dK=p, dV=p, dR=p, val=None):
        tail = (row_ptr, col_ind, val, etype, col_ptr, row_ind, val_idx, etype_csc, R, Q, K, V, out, mx, sm, grad, delta, ws,
                dQ, dK, dV, dR, None)
        if rect:
            return L.dfgnn_gt_bwd_typed_rect(m, 3, nnz, h, 4, T, *tail)
        return L.dfgnn_gt_bwd_typed(m, nnz, h, 4, T, *tail)

    for rect in (False, True):
        for fn in (fwd, bwd):
            assert fn(rect, m=-1) == -1 and fn(rect, nnz=-1) == -1
            assert fn(rect, T=0) == -1 and fn(rect, T=-3) == -1                # T >= 1
            assert fn(rect, T=0, m=0) == -1                                    # ... whatever the extents
            assert fn(rect, row_ptr=None) == -1 and fn(rect, col_ind=None) == -1
            for name in ("Q", "K", "V", "out", "etype", "R"):                  # a missing pointer (etype, R: nnz > 0)
                assert fn(rect, **{name: None}) == -1, (fn.__name__, name)
            assert fn(rect, h=70000) == -2                                     # h > 65535
        assert fwd(rect, mx=None) == -1 and fwd(rect, sm=None) == -1           # one statistic without the other
        for name in ("delta", "col_ptr", "row_ind", "etype_csc", "grad", "mx", "sm", "dQ", "dK", "dV"):
            assert bwd(rect, **{name: None}) == -1, name
        assert bwd(rect, val=p, val_idx=None) == -1                            # val_idx: needed exactly with edge values
        assert bwd(rect, ws=None) == -1                                        # ws == NULL with dR != NULL
        assert bwd(rect, T=3000) == -2 and bwd(rect, T=2049) == -2             # beyond T f <= 8192 with dR: before any launch
        assert bwd(rect, T=3000, ws=None) == -1
    # empty problems succeed (square: m == 0 is neither rows nor columns; nothing is launched or written)
    assert fwd(False, m=0, nnz=0) == 0 and fwd(False, m=0, nnz=0, Q=None, R=None, etype=None) == 0
    assert bwd(False, m=0, nnz=0, dR=None, ws=None) == 0
    assert bwd(False, m=0, nnz=0, dR=None, ws=None, Q=None, R=None, etype=None, etype_csc=None) == 0
    assert fwd(True, m=0, nnz=0, Q=None, out=None) == 0                        # a rectangular graph without rows
    assert fwd(False, m=3, nnz=2, h=0) == 0


def test_ws_floats_codes():
    import dfgnn_native
    ws = dfgnn_native.lib().dfgnn_gt_typed_bwd_ws_floats
    assert ws(64, 1, 128) > 0 and ws(512, 8, 16) > 0                           # T f == 8192: the supported range
    assert ws(64, 1, 128) % (64 * 128) == 0 and ws(64, 1, 128) == ws(64, 1, 128)
    assert ws(16, 8, 16) == ws(16, 1, 128)                                     # T h f floats per partial
    assert ws(-1, 1, 16) == -1 and ws(0, 1, 16) == -1 and ws(4, -1, 16) == -1 and ws(4, 1, -16) == -1
    assert ws(65, 1, 128) == -2 and ws(513, 8, 16) == -2 and ws(8193, 1, 1) == -2
    assert ws(4, 70000, 16) == -2
    assert ws(512, 65535, 16) == -2                                            # does not fit an int: never a wrapped size
    assert 304 * 7 <= 8192 and ws(304, 2, 7) > 0                               # the fp32-level (7, 2) cases run with dR
    import fused_gtconv
    assert fused_gtconv.gt_typed_dR_supported(304, 2, 7) and fused_gtconv.gt_typed_dR_supported(64, 1, 128)
    assert not fused_gtconv.gt_typed_dR_supported(304, 1, 32) and not fused_gtconv.gt_typed_dR_supported(65, 1, 128)


def test_operators_and_layers_import():
    import argparse

    import fused_gtconv
    from DFGNN.layers import SparseMHA_typed, load_graphconv_layer, load_prepfunc, preprocess_Hyper_fw_bw, preprocess_types
    from DFGNN.layers.GT import SparseMHA_typed_timing
    from DFGNN.operators.fused_gtconv import FusedGTFunction_typed, GTConvFuse_inference_typed, GTConvFuse_typed
    for name in ("gt_inference_typed", "gt_forward_typed", "gt_backward_typed", "gt_typed_dR_supported"):
        assert callable(getattr(fused_gtconv, name))
    assert callable(GTConvFuse_typed) and callable(GTConvFuse_inference_typed) and hasattr(FusedGTFunction_typed, "apply")
    assert callable(preprocess_types)
    args = argparse.Namespace(conv="gt", format="forward_typed", dim=64, heads=2)
    layer = load_graphconv_layer(args)
    assert isinstance(layer, SparseMHA_typed_timing) and layer.num_types == 16 and layer.rel.shape == (16, 64)
    assert load_prepfunc(args) is preprocess_Hyper_fw_bw
    layer = SparseMHA_typed(64, 64, 2, 5)
    assert layer.head_dim == 32 and layer.rel.shape == (5, 64) and layer.rel.requires_grad


def _params(row_ptr, col_ind, rows, n_cols, val=None):
    """The 9-tuple of preprocess_Hyper_fw_bw / preprocess_block as CPU tensors."""
    col_ptr, row_ind, val_idx = csc_of(row_ptr, col_ind, rows, n_cols)
    ti = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32))  # noqa: E731
    val = torch.ones(len(col_ind), dtype=torch.float64) if val is None else torch.from_numpy(val)
    return (None, ti(rows), ti(row_ptr), ti(col_ind), val, ti(col_ptr), ti(row_ind), ti(val_idx), 0)


def test_preprocess_types():
    from DFGNN.layers import preprocess_types
    rng = np.random.default_rng(3)
    row_ptr, col_ind, rows = random_graph(rng, 50, 5, empty_frac=0.1, dup_frac=0.1)
    nnz = len(col_ind)
    for n_cols in (50, 70):                                                    # square and rectangular params
        params = _params(row_ptr, col_ind, rows, n_cols)
        etype = torch.from_numpy(rng.integers(0, 9, nnz))                      # int64 in, int32 out
        et, et_csc = preprocess_types(params, etype, 9)
        assert et.dtype == et_csc.dtype == torch.int32 and et.is_contiguous() and et_csc.is_contiguous()
        assert torch.equal(et.long(), etype) and torch.equal(et_csc, et[params[7].long()])
        cols_csc = params[3][params[7].long()]                                 # the CSC order: by column
        assert (cols_csc[1:] >= cols_csc[:-1]).all()
        bad = etype.clone()
        bad[nnz // 2] = 9
        with pytest.raises(ValueError, match="edge types must lie in"):
            preprocess_types(params, bad, 9)
        bad[nnz // 2] = -1
        with pytest.raises(ValueError, match="edge types must lie in"):
            preprocess_types(params, bad, 9)
        with pytest.raises(ValueError, match="etype must have shape"):
            preprocess_types(params, etype[:-1], 9)
        with pytest.raises(ValueError):
            preprocess_types(params, etype.double(), 9)
    empty = _params(np.zeros(4, dtype=np.int32), np.zeros(0, dtype=np.int32), np.zeros(0, dtype=np.int32), 3)
    et, et_csc = preprocess_types(empty, torch.zeros(0, dtype=torch.int64), 2)
    assert et.numel() == et_csc.numel() == 0


# ---- the layer's torch branch and the tests' reference against the closed-form backward -----------------------------------
def _closed_form(row_ptr, col_ind, n_cols, val, etype, R, Q, K, V, dO):
    """The issue's equations, edge by edge in float64.  R: [T, h, f]."""
    m, h, f = Q.shape
    out, dQ = np.zeros((m, h, f)), np.zeros((m, h, f))
    dK, dV, dR = np.zeros((n_cols, h, f)), np.zeros((n_cols, h, f)), np.zeros_like(R)
    for i in range(m):
        lo, hi = row_ptr[i], row_ptr[i + 1]
        if hi == lo:
            continue                                                   # an empty row: zeros everywhere
        for hd in range(h):
            ke, ve = K[col_ind[lo:hi], hd] + R[etype[lo:hi], hd], V[col_ind[lo:hi], hd] + R[etype[lo:hi], hd]
            s = val[lo:hi] * (ke @ Q[i, hd])
            p = np.exp(s - s.max())
            p /= p.sum()
            out[i, hd] = p @ ve
            ds = p * (ve @ dO[i, hd] - dO[i, hd] @ out[i, hd])
            dQ[i, hd] = (ds * val[lo:hi]) @ ke
            np.add.at(dK[:, hd], col_ind[lo:hi], (ds * val[lo:hi])[:, None] * Q[i, hd])
            np.add.at(dV[:, hd], col_ind[lo:hi], p[:, None] * dO[i, hd])
            np.add.at(dR[:, hd], etype[lo:hi], (ds * val[lo:hi])[:, None] * Q[i, hd] + p[:, None] * dO[i, hd])
    return out, dQ, dK, dV, dR


def _small_graph(rng, m, T):
    """A graph with an empty row and a duplicate edge, and types of which one has no edge."""
    row_ptr, col_ind, rows = random_graph(rng, m, 4, empty_frac=0.1, dup_frac=0.1, max_deg=30)
    deg = np.diff(row_ptr)
    assert (deg == 0).any(), "the graph needs an empty row"
    assert any(len(set(col_ind[row_ptr[i]:row_ptr[i + 1]])) < deg[i] for i in range(m)), "the graph needs a duplicate edge"
    etype = rng.integers(0, T - 1, len(col_ind))
    etype[etype == 2] = T - 1                                          # type 2 has no edge, the last one has
    assert (etype != 2).all() and (etype == T - 1).any()
    return row_ptr, col_ind, rows, etype


def _close(name, a, b):
    assert np.isfinite(a).all(), name
    assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), (name, np.abs(a - b).max())


def test_layer_torch_branch_matches_closed_form():
    from DFGNN.layers import SparseMHA_typed, preprocess_types
    rng = np.random.default_rng(5)
    m, heads, dim, T = 40, 2, 12, 6
    row_ptr, col_ind, rows, etype = _small_graph(rng, m, T)
    val = rng.uniform(0.5, 1.5, len(col_ind))
    params = _params(row_ptr, col_ind, rows, m, val)
    types = preprocess_types(params, torch.from_numpy(etype), T)
    torch.manual_seed(0)
    layer = SparseMHA_typed(dim, dim, heads, T).double().train()
    x = torch.randn(m, dim, dtype=torch.float64)
    dO = torch.randn(m, heads, dim // heads, dtype=torch.float64)
    q, k, v = (t.detach() for t in layer._qkv_fused(x))
    R = layer.rel.detach().view(T, heads, dim // heads)
    want = _closed_form(row_ptr, col_ind, m, val, etype, R.numpy(), q.numpy(), k.numpy(), v.numpy(), dO.numpy())
    y = layer(params, x, types, fuse=False)
    assert y.shape == (m, dim)
    _close("out", y.detach().numpy().reshape(m, heads, -1), want[0])
    (g_rel,) = torch.autograd.grad(y, layer.rel, dO.reshape(m, -1))
    _close("d rel", g_rel.numpy().reshape(T, heads, -1), want[4])
    assert (g_rel[2] == 0).all() and (g_rel[T - 1] != 0).any()        # the type without an edge
    empty = np.diff(row_ptr) == 0
    assert (y.detach().numpy()[empty] == 0).all()


@pytest.mark.parametrize("n_cols", [30, 47], ids=["square", "rect"])
def test_reference_matches_closed_form(n_cols):
    """tests/gt_typed_cases.reference (the GPU tests' reference) against the closed form."""
    rng = np.random.default_rng(6)
    m, h, f, T = 30, 2, 5, 6
    row_ptr, col_ind, rows, etype = _small_graph(rng, m, T)
    val = rng.uniform(0.5, 1.5, len(col_ind))
    R = rng.standard_normal((T, h, f))
    Q, dO = (rng.standard_normal((m, h, f)) for _ in range(2))
    K, V = (rng.standard_normal((n_cols, h, f)) for _ in range(2))
    ref = tc.reference(row_ptr, col_ind, n_cols, val, etype, R, Q, K, V, dO)
    want = _closed_form(row_ptr, col_ind, n_cols, val, etype, R, Q, K, V, dO)
    for name, b in zip(("out", "dQ", "dK", "dV", "dR"), want):
        _close(name, ref[name], b)
    assert (ref["dR"][2] == 0).all() and (ref["dK"][m:] == 0).all()
    i = int(np.nonzero(np.diff(row_ptr) == 0)[0][0])
    assert (ref["row_max"][i] == tc.SENTINEL_MAX).all() and (ref["row_sum"][i] == 0).all()
    assert np.isfinite(ref["row_max"]).all()
    if n_cols == m:                                                    # ... and it is the edge pair's on E = R[etype]
        e = ec.reference(row_ptr, col_ind, val, R[etype], Q, K, V, dO)
        for name in ("out", "row_max", "row_sum", "dQ", "dK", "dV"):
            assert np.array_equal(ref[name], e[name]), name


def test_boundary_inputs_are_the_edge_pairs():
    """R[etype] == E exactly for all 32 cases: references, bounds and the power condition of the edge pair carry over."""
    cases = pc.case_ids("gt")
    assert len(cases) == 32
    with_dR = 0
    for case in cases:
        g = pc.graph(case[0], case[1])
        x = tc.boundary_inputs(case)
        f, h = case[2], case[3]
        assert x["R"].shape == (tc.BOUNDARY_T, h, f) and x["etype"].shape == (g["nnz"],) and x["etype"].dtype == np.int32
        assert 0 <= x["etype"].min() and x["etype"].max() < tc.BOUNDARY_T
        assert np.array_equal(x["R"][x["etype"].astype(np.int64)], x["E"])
        with_dR += tc.BOUNDARY_T * f <= 8192
    assert with_dR == 8 and 304 * 7 <= 8192                            # the (7, 2) cases


def test_boundary_bound_of_dR():
    """The dR bound of one case is positive and the float64 dR is the index_add of the edge pair's dE."""
    case = (False, False, 7, 2, False)
    assert case in pc.case_ids("gt")
    x, ref64, bounds = tc.boundary_references(case)
    assert set(bounds) == set(tc.OUTPUTS) and all(b > 0 for b in bounds.values())
    _, ref64e, bounds_e = ec.boundary_references(case)
    want = np.zeros((tc.BOUNDARY_T, 2, 7))
    np.add.at(want, x["etype"].astype(np.int64), ref64e["dE"])
    assert np.abs(ref64["dR"] - want).max() <= 1e-12 * np.abs(want).max()
    for k in ("out", "row_sum", "dQ", "dK", "dV"):
        assert bounds[k] == bounds_e[k] and ref64[k] is ref64e[k]
