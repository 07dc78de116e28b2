"""CPU: the GT pair with a typed attention bias (dfgnn_gt_fwd_tbias / dfgnn_gt_bwd_tbias, their _rect forms and
dfgnn_gt_tbias_bwd_ws_floats) is declared, exported, bound and validates its arguments before any GPU call; the operators
and layers import; and the layer's torch branch and tests/gt_tbias_cases.reference agree with a closed-form backward
written out here, square and rectangular, including a masked type that leaves one row fully and one partly masked."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gt_tbias_cases as zc
from conftest import ROOT, csc_of, random_graph

NAMES = ("dfgnn_gt_tbias_bwd_ws_floats", "dfgnn_gt_fwd_tbias", "dfgnn_gt_bwd_tbias", "dfgnn_gt_fwd_tbias_rect",
         "dfgnn_gt_bwd_tbias_rect")


def test_symbols_declared_exported_and_bound():
    import dfgnn_native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfgnn.h")).read(), flags=re.S)
    raw = ctypes.CDLL(dfgnn_native.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), n
        assert hasattr(raw, n), n
        assert n in dfgnn_native.SIGNATURES
    sig = dfgnn_native.SIGNATURES
    assert len(sig["dfgnn_gt_tbias_bwd_ws_floats"]) == 2
    assert len(sig["dfgnn_gt_fwd_tbias"]) == 17 and len(sig["dfgnn_gt_fwd_tbias_rect"]) == 18
    assert len(sig["dfgnn_gt_bwd_tbias"]) == 28 and len(sig["dfgnn_gt_bwd_tbias_rect"]) == 29
    assert dfgnn_native.lib().dfgnn_abi_version() == 11
    ext_src = open(os.path.join(ROOT, "df-gnn_amd", "csrc", "torch_ext.cpp")).read()
    for n in ("gt_fwd_tbias", "gt_bwd_tbias"):                         # the torch-extension transport binds both
        assert re.search(r'm\.def\("' + n + r'",\s*&' + n + r"\b", ext_src), n


def test_argument_checks_need_no_gpu():
    """Every check of the four entry points is answered before any launch."""
    import dfgnn_native
    L = dfgnn_native.lib()
    buf = (ctypes.c_float * 64)()
    idx = (ctypes.c_int * 8)(0, 1, 2, 2, 0, 0, 0, 0)
    p, i = ctypes.addressof(buf), ctypes.addressof(idx)

    def fwd(rect, m=3, nnz=2, h=1, T=2, row_ptr=i, col_ind=i, etype=i, B=p, Q=p, K=p, V=p, mx=p, sm=p, out=p):
        tail = (row_ptr, col_ind, None, etype, B, Q, K, V, mx, sm, out, None)
        if rect:
            return L.dfgnn_gt_fwd_tbias_rect(m, 3, nnz, h, 4, T, *tail)
        return L.dfgnn_gt_fwd_tbias(m, nnz, h, 4, T, *tail)

    def bwd(rect, m=3, nnz=2, h=1, T=2, row_ptr=i, col_ind=i, etype=i, col_ptr=i, row_ind=i, val_idx=None, etype_csc=i, B=p,
            Q=p, K=p, V=p, out=p, mx=p, sm=p, grad=p, delta=p, ws=p, dQ=p, dK=p, dV=p, dB=p, val=None):
        tail = (row_ptr, col_ind, val, etype, col_ptr, row_ind, val_idx, etype_csc, B, Q, K, V, out, mx, sm, grad, delta, ws,
                dQ, dK, dV, dB, None)
        if rect:
            return L.dfgnn_gt_bwd_tbias_rect(m, 3, nnz, h, 4, T, *tail)
        return L.dfgnn_gt_bwd_tbias(m, nnz, h, 4, T, *tail)

    for rect in (False, True):
        for fn in (fwd, bwd):
            assert fn(rect, m=-1) == -1 and fn(rect, nnz=-1) == -1
            assert fn(rect, T=0) == -1 and fn(rect, T=-3) == -1                # T >= 1
            assert fn(rect, T=0, m=0) == -1                                    # ... whatever the extents
            assert fn(rect, row_ptr=None) == -1 and fn(rect, col_ind=None) == -1
            for name in ("Q", "K", "V", "out", "etype", "B"):                  # a missing pointer (etype, B: nnz > 0)
                assert fn(rect, **{name: None}) == -1, (fn.__name__, name)
            assert fn(rect, h=70000) == -2                                     # h > 65535
        assert fwd(rect, mx=None) == -1 and fwd(rect, sm=None) == -1           # one statistic without the other
        for name in ("delta", "col_ptr", "row_ind", "etype_csc", "grad", "mx", "sm", "dQ", "dK", "dV"):
            assert bwd(rect, **{name: None}) == -1, name
        assert bwd(rect, val=p, val_idx=None) == -1                            # val_idx: needed exactly with edge values
        assert bwd(rect, ws=None) == -1                                        # ws == NULL with dB != NULL
        assert bwd(rect, T=4097) == -2 and bwd(rect, T=5000) == -2             # beyond T <= 4096 with dB: before any launch
        assert bwd(rect, T=4097, ws=None) == -1
    # empty problems succeed (square: m == 0 is neither rows nor columns; nothing is launched or written)
    assert fwd(False, m=0, nnz=0) == 0 and fwd(False, m=0, nnz=0, Q=None, B=None, etype=None) == 0
    assert bwd(False, m=0, nnz=0, dB=None, ws=None) == 0
    assert bwd(False, m=0, nnz=0, dB=None, ws=None, Q=None, B=None, etype=None, etype_csc=None) == 0
    assert bwd(False, m=0, nnz=0, dB=None, ws=None, T=5000) == 0               # without dB any T
    assert fwd(True, m=0, nnz=0, Q=None, out=None) == 0                        # a rectangular graph without rows
    assert fwd(False, m=3, nnz=2, h=0) == 0


def test_ws_floats_codes():
    import dfgnn_native
    import fused_gtconv
    ws = dfgnn_native.lib().dfgnn_gt_tbias_bwd_ws_floats
    assert ws(4096, 1) > 0 and ws(4096, 8) == 8 * ws(4096, 1)                  # the limit is supported
    assert ws(4097, 1) == -2 and ws(5000, 2) == -2
    assert ws(-1, 1) == -1 and ws(0, 1) == -1 and ws(4, -1) == -1
    assert ws(4, 70000) == -2
    assert ws(16, 0) == ws(16, 1)
    for T in (1, 5, 16, 64, 512, 2560, 2561, 3413, 3414, 4096):                # never above the typed pair's at f = 1
        for h in (1, 2, 8):
            n = ws(T, h)
            assert 0 < n <= 1024 * T * h and n % (T * h) == 0, (T, h, n)
    assert ws(16, 2) == 1024 * 16 * 2 and ws(4096, 1) == 512 * 4096            # the stated figures
    assert fused_gtconv.gt_tbias_dB_supported(4096, 8) and not fused_gtconv.gt_tbias_dB_supported(4097, 1)


def test_operators_and_layers_import():
    import argparse

    import fused_gtconv
    from DFGNN.layers import SparseMHA_tbias, load_graphconv_layer, load_prepfunc, preprocess_Hyper_fw_bw
    from DFGNN.layers.GT import SparseMHA_tbias_timing
    from DFGNN.operators.fused_gtconv import FusedGTFunction_tbias, GTConvFuse_inference_tbias, GTConvFuse_tbias
    for name in ("gt_inference_tbias", "gt_forward_tbias", "gt_backward_tbias", "gt_tbias_dB_supported"):
        assert callable(getattr(fused_gtconv, name))
    assert callable(GTConvFuse_tbias) and callable(GTConvFuse_inference_tbias) and hasattr(FusedGTFunction_tbias, "apply")
    args = argparse.Namespace(conv="gt", format="forward_tbias", dim=64, heads=2)
    layer = load_graphconv_layer(args)
    assert isinstance(layer, SparseMHA_tbias_timing) and layer.num_types == 16 and layer.rel_bias.shape == (16, 2)
    assert load_prepfunc(args) is preprocess_Hyper_fw_bw
    layer = SparseMHA_tbias(64, 64, 2, 5)
    assert layer.head_dim == 32 and layer.rel_bias.shape == (5, 2) and layer.rel_bias.requires_grad


# ---- the layer's torch branch and the tests' reference against the closed-form backward -----------------------------------
def _params(row_ptr, col_ind, rows, n_cols, val=None):
    """The 9-tuple of preprocess_Hyper_fw_bw / preprocess_block as CPU tensors."""
    col_ptr, row_ind, val_idx = csc_of(row_ptr, col_ind, rows, n_cols)
    ti = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32))  # noqa: E731
    val = torch.ones(len(col_ind), dtype=torch.float64) if val is None else torch.from_numpy(val)
    return (None, ti(rows), ti(row_ptr), ti(col_ind), val, ti(col_ptr), ti(row_ind), ti(val_idx), 0)


def _closed_form(row_ptr, col_ind, n_cols, val, etype, B, Q, K, V, dO):
    """The issue's equations, edge by edge in float64.  B: [T, h]; an edge whose B is -inf takes no part."""
    m, h, f = Q.shape
    out, dQ = np.zeros((m, h, f)), np.zeros((m, h, f))
    dK, dV, dB = np.zeros((n_cols, h, f)), np.zeros((n_cols, h, f)), np.zeros(B.shape)
    row_max, row_sum = np.full((m, h), -1e38), np.zeros((m, h))
    for i in range(m):
        for hd in range(h):
            es = [e for e in range(row_ptr[i], row_ptr[i + 1]) if B[etype[e], hd] != -np.inf]
            if not es:
                continue                                               # an empty or fully masked row: zeros everywhere
            c, t = col_ind[es], etype[es]
            s = val[es] * (K[c, hd] @ Q[i, hd]) + B[t, hd]
            row_max[i, hd] = s.max()
            p = np.exp(s - s.max())
            row_sum[i, hd] = p.sum()
            p /= p.sum()
            out[i, hd] = p @ V[c, hd]
            ds = p * (V[c, hd] @ dO[i, hd] - dO[i, hd] @ out[i, hd])
            dQ[i, hd] = (ds * val[es]) @ K[c, hd]
            np.add.at(dK[:, hd], c, (ds * val[es])[:, None] * Q[i, hd])
            np.add.at(dV[:, hd], c, p[:, None] * dO[i, hd])
            np.add.at(dB[:, hd], t, ds)
    return dict(out=out, row_max=row_max, row_sum=row_sum, dQ=dQ, dK=dK, dV=dV, dB=dB)


def _small_graph(rng, m, T):
    """A graph with an empty row and a duplicate edge; type 2 has no edge, type 1 covers row `full` entirely and row `part`
    in part (so B[1, hd] = -inf leaves one row fully and one partly masked)."""
    row_ptr, col_ind, rows = random_graph(rng, m, 4, empty_frac=0.1, dup_frac=0.1, max_deg=30)
    deg = np.diff(row_ptr)
    assert (deg == 0).any(), "the graph needs an empty row"
    assert any(len(set(col_ind[row_ptr[i]:row_ptr[i + 1]])) < deg[i] for i in range(m)), "the graph needs a duplicate edge"
    etype = rng.integers(0, T - 1, len(col_ind))
    etype[etype == 2] = T - 1                                          # type 2 has no edge, the last one has
    full, part = (int(i) for i in np.nonzero(deg >= 2)[0][:2])
    etype[row_ptr[full]:row_ptr[full + 1]] = 1
    etype[row_ptr[part]:row_ptr[part + 1]] = 0
    etype[row_ptr[part]] = 1
    assert (etype != 2).all() and (etype == T - 1).any()
    return row_ptr, col_ind, rows, etype, full, part


def _close(name, a, b):
    assert np.isfinite(a).all(), name
    assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), (name, np.abs(a - b).max())


@pytest.mark.parametrize("n_cols", [40, 55], ids=["square", "rect"])
def test_layer_torch_branch_matches_closed_form(n_cols):
    from DFGNN.layers import SparseMHA_tbias, preprocess_types
    rng = np.random.default_rng(5)
    m, heads, dim, T = 40, 2, 12, 6
    row_ptr, col_ind, rows, etype, _, _ = _small_graph(rng, m, T)
    val = rng.uniform(0.5, 1.5, len(col_ind))
    params = _params(row_ptr, col_ind, rows, n_cols, val)
    types = preprocess_types(params, torch.from_numpy(etype), T)
    torch.manual_seed(0)
    layer = SparseMHA_tbias(dim, dim, heads, T).double().train()
    x_rows = torch.randn(m, dim, dtype=torch.float64)
    x_cols = x_rows if n_cols == m else torch.randn(n_cols, dim, dtype=torch.float64)
    x = x_rows if n_cols == m else (x_cols, x_rows)
    dO = torch.randn(m, heads, dim // heads, dtype=torch.float64)
    q, k, v = (t.detach() for t in layer._qkv_fused(x))
    assert q.shape[0] == m and k.shape[0] == n_cols
    B = layer.rel_bias.detach()
    want = _closed_form(row_ptr, col_ind, n_cols, val, etype, B.numpy(), q.numpy(), k.numpy(), v.numpy(), dO.numpy())
    y = layer(params, x, types, fuse=False)
    assert y.shape == (m, dim)
    _close("out", y.detach().numpy().reshape(m, heads, -1), want["out"])
    (g_b,) = torch.autograd.grad(y, layer.rel_bias, dO.reshape(m, -1))
    _close("d rel_bias", g_b.numpy(), want["dB"])
    assert (g_b[2] == 0).all() and (g_b[T - 1] != 0).any()              # the type without an edge
    empty = np.diff(row_ptr) == 0
    assert (y.detach().numpy()[empty] == 0).all()


@pytest.mark.parametrize("n_cols", [30, 47, 21], ids=["square", "wide", "tall"])
def test_reference_matches_closed_form(n_cols):
    """tests/gt_tbias_cases.reference (the GPU tests' reference) against the closed form, without a mask and with type 1
    masked on head 0: one row fully masked (an empty row for that head), one partly."""
    rng = np.random.default_rng(6)
    m, h, f, T = 30, 2, 5, 6
    row_ptr, col_ind, rows, etype, full, part = _small_graph(rng, m, T)
    col_ind = col_ind % n_cols
    val = rng.uniform(0.5, 1.5, len(col_ind))
    Q, dO = (rng.standard_normal((m, h, f)) for _ in range(2))
    K, V = (rng.standard_normal((n_cols, h, f)) for _ in range(2))
    for masked in (False, True):
        B = rng.standard_normal((T, h))
        if masked:
            B[1, 0] = -np.inf
        ref = zc.reference(row_ptr, col_ind, n_cols, val, etype, B, Q, K, V, dO)
        want = _closed_form(row_ptr, col_ind, n_cols, val, etype, B, Q, K, V, dO)
        for name in zc.OUTPUTS:
            assert ref[name].shape == want[name].shape, name
            _close(name, ref[name], want[name])
        assert (ref["dB"][2] == 0).all()
        i = int(np.nonzero(np.diff(row_ptr) == 0)[0][0])
        assert (ref["row_max"][i] == zc.SENTINEL_MAX).all() and (ref["row_sum"][i] == 0).all()
        if masked:
            assert ref["dB"][1, 0] == 0 and ref["dB"][1, 1] != 0
            assert ref["row_max"][full, 0] == zc.SENTINEL_MAX and ref["row_sum"][full, 0] == 0
            assert (ref["out"][full, 0] == 0).all() and (ref["dQ"][full, 0] == 0).all() and (ref["out"][full, 1] != 0).any()
            assert ref["row_sum"][part, 0] > 0 and (ref["out"][part, 0] != 0).any()
            assert ref["dbias"][0, row_ptr[part]] == 0
