"""CPU: the GatedGCN pair (dfgnn_gatedgcn_fwd / dfgnn_gatedgcn_bwd and their _rect forms) is declared, exported, bound and
validates its arguments before any GPU call; the operators and layers import; the layer's torch branch and the GPU tests'
reference agree with the closed-form equations; and the power condition of tests/test_parity_cases_host.py holds for the
fp32-level cases that tests/test_gpu_gatedgcn.py runs (tests/gatedgcn_cases.py builds them), in both modes: losing one
boundary edge moves out, den, dX_row, Z and dE of every test row -- transposed: dX_col and dV of every test column -- by at
least POWER x bound."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gatedgcn_cases as gc
import parity_cases as pc
from conftest import ROOT, random_graph

NAMES = ("dfgnn_gatedgcn_fwd", "dfgnn_gatedgcn_bwd", "dfgnn_gatedgcn_fwd_rect", "dfgnn_gatedgcn_bwd_rect")
SEEN = set()


def test_symbols_declared_exported_and_bound():
    import dfgnn_native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfgnn.h")).read(), flags=re.S)
    raw = ctypes.CDLL(dfgnn_native.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), n
        assert hasattr(raw, n), n
        assert n in dfgnn_native.SIGNATURES
    assert len(dfgnn_native.SIGNATURES["dfgnn_gatedgcn_fwd"]) == 16
    assert len(dfgnn_native.SIGNATURES["dfgnn_gatedgcn_bwd"]) == 25
    assert len(dfgnn_native.SIGNATURES["dfgnn_gatedgcn_fwd_rect"]) == 17
    assert len(dfgnn_native.SIGNATURES["dfgnn_gatedgcn_bwd_rect"]) == 26
    assert dfgnn_native.lib().dfgnn_abi_version() == 11
    ext_src = open(os.path.join(ROOT, "df-gnn_amd", "csrc", "torch_ext.cpp")).read()
    for n in ("gatedgcn_fwd", "gatedgcn_bwd"):                              # the torch-extension transport binds both
        assert re.search(r'm\.def\("' + n + r'",\s*&' + n + r"\b", ext_src), n
    binding = open(os.path.join(ROOT, "df-gnn_amd", "fused_gtconv.py")).read()
    for n in ("dfgnn_gatedgcn_fwd_rect", "dfgnn_gatedgcn_bwd_rect", "ext.gatedgcn_fwd", "ext.gatedgcn_bwd"):
        assert n in binding, n                                              # the Python binding goes through both transports


def test_argument_checks_need_no_gpu():
    """Every check of the entry points is answered before any launch."""
    import dfgnn_native
    L = dfgnn_native.lib()
    buf = [(ctypes.c_float * 64)() for _ in range(3)]
    idx = (ctypes.c_int * 8)(0, 1, 2, 2, 0, 0, 0, 0)
    p, p2, p3 = (ctypes.addressof(b) for b in buf)
    i = ctypes.addressof(idx)

    def fwd(m=3, nnz=2, h=1, row_ptr=i, col_ind=i, X_row=p, X_col=p, V=p, E=p, normalize=1, eps=1e-6, den=p, out=p, Z=p,
            rect=False, f=4):
        if rect:
            return L.dfgnn_gatedgcn_fwd_rect(m, m, nnz, h, f, row_ptr, col_ind, X_row, X_col, V, E, normalize, eps, den, out, Z,
                                             None)
        return L.dfgnn_gatedgcn_fwd(m, nnz, h, f, row_ptr, col_ind, X_row, X_col, V, E, normalize, eps, den, out, Z, None)

    def bwd(m=3, nnz=2, h=1, row_ptr=i, col_ind=i, col_ptr=i, row_ind=i, val_idx=i, X_row=p, X_col=p, V=p, E=p, normalize=1,
            eps=1e-6, out=p, den=p, grad=p, G=p, dX_row=p, dX_col=p2, dV=p3, dE=p, ws=p, rect=False, f=4):
        args = (row_ptr, col_ind, col_ptr, row_ind, val_idx, X_row, X_col, V, E, normalize, eps, out, den, grad, G, dX_row,
                dX_col, dV, dE, ws, None)
        if rect:
            return L.dfgnn_gatedgcn_bwd_rect(m, m, nnz, h, f, *args)
        return L.dfgnn_gatedgcn_bwd(m, nnz, h, f, *args)

    wide = dict(f=2000)   # above every compiled lane layout: a call that passes the argument checks answers UNSUPPORTED
    for rect in (False, True):
        for base in (fwd, bwd):
            fn = lambda base=base, **kw: base(rect=rect, **kw)  # noqa: E731
            assert fn(m=-1) == -1 and fn(nnz=-1) == -1                      # check_rect
            assert fn(row_ptr=None) == -1 and fn(col_ind=None) == -1
            for name in ("X_row", "X_col", "V"):                            # a missing feature pointer
                assert fn(**{name: None}) == -1, (base.__name__, name)
                assert fn(**{name: None}, **wide) == -1, (base.__name__, name)
            assert fn(normalize=2) == -1 and fn(eps=-1.0) == -1 and fn(eps=float("nan")) == -1
            assert fn(h=70000) == -2                                        # h > 65535
            assert fn(m=0) == 0 and fn(m=0, X_row=None, E=None) == 0        # an empty problem succeeds
            assert fn(**wide) == -2
            assert fn(E=None, **wide) == -2                                 # E is optional
            for nz in (0, 1):
                assert fn(normalize=nz, **wide) == -2
        assert fwd(out=None, rect=rect) == -1
        assert fwd(den=None, rect=rect, **wide) == -2 and fwd(Z=None, rect=rect, **wide) == -2
        assert fwd(den=None, Z=None, E=None, rect=rect, **wide) == -2
        for name in ("col_ptr", "row_ind", "val_idx", "grad", "dX_row", "dX_col", "dV"):
            assert bwd(rect=rect, **{name: None}) == -1, name
            assert bwd(rect=rect, **{name: None}, **wide) == -1, name
        assert bwd(G=None, rect=rect, **wide) == -2 and bwd(dE=None, rect=rect, **wide) == -2
        assert bwd(E=None, G=None, dE=None, rect=rect, **wide) == -2
        for name in ("out", "den", "ws"):                                   # read with normalize = 1 only
            assert bwd(rect=rect, **{name: None}) == -1, name
            assert bwd(rect=rect, normalize=0, **{name: None}, **wide) == -2, name
        assert bwd(rect=rect, normalize=0, out=None, den=None, ws=None, **wide) == -2
        assert bwd(rect=rect, dX_col=p) == -1 and bwd(rect=rect, dV=p) == -1 and bwd(rect=rect, dV=p2) == -1   # one buffer twice


def test_operators_and_layers_import():
    import argparse

    import fused_gtconv
    from DFGNN.layers import GatedGCNConv, index_ops_gatedgcn, load_graphconv_layer, load_prepfunc, preprocess_Hyper_fw_bw
    from DFGNN.layers.GatedGCN import GatedGCNConv_plain_timing, GatedGCNConv_timing
    from DFGNN.layers.util import _GATEDGCN_LAYERS
    from DFGNN.operators.fused_gtconv import FusedGatedGCNFunction, GatedGCNConvFuse, GatedGCNConvFuse_inference
    for name in ("gatedgcn_inference", "gatedgcn_forward", "gatedgcn_backward"):
        assert callable(getattr(fused_gtconv, name))
    assert callable(GatedGCNConvFuse) and callable(GatedGCNConvFuse_inference) and hasattr(FusedGatedGCNFunction, "apply")
    assert callable(index_ops_gatedgcn) and set(_GATEDGCN_LAYERS) == {"forward", "forward_plain"}
    for fmt, cls in (("forward", GatedGCNConv_timing), ("forward_plain", GatedGCNConv_plain_timing)):
        args = argparse.Namespace(conv="gatedgcn", format=fmt, dim=64, heads=2)
        assert isinstance(load_graphconv_layer(args), cls)
        assert load_prepfunc(args) is preprocess_Hyper_fw_bw
    layer = GatedGCNConv(64, 64, 2, edge_dim=5)
    assert layer.head_dim == 32 and layer.lin_edge.weight.shape == (64, 5) and layer.lin_edge.bias is None
    assert layer.normalize and layer.edge_out and layer.eps == 1e-6
    maps = [layer.lin_self, layer.lin_msg, layer.lin_row, layer.lin_col, layer.lin_edge]
    assert len({id(x) for x in maps}) == 5 and all(x.weight.shape[0] == 64 for x in maps)
    assert not GatedGCNConv(64, 64, 2, normalize=False, edge_out=False).edge_out


# ---- the closed form --------------------------------------------------------------------------------------------------
def _closed_form(row_ptr, col_ind, E, G, X_row, X_col, V, dO, normalize, eps):
    """The operator's equations, edge by edge in float64.  E, G: [nnz, h, f].  -> out, den, Z, dX_row, dX_col, dV, dE."""
    m = X_row.shape[0]
    out, den, dXr = (np.zeros_like(X_row) for _ in range(3))
    dXc, dV = np.zeros_like(X_col), np.zeros_like(V)
    Z, dE = np.zeros_like(E), np.zeros_like(E)
    sig = lambda x: 1.0 / (1.0 + np.exp(-x))  # noqa: E731
    for i in range(m):
        for e in range(row_ptr[i], row_ptr[i + 1]):
            Z[e] = X_row[i] + X_col[col_ind[e]] + E[e]
            den[i] += sig(Z[e])
            out[i] += sig(Z[e]) * V[col_ind[e]]
        if normalize:
            out[i] /= den[i] + eps
    for i in range(m):
        for e in range(row_ptr[i], row_ptr[i + 1]):
            j, sg = col_ind[e], sig(Z[e])
            if normalize:
                dsg = dO[i] * (V[j] - out[i]) / (den[i] + eps)
                dV[j] += sg * dO[i] / (den[i] + eps)
            else:
                dsg = dO[i] * V[j]
                dV[j] += sg * dO[i]
            g = dsg * sg * (1 - sg) + G[e]
            dXr[i] += g
            dXc[j] += g
            dE[e] = g
    return out, den, Z, dXr, dXc, dV, dE


def _close(a, b, what):
    assert np.isfinite(a).all(), what
    assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), (what, np.abs(a - b).max())


def _small_graph(rng, m):
    row_ptr, col_ind, rows = random_graph(rng, m, 4, empty_frac=0.1, dup_frac=0.1, max_deg=30)
    deg = np.diff(row_ptr)
    assert (deg == 0).any(), "the graph needs an empty row"
    dup = any(len(set(col_ind[row_ptr[i]:row_ptr[i + 1]])) < deg[i] for i in range(m))
    assert dup, "the graph needs a duplicate edge"
    return row_ptr, col_ind, rows


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("with_E", [True, False])
def test_layer_torch_branch_matches_closed_form(normalize, with_E):
    from DFGNN.layers import GatedGCNConv, index_ops_gatedgcn
    rng = np.random.default_rng(5)
    m, heads, dim, edge_dim = 40, 2, 12, 5
    row_ptr, col_ind, rows = _small_graph(rng, m)
    nnz = len(col_ind)
    tt = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dt)  # noqa: E731
    params = (None, tt(rows, torch.int32), tt(row_ptr, torch.int32), tt(col_ind, torch.int32), None, None, None, None, 0)
    torch.manual_seed(0)
    layer = GatedGCNConv(dim, dim, heads, edge_dim=edge_dim, normalize=normalize).double().train()
    x = torch.randn(m, dim, dtype=torch.float64)
    edge_attr = torch.randn(nnz, edge_dim, dtype=torch.float64)
    dO = torch.randn(m, heads, dim // heads, dtype=torch.float64)
    G = torch.randn(nnz, heads, dim // heads, dtype=torch.float64)
    own, xr, xc, v = (t.detach() for t in layer.project(x))
    e = layer.lin_edge(edge_attr).view(nnz, heads, dim // heads).detach() if with_E else torch.zeros_like(G)
    want = _closed_form(row_ptr, col_ind, e.numpy(), G.numpy(), xr.numpy(), xc.numpy(), v.numpy(), dO.numpy(), normalize,
                        layer.eps)
    # the function of (x_row, x_col, v, e) ...
    xrg, xcg, vg, eg = (t.clone().requires_grad_(True) for t in (xr, xc, v, e))
    out, z = index_ops_gatedgcn(params[1], params[3], xrg, xcg, vg, eg if with_E else None, normalize, layer.eps)
    grads = torch.autograd.grad((out, z), (xrg, xcg, vg) + ((eg,) if with_E else ()), (dO, G))
    got = [out.detach().numpy(), z.detach().numpy()] + [t.numpy() for t in grads]
    for name, a, b in zip(("out", "Z", "dX_row", "dX_col", "dV", "dE"), got, (want[0],) + want[2:]):
        _close(a, b, name)
    empty = np.diff(row_ptr) == 0
    assert (got[0][empty] == 0).all() and (got[2][empty] == 0).all()
    # ... and the layer around it: h_out = self term + aggregate, e_out = Z; the gradient of lin_edge's weight is dE^T edge_attr
    y, e_out = layer(params, x, edge_attr if with_E else None, fuse=False)
    assert y.shape == (m, dim) and e_out.shape == (nnz, dim)
    _close((y - own).detach().numpy().reshape(m, heads, -1), want[0], "layer h_out")
    _close(e_out.detach().numpy().reshape(nnz, heads, -1), want[2], "layer e_out")
    if with_E:
        (gw,) = torch.autograd.grad((y, e_out), layer.lin_edge.weight, (dO.reshape(m, -1), G.reshape(nnz, -1)))
        _close(gw.numpy(), want[6].reshape(nnz, dim).T @ edge_attr.numpy(), "lin_edge.weight gradient")
    y2, none = GatedGCNConv(dim, dim, heads, edge_dim=edge_dim, edge_out=False).double()(params, x, edge_attr, fuse=False)
    assert none is None and y2.shape == (m, dim)


@pytest.mark.parametrize("normalize", [1, 0])
@pytest.mark.parametrize("with_E", [True, False])
@pytest.mark.parametrize("with_G", [True, False])
def test_reference_matches_closed_form(normalize, with_E, with_G):
    """tests/gatedgcn_cases.reference (the GPU tests' reference) against the closed form; E / G = None are zeros."""
    rng = np.random.default_rng(6)
    m, h, f = 30, 2, 5
    row_ptr, col_ind, rows = _small_graph(rng, m)
    nnz = len(col_ind)
    E, G = (rng.standard_normal((nnz, h, f)) for _ in range(2))
    X_row, X_col, V, dO = (rng.standard_normal((m, h, f)) for _ in range(4))
    ref = gc.reference(row_ptr, col_ind, E if with_E else None, G if with_G else None, X_row, X_col, V, dO, normalize, 1e-6)
    want = _closed_form(row_ptr, col_ind, E if with_E else np.zeros_like(E), G if with_G else np.zeros_like(G), X_row, X_col,
                        V, dO, normalize, 1e-6)
    for name, b in zip(gc.OUTPUTS, want):
        _close(ref[name], b, name)
    empty = np.diff(row_ptr) == 0
    assert (ref["out"][empty] == 0).all() and (ref["den"][empty] == 0).all() and (ref["dX_row"][empty] == 0).all()


# ---- the power condition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", gc.MODES)
@pytest.mark.parametrize("case", pc.case_ids("gt"), ids=str)
def test_power_gatedgcn(case, normalize):
    """Z_e depends on its own edge alone, and so does dE_e without normalize, so neither moves on the edges that stay when an
    edge is lost; what a kernel that loses an edge gets wrong is that edge's slot.  Both are therefore compared in the layout
    of the full graph, the lost edge's slot holding zeros (nothing written).  With normalize the dE of the edges that stay
    moves too, through den and out, but by less than the float32 error where G sets the size of dE (measured: 0.1 x the
    bound at 32 features); the lost slot is what shows, so dE is compared in the full layout in both modes."""
    g = pc.graph(case[0], case[1])
    x, ref64, bounds = gc.boundary_references(case, normalize)
    names = gc.COL_SIDE if g["transposed"] else gc.ROW_SIDE
    report = {}
    for mut, slots in pc.mutations(g).items():
        assert len(slots) == len(g["mutate"]) > 0
        row_ptr, col_ind, keep = pc.drop_slots(g, slots)
        assert keep.sum() == g["nnz"] - len(slots)
        moved = gc.mutated_reference(case, x, keep, row_ptr, col_ind, normalize)
        for name in names:
            if name in gc.PER_EDGE:
                full, rp_full = gc.edge_rows(ref64[name], g["row_ptr"])
                lost = np.zeros_like(ref64[name])
                lost[keep] = moved[name]
                e = pc.row_errors(gc.edge_rows(lost, g["row_ptr"])[0], full, rp_full)
            else:
                e = pc.row_errors(moved[name], ref64[name])
            e = e[g["mutate"]]
            fp32 = bounds[name] / pc.MARGIN
            assert fp32 > 0, (case, name)
            report[(mut, name)] = (float(e.min()), bounds[name], float(e.min()) / fp32)
    for (mut, name), (move, bound, ratio) in report.items():
        print(f"power gatedgcn {case} normalize={normalize} {mut} {name}: least move {move:.3e}, bound {bound:.3e}, "
              f"move / bound {move / bound:.1f}, move / fp32 error {ratio:.1f}")
    for (mut, name), (move, bound, ratio) in report.items():
        assert move >= pc.POWER * bound, (case, normalize, mut, name, move, bound)
    SEEN.add((case, normalize))


def test_zz_no_case_was_skipped(request):
    """Runs last in this module: all 32 cases went through the condition in both modes (when the whole module ran)."""
    wanted = {(c, n) for c in pc.case_ids("gt") for n in gc.MODES}
    assert len(wanted) == 64
    selected = [i.name for i in request.session.items if i.module is request.module and i.name.startswith("test_power")]
    if len(selected) == len(wanted):           # (a -k selection of single cases is not a skipped case)
        assert SEEN == wanted, sorted(wanted - SEEN)
