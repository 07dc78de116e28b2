"""CPU: the GATv2 pair with per-edge feature vectors inside the LeakyReLU (dfgnn_gatv2_fwd_edge / dfgnn_gatv2_bwd_edge and
their *_rect forms; csrc/gatv2_edge_train.hip) is declared, exported, bound and validates its arguments before any GPU call;
the operators and layers import; `--conv gatv2 --format forward_edge` resolves; and the layer's index-op branch agrees with
an independent float64 restatement of the formulas, edge by edge."""
import ctypes
import os
import re

import numpy as np
import torch

from conftest import ROOT, random_graph

SLOPE = 0.2
ARITY = {"dfgnn_gatv2_fwd_edge": 15, "dfgnn_gatv2_bwd_edge": 25, "dfgnn_gatv2_fwd_edge_rect": 16,
         "dfgnn_gatv2_bwd_edge_rect": 26}


def _header_arity(text, name):
    args = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", text, flags=re.S).group(1)
    return len(args.split(","))


def test_symbols_declared_exported_and_bound():
    import dfgnn_native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfgnn.h")).read(), flags=re.S)
    raw = ctypes.CDLL(dfgnn_native.LIB_PATH)
    for n, arity in ARITY.items():
        assert _header_arity(text, n) == arity, n
        assert hasattr(raw, n), n
        assert len(dfgnn_native.SIGNATURES[n]) == arity, n
    assert dfgnn_native.lib().dfgnn_abi_version() == 11
    ext_src = open(os.path.join(ROOT, "df-gnn_amd", "csrc", "torch_ext.cpp")).read()
    for n in ("gatv2_fwd_edge", "gatv2_bwd_edge"):                     # the torch-extension transport binds both
        assert re.search(r'm\.def\("' + n + r'",\s*&' + n + r"\b", ext_src), n


def test_argument_checks_need_no_gpu():
    """Every check of the entry points is answered before any launch."""
    import dfgnn_native
    L = dfgnn_native.lib()
    buf = (ctypes.c_float * 64)()
    idx = (ctypes.c_int * 8)(0, 1, 2, 2, 0, 0, 0, 0)
    p, i = ctypes.addressof(buf), ctypes.addressof(idx)

    def fwd(m=3, nnz=2, h=1, f=4, row_ptr=i, col_ind=i, attn=p, X_row=p, X_col=p, E=p, mx=p, sm=p, out=p, rect=False):
        if rect:
            return L.dfgnn_gatv2_fwd_edge_rect(m, m, nnz, h, f, row_ptr, col_ind, attn, SLOPE, X_row, X_col, E, mx, sm, out, None)
        return L.dfgnn_gatv2_fwd_edge(m, nnz, h, f, row_ptr, col_ind, attn, SLOPE, X_row, X_col, E, mx, sm, out, None)

    def bwd(m=3, nnz=2, h=1, f=4, row_ptr=i, col_ind=i, col_ptr=i, row_ind=i, val_idx=i, attn=p, X_row=p, X_col=p, E=p, out=p,
            mx=p, sm=p, grad=p, delta=p, ws=p, dX_row=p, dX_col=p + 128, dattn=p, dE=p, rect=False):
        a = (row_ptr, col_ind, col_ptr, row_ind, val_idx, attn, SLOPE, X_row, X_col, E, out, mx, sm, grad, delta, ws, dX_row,
             dX_col, dattn, dE, None)
        if rect:
            return L.dfgnn_gatv2_bwd_edge_rect(m, m, nnz, h, f, *a)
        return L.dfgnn_gatv2_bwd_edge(m, nnz, h, f, *a)

    for rect in (False, True):
        for fn in (fwd, bwd):
            assert fn(m=-1, rect=rect) == -1 and fn(nnz=-1, rect=rect) == -1
            assert fn(row_ptr=None, rect=rect) == -1 and fn(col_ind=None, rect=rect) == -1
            for name in ("attn", "X_row", "X_col", "out"):
                assert fn(**{name: None}, rect=rect) == -1, (fn.__name__, name)
            assert fn(E=None, rect=rect) == -1                          # E == NULL with nnz > 0
            assert fn(h=70000, rect=rect) == -2                         # h > 65535
        assert fwd(mx=None, rect=rect) == -1 and fwd(sm=None, rect=rect) == -1   # one statistic without the other
        assert fwd(m=0, rect=rect) == 0
        for name in ("delta", "ws", "col_ptr", "row_ind", "val_idx", "grad", "mx", "sm", "dX_row", "dX_col", "dattn"):
            assert bwd(**{name: None}, rect=rect) == -1, name
        assert bwd(dX_col=p, rect=rect) == -1                           # dX_row and dX_col are distinct buffers
        assert bwd(h=4096, f=1024, rect=rect) == -2                     # the workspace does not fit an int: as dfgnn_gatv2_bwd


def test_operators_and_layers_import():
    import argparse

    import fused_gatconv
    from DFGNN.layers import GATv2Conv_edge, load_graphconv_layer, load_prepfunc, preprocess_Hyper_fw_bw
    from DFGNN.layers.GATv2 import GATv2Conv_edge_timing
    from DFGNN.operators.fused_gatconv import FusedGATv2Function_edge, GATv2ConvFuse_edge, GATv2ConvFuse_inference_edge
    for name in ("gatv2_inference_edge", "gatv2_forward_edge", "gatv2_backward_edge"):
        assert callable(getattr(fused_gatconv, name))
    assert callable(GATv2ConvFuse_edge) and callable(GATv2ConvFuse_inference_edge)
    assert hasattr(FusedGATv2Function_edge, "apply")
    args = argparse.Namespace(conv="gatv2", format="forward_edge", dim=64, heads=2)
    assert isinstance(load_graphconv_layer(args), GATv2Conv_edge_timing)
    assert load_prepfunc(args) is preprocess_Hyper_fw_bw
    layer = GATv2Conv_edge(24, 8, 3, edge_dim=5)
    assert layer.lin_edge.weight.shape == (24, 5) and layer.lin_edge.bias is None
    assert GATv2Conv_edge(24, 8, 3).lin_edge.weight.shape == (24, 24)      # edge_dim defaults to in_size
    shared = GATv2Conv_edge(24, 8, 3, share_weights=True, edge_dim=5)
    assert shared.fc_col is shared.fc_row and len(list(shared.parameters())) == 4


# ---- the layer's index-op branch against the formulas, edge by edge ---------------------------------------------------------
def _closed_form(row_ptr, col_ind, a, Xr, Xc, E, dO):
    """The equations of include/dfgnn.h in float64, one (row, head) at a time.  E: [nnz, h, f]."""
    m, h, f = Xr.shape
    out, dXr, dXc = np.zeros((m, h, f)), np.zeros((m, h, f)), np.zeros_like(Xc)
    dE, da = np.zeros_like(E), np.zeros((h, f))
    for i in range(m):
        lo, hi = row_ptr[i], row_ptr[i + 1]
        if hi == lo:
            continue                                                   # an empty row: zeros everywhere
        for hd in range(h):
            xc = Xc[col_ind[lo:hi], hd]
            z = Xr[i, hd] + xc + E[lo:hi, hd]
            lz = np.where(z > 0, z, SLOPE * z)
            s = lz @ a[hd]
            p = np.exp(s - s.max())
            p /= p.sum()
            out[i, hd] = p @ xc
            ds = p * (xc @ dO[i, hd] - dO[i, hd] @ out[i, hd])
            g = ds[:, None] * a[hd] * np.where(z > 0, 1.0, SLOPE)
            dXr[i, hd] = g.sum(0)
            np.add.at(dXc[:, hd], col_ind[lo:hi], p[:, None] * dO[i, hd] + g)
            da[hd] += ds @ lz
            dE[lo:hi, hd] = g
    return out, dXr, dXc, da, dE


def test_layer_index_op_branch_matches_closed_form():
    from DFGNN.layers import GATv2Conv_edge
    from DFGNN.layers.GATv2.gatv2conv_layers import index_ops_gatv2_edge
    rng = np.random.default_rng(5)
    m, heads, f, in_dim, edge_dim = 40, 2, 5, 12, 3
    row_ptr, col_ind, rows = random_graph(rng, m, 4, empty_frac=0.1, dup_frac=0.1, max_deg=30)
    deg = np.diff(row_ptr)
    assert (deg == 0).any(), "the graph needs an empty row"
    assert any(len(set(col_ind[row_ptr[i]:row_ptr[i + 1]])) < deg[i] for i in range(m)), "the graph needs a duplicate edge"
    nnz = len(col_ind)
    tt = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dt)  # noqa: E731
    params = (None, tt(rows, torch.int32), tt(row_ptr, torch.int32), tt(col_ind, torch.int32), None, None, None, None, 0)
    torch.manual_seed(0)
    layer = GATv2Conv_edge(in_dim, f, heads, negative_slope=SLOPE, edge_dim=edge_dim).double().train()
    x = torch.randn(m, in_dim, dtype=torch.float64)
    edge_attr = torch.randn(nnz, edge_dim, dtype=torch.float64)
    dO = torch.randn(m, heads, f, dtype=torch.float64)
    xr, xc = (t.detach() for t in layer.project(x))
    e = layer.lin_edge(edge_attr).view(nnz, heads, f).detach()
    a = layer.attn.detach()
    want = _closed_form(row_ptr, col_ind, a.numpy(), xr.numpy(), xc.numpy(), e.numpy(), dO.numpy())
    # the function of (x_row, x_col, attn, e) ...
    xrg, xcg, ag, eg = (t.clone().requires_grad_(True) for t in (xr, xc, a, e))
    out = index_ops_gatv2_edge(params[1], params[3], ag, SLOPE, xrg, xcg, eg)
    grads = torch.autograd.grad(out, (xrg, xcg, ag, eg), dO)
    got = [out.detach().numpy()] + [t.numpy() for t in grads]
    for name, g_, w_ in zip(("out", "dX_row", "dX_col", "dattn", "dE"), got, want):
        assert np.isfinite(g_).all(), name
        assert np.abs(g_ - w_).max() <= 1e-12 * max(1.0, np.abs(w_).max()), (name, np.abs(g_ - w_).max())
    empty = deg == 0
    assert (got[0][empty] == 0).all() and (got[1][empty] == 0).all()
    # ... and the layer around it: the gradient of lin_edge's weight is dE^T edge_attr
    y = layer(params, x, edge_attr, fuse=False)
    assert y.shape == (m, heads * f) and np.abs(y.detach().numpy().reshape(m, heads, f) - want[0]).max() <= 1e-12
    (gw,) = torch.autograd.grad(y, layer.lin_edge.weight, dO.reshape(m, -1))
    want_w = want[4].reshape(nnz, heads * f).T @ edge_attr.numpy()
    assert np.abs(gw.numpy() - want_w).max() <= 1e-12 * max(1.0, np.abs(want_w).max())
    # E = 0: the plain layer's arithmetic
    plain = layer.conv_nofuse(type("A", (), dict(row=params[1], col=params[3]))(), xr, xc)
    zero = index_ops_gatv2_edge(params[1], params[3], a, SLOPE, xr, xc, torch.zeros_like(e))
    assert np.abs((plain - zero).detach().numpy()).max() <= 1e-12
