"""CPU: the GATv2 entry points (dfgnn_gatv2_fwd / dfgnn_gatv2_bwd / dfgnn_gatv2_bwd_ws_floats) are declared, exported, bound
and validate their arguments before any GPU call; the operators and layers import and resolve; the layers' non-fused
branch agrees in float64 with the closed-form backward the kernels implement (include/dfgnn.h)."""
import argparse
import ctypes
import os
import re
import types

import numpy as np
import torch

from conftest import ROOT, random_graph

NAMES = ("dfgnn_gatv2_bwd_ws_floats", "dfgnn_gatv2_fwd", "dfgnn_gatv2_bwd")


def test_symbols_declared_exported_and_bound():
    import dfgnn_native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfgnn.h")).read(), flags=re.S)
    raw = ctypes.CDLL(dfgnn_native.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), n
        assert hasattr(raw, n), n
        assert n in dfgnn_native.SIGNATURES
    assert [len(dfgnn_native.SIGNATURES[n]) for n in NAMES] == [2, 14, 22]
    assert dfgnn_native.lib().dfgnn_abi_version() == 11


def test_workspace_query():
    """The partials buffer of dattn depends on (h, f) only -- the query takes no m -- and is bounded by 4096 h f floats."""
    import dfgnn_native
    L = dfgnn_native.lib()
    assert L.dfgnn_gatv2_bwd_ws_floats(2, 16) > 0
    h, f = 1, 8
    assert 0 < L.dfgnn_gatv2_bwd_ws_floats(h, f) <= 4096 * h * f
    assert L.dfgnn_gatv2_bwd_ws_floats(h, f) == L.dfgnn_gatv2_bwd_ws_floats(h, f)
    assert L.dfgnn_gatv2_bwd_ws_floats(-1, 8) == -1
    assert L.dfgnn_gatv2_bwd_ws_floats(70000, 8) == -2
    assert L.dfgnn_gatv2_bwd_ws_floats(65535, 1024) == -2          # does not fit an int: never a wrapped positive size


def test_argument_checks_need_no_gpu():
    """A missing pointer is DFGNN_E_BADARG, an empty problem succeeds, too many heads is DFGNN_E_UNSUPPORTED: all answered
    before any launch."""
    import dfgnn_native
    L = dfgnn_native.lib()
    buf, buf2 = (ctypes.c_float * 64)(), (ctypes.c_float * 64)()
    idx = (ctypes.c_int * 8)(0, 1, 2, 2, 0, 0, 0, 0)
    p, p2, i = ctypes.addressof(buf), ctypes.addressof(buf2), ctypes.addressof(idx)

    def fwd(m, X_row, mx=p, sm=p, h=1):
        return L.dfgnn_gatv2_fwd(m, 2, h, 4, i, i, p, 0.2, X_row, p, mx, sm, p, None)

    def bwd(m, X_row, delta=p, ws=p, h=1):
        return L.dfgnn_gatv2_bwd(m, 2, h, 4, i, i, i, i, p, 0.2, X_row, p, p, p, p, p, delta, ws, p, p2, p, None)

    assert fwd(3, None) == -1 and bwd(3, None) == -1
    assert fwd(3, p, mx=None) == -1 and fwd(3, p, sm=None) == -1      # one statistic without the other
    assert bwd(3, p, ws=None) == -1 and bwd(3, p, delta=None) == -1
    assert fwd(-1, p) == -1 and bwd(-1, p) == -1
    assert fwd(0, p) == 0 and bwd(0, p) == 0
    assert fwd(0, None) == 0 and bwd(0, None) == 0
    assert fwd(3, p, h=70000) == -2 and bwd(3, p, h=70000) == -2


def test_surface_imports_and_resolves():
    import fused_gatconv
    from DFGNN.layers import (GATv2Conv_forward, GATv2Conv_tiling, GATv2ConvDGL, load_graphconv_layer, load_prepfunc,
                              preprocess_CSR, preprocess_Hyper_fw_bw)
    from DFGNN.layers.GATv2 import GATv2Conv_forward as F2, GATv2Conv_tiling as T2
    from DFGNN.operators.fused_gatconv import FusedGATv2Function, GATv2ConvFuse, GATv2ConvFuse_inference
    assert F2 is GATv2Conv_forward and T2 is GATv2Conv_tiling
    for fn in (fused_gatconv.gatv2_inference, fused_gatconv.gatv2_forward, fused_gatconv.gatv2_backward, GATv2ConvFuse,
               GATv2ConvFuse_inference):
        assert callable(fn)
    assert hasattr(FusedGATv2Function, "apply")
    for fmt, cls, prep in (("tiling", GATv2Conv_tiling, preprocess_CSR), ("csr", GATv2Conv_tiling, preprocess_CSR),
                           ("forward", GATv2Conv_forward, preprocess_Hyper_fw_bw)):
        args = argparse.Namespace(conv="gatv2", format=fmt, dim=64, heads=2)
        layer = load_graphconv_layer(args)
        assert type(layer) is cls and isinstance(layer, GATv2ConvDGL)
        assert load_prepfunc(args) is prep
        assert tuple(layer.attn.shape) == (2, 64) and layer.fc_row is not layer.fc_col
    shared = GATv2ConvDGL(8, 4, 3, share_weights=True)
    assert shared.fc_row is shared.fc_col and len(list(shared.parameters())) == 3


def _closed_form(row, col, n, attn, slope, xr, xc, dO):
    """float64 numpy: out, dX_row, dX_col, dattn by the formulas of include/dfgnn.h, edge by edge sums with np.add.at."""
    z = xr[row] + xc[col]                                          # [E, h, f]
    lr = np.where(z > 0, z, slope * z)
    s = (lr * attn).sum(-1)                                        # [E, h]
    mx = np.full((n, s.shape[1]), -np.inf)
    np.maximum.at(mx, row, s)
    p = np.exp(s - mx[row])
    den = np.zeros_like(mx)
    np.add.at(den, row, p)
    P = p / den[row]
    out = np.zeros_like(xr)
    np.add.at(out, row, P[:, :, None] * xc[col])
    delta = (dO * out).sum(-1)                                     # [n, h]
    dP = (dO[row] * xc[col]).sum(-1)
    dS = P * (dP - delta[row])
    g = dS[:, :, None] * attn * np.where(z > 0, 1.0, slope)
    dxr, dxc = np.zeros_like(xr), np.zeros_like(xc)
    np.add.at(dxr, row, g)
    np.add.at(dxc, col, P[:, :, None] * dO[row] + g)
    return out, dxr, dxc, (dS[:, :, None] * lr).sum(0)


def test_nonfused_branch_matches_closed_form_backward():
    """The layers' torch branch (autograd, float64) against the closed-form backward on a 97-node graph with empty rows and
    columns, duplicate edges and a 70-edge row.  Both are float64: they agree to rounding (1e-10 of the largest value)."""
    from DFGNN.layers import GATv2ConvDGL
    rng = np.random.default_rng(97)
    m, h, f, slope = 97, 3, 5, 0.2
    indptr, indices, rows = random_graph(rng, m, 2.8, empty_frac=0.2, dup_frac=0.1, max_deg=70)
    indices[indices == 11] = 12                                     # an empty column for certain
    deg, indeg = np.diff(indptr), np.bincount(indices, minlength=m)
    assert (deg == 0).any() and (indeg == 0).any() and deg.max() == 70
    assert (np.diff(indices)[np.diff(rows) == 0] == 0).any()        # a duplicate edge
    A = types.SimpleNamespace(row=torch.from_numpy(rows.astype(np.int64)), col=torch.from_numpy(indices.astype(np.int64)))
    torch.manual_seed(5)
    layer = GATv2ConvDGL(6, f, h, negative_slope=slope).double()
    xr = torch.randn(m, h, f, dtype=torch.float64, requires_grad=True)
    xc = torch.randn(m, h, f, dtype=torch.float64, requires_grad=True)
    dO = torch.randn(m, h, f, dtype=torch.float64)
    out = layer.conv_nofuse(A, xr, xc)
    g_xr, g_xc, g_attn = torch.autograd.grad(out, (xr, xc, layer.attn), dO)
    want = _closed_form(rows, indices, m, layer.attn.detach().numpy(), slope, xr.detach().numpy(), xc.detach().numpy(),
                        dO.numpy())
    for name, got, ref in zip(("out", "dX_row", "dX_col", "dattn"), (out, g_xr, g_xc, g_attn), want):
        err = float(np.abs(got.detach().numpy() - ref).max())
        print(f"gatv2 nofuse vs closed form {name}: max abs err {err:.3e}")
        assert err < 1e-10 * max(1.0, float(np.abs(ref).max())), (name, err)
    assert (out.detach().numpy()[deg == 0] == 0).all() and (want[1][deg == 0] == 0).all() and (want[2][indeg == 0] == 0).all()
    # the whole layer: shared weights feed one tensor to both sides and its gradient is the sum
    shared = GATv2ConvDGL(6, f, h, negative_slope=slope, share_weights=True).double()
    feat = torch.randn(m, 6, dtype=torch.float64)
    x = shared.fc_row(feat).view(-1, h, f)
    o = shared.forward_nofuse(A, feat)
    (o * dO).sum().backward()
    w = _closed_form(rows, indices, m, shared.attn.detach().numpy(), slope, x.detach().numpy(), x.detach().numpy(), dO.numpy())
    dx = torch.from_numpy(w[1] + w[2]).reshape(m, h * f)
    assert torch.allclose(shared.fc_row.weight.grad, dx.t() @ feat, rtol=0, atol=1e-9)
    assert torch.allclose(shared.attn.grad, torch.from_numpy(w[3]), rtol=0, atol=1e-9)
