"""CPU: the AGNN / dot-product entry points with tied keys and values (dfgnn_agnn_fwd / dfgnn_agnn_bwd and their _rect forms)
are declared, exported, bound and validate their arguments before any GPU call; the operators and layers import and
resolve; the closed-form backward the kernels implement (include/dfgnn.h), restated here with index ops, agrees in float64
with torch.autograd.grad of the new layers' non-fused branches."""
import argparse
import ctypes
import os
import re
import types

import numpy as np
import torch

from conftest import ROOT, random_graph

NAMES = ("dfgnn_agnn_fwd", "dfgnn_agnn_bwd", "dfgnn_agnn_fwd_rect", "dfgnn_agnn_bwd_rect")


def test_symbols_declared_exported_and_bound():
    import dfgnn_native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfgnn.h")).read(), flags=re.S)
    raw = ctypes.CDLL(dfgnn_native.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), n
        assert hasattr(raw, n), n
        assert n in dfgnn_native.SIGNATURES
    assert [len(dfgnn_native.SIGNATURES[n]) for n in NAMES] == [14, 21, 15, 22]
    for n in NAMES:                                                    # `cosine` is the one int among the pointers
        assert dfgnn_native.SIGNATURES[n].count(ctypes.c_int) == (5 if n.endswith("_rect") else 4) + 1
    assert dfgnn_native.lib().dfgnn_abi_version() == 11
    ext_src = open(os.path.join(ROOT, "df-gnn_amd", "csrc", "torch_ext.cpp")).read()
    assert "dfgnn_agnn_fwd_rect(" in ext_src and "dfgnn_agnn_bwd_rect(" in ext_src


def test_argument_checks_need_no_gpu():
    """A missing pointer, one statistic without the other, a cosine other than 0 / 1, a negative extent and an edge
    without a column are DFGNN_E_BADARG; an empty problem succeeds; too many heads is DFGNN_E_UNSUPPORTED: all answered
    before any launch."""
    import dfgnn_native
    L = dfgnn_native.lib()
    buf, buf2 = (ctypes.c_float * 64)(), (ctypes.c_float * 64)()
    idx = (ctypes.c_int * 8)(0, 1, 2, 2, 0, 0, 0, 0)
    p, p2, i = ctypes.addressof(buf), ctypes.addressof(buf2), ctypes.addressof(idx)

    def fwd(m, X_row, beta=p, mx=p, sm=p, h=1, cosine=1, nnz=2):
        return L.dfgnn_agnn_fwd(m, nnz, h, 4, i, i, beta, cosine, X_row, p, mx, sm, p, None)

    def bwd(m, X_row, beta=p, delta=p, h=1, cosine=1, nnz=2, dX_col=p2):
        return L.dfgnn_agnn_bwd(m, nnz, h, 4, i, i, i, i, beta, cosine, X_row, p, p, p, p, p, delta, p, dX_col, p, None)

    def fwd_rect(m, n_cols, nnz):
        return L.dfgnn_agnn_fwd_rect(m, n_cols, nnz, 1, 4, i, i, p, 1, p, p, p, p, p, None)

    def bwd_rect(m, n_cols, nnz):
        return L.dfgnn_agnn_bwd_rect(m, n_cols, nnz, 1, 4, i, i, i, i, p, 1, p, p, p, p, p, p, p, p, p2, p, None)

    assert fwd(3, None) == -1 and bwd(3, None) == -1
    assert fwd(3, p, beta=None) == -1 and bwd(3, p, beta=None) == -1
    assert bwd(3, p, delta=None) == -1
    assert fwd(3, p, mx=None) == -1 and fwd(3, p, sm=None) == -1      # one statistic without the other
    assert fwd(3, p, cosine=2) == -1 and bwd(3, p, cosine=2) == -1 and fwd(3, p, cosine=-1) == -1
    assert fwd(-1, p) == -1 and bwd(-1, p) == -1 and fwd(3, p, nnz=-1) == -1 and bwd(3, p, nnz=-1) == -1
    assert fwd_rect(3, -1, 0) == -1 and bwd_rect(3, -1, 0) == -1
    assert fwd_rect(3, 0, 2) == -1 and bwd_rect(3, 0, 2) == -1        # an edge needs a column
    assert bwd(3, p, dX_col=p) == -1                                  # dX_row and dX_col are distinct buffers
    assert fwd(0, p, nnz=0) == 0 and bwd(0, p, nnz=0) == 0
    assert fwd(0, None, nnz=0) == 0 and bwd(0, None, nnz=0) == 0
    assert fwd(3, p, h=70000) == -2 and bwd(3, p, h=70000) == -2


def test_surface_imports_and_resolves():
    import fused_gtconv
    from DFGNN.layers import AGNNConv_beta, DOTGATConv_forward, load_graphconv_layer, load_prepfunc, preprocess_Hyper_fw_bw
    from DFGNN.layers.AGNN import AGNNConv_beta as A2, index_ops_agnn
    from DFGNN.layers.GAT_DOT import DOTGATConv_forward as D2
    from DFGNN.operators.fused_gtconv import AGNNConvFuse, AGNNConvFuse_inference, FusedAGNNFunction
    from DFGNN.utils.graph import Graph
    assert A2 is AGNNConv_beta and D2 is DOTGATConv_forward
    for fn in (fused_gtconv.agnn_inference, fused_gtconv.agnn_forward, fused_gtconv.agnn_backward, AGNNConvFuse,
               AGNNConvFuse_inference, index_ops_agnn):
        assert callable(fn)
    assert hasattr(FusedAGNNFunction, "apply")
    args = argparse.Namespace(conv="agnn", format="forward_beta", dim=64, heads=2)
    layer = load_graphconv_layer(args)
    assert type(layer) is AGNNConv_beta and load_prepfunc(args) is preprocess_Hyper_fw_bw
    assert tuple(layer.beta.shape) == (2,) and layer.beta.requires_grad and (layer.beta == 1).all()
    assert layer.proj.out_features == 128 and dict(layer.named_parameters()).keys() == {"proj.weight", "proj.bias", "beta"}
    args = argparse.Namespace(conv="dotgat", format="forward", dim=64, heads=2)
    layer = load_graphconv_layer(args)
    assert type(layer) is DOTGATConv_forward
    assert dict(layer.named_parameters()).keys() == {"conv_nofuse.fc.weight"}          # beta is a buffer
    assert "beta" in dict(layer.named_buffers()) and torch.allclose(layer.beta, torch.full((2,), 64 ** -0.5))
    g = Graph([0, 1, 2, 2], [1, 2, 0, 1], 3)
    params = load_prepfunc(args)(g)
    assert params[0] is g and len(params) == 10 and params[3].tolist() == [0, 1, 2, 4]      # (g, A, rows, row_ptr, ...)


def _closed_form(row, col, m, n_cols, beta, cosine, xr, xc, dO):
    """float64 numpy: out, dX_row, dX_col, dbeta by the formulas of include/dfgnn.h, edge sums with np.add.at."""
    k = 1.0 if cosine else 0.0
    if cosine:
        r = 1.0 / np.maximum(np.sqrt((xr * xr).sum(-1)), 1e-12)     # [m, h]
        q = 1.0 / np.maximum(np.sqrt((xc * xc).sum(-1)), 1e-12)     # [n_cols, h]
    else:
        r, q = np.ones(xr.shape[:2]), np.ones(xc.shape[:2])
    c = r[row] * q[col] * (xr[row] * xc[col]).sum(-1)                # [E, h]
    s = beta * c
    mx = np.full((m, s.shape[1]), -np.inf)
    np.maximum.at(mx, row, s)
    p = np.exp(s - mx[row])
    den = np.zeros_like(mx)
    np.add.at(den, row, p)
    P = p / den[row]
    out = np.zeros_like(xr)
    np.add.at(out, row, P[:, :, None] * xc[col])
    delta = (dO * out).sum(-1)
    dS = P * ((dO[row] * xc[col]).sum(-1) - delta[row])
    g, gp = np.zeros((m, s.shape[1])), np.zeros((n_cols, s.shape[1]))
    np.add.at(g, row, dS * c)
    np.add.at(gp, col, dS * c)
    a_row, a_col, msg = np.zeros_like(xr), np.zeros_like(xc), np.zeros_like(xc)
    np.add.at(a_row, row, (dS * q[col])[:, :, None] * xc[col])
    np.add.at(a_col, col, (dS * r[row])[:, :, None] * xr[row])
    np.add.at(msg, col, P[:, :, None] * dO[row])
    dxr = (beta * r)[:, :, None] * (a_row - k * (g * r)[:, :, None] * xr)
    dxc = msg + (beta * q)[:, :, None] * (a_col - k * (gp * q)[:, :, None] * xc)
    return out, dxr, dxc, g.sum(0)


def _graphs():
    """square: 97 nodes with empty rows and columns, duplicate edges and a 70-edge row; rect: 96 rows x 257 columns."""
    rng = np.random.default_rng(97)
    m = 97
    indptr, indices, rows = random_graph(rng, m, 2.8, empty_frac=0.2, dup_frac=0.1, max_deg=70)
    indices[indices == 11] = 12                                     # an empty column for certain
    deg, indeg = np.diff(indptr), np.bincount(indices, minlength=m)
    assert (deg == 0).any() and (indeg == 0).any() and deg.max() == 70
    assert (np.diff(indices)[np.diff(rows) == 0] == 0).any()        # a duplicate edge
    rng = np.random.default_rng(96257)
    rptr, _, rrows = random_graph(rng, 96, 10, max_deg=70)
    rcols = rng.integers(0, 257, len(rrows)).astype(np.int32)
    assert rcols.max() >= 96 and np.diff(rptr).max() == 70
    return dict(square=(rows, indices, m, m), rect=(rrows, rcols, 96, 257))


def _compare(names, got, want, what):
    for name, a, b in zip(names, got, want):
        a = a.detach().numpy() if isinstance(a, torch.Tensor) else a
        err = float(np.abs(a - b).max())
        print(f"agnn {what} {name}: max abs err {err:.3e}")
        assert err < 1e-10 * max(1.0, float(np.abs(b).max())), (what, name, err)


def test_nonfused_branches_match_closed_form_backward():
    """float64, both modes, distinct operands, the square and the 96 x 257 graph: the closed form against
    torch.autograd.grad of AGNNConv_beta.conv_nofuse (cosine) and of the index ops it is made of (dot mode)."""
    from DFGNN.layers import AGNNConv_beta
    from DFGNN.layers.AGNN import index_ops_agnn
    h, f = 3, 5
    for kind, (rows, cols, m, n_cols) in _graphs().items():
        A = types.SimpleNamespace(row=torch.from_numpy(rows.astype(np.int64)), col=torch.from_numpy(cols.astype(np.int64)))
        torch.manual_seed(5)
        layer = AGNNConv_beta(6, f, h).double()
        with torch.no_grad():
            layer.beta.copy_(torch.rand(h, dtype=torch.float64) * 4 + 0.5)
        xr = torch.randn(m, h, f, dtype=torch.float64, requires_grad=True)
        xc = torch.randn(n_cols, h, f, dtype=torch.float64, requires_grad=True)
        dO = torch.randn(m, h, f, dtype=torch.float64)
        out = layer.conv_nofuse(A, xr, xc)
        grads = torch.autograd.grad(out, (xr, xc, layer.beta), dO)
        want = _closed_form(rows, cols, m, n_cols, layer.beta.detach().numpy(), True, xr.detach().numpy(),
                            xc.detach().numpy(), dO.numpy())
        _compare(("out", "dX_row", "dX_col", "dbeta"), (out,) + grads, want, f"cosine {kind}")
        deg = np.bincount(rows, minlength=m)
        assert (out.detach().numpy()[deg == 0] == 0).all() and (want[1][deg == 0] == 0).all()
        assert (want[2][np.bincount(cols, minlength=n_cols) == 0] == 0).all()
        beta = (torch.rand(h, dtype=torch.float64) * 4 + 0.5) * f ** -0.5
        beta.requires_grad_(True)
        out = index_ops_agnn(A.row, A.col, beta, xr, xc, cosine=False)
        grads = torch.autograd.grad(out, (xr, xc, beta), dO)
        want = _closed_form(rows, cols, m, n_cols, beta.detach().numpy(), False, xr.detach().numpy(), xc.detach().numpy(),
                            dO.numpy())
        _compare(("out", "dX_row", "dX_col", "dbeta"), (out,) + grads, want, f"dot {kind}")


def test_layers_shared_operand_match_closed_form_backward():
    """The whole layers, non-fused branch, float64, on the square graph: one tensor feeds both sides and its gradient is the
    sum of the two closed-form gradients -- AGNNConv_beta (proj weight and beta) and DOTGATConv_forward (fc weight; its
    DotGatConv is given the transposed edge list, so it normalises over a row's out-edges like the fused operator)."""
    from DFGNN.layers import AGNNConv_beta, DOTGATConv_forward
    rows, cols, m, _ = _graphs()["square"]
    A = types.SimpleNamespace(row=torch.from_numpy(rows.astype(np.int64)), col=torch.from_numpy(cols.astype(np.int64)))
    params = (A,) + (None,) * 8
    h, f = 3, 5
    torch.manual_seed(7)
    feat = torch.randn(m, 6, dtype=torch.float64)
    dO = torch.randn(m, h, f, dtype=torch.float64)

    agnn = AGNNConv_beta(6, f, h).double()
    with torch.no_grad():
        agnn.beta.copy_(torch.rand(h, dtype=torch.float64) * 4 + 0.5)
    x = agnn.proj(feat).view(-1, h, f).detach().numpy()
    out = agnn(params, feat, fuse=False)
    (out.view(m, h, f) * dO).sum().backward()
    w = _closed_form(rows, cols, m, m, agnn.beta.detach().numpy(), True, x, x, dO.numpy())
    dx = torch.from_numpy(w[1] + w[2]).reshape(m, h * f)
    _compare(("out", "dproj.weight", "dproj.bias", "dbeta"),
             (out.view(m, h, f), agnn.proj.weight.grad, agnn.proj.bias.grad, agnn.beta.grad),
             (w[0], (dx.t() @ feat).numpy(), dx.sum(0).numpy(), w[3]), "AGNNConv_beta")

    dot = DOTGATConv_forward(6, f, h).double()
    assert torch.allclose(dot.beta, torch.full((h,), f ** -0.5, dtype=torch.float64), rtol=1e-7, atol=0)   # (made in fp32)
    x = dot.conv_nofuse.fc(feat).view(-1, h, f).detach().numpy()
    out = dot((None,) + params, feat, fuse=False)
    (out.view(m, h, f) * dO).sum().backward()
    w = _closed_form(rows, cols, m, m, np.full(h, f ** -0.5), False, x, x, dO.numpy())   # DotGatConv's own 1 / sqrt(out)
    dx = torch.from_numpy(w[1] + w[2]).reshape(m, h * f)
    _compare(("out", "dfc.weight"), (out.view(m, h, f), dot.conv_nofuse.fc.weight.grad), (w[0], (dx.t() @ feat).numpy()),
             "DOTGATConv_forward")
