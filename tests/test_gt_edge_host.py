"""CPU: the GT pair with per-edge feature vectors in keys and values (dfgnn_gt_fwd_edge / dfgnn_gt_bwd_edge) is declared,
exported, bound and validates its arguments before any GPU call; the operators and layers import; the layer's torch branch
agrees with the closed-form backward; and the power condition of tests/test_parity_cases_host.py holds for the fp32-level
cases that tests/test_gpu_gt_edge.py runs (tests/gt_edge_cases.py builds them): losing one boundary edge moves out, row_sum,
dQ and dE of every test row -- transposed: dK and dV of every test column -- by at least POWER x bound."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gt_edge_cases as ec
import parity_cases as pc
from conftest import ROOT, random_graph

NAMES = ("dfgnn_gt_fwd_edge", "dfgnn_gt_bwd_edge")
SEEN = set()


def test_symbols_declared_exported_and_bound():
    import dfgnn_native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfgnn.h")).read(), flags=re.S)
    raw = ctypes.CDLL(dfgnn_native.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), n
        assert hasattr(raw, n), n
        assert n in dfgnn_native.SIGNATURES
    assert len(dfgnn_native.SIGNATURES["dfgnn_gt_fwd_edge"]) == 15
    assert len(dfgnn_native.SIGNATURES["dfgnn_gt_bwd_edge"]) == 24
    assert dfgnn_native.lib().dfgnn_abi_version() == 11
    ext_src = open(os.path.join(ROOT, "df-gnn_amd", "csrc", "torch_ext.cpp")).read()
    for n in ("gt_fwd_edge", "gt_bwd_edge"):                           # the torch-extension transport binds both
        assert re.search(r'm\.def\("' + n + r'",\s*&' + n + r"\b", ext_src), n


def test_argument_checks_need_no_gpu():
    """Every check of the two entry points is answered before any launch."""
    import dfgnn_native
    L = dfgnn_native.lib()
    buf = (ctypes.c_float * 64)()
    idx = (ctypes.c_int * 8)(0, 1, 2, 2, 0, 0, 0, 0)
    p, i = ctypes.addressof(buf), ctypes.addressof(idx)

    def fwd(m=3, nnz=2, h=1, row_ptr=i, col_ind=i, E=p, Q=p, K=p, V=p, mx=p, sm=p, out=p):
        return L.dfgnn_gt_fwd_edge(m, nnz, h, 4, row_ptr, col_ind, None, E, Q, K, V, mx, sm, out, None)

    def bwd(m=3, nnz=2, h=1, row_ptr=i, col_ind=i, E=p, col_ptr=i, row_ind=i, val_idx=i, Q=p, K=p, V=p, out=p, mx=p, sm=p,
            grad=p, delta=p, dQ=p, dK=p, dV=p, dE=p):
        return L.dfgnn_gt_bwd_edge(m, nnz, h, 4, row_ptr, col_ind, None, E, col_ptr, row_ind, val_idx, Q, K, V, out, mx, sm,
                                   grad, delta, dQ, dK, dV, dE, None)

    for fn in (fwd, bwd):
        assert fn(m=-1) == -1 and fn(nnz=-1) == -1                      # check_common
        assert fn(row_ptr=None) == -1 and fn(col_ind=None) == -1
        for name in ("Q", "K", "V", "out"):                             # a missing feature pointer
            assert fn(**{name: None}) == -1, (fn.__name__, name)
        assert fn(E=None) == -1                                         # E == NULL with nnz > 0
        assert fn(h=70000) == -2                                        # h > 65535
        assert fn(m=0) == 0 and fn(m=0, Q=None, E=None) == 0            # an empty problem succeeds
    assert fwd(mx=None) == -1 and fwd(sm=None) == -1                    # one statistic without the other
    for name in ("delta", "col_ptr", "row_ind", "val_idx", "grad", "mx", "sm", "dQ", "dK", "dV"):
        assert bwd(**{name: None}) == -1, name                          # (val_idx: required even for unit values)


def test_operators_and_layers_import():
    import argparse

    import fused_gtconv
    from DFGNN.layers import SparseMHA_edge, load_graphconv_layer, load_prepfunc, preprocess_Hyper_fw_bw
    from DFGNN.layers.GT import SparseMHA_edge_timing
    from DFGNN.operators.fused_gtconv import FusedGTFunction_edge, GTConvFuse_edge, GTConvFuse_inference_edge
    for name in ("gt_inference_edge", "gt_forward_edge", "gt_backward_edge"):
        assert callable(getattr(fused_gtconv, name))
    assert callable(GTConvFuse_edge) and callable(GTConvFuse_inference_edge) and hasattr(FusedGTFunction_edge, "apply")
    args = argparse.Namespace(conv="gt", format="forward_edge", dim=64, heads=2)
    assert isinstance(load_graphconv_layer(args), SparseMHA_edge_timing)
    assert load_prepfunc(args) is preprocess_Hyper_fw_bw
    layer = SparseMHA_edge(64, 64, 2, edge_dim=5)
    assert layer.head_dim == 32 and layer.lin_edge.weight.shape == (64, 5) and layer.lin_edge.bias is None


# ---- the layer's torch branch against the closed-form backward ------------------------------------------------------------
def _closed_form(row_ptr, col_ind, val, E, Q, K, V, dO):
    """The issue's equations, edge by edge in float64.  E: [nnz, h, f]."""
    m, h, f = Q.shape
    out, dQ, dK, dV = (np.zeros((m, h, f)) for _ in range(4))
    dE = np.zeros_like(E)
    for i in range(m):
        lo, hi = row_ptr[i], row_ptr[i + 1]
        if hi == lo:
            continue                                                   # an empty row: zeros everywhere
        for hd in range(h):
            ke, ve = K[col_ind[lo:hi], hd] + E[lo:hi, hd], V[col_ind[lo:hi], hd] + E[lo:hi, hd]
            s = val[lo:hi] * (ke @ Q[i, hd])
            p = np.exp(s - s.max())
            p /= p.sum()
            out[i, hd] = p @ ve
            ds = p * (ve @ dO[i, hd] - dO[i, hd] @ out[i, hd])
            dQ[i, hd] = (ds * val[lo:hi]) @ ke
            np.add.at(dK[:, hd], col_ind[lo:hi], (ds * val[lo:hi])[:, None] * Q[i, hd])
            np.add.at(dV[:, hd], col_ind[lo:hi], p[:, None] * dO[i, hd])
            dE[lo:hi, hd] = (ds * val[lo:hi])[:, None] * Q[i, hd] + p[:, None] * dO[i, hd]
    return out, dQ, dK, dV, dE


def _small_graph(rng, m):
    row_ptr, col_ind, rows = random_graph(rng, m, 4, empty_frac=0.1, dup_frac=0.1, max_deg=30)
    deg = np.diff(row_ptr)
    assert (deg == 0).any(), "the graph needs an empty row"
    dup = any(len(set(col_ind[row_ptr[i]:row_ptr[i + 1]])) < deg[i] for i in range(m))
    assert dup, "the graph needs a duplicate edge"
    return row_ptr, col_ind, rows


def test_layer_torch_branch_matches_closed_form():
    from DFGNN.layers import SparseMHA_edge
    from DFGNN.layers.GT.gtconv_layer_edge import index_ops_mha_edge
    rng = np.random.default_rng(5)
    m, heads, dim, edge_dim = 40, 2, 12, 5
    row_ptr, col_ind, rows = _small_graph(rng, m)
    nnz = len(col_ind)
    val = rng.uniform(0.5, 1.5, nnz)
    tt = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dt)  # noqa: E731
    params = (None, tt(rows, torch.int32), tt(row_ptr, torch.int32), tt(col_ind, torch.int32), tt(val), None, None, None, 0)
    torch.manual_seed(0)
    layer = SparseMHA_edge(dim, dim, heads, edge_dim=edge_dim).double().train()
    x = torch.randn(m, dim, dtype=torch.float64)
    edge_attr = torch.randn(nnz, edge_dim, dtype=torch.float64)
    dO = torch.randn(m, heads, dim // heads, dtype=torch.float64)
    q, k, v = (t.detach() for t in layer._qkv_fused(x))
    e = layer.lin_edge(edge_attr).view(nnz, heads, dim // heads).detach()
    want = _closed_form(row_ptr, col_ind, val, e.numpy(), q.numpy(), k.numpy(), v.numpy(), dO.numpy())
    # the function of (q, k, v, e) ...
    qg, kg, vg, eg = (t.clone().requires_grad_(True) for t in (q, k, v, e))
    out = index_ops_mha_edge(params[1], params[3], params[4], qg, kg, vg, eg)
    grads = torch.autograd.grad(out, (qg, kg, vg, eg), dO)
    got = [out.detach().numpy()] + [t.numpy() for t in grads]
    for name, a, b in zip(("out", "dQ", "dK", "dV", "dE"), got, want):
        assert np.isfinite(a).all(), name
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), (name, np.abs(a - b).max())
    empty = np.diff(row_ptr) == 0
    assert (got[0][empty] == 0).all() and (got[1][empty] == 0).all()
    # ... and the layer around it: the gradient of lin_edge's weight is dE^T edge_attr
    y = layer(params, x, edge_attr, fuse=False)
    assert y.shape == (m, dim) and np.abs(y.detach().numpy().reshape(m, heads, -1) - want[0]).max() <= 1e-12
    (gw,) = torch.autograd.grad(y, layer.lin_edge.weight, dO.reshape(m, -1))
    want_w = want[4].reshape(nnz, dim).T @ edge_attr.numpy()
    assert np.abs(gw.numpy() - want_w).max() <= 1e-12 * max(1.0, np.abs(want_w).max())


def test_reference_matches_closed_form():
    """tests/gt_edge_cases.reference (the GPU tests' reference) against the closed form."""
    rng = np.random.default_rng(6)
    m, h, f = 30, 2, 5
    row_ptr, col_ind, rows = _small_graph(rng, m)
    nnz = len(col_ind)
    val = rng.uniform(0.5, 1.5, nnz)
    E = rng.standard_normal((nnz, h, f))
    Q, K, V, dO = (rng.standard_normal((m, h, f)) for _ in range(4))
    ref = ec.reference(row_ptr, col_ind, val, E, Q, K, V, dO)
    want = _closed_form(row_ptr, col_ind, val, E, Q, K, V, dO)
    for name, b in zip(("out", "dQ", "dK", "dV", "dE"), want):
        assert np.abs(ref[name] - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), name
    i = int(np.nonzero(np.diff(row_ptr) == 0)[0][0])
    assert (ref["row_max"][i] == ec.SENTINEL_MAX).all() and (ref["row_sum"][i] == 0).all()
    assert np.isfinite(ref["row_max"]).all()


# ---- the power condition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.case_ids("gt"), ids=str)
def test_power_gt_edge(case):
    g = pc.graph(case[0], case[1])
    x, ref64, bounds = ec.boundary_references(case)
    names = ec.COL_SIDE if g["transposed"] else ec.ROW_SIDE
    report = {}
    for mut, slots in pc.mutations(g).items():
        assert len(slots) == len(g["mutate"]) > 0
        row_ptr, col_ind, keep = pc.drop_slots(g, slots)
        assert keep.sum() == g["nnz"] - len(slots)
        moved = ec.mutated_reference(case, x, keep, row_ptr, col_ind)
        for name in names:
            if name == "dE":                     # the edges that stay, grouped by the rows of the mutated graph
                full, rp_full = ec.edge_rows(ref64[name], g["row_ptr"])
                a, rp = ec.edge_rows(moved[name], row_ptr)
                e = pc.row_errors(a, ec.edge_rows(ref64[name][keep], row_ptr)[0], rp, floor=pc.floor_of(full, rp_full))
            else:
                e = pc.row_errors(moved[name], ref64[name])
            e = e[g["mutate"]]
            fp32 = bounds[name] / pc.MARGIN / (ec.DK_FACTOR if name == "dK" else 1.0)
            assert fp32 > 0, (case, name)
            report[(mut, name)] = (float(e.min()), bounds[name], float(e.min()) / fp32)
    for (mut, name), (move, bound, ratio) in report.items():
        print(f"power gt_edge {case} {mut} {name}: least move {move:.3e}, bound {bound:.3e}, move / fp32 error {ratio:.1f}")
    for (mut, name), (move, bound, ratio) in report.items():
        assert move >= pc.POWER * bound, (case, mut, name, move, bound)
    SEEN.add(case)


def test_zz_no_case_was_skipped(request):
    """Runs last in this module: all 32 cases went through the condition (when the whole module ran)."""
    wanted = set(pc.case_ids("gt"))
    assert len(wanted) == 32
    selected = [i.name for i in request.session.items if i.module is request.module and i.name.startswith("test_power")]
    if len(selected) == len(wanted):           # (a -k selection of single cases is not a skipped case)
        assert SEEN == wanted, sorted(wanted - SEEN)
