"""CPU: the GT pair with a per-edge additive attention bias (dfgnn_gt_fwd_bias / dfgnn_gt_bwd_bias) is declared, exported,
bound and validates its arguments before any GPU call; the operators and layers import; the layer's torch branch agrees
with the closed-form backward, masks included; and the power condition of tests/test_parity_cases_host.py holds for the
fp32-level cases that tests/test_gpu_gt_bias.py runs (tests/gt_bias_cases.py builds them): losing one boundary edge moves
out, row_sum, dQ and dbias of every test row -- transposed: dK and dV of every test column -- by at least POWER x bound."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gt_bias_cases as bc
import parity_cases as pc
from conftest import ROOT, csc_of, random_graph

NAMES = ("dfgnn_gt_fwd_bias", "dfgnn_gt_bwd_bias")
SEEN = set()


def test_symbols_declared_exported_and_bound():
    import dfgnn_native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfgnn.h")).read(), flags=re.S)
    raw = ctypes.CDLL(dfgnn_native.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), n
        assert hasattr(raw, n), n
        assert n in dfgnn_native.SIGNATURES
    assert len(dfgnn_native.SIGNATURES["dfgnn_gt_fwd_bias"]) == 15
    assert len(dfgnn_native.SIGNATURES["dfgnn_gt_bwd_bias"]) == 24
    assert dfgnn_native.lib().dfgnn_abi_version() == 11


def test_argument_checks_need_no_gpu():
    """Every check of the two entry points is answered before any launch."""
    import dfgnn_native
    L = dfgnn_native.lib()
    buf = (ctypes.c_float * 64)()
    idx = (ctypes.c_int * 8)(0, 1, 2, 2, 0, 0, 0, 0)
    p, i = ctypes.addressof(buf), ctypes.addressof(idx)

    def fwd(m=3, nnz=2, h=1, row_ptr=i, col_ind=i, bias=p, Q=p, K=p, V=p, mx=p, sm=p, out=p):
        return L.dfgnn_gt_fwd_bias(m, nnz, h, 4, row_ptr, col_ind, None, bias, Q, K, V, mx, sm, out, None)

    def bwd(m=3, nnz=2, h=1, row_ptr=i, col_ind=i, bias=p, col_ptr=i, row_ind=i, val_idx=i, Q=p, K=p, V=p, out=p, mx=p, sm=p,
            grad=p, delta=p, dQ=p, dK=p, dV=p, dbias=p):
        return L.dfgnn_gt_bwd_bias(m, nnz, h, 4, row_ptr, col_ind, None, bias, col_ptr, row_ind, val_idx, Q, K, V, out, mx, sm,
                                   grad, delta, dQ, dK, dV, dbias, None)

    for fn in (fwd, bwd):
        assert fn(m=-1) == -1 and fn(nnz=-1) == -1                      # check_common
        assert fn(row_ptr=None) == -1 and fn(col_ind=None) == -1
        for name in ("Q", "K", "V", "out"):                             # a missing feature pointer
            assert fn(**{name: None}) == -1, (fn.__name__, name)
        assert fn(bias=None) == -1                                      # bias == NULL with nnz > 0
        assert fn(h=70000) == -2                                        # h > 65535
        assert fn(m=0) == 0 and fn(m=0, Q=None, bias=None) == 0         # an empty problem succeeds
    assert fwd(mx=None) == -1 and fwd(sm=None) == -1                    # one statistic without the other
    for name in ("delta", "col_ptr", "row_ind", "val_idx", "grad", "mx", "sm", "dQ", "dK", "dV"):
        assert bwd(**{name: None}) == -1, name                          # (val_idx: required even for unit values)


def test_operators_and_layers_import():
    import argparse

    import fused_gtconv
    from DFGNN.layers import SparseMHA_bias, load_graphconv_layer, load_prepfunc, preprocess_Hyper_fw_bw
    from DFGNN.layers.GT import SparseMHA_bias_timing
    from DFGNN.operators.fused_gtconv import FusedGTFunction_bias, GTConvFuse_bias, GTConvFuse_inference_bias
    for name in ("gt_inference_bias", "gt_forward_bias", "gt_backward_bias"):
        assert callable(getattr(fused_gtconv, name))
    assert callable(GTConvFuse_bias) and callable(GTConvFuse_inference_bias) and hasattr(FusedGTFunction_bias, "apply")
    args = argparse.Namespace(conv="gt", format="forward_bias", dim=64, heads=2)
    assert isinstance(load_graphconv_layer(args), SparseMHA_bias_timing)
    assert load_prepfunc(args) is preprocess_Hyper_fw_bw
    assert SparseMHA_bias(64, 64, 2).head_dim == 32


# ---- the layer's torch branch against the closed-form backward ------------------------------------------------------------
def _closed_form(row_ptr, col_ind, val, bias, Q, K, V, dO):
    """The header comment's formulas, edge by edge in float64.  bias: [h, nnz]."""
    m, h, f = Q.shape
    out, dQ, dK, dV = (np.zeros((m, h, f)) for _ in range(4))
    dbias = np.zeros_like(bias)
    for i in range(m):
        lo, hi = row_ptr[i], row_ptr[i + 1]
        for hd in range(h):
            s = val[lo:hi] * (K[col_ind[lo:hi], hd] @ Q[i, hd]) + bias[hd, lo:hi]
            live = np.isfinite(s)
            if not live.any():
                continue                                               # empty or fully masked: zeros everywhere
            p = np.where(live, np.exp(np.where(live, s, 0.0) - s[live].max()), 0.0)
            p /= p.sum()
            out[i, hd] = p @ V[col_ind[lo:hi], hd]
            ds = p * (V[col_ind[lo:hi], hd] @ dO[i, hd] - dO[i, hd] @ out[i, hd])
            dbias[hd, lo:hi] = ds
            dQ[i, hd] = (ds * val[lo:hi]) @ K[col_ind[lo:hi], hd]
            np.add.at(dK[:, hd], col_ind[lo:hi], (ds * val[lo:hi])[:, None] * Q[i, hd])
            np.add.at(dV[:, hd], col_ind[lo:hi], p[:, None] * dO[i, hd])
    return out, dQ, dK, dV, dbias


@pytest.mark.parametrize("masked", [False, True])
def test_layer_torch_branch_matches_closed_form(masked):
    from DFGNN.layers import SparseMHA_bias
    from DFGNN.layers.GT.gtconv_layer_bias import index_ops_mha_bias
    rng = np.random.default_rng(5)
    m, heads, dim = 40, 2, 12
    row_ptr, col_ind, rows = random_graph(rng, m, 4, empty_frac=0.1, dup_frac=0.1, max_deg=30)
    nnz = len(col_ind)
    val = rng.uniform(0.5, 1.5, nnz)
    edge_bias = rng.standard_normal((nnz, heads))
    if masked:
        edge_bias[rng.random((nnz, heads)) < 0.3] = -np.inf
        full = np.nonzero(np.diff(row_ptr) > 0)[0][:3]
        for i in full[:2]:
            edge_bias[row_ptr[i]:row_ptr[i + 1], :] = -np.inf         # every edge of a row, both heads
        edge_bias[row_ptr[full[2]]:row_ptr[full[2] + 1], 0] = -np.inf  # ... and of another row in head 0 only
    tt = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dt)  # noqa: E731
    params = (None, tt(rows, torch.int32), tt(row_ptr, torch.int32), tt(col_ind, torch.int32), tt(val), None, None, None, 0)
    torch.manual_seed(0)
    layer = SparseMHA_bias(dim, dim, heads).double().train()
    x = torch.randn(m, dim, dtype=torch.float64)
    dO = torch.randn(m, heads, dim // heads, dtype=torch.float64)
    q, k, v = (t.detach() for t in layer._qkv_fused(x))
    want = _closed_form(row_ptr, col_ind, val, edge_bias.T, q.numpy(), k.numpy(), v.numpy(), dO.numpy())
    # the function of (q, k, v, edge_bias) ...
    qg, kg, vg, bg = (t.clone().requires_grad_(True) for t in (q, k, v, tt(edge_bias)))
    out = index_ops_mha_bias(params[1], params[3], params[4], qg, kg, vg, bg)
    grads = torch.autograd.grad(out, (qg, kg, vg, bg), dO)
    got = [out.detach().numpy()] + [t.numpy() for t in grads[:3]] + [grads[3].numpy().T]
    for name, a, b in zip(("out", "dQ", "dK", "dV", "dbias"), got, want):
        assert np.isfinite(a).all(), name
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), (name, np.abs(a - b).max())
    if masked:
        assert (got[4][~np.isfinite(edge_bias.T)] == 0).all()
        assert (got[0][full[:2]] == 0).all() and (got[1][full[:2]] == 0).all() and (got[0][full[2], 0] == 0).all()
    # ... and the layer around it
    eb = tt(edge_bias).requires_grad_(True)
    y = layer(params, x, eb, fuse=False)
    assert y.shape == (m, dim) and np.abs(y.detach().numpy().reshape(m, heads, -1) - want[0]).max() <= 1e-12
    (geb,) = torch.autograd.grad(y, eb, dO.reshape(m, -1))
    assert np.abs(geb.numpy().T - want[4]).max() <= 1e-12 * max(1.0, np.abs(want[4]).max())


def test_reference_removes_masked_edges():
    """tests/gt_bias_cases.reference (the GPU tests' reference) against the closed form, with masks."""
    rng = np.random.default_rng(6)
    m, h, f = 30, 2, 5
    row_ptr, col_ind, rows = random_graph(rng, m, 5, empty_frac=0.1)
    nnz = len(col_ind)
    val = rng.uniform(0.5, 1.5, nnz)
    bias = rng.standard_normal((h, nnz))
    bias[rng.random((h, nnz)) < 0.3] = -np.inf
    i = int(np.nonzero(np.diff(row_ptr) > 0)[0][0])
    bias[:, row_ptr[i]:row_ptr[i + 1]] = -np.inf
    Q, K, V, dO = (rng.standard_normal((m, h, f)) for _ in range(4))
    ref = bc.reference(row_ptr, col_ind, val, bias, Q, K, V, dO)
    want = _closed_form(row_ptr, col_ind, val, bias, Q, K, V, dO)
    for name, b in zip(("out", "dQ", "dK", "dV", "dbias"), want):
        assert np.abs(ref[name] - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), name
    assert (ref["row_max"][i] == bc.SENTINEL_MAX).all() and (ref["row_sum"][i] == 0).all()
    assert np.isfinite(ref["row_max"]).all()


# ---- the power condition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.case_ids("gt"), ids=str)
def test_power_gt_bias(case):
    g = pc.graph(case[0], case[1])
    x, ref64, bounds = bc.boundary_references(case)
    names = bc.COL_SIDE if g["transposed"] else bc.ROW_SIDE
    report = {}
    for mut, slots in pc.mutations(g).items():
        assert len(slots) == len(g["mutate"]) > 0
        row_ptr, col_ind, keep = pc.drop_slots(g, slots)
        assert keep.sum() == g["nnz"] - len(slots)
        moved = bc.mutated_reference(case, x, keep, row_ptr, col_ind)
        for name in names:
            if name == "dbias":                  # the edges that stay, grouped by the rows of the mutated graph
                e = pc.row_errors(moved[name], ref64[name][:, keep], row_ptr, floor=pc.floor_of(ref64[name], g["row_ptr"]))
            else:
                e = pc.row_errors(moved[name], ref64[name])
            e = e[g["mutate"]]
            fp32 = bounds[name] / pc.MARGIN / (bc.DK_FACTOR if name == "dK" else 1.0)
            assert fp32 > 0, (case, name)
            report[(mut, name)] = (float(e.min()), bounds[name], float(e.min()) / fp32)
    for (mut, name), (move, bound, ratio) in report.items():
        print(f"power gt_bias {case} {mut} {name}: least move {move:.3e}, bound {bound:.3e}, move / fp32 error {ratio:.1f}")
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
