"""CPU: the GT pair with a per-edge multiplicative gate on the keys and an edge output (dfgnn_gt_fwd_gate /
dfgnn_gt_bwd_gate and their _rect forms) is declared, exported, bound and validates its arguments before any GPU call; the
operators and layers import; the layer's torch branch and the GPU tests' reference agree with the closed-form equations;
and the power condition of tests/test_parity_cases_host.py holds for the fp32-level cases that tests/test_gpu_gt_gate.py
runs (tests/gt_gate_cases.py builds them): losing one boundary edge moves out, W, row_sum, dQ and dE of every test row --
transposed: dK and dV of every test column -- by at least POWER x bound."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gt_gate_cases as gc
import parity_cases as pc
from conftest import ROOT, random_graph

NAMES = ("dfgnn_gt_fwd_gate", "dfgnn_gt_bwd_gate", "dfgnn_gt_fwd_gate_rect", "dfgnn_gt_bwd_gate_rect")
SEEN = set()


def test_symbols_declared_exported_and_bound():
    import dfgnn_native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfgnn.h")).read(), flags=re.S)
    raw = ctypes.CDLL(dfgnn_native.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), n
        assert hasattr(raw, n), n
        assert n in dfgnn_native.SIGNATURES
    assert len(dfgnn_native.SIGNATURES["dfgnn_gt_fwd_gate"]) == 16          # the edge pair's + W
    assert len(dfgnn_native.SIGNATURES["dfgnn_gt_bwd_gate"]) == 25          # the edge pair's + G
    assert len(dfgnn_native.SIGNATURES["dfgnn_gt_fwd_gate_rect"]) == 17
    assert len(dfgnn_native.SIGNATURES["dfgnn_gt_bwd_gate_rect"]) == 26
    assert dfgnn_native.lib().dfgnn_abi_version() == 11
    ext_src = open(os.path.join(ROOT, "df-gnn_amd", "csrc", "torch_ext.cpp")).read()
    for n in ("gt_fwd_gate", "gt_bwd_gate"):                                # the torch-extension transport binds both
        assert re.search(r'm\.def\("' + n + r'",\s*&' + n + r"\b", ext_src), n
    binding = open(os.path.join(ROOT, "df-gnn_amd", "fused_gtconv.py")).read()
    for n in ("dfgnn_gt_fwd_gate_rect", "dfgnn_gt_bwd_gate_rect", "ext.gt_fwd_gate", "ext.gt_bwd_gate"):
        assert n in binding, n                                              # the Python binding goes through both transports


def test_argument_checks_need_no_gpu():
    """Every check of the entry points is answered before any launch."""
    import dfgnn_native
    L = dfgnn_native.lib()
    buf = (ctypes.c_float * 64)()
    idx = (ctypes.c_int * 8)(0, 1, 2, 2, 0, 0, 0, 0)
    p, i = ctypes.addressof(buf), ctypes.addressof(idx)

    def fwd(m=3, nnz=2, h=1, row_ptr=i, col_ind=i, E=p, Q=p, K=p, V=p, mx=p, sm=p, out=p, W=p, rect=False, f=4):
        if rect:
            return L.dfgnn_gt_fwd_gate_rect(m, m, nnz, h, f, row_ptr, col_ind, None, E, Q, K, V, mx, sm, out, W, None)
        return L.dfgnn_gt_fwd_gate(m, nnz, h, f, row_ptr, col_ind, None, E, Q, K, V, mx, sm, out, W, None)

    def bwd(m=3, nnz=2, h=1, row_ptr=i, col_ind=i, E=p, col_ptr=i, row_ind=i, val_idx=i, Q=p, K=p, V=p, out=p, mx=p, sm=p,
            grad=p, G=p, delta=p, dQ=p, dK=p, dV=p, dE=p, rect=False, f=4):
        if rect:
            return L.dfgnn_gt_bwd_gate_rect(m, m, nnz, h, f, row_ptr, col_ind, None, E, col_ptr, row_ind, val_idx, Q, K, V,
                                            out, mx, sm, grad, G, delta, dQ, dK, dV, dE, None)
        return L.dfgnn_gt_bwd_gate(m, nnz, h, f, row_ptr, col_ind, None, E, col_ptr, row_ind, val_idx, Q, K, V, out, mx, sm,
                                   grad, G, delta, dQ, dK, dV, dE, None)

    for rect in (False, True):
        for base in (fwd, bwd):
            fn = lambda base=base, **kw: base(rect=rect, **kw)  # noqa: E731
            assert fn(m=-1) == -1 and fn(nnz=-1) == -1                      # check_common
            assert fn(row_ptr=None) == -1 and fn(col_ind=None) == -1
            for name in ("Q", "K", "V", "out"):                             # a missing feature pointer
                assert fn(**{name: None}) == -1, (base.__name__, name)
            assert fn(E=None) == -1                                         # E == NULL with nnz > 0
            assert fn(h=70000) == -2                                        # h > 65535
            assert fn(m=0) == 0 and fn(m=0, Q=None, E=None) == 0            # an empty problem succeeds
        assert fwd(mx=None, rect=rect) == -1 and fwd(sm=None, rect=rect) == -1      # one statistic without the other
        for name in ("delta", "col_ptr", "row_ind", "val_idx", "grad", "mx", "sm", "dQ", "dK", "dV"):
            assert bwd(rect=rect, **{name: None}) == -1, name               # (val_idx: required even for unit values)
    # W, G and dE are optional.  At f = 2000 (above every compiled lane layout) a call that passes the argument checks is
    # answered DFGNN_E_UNSUPPORTED by the layout dispatch, before any launch: NULL in one of the three gets there, NULL in a
    # required array does not
    wide = dict(f=2000)
    assert fwd(**wide) == -2 and bwd(**wide) == -2
    assert fwd(W=None, **wide) == -2 and fwd(W=None, mx=None, sm=None, **wide) == -2
    assert bwd(G=None, **wide) == -2 and bwd(dE=None, **wide) == -2 and bwd(G=None, dE=None, **wide) == -2
    assert fwd(W=None, rect=True, **wide) == -2 and bwd(G=None, dE=None, rect=True, **wide) == -2
    assert fwd(W=None, Q=None, **wide) == -1 and bwd(G=None, dE=None, dQ=None, **wide) == -1


def test_operators_and_layers_import():
    import argparse

    import fused_gtconv
    from DFGNN.layers import SparseMHA_gate, load_graphconv_layer, load_prepfunc, preprocess_Hyper_fw_bw
    from DFGNN.layers.GT import SparseMHA_gate_timing
    from DFGNN.operators.fused_gtconv import FusedGTFunction_gate, GTConvFuse_gate, GTConvFuse_inference_gate
    for name in ("gt_inference_gate", "gt_forward_gate", "gt_backward_gate"):
        assert callable(getattr(fused_gtconv, name))
    assert callable(GTConvFuse_gate) and callable(GTConvFuse_inference_gate) and hasattr(FusedGTFunction_gate, "apply")
    args = argparse.Namespace(conv="gt", format="forward_gate", dim=64, heads=2)
    assert isinstance(load_graphconv_layer(args), SparseMHA_gate_timing)
    assert load_prepfunc(args) is preprocess_Hyper_fw_bw
    layer = SparseMHA_gate(64, 64, 2, edge_dim=5)
    assert layer.head_dim == 32 and layer.lin_edge.weight.shape == (64, 5) and layer.lin_edge.bias is None
    assert layer.edge_out and not SparseMHA_gate(64, 64, 2, edge_out=False).edge_out


# ---- the closed form --------------------------------------------------------------------------------------------------
def _closed_form(row_ptr, col_ind, val, E, G, Q, K, V, dO):
    """The operator's equations, edge by edge in float64.  E, G: [nnz, h, f].  -> out, W, dQ, dK, dV, dE."""
    m, h, f = Q.shape
    out, dQ, dK, dV = (np.zeros((m, h, f)) for _ in range(4))
    W, dE = np.zeros_like(E), np.zeros_like(E)
    for i in range(m):
        lo, hi = row_ptr[i], row_ptr[i + 1]
        if hi == lo:
            continue                                                   # an empty row: zeros everywhere
        c = col_ind[lo:hi]
        for hd in range(h):
            ke = K[c, hd] * E[lo:hi, hd]                               # [deg, f]
            w = val[lo:hi, None] * Q[i, hd] * ke
            W[lo:hi, hd] = w
            s = w.sum(-1)
            p = np.exp(s - s.max())
            p /= p.sum()
            out[i, hd] = p @ V[c, hd]
            ds = p * (V[c, hd] @ dO[i, hd] - dO[i, hd] @ out[i, hd])
            g = (ds[:, None] + G[lo:hi, hd]) * val[lo:hi, None]        # val_e g_e[d]
            dQ[i, hd] = (g * ke).sum(0)
            np.add.at(dK[:, hd], c, g * Q[i, hd] * E[lo:hi, hd])
            np.add.at(dV[:, hd], c, p[:, None] * dO[i, hd])
            dE[lo:hi, hd] = g * Q[i, hd] * K[c, hd]
    return out, W, dQ, dK, dV, dE


NAMES6 = ("out", "W", "dQ", "dK", "dV", "dE")


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


def test_layer_torch_branch_matches_closed_form():
    from DFGNN.layers import SparseMHA_gate
    from DFGNN.layers.GT.gtconv_layer_gate import index_ops_mha_gate
    rng = np.random.default_rng(5)
    m, heads, dim, edge_dim = 40, 2, 12, 5
    row_ptr, col_ind, rows = _small_graph(rng, m)
    nnz = len(col_ind)
    val = rng.uniform(0.5, 1.5, nnz)
    tt = lambda a, dt=torch.float64: torch.from_numpy(np.ascontiguousarray(a)).to(dt)  # noqa: E731
    params = (None, tt(rows, torch.int32), tt(row_ptr, torch.int32), tt(col_ind, torch.int32), tt(val), None, None, None, 0)
    torch.manual_seed(0)
    layer = SparseMHA_gate(dim, dim, heads, edge_dim=edge_dim).double().train()
    x = torch.randn(m, dim, dtype=torch.float64)
    edge_attr = torch.randn(nnz, edge_dim, dtype=torch.float64)
    dO = torch.randn(m, heads, dim // heads, dtype=torch.float64)
    G = torch.randn(nnz, heads, dim // heads, dtype=torch.float64)
    q, k, v = (t.detach() for t in layer._qkv_fused(x))
    e = layer.lin_edge(edge_attr).view(nnz, heads, dim // heads).detach()
    want = _closed_form(row_ptr, col_ind, val, e.numpy(), G.numpy(), q.numpy(), k.numpy(), v.numpy(), dO.numpy())
    # the function of (q, k, v, e) ...
    qg, kg, vg, eg = (t.clone().requires_grad_(True) for t in (q, k, v, e))
    out, w = index_ops_mha_gate(params[1], params[3], params[4], qg, kg, vg, eg)
    grads = torch.autograd.grad((out, w), (qg, kg, vg, eg), (dO, G))
    got = [out.detach().numpy(), w.detach().numpy()] + [t.numpy() for t in grads]
    for name, a, b in zip(NAMES6, got, want):
        _close(a, b, name)
    empty = np.diff(row_ptr) == 0
    assert (got[0][empty] == 0).all() and (got[2][empty] == 0).all()
    # ... and the layer around it: the gradient of lin_edge's weight is dE^T edge_attr
    y, e_out = layer(params, x, edge_attr, fuse=False)
    assert y.shape == (m, dim) and e_out.shape == (nnz, dim)
    _close(y.detach().numpy().reshape(m, heads, -1), want[0], "layer h_out")
    _close(e_out.detach().numpy().reshape(nnz, heads, -1), want[1], "layer e_out")
    (gw,) = torch.autograd.grad((y, e_out), layer.lin_edge.weight, (dO.reshape(m, -1), G.reshape(nnz, -1)))
    want_w = want[5].reshape(nnz, dim).T @ edge_attr.numpy()
    _close(gw.numpy(), want_w, "lin_edge.weight gradient")
    y2, none = SparseMHA_gate(dim, dim, heads, edge_dim=edge_dim, edge_out=False).double()(params, x, edge_attr, fuse=False)
    assert none is None and y2.shape == (m, dim)


@pytest.mark.parametrize("with_G", [True, False])
def test_reference_matches_closed_form(with_G):
    """tests/gt_gate_cases.reference (the GPU tests' reference) against the closed form; G = None is G = 0."""
    rng = np.random.default_rng(6)
    m, h, f = 30, 2, 5
    row_ptr, col_ind, rows = _small_graph(rng, m)
    nnz = len(col_ind)
    val = rng.uniform(0.5, 1.5, nnz)
    E, G = (rng.standard_normal((nnz, h, f)) for _ in range(2))
    Q, K, V, dO = (rng.standard_normal((m, h, f)) for _ in range(4))
    ref = gc.reference(row_ptr, col_ind, val, E, G if with_G else None, Q, K, V, dO)
    want = _closed_form(row_ptr, col_ind, val, E, G if with_G else np.zeros_like(G), Q, K, V, dO)
    for name, b in zip(NAMES6, want):
        _close(ref[name], b, name)
    i = int(np.nonzero(np.diff(row_ptr) == 0)[0][0])
    assert (ref["row_max"][i] == gc.SENTINEL_MAX).all() and (ref["row_sum"][i] == 0).all()
    assert np.isfinite(ref["row_max"]).all()


def test_boundary_logits_are_the_proven_cases():
    """The gate 2^c and Q 2^-c leave every logit of a parity case as it is -- in float32 arithmetic, product by product."""
    case = pc.case_ids("gt")[0]
    g = pc.graph(case[0], case[1])
    x, base = gc.boundary_inputs(case), pc.gt_inputs(*case)
    rows, cols = g["rows"].astype(np.int64)[:4096], g["col_ind"].astype(np.int64)[:4096]
    gated = x["Q"][rows] * (x["K"][cols] * x["E"][:4096])               # float32 products, as the kernels form them
    assert gated.dtype == np.float32 and (gated == base["Q"][rows] * base["K"][cols]).all()
    assert set(np.unique(x["E"])) == {np.float32(0.5), np.float32(1.0), np.float32(2.0)}
    assert 0.5 * gc.G_SCALE < np.abs(x["G"]).mean() / np.sqrt(2 / np.pi) < 2 * gc.G_SCALE


# ---- the power condition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.case_ids("gt"), ids=str)
def test_power_gt_gate(case):
    """W_e depends on its own edge alone, so the W of the edges that stay does not move when an edge is lost; what a kernel
    that loses an edge gets wrong is that edge's slot.  W is therefore compared in the layout of the full graph, the lost
    edge's slot holding zeros (nothing written); dE, whose every value depends on the row's softmax, is compared on the
    edges that stay, as in tests/test_gt_edge_host.py."""
    g = pc.graph(case[0], case[1])
    x, ref64, bounds = gc.boundary_references(case)
    names = gc.COL_SIDE if g["transposed"] else gc.ROW_SIDE
    report = {}
    for mut, slots in pc.mutations(g).items():
        assert len(slots) == len(g["mutate"]) > 0
        row_ptr, col_ind, keep = pc.drop_slots(g, slots)
        assert keep.sum() == g["nnz"] - len(slots)
        moved = gc.mutated_reference(case, x, keep, row_ptr, col_ind)
        for name in names:
            if name == "W":
                full, rp_full = gc.edge_rows(ref64[name], g["row_ptr"])
                lost = np.zeros_like(ref64[name])
                lost[keep] = moved[name]
                e = pc.row_errors(gc.edge_rows(lost, g["row_ptr"])[0], full, rp_full)
            elif name == "dE":                   # the edges that stay, grouped by the rows of the mutated graph
                full, rp_full = gc.edge_rows(ref64[name], g["row_ptr"])
                a, rp = gc.edge_rows(moved[name], row_ptr)
                e = pc.row_errors(a, gc.edge_rows(ref64[name][keep], row_ptr)[0], rp, floor=pc.floor_of(full, rp_full))
            else:
                e = pc.row_errors(moved[name], ref64[name])
            e = e[g["mutate"]]
            fp32 = bounds[name] / pc.MARGIN / (gc.DK_FACTOR if name == "dK" else 1.0)
            assert fp32 > 0, (case, name)
            report[(mut, name)] = (float(e.min()), bounds[name], float(e.min()) / fp32)
    for (mut, name), (move, bound, ratio) in report.items():
        print(f"power gt_gate {case} {mut} {name}: least move {move:.3e}, bound {bound:.3e}, move / fp32 error {ratio:.1f}")
    for (mut, name), (move, bound, ratio) in report.items():
        assert move >= pc.POWER * bound, (case, mut, name, move, bound)
    # the float32 reference alone stays inside the bounds, by construction: bound = MARGIN x its error
    SEEN.add(case)


def test_zz_no_case_was_skipped(request):
    """Runs last in this module: all 32 cases went through the condition (when the whole module ran)."""
    wanted = set(pc.case_ids("gt"))
    assert len(wanted) == 32
    selected = [i.name for i in request.session.items if i.module is request.module and i.name.startswith("test_power")]
    if len(selected) == len(wanted):           # (a -k selection of single cases is not a skipped case)
        assert SEEN == wanted, sorted(wanted - SEEN)
