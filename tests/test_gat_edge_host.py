"""CPU: the any-graph GAT pair with a per-edge attention term (dfgnn_gat_fwd_edge / dfgnn_gat_bwd_edge and their _rect forms)
is declared, exported, bound and validates its arguments before any GPU call; the operators and layers import; the closed-form
equations of include/dfgnn.h, edge by edge in float64, agree with torch.autograd.grad (the GPU tests' reference and the
layers' torch branch) to 1e-12; and the power condition of tests/test_parity_cases_host.py holds for the fp32-level cases
that tests/test_gpu_gat_edge.py runs (tests/gat_edge_cases.py builds them): losing one boundary edge moves out, edge_sum,
grad_attn_row and grad_score of every test row -- transposed: grad_feat and grad_attn_col of every test column -- by at
least POWER x bound.

Not under the condition: edge_max, as in tests/test_parity_cases_host.py (NOT_UNDER_CONDITION) and for its reason: a maximum
is no sum, a lost edge moves it only when it was the row's argmax, and both ends of a row (two sentinels at +3) cannot be
that at once; edge_sum and `out`, taken relative to it, are under the condition."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import gat_edge_cases as ge
import parity_cases as pc
from conftest import ROOT, random_graph

NAMES = ("dfgnn_gat_fwd_edge", "dfgnn_gat_bwd_edge", "dfgnn_gat_fwd_edge_rect", "dfgnn_gat_bwd_edge_rect")
NOT_UNDER_CONDITION = ("edge_max",)
SEEN = set()


def test_symbols_declared_exported_and_bound():
    import dfgnn_native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfgnn.h")).read(), flags=re.S)
    raw = ctypes.CDLL(dfgnn_native.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), n
        assert hasattr(raw, n), n
        assert n in dfgnn_native.SIGNATURES
    assert len(dfgnn_native.SIGNATURES["dfgnn_gat_fwd_edge"]) == 17
    assert len(dfgnn_native.SIGNATURES["dfgnn_gat_bwd_edge"]) == 25
    assert len(dfgnn_native.SIGNATURES["dfgnn_gat_fwd_edge_rect"]) == 18
    assert len(dfgnn_native.SIGNATURES["dfgnn_gat_bwd_edge_rect"]) == 26
    assert dfgnn_native.lib().dfgnn_abi_version() == 11
    ext_src = open(os.path.join(ROOT, "df-gnn_amd", "csrc", "torch_ext.cpp")).read()
    for n in ("gat_fwd_edge", "gat_bwd_edge"):                              # the torch-extension transport binds both
        assert re.search(r'm\.def\("' + n + r'",\s*&' + n + r"\b", ext_src), n
    binding = open(os.path.join(ROOT, "df-gnn_amd", "fused_gatconv.py")).read()
    for n in ("dfgnn_gat_fwd_edge_rect", "dfgnn_gat_bwd_edge_rect", "ext.gat_fwd_edge", "ext.gat_bwd_edge"):
        assert n in binding, n                                              # the Python binding goes through both transports


def test_constants_do_not_collide():
    """The new file's threshold has its own name (parity_cases.caps() counts the four shared ones) and the value of the
    pairs it is modelled on."""
    assert sorted(pc.caps()) == sorted(pc.CAP_NAMES)
    src = open(os.path.join(pc.CSRC, "gat_edge_train.hip")).read()
    assert re.search(r"constexpr\s+int\s+kGatEdgeGroupMaxDegree\s*=\s*24\s*;", src)


def test_argument_checks_need_no_gpu():
    """Every check of the entry points is answered before any launch."""
    import dfgnn_native
    L = dfgnn_native.lib()
    buf = (ctypes.c_float * 64)()
    idx = (ctypes.c_int * 8)(0, 1, 2, 2, 0, 0, 0, 0)
    p, i = ctypes.addressof(buf), ctypes.addressof(idx)

    def fwd(m=3, nnz=2, h=1, f=4, row_ptr=i, col_ind=i, attn_row=p, attn_col=p, slope=0.2, score=p, X=p, mask=p, drop=0.5,
            edge_max=p, edge_sum=p, out=p, rect=False):
        args = (row_ptr, col_ind, attn_row, attn_col, slope, score, X, mask, drop, edge_max, edge_sum, out, None)
        return L.dfgnn_gat_fwd_edge_rect(m, m, nnz, h, f, *args) if rect else L.dfgnn_gat_fwd_edge(m, nnz, h, f, *args)

    def bwd(m=3, nnz=2, h=1, f=4, row_ptr=i, col_ind=i, col_ptr=i, row_ind=i, val_idx=i, attn_row=p, attn_col=p, slope=0.2,
            score=p, X=p, mask=p, drop=0.5, out=p, edge_max=p, edge_sum=p, grad=p, delta=p, grad_feat=p, grad_attn_row=p,
            grad_attn_col=p, grad_score=p, rect=False):
        if out is None:            # (the backward takes no `out`: grad stands in for the loop over both entry points)
            grad = None
        args = (row_ptr, col_ind, col_ptr, row_ind, val_idx, attn_row, attn_col, slope, score, X, mask, drop, edge_max,
                edge_sum, grad, delta, grad_feat, grad_attn_row, grad_attn_col, grad_score, None)
        return L.dfgnn_gat_bwd_edge_rect(m, m, nnz, h, f, *args) if rect else L.dfgnn_gat_bwd_edge(m, nnz, h, f, *args)

    wide = dict(f=2000)   # above every compiled lane layout: a call that passes the argument checks answers UNSUPPORTED
    for rect in (False, True):
        for base in (fwd, bwd):
            fn = lambda base=base, **kw: base(rect=rect, **kw)  # noqa: E731
            assert fn(m=-1) == -1 and fn(nnz=-1) == -1                      # check_rect
            assert fn(row_ptr=None) == -1 and fn(col_ind=None) == -1
            for name in ("attn_row", "attn_col", "X", "out"):               # a missing pointer
                assert fn(**{name: None}) == -1, (base.__name__, name)
                assert fn(**{name: None}, **wide) == -1, (base.__name__, name)
            for bad in (1.0, -0.1, 1.5, float("nan")):                      # the dropout rate of a given mask
                assert fn(drop=bad) == -1, bad
            assert fn(drop=1.5, mask=None, **wide) == -2                    # ... is not read without one
            assert fn(h=70000) == -2                                        # h > 65535
            assert fn(m=0) == 0 and fn(m=0, nnz=0, attn_row=None, X=None, score=None) == 0   # an empty problem succeeds
            assert fn(**wide) == -2
            assert fn(score=None, **wide) == -2 and fn(mask=None, **wide) == -2 and fn(score=None, mask=None, **wide) == -2
        assert fwd(edge_max=None, rect=rect) == -1 and fwd(edge_sum=None, rect=rect) == -1     # both statistics or neither
        assert fwd(edge_max=None, edge_sum=None, rect=rect, **wide) == -2
        for name in ("col_ptr", "row_ind", "edge_max", "edge_sum", "grad", "delta", "grad_feat", "grad_attn_row",
                     "grad_attn_col"):
            assert bwd(rect=rect, **{name: None}) == -1, name
            assert bwd(rect=rect, **{name: None}, **wide) == -1, name
        assert bwd(grad_score=None, rect=rect, **wide) == -2                # optional
        assert bwd(val_idx=None, rect=rect) == -1                           # needed for a score or a mask ...
        assert bwd(val_idx=None, score=None, rect=rect) == -1 and bwd(val_idx=None, mask=None, rect=rect) == -1
        assert bwd(val_idx=None, score=None, mask=None, rect=rect, **wide) == -2    # ... and for nothing else


def test_operators_and_layers_import():
    import argparse

    import fused_gatconv
    from DFGNN.layers import (GATConv_edge, GATConv_forward, index_ops_gat_edge, load_graphconv_layer, load_prepfunc,
                              preprocess_Hyper_fw_bw)
    from DFGNN.layers.GAT import GATConv_edge_timing
    from DFGNN.operators.fused_gatconv import FusedGATFunction_edge, GATConvFuse_edge, GATConvFuse_inference_edge
    for name in ("gat_inference_edge", "gat_forward_edge", "gat_backward_edge"):
        assert callable(getattr(fused_gatconv, name))
    assert callable(GATConvFuse_edge) and callable(GATConvFuse_inference_edge) and hasattr(FusedGATFunction_edge, "apply")
    assert callable(index_ops_gat_edge)
    for fmt, cls in (("forward", GATConv_forward), ("forward_edge", GATConv_edge_timing)):
        args = argparse.Namespace(conv="gat", format=fmt, dim=64, heads=2)
        assert type(load_graphconv_layer(args)) is cls
        assert load_prepfunc(args) is preprocess_Hyper_fw_bw
    layer = GATConv_edge(16, 8, 2, edge_dim=5)
    assert layer.lin_edge.weight.shape == (16, 5) and layer.lin_edge.bias is None and layer.att_edge.shape == (2, 8)
    with pytest.raises(RuntimeError, match="val_idx is required"):
        fused_gatconv.gat_backward_edge(0.2, 0.0, *([None] * 4), None, *([None] * 6))


# ---- the closed form --------------------------------------------------------------------------------------------------
def _closed_form(row_ptr, col_ind, ar, ac, score, X, dO, slope, mask, drop):
    """The operator's equations (include/dfgnn.h), edge by edge in float64.  score: [h, nnz] or None, mask: [nnz, h] or None."""
    m, h = ar.shape
    lrelu = lambda v: v if v > 0 else slope * v  # noqa: E731
    out = np.zeros((m,) + X.shape[1:])
    emax, esum, gar = np.full((m, h), ge.EMPTY_MAX), np.zeros((m, h)), np.zeros((m, h))
    gac, gx, gs = np.zeros_like(ac), np.zeros_like(X), np.zeros((h, len(col_ind)))
    for hd in range(h):
        pre = lambda i, e: ar[i, hd] + ac[col_ind[e], hd] + (score[hd, e] if score is not None else 0.0)  # noqa: E731
        k = lambda e: 1.0 if mask is None else float(mask[e, hd] > drop) / (1.0 - drop)  # noqa: E731
        for i in range(m):
            es = range(row_ptr[i], row_ptr[i + 1])
            if not len(es):
                continue
            emax[i, hd] = max(lrelu(pre(i, e)) for e in es)
            esum[i, hd] = sum(np.exp(lrelu(pre(i, e)) - emax[i, hd]) for e in es)
            P = {e: np.exp(lrelu(pre(i, e)) - emax[i, hd]) / esum[i, hd] for e in es}
            for e in es:
                out[i, hd] += k(e) * P[e] * X[col_ind[e], hd]
            delta = dO[i, hd] @ out[i, hd]
            for e in es:
                j = col_ind[e]
                dS = P[e] * (k(e) * (dO[i, hd] @ X[j, hd]) - delta)
                G = dS * (1.0 if pre(i, e) > 0 else slope)
                gar[i, hd] += G
                gac[j, hd] += G
                gs[hd, e] = G
                gx[j, hd] += k(e) * P[e] * dO[i, hd]
    return dict(out=out, edge_max=emax, edge_sum=esum, grad_feat=gx, grad_attn_row=gar, grad_attn_col=gac, grad_score=gs)


def _close(a, b, what):
    assert np.isfinite(a).all(), what
    assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), (what, np.abs(a - b).max())


def _small_case(rect, seed=5):
    """-> (row_ptr, col_ind, m, n_cols): a graph with an empty row and a duplicate edge; rect: 40 rows x 23 columns."""
    rng = np.random.default_rng(seed)
    m = 40
    row_ptr, col_ind, _ = random_graph(rng, m, 4, empty_frac=0.1, dup_frac=0.1, max_deg=30)
    assert (np.diff(row_ptr) == 0).any(), "the graph needs an empty row"
    n_cols = m
    if rect:
        n_cols = 23
        col_ind = (col_ind % n_cols).astype(np.int32)
    return row_ptr, col_ind, m, n_cols


@pytest.mark.parametrize("rect", [False, True], ids=["square", "rect"])
@pytest.mark.parametrize("with_mask", [False, True], ids=["nodrop", "drop"])
@pytest.mark.parametrize("with_score", [False, True], ids=["plain", "score"])
def test_reference_matches_closed_form(with_score, with_mask, rect):
    """tests/gat_edge_cases.reference (autograd; the GPU tests' reference) against the closed form; score = None is zeros."""
    row_ptr, col_ind, m, n_cols = _small_case(rect)
    rng = np.random.default_rng(6)
    h, f, nnz = 2, 5, len(col_ind)
    ar, ac = rng.standard_normal((m, h)), rng.standard_normal((n_cols, h))
    X, dO = rng.standard_normal((n_cols, h, f)), rng.standard_normal((m, h, f))
    score = rng.standard_normal((h, nnz)) if with_score else None
    mask, drop = (rng.uniform(size=(nnz, h)), 0.4) if with_mask else (None, 0.0)
    ref = ge.reference(row_ptr, col_ind, ar, ac, score, X, dO, 0.2, mask, drop)
    want = _closed_form(row_ptr, col_ind, ar, ac, score, X, dO, 0.2, mask, drop)
    for name in ge.OUTPUTS:
        _close(ref[name], want[name], name)
    empty = np.diff(row_ptr) == 0
    assert (ref["out"][empty] == 0).all() and (ref["edge_sum"][empty] == 0).all() and (ref["edge_max"][empty] == -1e38).all()
    if with_score:      # a masked edge and a fully masked (row, head): finite, the empty-row conventions
        full = int(np.argmax(np.diff(row_ptr) >= 2))
        one = int(np.nonzero(np.diff(row_ptr) >= 2)[0][1])
        score[0, row_ptr[full]:row_ptr[full + 1]] = -np.inf
        score[1, row_ptr[one]] = -np.inf
        ref = ge.reference(row_ptr, col_ind, ar, ac, score, X, dO, 0.2, mask, drop)
        assert all(np.isfinite(v).all() for v in ref.values())
        assert (ref["out"][full, 0] == 0).all() and ref["edge_sum"][full, 0] == 0 and ref["edge_max"][full, 0] == -1e38
        assert ref["grad_attn_row"][full, 0] == 0 and (ref["grad_score"][0, row_ptr[full]:row_ptr[full + 1]] == 0).all()
        assert ref["grad_score"][1, row_ptr[one]] == 0 and ref["edge_sum"][one, 1] > 0


@pytest.mark.parametrize("rect", [False, True], ids=["square", "rect"])
def test_layer_torch_branches_match_closed_form(rect):
    """index_ops_gat_edge, GATConv_forward and GATConv_edge (non-fused, float64) against the closed form; the folded edge
    term equals <lin_edge(edge_attr)[h], att_edge[h]> and autograd through it gives the parameters' gradients."""
    from DFGNN.layers import GATConv_edge, GATConv_forward
    row_ptr, col_ind, m, n_cols = _small_case(rect, seed=7)
    nnz, heads, dim, edge_dim = len(col_ind), 2, 6, 5
    rows = np.repeat(np.arange(m), np.diff(row_ptr))
    ti = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(torch.int32)  # noqa: E731

    class _A:
        row, col = ti(rows), ti(col_ind)
    params = (_A, ti(rows), ti(row_ptr), ti(col_ind), None, None, None, None, 0)
    torch.manual_seed(0)
    feat_c, feat_r = torch.randn(n_cols, 9, dtype=torch.float64), torch.randn(m, 9, dtype=torch.float64)
    feat = (feat_c, feat_r) if rect else feat_c
    edge_attr = torch.randn(nnz, edge_dim, dtype=torch.float64)
    dO = torch.randn(m, heads, dim, dtype=torch.float64)
    for cls in (GATConv_forward, GATConv_edge):
        layer = (cls(9, dim, heads, edge_dim=edge_dim) if cls is GATConv_edge else cls(9, dim, heads)).double().eval()
        ar, ac, x = (t.detach().numpy() for t in layer.project(feat))
        score = None
        if cls is GATConv_edge:
            sc = layer.edge_score(edge_attr)
            explicit = (layer.lin_edge(edge_attr).view(nnz, heads, dim) * layer.att_edge).sum(-1)
            _close(sc.detach().numpy(), explicit.detach().numpy(), "folded edge score")
            score = sc.detach().numpy().T
            y = layer(params, feat, edge_attr, fuse=False)
        else:
            y = layer(params, feat, fuse=False)
        want = _closed_form(row_ptr, col_ind, ar, ac, score, x, dO.numpy(), layer.negative_slope, None, 0.0)
        assert y.shape == (m, heads * dim)
        _close(y.detach().numpy().reshape(m, heads, dim), want["out"], cls.__name__)
        if cls is GATConv_edge:
            gw, ga = torch.autograd.grad(y, (layer.lin_edge.weight, layer.att_edge), dO.reshape(m, -1))
            gs = torch.from_numpy(want["grad_score"].T)                                   # [nnz, heads]
            gw_want, ga_want = torch.autograd.grad(explicit, (layer.lin_edge.weight, layer.att_edge), gs)
            _close(gw.numpy(), gw_want.numpy(), "lin_edge.weight gradient")
            _close(ga.numpy(), ga_want.numpy(), "att_edge gradient")


# ---- the power condition ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", pc.case_ids("gat"), ids=str)
def test_power_gat_edge(case):
    """grad_score_e of an edge that stays moves with its row's statistics, but what a kernel that loses an edge gets wrong
    first is that edge's slot: grad_score is compared in the layout of the full graph, the lost edge's slot holding zeros
    (nothing written)."""
    g = pc.graph(case[0], case[1])
    x, ref64, bounds = ge.boundary_references(case)
    pre = x["attn_row"][g["rows"]] + x["attn_col"][g["col_ind"]] + x["score"].T
    _, _, slots = pc._sentinels(g) if g["transposed"] else pc._sentinels(g, 3)
    assert np.abs(pre[slots] - pc.SENTINEL_LOGIT).max() < 1e-5, "the sentinels' logits are +3 with the score included"
    names = ge.COL_SIDE if g["transposed"] else ge.ROW_SIDE
    report = {}
    for mut, slots in pc.mutations(g).items():
        assert len(slots) == len(g["mutate"]) > 0
        row_ptr, col_ind, keep = pc.drop_slots(g, slots)
        assert keep.sum() == g["nnz"] - len(slots)
        moved = ge.mutated_reference(x, keep, row_ptr, col_ind)
        for name in names:
            if name in NOT_UNDER_CONDITION:
                continue
            if name == "grad_score":
                lost = np.zeros_like(ref64[name])
                lost[:, keep] = moved[name]
                e = pc.row_errors(lost, ref64[name], g["row_ptr"])
            else:
                e = pc.row_errors(moved[name], ref64[name])
            e = e[g["mutate"]]
            fp32 = bounds[name] / pc.MARGIN
            assert fp32 > 0, (case, name)
            report[(mut, name)] = (float(e.min()), bounds[name], float(e.min()) / fp32)
    for (mut, name), (move, bound, ratio) in report.items():
        print(f"power gat_edge {case} {mut} {name}: least move {move:.3e}, bound {bound:.3e}, "
              f"move / bound {move / bound:.1f}, move / fp32 error {ratio:.1f}")
    for (mut, name), (move, bound, ratio) in report.items():
        assert move >= pc.POWER * bound, (case, mut, name, move, bound)
    SEEN.add(case)


def test_zz_no_case_was_skipped(request):
    """Runs last in this module: all 16 cases went through the condition (when the whole module ran)."""
    wanted = set(pc.case_ids("gat"))
    assert len(wanted) == 16
    selected = [i.name for i in request.session.items if i.module is request.module and i.name.startswith("test_power")]
    if len(selected) == len(wanted):           # (a -k selection of single cases is not a skipped case)
        assert SEEN == wanted, sorted(wanted - SEEN)
