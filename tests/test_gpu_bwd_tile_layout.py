"""One-head attn_edge backward on the swizzled P / dS tile and the row-exchanged K image (csrc/dfgnn_lds_layout.hpp; run with
`-m gpu` on an MI355X).  The `narrow` and `wide` batches of tests/dense_cases.py hold one range of every size next to a strip,
column-block and size-class boundary (2, 15 - 17, ..., 127 - 129, 143 - 145, 159 - 162, 175 - 177, 191 - 193, ... 255), each a
dense range of its own (asserted from the plan), with edges at every tile corner; a third batch holds a one-node graph and a
128-node graph with a row without edges and a row with all 128.  At f = 64 and 128, one head, unit edge values, the backward
runs once through the autograd function (the rank-ordered pair) and once through gt_backward (dfgnn_gt_bwd, CSR order): the
two must be bit-equal -- a misplaced tile element or K row is an error of order one in one of them, and they scatter P in
different orders -- and both stay inside the fp32-level bounds of dense_cases (MARGIN x the plain-fp32 reference's own error
against float64; nothing measured on the kernels enters)."""
import functools

import numpy as np
import pytest
import torch

import dense_cases as dc
import parity_cases as pc
from conftest import csc_of
from test_gpu_dense_exact import _assert_plan, _Checker, _dev, _np, _on_device

pytestmark = pytest.mark.gpu

EXTRA_SIZES = (1, 128)
EXTRA_EMPTY_ROW, EXTRA_FULL_ROW = 37, 90          # local nodes of the 128-node member


@pytest.fixture(scope="module", autouse=True)
def _leave_no_device_memory_behind():
    yield
    import gc
    import _binding_util as bu
    import test_gpu_dense_exact as tde
    tde._DEVICE.clear()
    for cache in (bu._unit_cache, bu._plan_cache, bu._rows_cache, bu._weights_cache):
        cache.d.clear()
    gc.collect()
    torch.cuda.empty_cache()


@functools.lru_cache(maxsize=None)
def _extra_graph():
    """A one-node graph (its self-loop) and a 128-node graph (p = 0.4) whose node EXTRA_EMPTY_ROW has no out-edge and whose
    node EXTRA_FULL_ROW has all 128, in the form of dense_cases.graph()."""
    rng = np.random.default_rng(4103)
    members, ranges, src, dst, n0 = [], [], [], [], 0
    for n in EXTRA_SIZES:
        adj = rng.random((n, n)) < 0.4 if n > 1 else np.ones((1, 1), dtype=bool)
        if n > 1:
            adj[EXTRA_EMPTY_ROW, :] = False
            adj[EXTRA_FULL_ROW, :] = True
            adj[0, n - 1] = adj[n - 1, 0] = True
        s, d = [], []
        for i in range(n):
            cols = rng.permutation(np.nonzero(adj[i])[0])
            s.append(np.full(len(cols), i, dtype=np.int64))
            d.append(cols.astype(np.int64))
        s, d = np.concatenate(s), np.concatenate(d)
        members.append((s, d, n))
        src.append(s + n0)
        dst.append(d + n0)
        ranges.append(dict(n0=n0, n=n, hole=False))
        n0 += n
    m, src, dst = n0, np.concatenate(src), np.concatenate(dst)
    rows, col_ind = src.astype(np.int32), dst.astype(np.int32)
    row_ptr = np.zeros(m + 1, dtype=np.int64)
    np.add.at(row_ptr, src + 1, 1)
    row_ptr = np.cumsum(row_ptr).astype(np.int32)
    col_ptr, row_ind, val_idx = csc_of(row_ptr, col_ind, rows, m)
    deg = np.diff(row_ptr)
    assert deg[1 + EXTRA_EMPTY_ROW] == 0 and deg[1 + EXTRA_FULL_ROW] == 128 and deg[0] == 1
    return dict(name="narrow", m=m, nnz=len(src), row_ptr=row_ptr, col_ind=col_ind, rows=rows, col_ptr=col_ptr, row_ind=row_ind,
                val_idx=val_idx, ranges=ranges, members=members)


@functools.lru_cache(maxsize=2)
def _extra_references(f):
    """Plain random inputs at the scales of parity_cases -> (inputs, ref64, bounds) as dense_cases.gt_references."""
    g = _extra_graph()
    rng = np.random.default_rng(77 + f)
    Q, K = (rng.standard_normal((g["m"], 1, f)) * f ** -0.25 for _ in range(2))
    V, dO = (rng.standard_normal((g["m"], 1, f)) for _ in range(2))
    x = dict(zip(("val", "Q", "K", "V", "dO"), dc._f32(np.ones(g["nnz"]), Q, K, V, dO)))
    ref64 = pc.gt_reference(g["row_ptr"], g["col_ind"], x, "f64")
    ref32 = pc.gt_reference(g["row_ptr"], g["col_ind"], x, "f32")
    return x, ref64, dc.bounds_of(g, ref32, ref64)


def _case(name, f):
    if name == "extra":
        return (_extra_graph(),) + _extra_references(f)
    x, ref64, _, bounds = dc.gt_references(name, 1, f, True)
    return dc.graph(name), x, ref64, bounds


@pytest.mark.parametrize("f", (128, 64))
@pytest.mark.parametrize("name", dc.BATCHES + ("extra",))
def test_backward_on_the_swizzled_tile(oracle_mod, name, f):
    import fused_gtconv as gt
    from DFGNN.operators.fused_gtconv import GTConvFuse_hyper
    g, x, ref64, bounds = _case(name, f)
    d = _on_device(g, ("tile-layout", name))
    Q, K, V, dO = (_dev(x[k]) for k in ("Q", "K", "V", "dO"))
    rp, ci, val = d["row_ptr"], d["col_ind"], d["val"]
    pair, plan = gt.gt_training_pair(rp, ci, val, Q)
    assert pair == "ranked", pair
    _assert_plan(plan, g)                           # every member is a dense range of its own
    what = f"tile layout {name} f={f}"
    c = _Checker(g, ref64, bounds, what)
    # the rank-ordered pair, through the autograd function
    Qg, Kg, Vg = (t.clone().requires_grad_(True) for t in (Q, K, V))
    out = GTConvFuse_hyper(d["rows"], rp, ci, val, d["col_ptr"], d["row_ind"], d["val_idx"], d["smem"], Qg, Kg, Vg)
    ranked = torch.autograd.grad(out, (Qg, Kg, Vg), dO)
    # the CSR-ordered pair: gt_hyper_forward -> gt_backward (dfgnn_gt_bwd)
    args = (rp, ci, d["rows"], val, d["col_ptr"], d["row_ind"], d["val_idx"], d["smem"], Q, K, V)
    out_csr, attn = gt.gt_hyper_forward(*args)
    csr = gt.gt_backward(*args, attn, dO)
    torch.cuda.synchronize()
    c.check("ranked pair", "out", out)
    c.check("attn_edge pair", "out", out_csr)
    for nm, a, b in zip(("dQ", "dK", "dV"), ranked, csr):
        c.check("ranked pair", nm, a)
        c.check("attn_edge pair", nm, b)
        assert torch.equal(a, b), (what, nm, float((a - b).abs().max()))
    er, ec = np.diff(g["row_ptr"]) == 0, np.diff(g["col_ptr"]) == 0
    for nm, t, empty in (("dQ", csr[0], er), ("dK", csr[1], ec), ("dV", csr[2], ec)):
        assert (_np(t)[empty] == 0).all(), (what, nm)
    if name == "extra":
        assert er.sum() == 1 and er[1 + EXTRA_EMPTY_ROW]
    c.done()
