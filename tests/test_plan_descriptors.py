"""The dense ranges' descriptors in a block plan, behind its spill list (csrc/plan.hip, dfgnn_launch.hpp: PlanDesc; include/dfgnn.h:
dfgnn_plan_desc_off) -- one 16-byte entry (n0, n1 | flags, row_ptr[n0], row_ptr[n1] - row_ptr[n0]) per dense range, which
every matrix-core kernel reads where it used to read the fit pair and two row_ptr words -- and every kernel that reads
them, against the CPU oracle: a range that got a wrong e0 / ne misplaces its attention values."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FLAGS = (1 << 30) | (1 << 29)     # dfgnn_launch.hpp: kPlanEdgeGlobal | kPlanDense


def _n(t):
    return t.detach().cpu().numpy()


def _mixed_batch():
    """Dense ranges, then fit ranges that are NOT dense (a band graph of 4 edges per row on 200 nodes: one closed range,
    below one edge per 32 node pairs, merged with nothing), then -- at f = 128 -- a spill range (300 nodes: too many rows
    for the matrix-core kernels and for the LDS).  The dense ranges do not end at m."""
    from DFGNN.utils import Graph, batch
    rng = np.random.default_rng(11)

    def er(n, p):
        iu, ju = np.triu_indices(n, k=1)
        keep = rng.random(len(iu)) < p
        return Graph(np.concatenate([iu[keep], ju[keep]]), np.concatenate([ju[keep], iu[keep]]), n)

    i = np.arange(200)
    s = np.concatenate([i, i, i, i])
    d = np.concatenate([(i + 1) % 200, (i - 1) % 200, (i + 2) % 200, (i - 2) % 200])
    return batch([er(40, 0.6), er(130, 0.4), er(100, 0.5), Graph(s, d, 200), er(300, 0.3)]).to(DEV)


@pytest.fixture(scope="module")
def geometry():
    """The 13-graph batch of every range class (16 / 17 / 127 / 128 / 129 / 160 / 161 / 192 / 255-node neighbourhoods),
    preprocessed once for the tests below."""
    from DFGNN.layers import preprocess_Hyper_fw_bw
    from test_gpu_stats_pair import _geometry_batch
    g = _geometry_batch(77)
    return g, preprocess_Hyper_fw_bw(g)


def _build(row_ptr, col_ind, f, fill):
    """dfgnn_plan_build into a buffer prefilled with `fill`: (buffer as numpy int32, header words)."""
    import dfgnn_native
    L = dfgnn_native.lib()
    m, nnz = row_ptr.numel() - 1, col_ind.numel()
    buf = torch.full((int(L.dfgnn_plan_ints(m, nnz)),), fill, dtype=torch.int32, device=DEV)
    meta = (ctypes.c_int * 12)()
    rc = L.dfgnn_plan_build(m, nnz, f, row_ptr.data_ptr(), col_ind.data_ptr(), buf.data_ptr(), ctypes.addressof(meta), None)
    assert rc == 0
    return buf.cpu().numpy(), list(meta)


def _check_plan(row_ptr, col_ind, f):
    import dfgnn_native
    L = dfgnn_native.lib()
    m, nnz = row_ptr.numel() - 1, col_ind.numel()
    rp, ci = _n(row_ptr).astype(np.int64), _n(col_ind).astype(np.int64)
    buf, meta = _build(row_ptr, col_ind, f, 0x5A5A5A5A)
    buf2, meta2 = _build(row_ptr, col_ind, f, 0x33CC33CC)
    assert meta == meta2
    num_fit, num_spill, num_dense, coords_off = meta[0], meta[1], meta[9], meta[11]
    # the buffer has the size and the layout it had without the descriptors: they lie over the scratch of the build, behind
    # the spill list and in front of the coordinates
    mask_off = (coords_off + (nnz + 1) // 2 + 4 + 3) & ~3
    ranked_off = mask_off + 16 * m
    old_len = ranked_off + (nnz + 1) // 2 + 4
    assert int(L.dfgnn_plan_ints(m, nnz)) == old_len == len(buf)
    desc_off = int(L.dfgnn_plan_desc_off(m, nnz))
    assert desc_off == 12 + 4 * m and desc_off % 4 == 0 and desc_off + 4 * num_dense <= coords_off
    ext = dfgnn_native.ext()
    assert ext is None or ext.plan_desc_off(m, nnz) == desc_off
    # the descriptors
    fit = buf[12:12 + 2 * num_fit].reshape(-1, 2)
    desc = buf[desc_off:desc_off + 4 * num_dense].reshape(-1, 4)
    for k in range(num_dense):
        n0, n1f = int(fit[k, 0]), int(fit[k, 1])
        n1 = n1f & ~FLAGS
        assert n1f & (1 << 29)
        assert tuple(desc[k]) == (n0, n1f, rp[n0], rp[n1] - rp[n0]), k
    assert not any(int(n1f) & (1 << 29) for n1f in fit[num_dense:, 1])
    # ... and the slack at the end of the buffer is untouched
    assert (buf[old_len - 4:] == 0x5A5A5A5A).all() and (buf2[old_len - 4:] == 0x33CC33CC).all()
    # everything else: the two builds agree on every word the plan defines ...
    old, old2 = buf[:old_len], buf2[:old_len]
    spill = old[12 + 2 * m:12 + 2 * m + 2 * num_spill]
    assert np.array_equal(old[:12 + 2 * num_fit], old2[:12 + 2 * num_fit]) and np.array_equal(spill, old2[12 + 2 * m:12 + 2 * m + 2 * num_spill])
    dn = fit[:num_dense].astype(np.int64)
    first = np.full(m, -1, np.int64)                       # node -> first node of its dense range
    for n0, n1f in dn:
        first[n0:n1f & ~FLAGS] = n0
    row_of = np.repeat(np.arange(m), np.diff(rp))
    in_dense = first[row_of] >= 0
    nodes = np.nonzero(first >= 0)[0]
    u16 = lambda a, off: a[off:off + (nnz + 1) // 2].view(np.uint16)[:nnz]   # noqa: E731
    coords, ranked = u16(old, coords_off), u16(old, ranked_off)
    mask = old[mask_off:mask_off + 8 * m].view(np.uint32).reshape(m, 8)
    maskT = old[mask_off + 8 * m:mask_off + 16 * m].view(np.uint32).reshape(m, 8)
    assert np.array_equal(coords[in_dense], u16(old2, coords_off)[in_dense])
    assert np.array_equal(ranked[in_dense], u16(old2, ranked_off)[in_dense])
    assert np.array_equal(old[mask_off:ranked_off].reshape(2, m, 8)[:, nodes], old2[mask_off:ranked_off].reshape(2, m, 8)[:, nodes])
    # ... and those words are what they were: coordinates, rank-ordered coordinates and bitmaps from the CSR arrays
    r, c = row_of - first[row_of], ci - first[row_of]
    want = ((r << 8) | c).astype(np.uint16)
    assert np.array_equal(coords[in_dense], want[in_dense])
    order = np.lexsort((ci, row_of))
    assert np.array_equal(ranked[in_dense], want[order][in_dense[order]])
    wm, wt = np.zeros((m, 8), np.uint32), np.zeros((m, 8), np.uint32)
    e = np.nonzero(in_dense)[0]
    np.bitwise_or.at(wm, (row_of[e], c[e] >> 5), (np.uint32(1) << (c[e] & 31).astype(np.uint32)))
    np.bitwise_or.at(wt, (ci[e], r[e] >> 5), (np.uint32(1) << (r[e] & 31).astype(np.uint32)))
    assert np.array_equal(mask[nodes], wm[nodes]) and np.array_equal(maskT[nodes], wt[nodes])
    return meta, fit, desc


@pytest.mark.parametrize("f", [128, 16])
def test_descriptors_of_every_range_class(geometry, f):
    """Batch of all range classes: every fit range is dense, one of them ends at m (row_ptr[n1] == nnz)."""
    g, (A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem) = geometry
    meta, fit, desc = _check_plan(row_ptr, col_ind, f)
    assert meta[9] == meta[0] > 0 and meta[1] == 0
    sizes = (desc[:, 1] & ~FLAGS) - desc[:, 0]          # (the small graphs are merged up to 128 nodes)
    assert (sizes <= 128).any() and ((sizes > 128) & (sizes <= 160)).any() and ((sizes > 160) & (sizes <= 192)).any() and sizes.max() == 255
    last = np.nonzero((desc[:, 1] & ~FLAGS) == g.num_nodes())[0]
    assert len(last) == 1 and desc[last[0], 2] + desc[last[0], 3] == g.num_edges()


@pytest.mark.parametrize("f", [128, 16])
def test_descriptors_stop_at_the_last_dense_range(f):
    """num_dense < num_fit, and at f = 128 a spill range: only the dense ranges get a descriptor."""
    from DFGNN.layers import preprocess_Hyper_fw_bw
    g = _mixed_batch()
    A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem = preprocess_Hyper_fw_bw(g)
    meta, fit, desc = _check_plan(row_ptr, col_ind, f)
    assert 0 < meta[9] < meta[0]
    assert (meta[1] > 0) == (f == 128)
    assert ((desc[:, 1] & ~FLAGS) < g.num_nodes()).all()


def test_descriptors_of_one_node_ranges():
    """The most descriptors per node the merge of small ranges leaves: dense ranges of ONE node (a self-loop) between
    128-node graphs, which they cannot be merged with.  Each gets its descriptor (ne = 1) and all of them fit in front of
    the coordinates (checked in _check_plan)."""
    from DFGNN.layers import preprocess_Hyper_fw_bw
    from DFGNN.utils import Graph, batch
    rng = np.random.default_rng(5)
    graphs = []
    for _ in range(3):
        iu, ju = np.triu_indices(128, k=1)
        keep = rng.random(len(iu)) < 0.4
        graphs.append(Graph(np.concatenate([iu[keep], ju[keep]]), np.concatenate([ju[keep], iu[keep]]), 128))
        graphs.append(Graph(np.zeros(1, np.int64), np.zeros(1, np.int64), 1))
    g = batch(graphs).to(DEV)
    A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem = preprocess_Hyper_fw_bw(g)
    meta, fit, desc = _check_plan(row_ptr, col_ind, 128)
    sizes = (desc[:, 1] & ~FLAGS) - desc[:, 0]
    assert meta[9] == meta[0] == 6 and sorted(sizes) == [1, 1, 1, 128, 128, 128]
    assert (desc[sizes == 1, 3] == 1).all()


def test_ranked_pair_reads_the_descriptors(geometry, oracle_mod):
    """One head of 128 features through the autograd function (the rank-ordered pair, every range class): bit-identical to
    the CSR-ordered pair, and the oracle's results."""
    import fused_gtconv as gt
    from DFGNN.operators.fused_gtconv import GTConvFuse_hyper
    from DFGNN.utils import synthetic as S
    from test_gpu_stats_pair import _close
    g, (A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem) = geometry
    m = g.num_nodes()
    Q, K, V = (t.requires_grad_(True) for t in S.gt_features(m, 1, 128, seed=7, device=DEV))
    dO = torch.randn(m, 1, 128, generator=torch.Generator().manual_seed(3)).to(DEV)
    assert gt.gt_ranked_pair_chosen(row_ptr, col_ind, val, Q) is not None
    out = GTConvFuse_hyper(rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem, Q, K, V)
    dQ, dK, dV = torch.autograd.grad(out, (Q, K, V), dO)
    args = (row_ptr, col_ind, rows, val, col_ptr, row_ind, val_idx, smem, Q.detach(), K.detach(), V.detach())
    out_a, attn = gt.gt_hyper_forward(*args)
    dQ_a, dK_a, dV_a = gt.gt_backward(*args, attn, dO)
    for a, b, what in ((out.detach(), out_a, "out"), (dQ, dQ_a, "dQ"), (dK, dK_a, "dK"), (dV, dV_a, "dV")):
        assert torch.equal(a, b), what
    ref = (_n(row_ptr), _n(col_ind), _n(val), _n(Q), _n(K), _n(V))
    wq, wk, wv = oracle_mod.gt_backward(*ref, _n(dO))
    _close(out, oracle_mod.gt_forward(*ref), "out")
    _close(dQ, wq, "dQ"); _close(dK, wk, "dK"); _close(dV, wv, "dV")
    (inf,) = gt.gt_hyper_inference(row_ptr, col_ind, rows, val, smem, Q.detach(), K.detach(), V.detach())
    _close(inf, oracle_mod.gt_forward(*ref), "inference")   # (the forward without attention values)


def test_two_per_cu_forward_reads_the_descriptors(oracle_mod):
    """A batch without ranges of more than 128 nodes: the 256-thread forward in its rank-ordered, CSR-ordered, inference
    and statistics forms."""
    import fused_gtconv as gt
    from DFGNN.layers import preprocess_Hyper_fw_bw
    from DFGNN.utils import synthetic as S
    from test_gpu_stats_pair import _close
    g = S.pattern_like(batch_size=12, seed=5, mean_nodes=90.0, std_nodes=25.0, lo=20, hi=128, mean_deg=30.0).to(DEV)
    A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem = preprocess_Hyper_fw_bw(g)
    Q, K, V = S.gt_features(g.num_nodes(), 1, 128, seed=8, device=DEV)
    dO = torch.randn(g.num_nodes(), 1, 128, generator=torch.Generator().manual_seed(5)).to(DEV)
    plan = gt.gt_ranked_pair_chosen(row_ptr, col_ind, val, Q)
    assert plan is not None and plan.num_dense_wide == 0
    out, attn_r = gt.gt_hyper_forward_ranked(row_ptr, col_ind, Q, K, V, plan=plan)
    dQ, dK, dV = gt.gt_backward_ranked(row_ptr, col_ind, Q, K, V, attn_r, dO, plan=plan)
    args = (row_ptr, col_ind, rows, val, col_ptr, row_ind, val_idx, smem, Q, K, V)
    out_a, attn = gt.gt_hyper_forward(*args)
    dQ_a, dK_a, dV_a = gt.gt_backward(*args, attn, dO)
    assert torch.equal(out, out_a) and torch.equal(dQ, dQ_a) and torch.equal(dK, dK_a) and torch.equal(dV, dV_a)
    ref = (_n(row_ptr), _n(col_ind), _n(val), _n(Q), _n(K), _n(V))
    want, want_attn = oracle_mod.gt_forward(*ref, want_attn=True)
    wq, wk, wv = oracle_mod.gt_backward(*ref, _n(dO))
    _close(out, want, "out"); _close(attn, want_attn, "attn_edge")
    _close(dQ, wq, "dQ"); _close(dK, wk, "dK"); _close(dV, wv, "dV")
    _close(gt.gt_hyper_inference(row_ptr, col_ind, rows, val, smem, Q, K, V)[0], want, "inference")
    out_s, mx, sm = gt.gt_hyper_forward_stats(row_ptr, col_ind, Q, K, V)
    _close(out_s, want, "out (statistics forward)")
    dQ_s, dK_s, dV_s = gt.gt_backward_stats(row_ptr, col_ind, Q, K, V, mx, sm, dO)
    _close(dQ_s, wq, "dQ (statistics)"); _close(dK_s, wk, "dK (statistics)"); _close(dV_s, wv, "dV (statistics)")


def test_statistics_pair_and_gat_read_the_descriptors(geometry, oracle_mod):
    """Two heads of 64 features: the statistics pair (unit and other edge values) and the rank-ordered pair's several-heads
    forward; the dense GAT forward, training forward and backward -- every range class, against the oracle."""
    import fused_gatconv as gat
    import fused_gtconv as gt
    from DFGNN.operators.fused_gatconv import GATConvFuse
    from DFGNN.operators.fused_gtconv import GTConvFuse_hyper
    from DFGNN.utils import synthetic as S
    from test_gpu_stats_pair import _close
    g, (A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem) = geometry
    m, h, f = g.num_nodes(), 2, 64
    Q, K, V = (t.requires_grad_(True) for t in S.gt_features(m, h, f, seed=7, device=DEV))
    dO = torch.randn(m, h, f, generator=torch.Generator().manual_seed(3)).to(DEV)
    assert gt.gt_stats_pair_chosen(row_ptr, col_ind, val, Q) is not None
    out = GTConvFuse_hyper(rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem, Q, K, V)
    dQ, dK, dV = torch.autograd.grad(out, (Q, K, V), dO)
    ref = (_n(row_ptr), _n(col_ind), _n(val), _n(Q), _n(K), _n(V))
    want = oracle_mod.gt_forward(*ref)
    wq, wk, wv = oracle_mod.gt_backward(*ref, _n(dO))
    _close(out, want, "out"); _close(dQ, wq, "dQ"); _close(dK, wk, "dK"); _close(dV, wv, "dV")
    Qd, Kd, Vd = Q.detach(), K.detach(), V.detach()
    out_r, attn_r = gt.gt_hyper_forward_ranked(row_ptr, col_ind, Qd, Kd, Vd)
    dQ_r, dK_r, dV_r = gt.gt_backward_ranked(row_ptr, col_ind, Qd, Kd, Vd, attn_r, dO)
    _close(out_r, want, "out (ranked)"); _close(dQ_r, wq, "dQ (ranked)"); _close(dK_r, wk, "dK (ranked)"); _close(dV_r, wv, "dV (ranked)")
    wval = (torch.rand(val.numel(), generator=torch.Generator().manual_seed(9)) * 2.5 - 1.0).to(DEV)
    out_w, mx, sm = gt.gt_hyper_forward_stats(row_ptr, col_ind, Qd, Kd, Vd, val=wval)
    dQ_w, dK_w, dV_w = gt.gt_backward_stats(row_ptr, col_ind, Qd, Kd, Vd, mx, sm, dO, val=wval)
    refw = (ref[0], ref[1], _n(wval)) + ref[3:]
    wq, wk, wv = oracle_mod.gt_backward(*refw, _n(dO))
    _close(out_w, oracle_mod.gt_forward(*refw), "out (weighted)")
    _close(dQ_w, wq, "dQ (weighted)"); _close(dK_w, wk, "dK (weighted)"); _close(dV_w, wv, "dV (weighted)")
    # GAT on the same batch
    ar, ac, X = (t.requires_grad_(True) for t in S.gat_features(m, h, f, seed=9, device=DEV))
    o = GATConvFuse(ar, ac, row_ptr, col_ind, col_ptr, row_ind, val_idx, 0.2, X, 0.0)
    gx, gr, gc = torch.autograd.grad(o, (X, ar, ac), dO)
    args = (_n(row_ptr), _n(col_ind), _n(ar), _n(ac), 0.2, _n(X))
    w_out, _, _ = oracle_mod.gat_train_forward(*args, None, 0.0)
    w_gf, w_gr, w_gc = oracle_mod.gat_backward(*args, _n(dO), None, 0.0)
    for got, refv, what in ((o, w_out, "out"), (gx, w_gf, "grad_feat"), (gr, w_gr, "grad_attn_row"), (gc, w_gc, "grad_attn_col")):
        _close(got, refv, f"GAT training {what}")
    _close(gat.gat_inference_hyper(smem, ar.detach(), ac.detach(), row_ptr, col_ind, rows, 0.2, X.detach()),
           oracle_mod.gat_forward(*args), "GAT inference")
