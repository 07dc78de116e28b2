"""GPU tests of the general statistics pair (include/dfgnn.h: dfgnn_gt_fwd_rowstats / dfgnn_gt_bwd_rowstats;
csrc/gt_train.hip): a GT training forward that saves two floats per (row, head) instead of attn_edge[h, nnz] on ANY
graph, and a backward that recomputes each edge's attention from the rows it gathers anyway.  Everything is compared with
the float64 CPU oracle (oracle/oracle.c) on identical inputs at the project's parity bar, as smoke() applies it:
max abs error < 1e-3 * max(1, max |ref|)."""
import numpy as np
import pytest
import torch

from conftest import csc_of, random_graph

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-3


def _np(t):
    return t.detach().cpu().numpy()


def _check(got, ref, what):
    """The parity bar; prints the measured figure first (pytest -s / a failing run shows it)."""
    got = _np(got).astype(np.float64) if isinstance(got, torch.Tensor) else np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    bound = BAR * max(1.0, float(np.abs(ref).max()) if ref.size else 0.0)
    print(f"rowstats {what}: max abs err {err:.3e} (bound {bound:.3e})")
    assert np.isfinite(got).all(), what
    assert err < bound, (what, err, bound)
    return err


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _row_stats(row_ptr, col_ind, val, Q, K):
    """float64 logit maximum and sum of exponentials per (row, head), from the oracle's logits val_e <Q_i, K_j>."""
    m, h, _ = Q.shape
    mx = np.full((m, h), -1e38)
    sm = np.zeros((m, h))
    for i in range(m):
        lo, hi = row_ptr[i], row_ptr[i + 1]
        if hi > lo:
            s = np.einsum("hf,jhf->jh", Q[i].astype(np.float64), K[col_ind[lo:hi]].astype(np.float64))
            s = s * val[lo:hi, None].astype(np.float64)
            mx[i] = s.max(axis=0)
            sm[i] = np.exp(s - mx[i]).sum(axis=0)
    return mx, sm


def _pair(row_ptr, col_ind, val, col_ptr, row_ind, val_idx, Q, K, V, dO):
    import fused_gtconv as gt
    out, mx, sm = gt.gt_forward_rowstats(row_ptr, col_ind, val, Q, K, V)
    dQ, dK, dV = gt.gt_backward_rowstats(row_ptr, col_ind, val, col_ptr, row_ind, val_idx, Q, K, V, out, mx, sm, dO)
    torch.cuda.synchronize()
    return out, mx, sm, dQ, dK, dV


def _against_oracle(oracle_mod, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, Q, K, V, dO, what):
    out, mx, sm, dQ, dK, dV = _pair(row_ptr, col_ind, val, col_ptr, row_ind, val_idx, Q, K, V, dO)
    args = (_np(row_ptr), _np(col_ind), _np(val), _np(Q), _np(K), _np(V))
    want = oracle_mod.gt_forward(*args)
    wq, wk, wv = oracle_mod.gt_backward(*args, _np(dO))
    for got, ref, name in ((out, want, "out"), (dQ, wq, "dQ"), (dK, wk, "dK"), (dV, wv, "dV")):
        _check(got, ref, f"{what} {name}")
    return out, mx, sm, dQ, dK, dV


FIXTURES = ["batch_small_h1_f128", "dups_selfloops_val_h2_f16", "multihead_h4_f32_isolated", "oddf_h2_f7", "oddf_h3_f20",
            "star1500_h1_f16", "star200_h1_f64"]


def test_fixture_list_is_complete(golden):
    assert sorted(golden) == FIXTURES


@pytest.mark.parametrize("name", FIXTURES)
def test_golden_fixtures(oracle_mod, golden, name):
    """Every stored fixture (weighted edges, duplicates, self-loops, isolated rows, f = 7, f = 20, a 1500-edge row): out,
    dQ, dK, dV against the oracle and against the stored arrays, the row statistics against numpy."""
    d = golden[name]
    row_ptr, col_ind, col_ptr, row_ind, val_idx = (_dev(d[k], torch.int32) for k in
                                                   ("row_ptr", "col_ind", "col_ptr", "row_ind", "val_idx"))
    val, Q, K, V, dO = (_dev(d[k], torch.float32) for k in ("val", "Q", "K", "V", "dO"))
    out, mx, sm, dQ, dK, dV = _against_oracle(oracle_mod, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, Q, K, V, dO, name)
    for got, key in ((out, "out"), (dQ, "dQ"), (dK, "dK"), (dV, "dV")):
        _check(got, d[key], f"{name} stored {key}")
    want_mx, want_sm = _row_stats(d["row_ptr"], d["col_ind"], d["val"], d["Q"], d["K"])
    empty = np.diff(d["row_ptr"]) == 0
    _check(_np(mx)[~empty], want_mx[~empty], f"{name} row_max")
    _check(sm, want_sm, f"{name} row_sum")
    assert (_np(mx)[empty] == np.float32(-1e38)).all() and (_np(sm)[empty] == 0).all()
    if name == "multihead_h4_f32_isolated":
        assert empty.any()
        assert (_np(out)[empty] == 0).all() and (_np(dQ)[empty] == 0).all()
        no_in = np.diff(d["col_ptr"]) == 0
        assert no_in.any()
        assert (_np(dK)[no_in] == 0).all() and (_np(dV)[no_in] == 0).all()


def _synthetic(kind):
    from DFGNN.utils import synthetic as S
    if kind == "cora":
        return S.cora_like()
    if kind == "peptides":
        return S.peptides_like(batch_size=256)
    if kind == "reddit":
        return S.reddit_like(scale=0.02)
    return S.pattern_like(batch_size=24)


@pytest.mark.parametrize("kind,h,f,weighted", [
    ("cora", 1, 64, False), ("cora", 8, 16, False),          # low-degree form with hub rows -> COOP
    ("peptides", 8, 16, False),                                # config 5 of BASELINE.json at full size
    ("reddit", 1, 128, False), ("reddit", 2, 64, False),       # wave form, rows of thousands of edges
    ("pattern", 1, 128, True),                                 # edge values: the CSC pass goes through val_idx
])
def test_forms_and_sizes(oracle_mod, kind, h, f, weighted):
    from DFGNN.layers import preprocess_Hyper_fw_bw
    from DFGNN.utils import synthetic as S
    g = _synthetic(kind).to(DEV)
    A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem = preprocess_Hyper_fw_bw(g)
    m, nnz = g.num_nodes(), col_ind.numel()
    low = nnz < 8 * m
    assert low == (kind in ("cora", "peptides"))                # the form each case is meant to take
    if kind == "cora":
        assert int((row_ptr[1:] - row_ptr[:-1]).max()) > 24     # a hub row: the COOP treatment
    if kind == "reddit":
        assert int((row_ptr[1:] - row_ptr[:-1]).max()) > 1000
    if weighted:
        val = (torch.rand(nnz, generator=torch.Generator().manual_seed(11)) + 0.5).to(DEV)
    Q, K, V = S.gt_features(m, h, f, seed=5, device=DEV)
    dO = torch.randn(m, h, f, generator=torch.Generator().manual_seed(3)).to(DEV)
    _against_oracle(oracle_mod, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, Q, K, V, dO, f"{kind} h{h} f{f}")


def _random_case(seed, m, avg_deg, h, f, max_deg=None, weighted=True, offset=0):
    """A random graph with empty rows, duplicate edges and one heavy row; features optionally `offset` floats into their
    storage (4 bytes off a 16-byte boundary: the scalar path)."""
    rng = np.random.default_rng(seed)
    indptr, indices, rows = random_graph(rng, m, avg_deg, empty_frac=0.1, dup_frac=0.05, max_deg=max_deg)
    col_ptr, row_ind, val_idx = csc_of(indptr, indices, rows, m)
    val = (rng.random(len(indices)) + 0.5).astype(np.float32) if weighted else np.ones(len(indices), np.float32)

    def feat(scale=1.0):
        base = torch.from_numpy((rng.standard_normal(m * h * f + offset) * scale).astype(np.float32)).to(DEV)
        t = base[offset:].view(m, h, f)
        assert t.is_contiguous() and t.data_ptr() % 16 == (4 * offset) % 16
        return t

    Q, K, V, dO = feat(f ** -0.25), feat(f ** -0.25), feat(), feat()
    graph = tuple(_dev(a, torch.int32) for a in (indptr, indices))
    csc = tuple(_dev(a, torch.int32) for a in (col_ptr, row_ind, val_idx))
    return graph + (_dev(val),) + csc + (Q, K, V, dO)


@pytest.mark.parametrize("avg_deg", [3, 20])                    # lane-group form / wave form
def test_width_20(oracle_mod, avg_deg):
    _against_oracle(oracle_mod, *_random_case(21, 700, avg_deg, 3, 20, max_deg=300), f"f20 deg{avg_deg}")


@pytest.mark.parametrize("avg_deg", [3, 20])
def test_unaligned_feature_pointers(oracle_mod, avg_deg):
    _against_oracle(oracle_mod, *_random_case(22, 500, avg_deg, 2, 16, max_deg=200, offset=1), f"unaligned deg{avg_deg}")


def _reddit_case(h, f):
    from DFGNN.layers import preprocess_Hyper_fw_bw
    from DFGNN.utils import synthetic as S
    g = S.reddit_like(scale=0.02).to(DEV)
    params = preprocess_Hyper_fw_bw(g)
    m = g.num_nodes()
    Q, K, V = S.gt_features(m, h, f, seed=7, device=DEV)
    dO = torch.randn(m, h, f, generator=torch.Generator().manual_seed(4)).to(DEV)
    return params, Q, K, V, dO


@pytest.mark.parametrize("h,f", [(1, 128), (2, 64)])
def test_public_surface_and_saved_state(h, f):
    """GTConvFuse_rowstats + autograd.grad equals the raw binding calls bit for bit; nothing of size h nnz in floating
    point is kept between forward and backward; one step peaks at least attn_edge (4 h nnz bytes) below GTConvFuse_hyper."""
    from DFGNN.operators.fused_gtconv import GTConvFuse_hyper, GTConvFuse_rowstats
    (A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem), Q, K, V, dO = _reddit_case(h, f)
    m, nnz = Q.size(0), col_ind.numel()
    assert nnz > m * f                                           # so that Q, K, V, out themselves are smaller than h nnz
    raw = _pair(row_ptr, col_ind, val, col_ptr, row_ind, val_idx, Q, K, V, dO)
    q, k, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
    out = GTConvFuse_rowstats(rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem, q, k, v)
    saved = out.grad_fn.saved_tensors
    big = [tuple(t.shape) for t in saved if t.is_floating_point() and t.numel() >= h * nnz]
    assert not big, big
    grads = torch.autograd.grad(out, (q, k, v), dO)
    assert torch.equal(out, raw[0])
    for a, b in zip(grads, raw[3:]):
        assert torch.equal(a, b)
    del out, saved, grads, raw

    def peak(op):
        q, k, v = (t.clone().requires_grad_(True) for t in (Q, K, V))

        def step():
            o = op(rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem, q, k, v)
            return torch.autograd.grad(o, (q, k, v), dO)

        step()                                                   # plan and other per-structure caches are built here
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base

    p_hyper, p_row = peak(GTConvFuse_hyper), peak(GTConvFuse_rowstats)
    print(f"rowstats peak of one fwd+bwd, h{h} f{f}: hyper {p_hyper} B, rowstats {p_row} B, 4 h nnz = {4 * h * nnz} B")
    assert p_hyper - p_row >= 4 * h * nnz


def test_layer_and_format_lookup():
    """SparseMHA_rowstats(fuse=True) in training mode against its own fuse=False branch (one head, where the two layouts
    coincide): output and projection-weight gradients; --conv gt --format forward_rowstats resolves."""
    import argparse

    from DFGNN.layers import SparseMHA_rowstats, load_graphconv_layer, load_prepfunc, preprocess_Hyper_fw_bw
    from DFGNN.layers.GT import SparseMHA_forward_timing, SparseMHA_rowstats_timing
    from DFGNN.utils import synthetic as S
    torch.manual_seed(1)
    g = S.cora_like().to(DEV)
    params = preprocess_Hyper_fw_bw(g)
    layer = SparseMHA_rowstats(64, 64, 1).to(DEV).train()
    x = torch.randn(g.num_nodes(), 64, device=DEV)
    outs, grads = [], []
    for fuse in (False, True):
        layer.zero_grad()
        out = layer(params, x, fuse=fuse)
        (out * torch.linspace(-1, 1, out.numel(), device=DEV).reshape(out.shape)).sum().backward()
        outs.append(out.detach())
        grads.append([p.grad.clone() for p in (layer.q_proj.weight, layer.k_proj.weight, layer.v_proj.weight)])
    _check(outs[1], _np(outs[0]), "layer out")
    for name, a, b in zip("qkv", *grads):
        _check(b, _np(a), f"layer d{name}_proj.weight")
    args = argparse.Namespace(conv="gt", format="forward_rowstats", dim=64, heads=1)
    assert isinstance(load_graphconv_layer(args), SparseMHA_rowstats_timing)
    assert load_prepfunc(args) is preprocess_Hyper_fw_bw
    out, ms = load_graphconv_layer(args).to(DEV).train()(params, x, fuse=True)
    assert out.shape == (g.num_nodes(), 64) and ms > 0
    args.format = "forward"
    assert type(load_graphconv_layer(args)) is SparseMHA_forward_timing


@pytest.mark.parametrize("shape", ["peptides", "reddit"])
def test_hipgraph_capture(shape):
    """fwd + bwd recorded into a HIP graph (one stream) replays bit-identically, also after Q / V were overwritten in place."""
    import fused_gtconv as gt
    from DFGNN.layers import preprocess_Hyper_fw_bw
    from DFGNN.utils import GraphedStep
    from DFGNN.utils import synthetic as S
    if shape == "peptides":
        g, h, f = S.peptides_like(batch_size=32, seed=3).to(DEV), 4, 32      # lane-group form
    else:
        g, h, f = S.reddit_like(scale=0.005).to(DEV), 1, 128                 # wave form
    A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem = preprocess_Hyper_fw_bw(g)
    m = g.num_nodes()
    Q, K, V = S.gt_features(m, h, f, seed=3, device=DEV)
    dO = torch.randn(m, h, f, device=DEV)

    def step():
        out, mx, sm = gt.gt_forward_rowstats(row_ptr, col_ind, val, Q, K, V)
        return [out] + list(gt.gt_backward_rowstats(row_ptr, col_ind, val, col_ptr, row_ind, val_idx, Q, K, V, out, mx, sm, dO))

    eager = [t.clone() for t in step()]
    graphed = GraphedStep(step)
    for a, b in zip(eager, graphed.replay()):
        assert torch.equal(a, b)
    Q.mul_(0.5)                                            # next "batch" of features, same structure
    V.add_(1.0)
    again = [t.clone() for t in graphed.replay()]
    for a, b in zip(step(), again):
        assert torch.equal(a, b)
    assert not torch.equal(again[0], eager[0])


def test_bindings_agree_and_backward_is_deterministic():
    """The torch C++ extension and the ctypes binding give bit-identical results (weighted and unit values, both forms), the
    same RuntimeError for a bad argument; two runs of the backward agree bit for bit (no atomics)."""
    import dfgnn_native
    assert dfgnn_native.ext() is not None and hasattr(dfgnn_native.ext(), "gt_bwd_rowstats")
    cases = [_random_case(31, 600, 3, 2, 32, max_deg=100), _random_case(32, 400, 25, 4, 16, max_deg=900),
             _random_case(33, 400, 25, 1, 64, max_deg=900, weighted=False)]

    def run():
        import fused_gtconv as gt
        res = []
        for c in cases:
            res += list(_pair(*c))
        try:
            c = cases[0]
            gt.gt_forward_rowstats(c[0].long(), *c[1:3], *c[6:9])
            err = None
        except RuntimeError as e:
            err = str(e)
        return res, err

    via_ext, err_ext = run()
    again, _ = run()
    saved = dfgnn_native._ext
    dfgnn_native._ext = None                      # force the ctypes path
    try:
        via_ctypes, err_ctypes = run()
    finally:
        dfgnn_native._ext = saved
    assert len(via_ext) == len(via_ctypes) == 18
    for a, b, c in zip(via_ext, via_ctypes, again):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert err_ext and err_ctypes and "int32" in err_ext and "int32" in err_ctypes


def test_operator_with_edge_values_and_inference_form():
    """GTConvFuse_rowstats with edge values other than ones (the one case in which `val` is kept for the backward) equals the
    raw calls bit for bit; the C ABI's forward without statistics (row_max = row_sum = NULL: inference) gives the same out."""
    import dfgnn_native
    from _binding_util import stream_ptr
    from DFGNN.operators.fused_gtconv import GTConvFuse_rowstats
    for avg_deg in (3, 20):
        row_ptr, col_ind, val, col_ptr, row_ind, val_idx, Q, K, V, dO = _random_case(41, 500, avg_deg, 2, 32, max_deg=150)
        raw = _pair(row_ptr, col_ind, val, col_ptr, row_ind, val_idx, Q, K, V, dO)
        q, k, v = (t.clone().requires_grad_(True) for t in (Q, K, V))
        out = GTConvFuse_rowstats(None, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, 0, q, k, v)
        assert any(t.data_ptr() == val.data_ptr() for t in out.grad_fn.saved_tensors)
        grads = torch.autograd.grad(out, (q, k, v), dO)
        assert torch.equal(out, raw[0])
        for a, b in zip(grads, raw[3:]):
            assert torch.equal(a, b)
        m, h, f = Q.shape
        plain = torch.full_like(Q, float("nan"))
        rc = dfgnn_native.lib().dfgnn_gt_fwd_rowstats(m, col_ind.numel(), h, f, row_ptr.data_ptr(), col_ind.data_ptr(),
                                                      val.data_ptr(), Q.data_ptr(), K.data_ptr(), V.data_ptr(), None, None,
                                                      plain.data_ptr(), stream_ptr(Q.device))
        torch.cuda.synchronize()
        assert rc == 0 and torch.equal(plain, raw[0])
