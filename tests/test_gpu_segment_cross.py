"""GPU: the segment cross attention pair (include/dfgnn_segment_cross.h), both forms, against a plain per-segment torch loop
in float64 on the CPU.

The bound is that of tests/test_gpu_segment_mha.py: parity_cases.MARGIN x the error of the same loop in float32, on the
same inputs (Q, K ~ N(0, 1) f^-1/4, V, dO ~ N(0, 1), scale 1); nothing of the kernel enters it.  Where a key segment has one
row, P = 1 and dQ = dK = 0 exactly, so the dO rows of its queries are made orthogonal to that key's V in float64 before
the cast."""
import functools

import numpy as np
import pytest
import torch

import parity_cases as P
import test_gpu_segment_mha as S
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

WIDE, SPLIT = 1, 2
# (query sizes, key sizes) per segment.  readout: one query per graph, keys on, before and after block (32), tile (128) and
# strip edges, empty graphs, a strip whose keys span several tiles.  boundary: strip and window edges on the query side against
# the same on the key side, empty queries over 129 keys, 1 query over 0 keys, 128 queries over 3 keys.  long: windows inside
# one segment, multi-tile key ranges, a few queries over many keys.
BATCHES = {
    "readout": ((1,) * 20, (0, 1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 0, 5, 300, 40)),
    "boundary": ((0, 1, 2, 3, 15, 16, 17, 0, 63, 64, 65, 127, 128, 129, 0), (129, 0, 128, 127, 1, 65, 64, 63, 17, 0, 16, 15, 3, 2, 1)),
    "long": ((257, 5, 300, 8), (5, 640, 130, 700)),
}
OUTPUTS = S.OUTPUTS
ptr_of = S.seg_ptr_of


def reference(qsizes, ksizes, x, dtype):
    """Every output of the pair by a loop over the segments in `dtype` on the CPU (scale 1)."""
    Q, K, V, dO = (torch.from_numpy(x[k]).to(dtype) for k in ("Q", "K", "V", "dO"))
    h = Q.shape[1]
    r = dict(out=torch.zeros_like(Q), dQ=torch.zeros_like(Q), dK=torch.zeros_like(K), dV=torch.zeros_like(K),
             row_max=torch.full((len(Q), h), -1e38, dtype=dtype), row_sum=torch.zeros(len(Q), h, dtype=dtype))
    eq, ek = ptr_of(qsizes).tolist(), ptr_of(ksizes).tolist()
    for a, b, lo, hi in zip(eq[:-1], eq[1:], ek[:-1], ek[1:]):
        if a == b or lo == hi:
            continue
        q, g = (t[a:b].transpose(0, 1) for t in (Q, dO))         # [h, n, f]
        k, v = (t[lo:hi].transpose(0, 1) for t in (K, V))
        s = q @ k.transpose(1, 2)
        mx = s.max(dim=2, keepdim=True).values
        e = torch.exp(s - mx)
        sm = e.sum(dim=2, keepdim=True)
        p = e / sm
        dp = g @ v.transpose(1, 2)
        ds = p * (dp - (p * dp).sum(dim=2, keepdim=True))
        r["out"][a:b], r["dQ"][a:b] = (p @ v).transpose(0, 1), (ds @ k).transpose(0, 1)
        r["dK"][lo:hi], r["dV"][lo:hi] = (ds.transpose(1, 2) @ q).transpose(0, 1), (p.transpose(1, 2) @ g).transpose(0, 1)
        r["row_max"][a:b], r["row_sum"][a:b] = mx[:, :, 0].T, sm[:, :, 0].T
    return {k: v.numpy() for k, v in r.items()}


@functools.lru_cache(maxsize=None)
def case(batch, h, f):
    """-> (inputs float32, ref64, bounds per output); computed once, nobody writes to it."""
    qsizes, ksizes = BATCHES[batch]
    rng = np.random.default_rng(1000 * h + f + len(qsizes))
    x = {k: rng.standard_normal((int(sum(qsizes if k in ("Q", "dO") else ksizes)), h, f)) * (f ** -0.25 if k in "QK" else 1.0)
         for k in ("Q", "K", "V", "dO")}
    eq, ek = ptr_of(qsizes), ptr_of(ksizes)
    for g in np.flatnonzero(np.diff(ek) == 1):
        v, rows = x["V"][ek[g]], slice(eq[g], eq[g + 1])
        x["dO"][rows] -= (x["dO"][rows] * v).sum(-1, keepdims=True) / (v * v).sum(-1, keepdims=True) * v
    x = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in x.items()}
    ref64, ref32 = reference(qsizes, ksizes, x, torch.float64), reference(qsizes, ksizes, x, torch.float32)
    return x, ref64, {k: P.MARGIN * P.worst(ref32[k], ref64[k]) for k in OUTPUTS}


def run_pair(x, qsizes, ksizes, form, stats=True, alloc=None):
    """The C entries on NaN-filled outputs -> dict of tensors (the bounds, the six outputs, delta).  alloc: a guarded Arena."""
    from _binding_util import call
    dev = torch.device("cuda")
    (m_q, h, f), m_k = x["Q"].shape, x["K"].shape[0]
    if alloc is None:
        t = {k: torch.from_numpy(v).to(dev) for k, v in x.items()}
        sq, sk = (torch.from_numpy(ptr_of(s)).to(dev) for s in (qsizes, ksizes))
        new = lambda name, shape, dtype=torch.float32: torch.full(  # noqa: E731
            shape, float("nan") if dtype == torch.float32 else -7, dtype=dtype, device=dev)
    else:
        t = {k: alloc.input(k, v) for k, v in x.items()}
        sq, sk = alloc.input("seg_ptr_q", ptr_of(qsizes)), alloc.input("seg_ptr_k", ptr_of(ksizes))
        new = alloc.output
    o = dict(qbounds=new("qbounds", (2 * m_q,), torch.int32), kbounds=new("kbounds", (2 * m_k,), torch.int32), out=new("out", (m_q, h, f)))
    call("dfgnn_segment_cross_bounds", "bounds", dev, m_q, m_k, len(qsizes), sq, sk, o["qbounds"], o["kbounds"])
    if not stats:
        call("dfgnn_segment_mha_cross_fwd", "fwd", dev, m_q, m_k, h, f, 1.0, form, o["qbounds"], t["Q"], t["K"], t["V"], o["out"], None, None)
        return o
    o.update(row_max=new("row_max", (m_q, h)), row_sum=new("row_sum", (m_q, h)), dQ=new("dQ", (m_q, h, f)),
             dK=new("dK", (m_k, h, f)), dV=new("dV", (m_k, h, f)))
    o["delta"] = new("delta", (m_q, h)) if alloc is None else alloc.scratch("delta", m_q * h)
    call("dfgnn_segment_mha_cross_fwd", "fwd", dev, m_q, m_k, h, f, 1.0, form, o["qbounds"], t["Q"], t["K"], t["V"], o["out"],
         o["row_max"], o["row_sum"])
    call("dfgnn_segment_mha_cross_bwd", "bwd", dev, m_q, m_k, h, f, 1.0, form, o["qbounds"], o["kbounds"], t["Q"], t["K"], t["V"],
         o["row_max"], o["row_sum"], t["dO"], o["dQ"], o["dK"], o["dV"], o["delta"])
    return o


def within(got, ref64, bound, what):
    errs = {k: P.worst(got[k].cpu().numpy(), ref64[k]) for k in OUTPUTS}
    print(f"{what}: " + ", ".join(f"{k} {errs[k] / bound[k] if bound[k] else errs[k]:.3f}" for k in OUTPUTS) + " of the bound")
    for k in OUTPUTS:
        assert errs[k] <= bound[k], (k, errs[k], bound[k])


def other_side_bounds(mine, other):
    """numpy: per row of `mine` the range of its segment in `other`."""
    seg = np.searchsorted(mine, np.arange(mine[-1]), side="right") - 1
    return np.stack([other[seg], other[seg + 1]], axis=1)


@pytest.mark.parametrize("h,f", S.SHAPES)
@pytest.mark.parametrize("batch", BATCHES)
@pytest.mark.parametrize("form", (WIDE, SPLIT))
def test_pair_at_fp32_level(form, batch, h, f):
    x, ref64, bound = case(batch, h, f)
    qsizes, ksizes = BATCHES[batch]
    got = run_pair(x, qsizes, ksizes, form)
    eq, ek = ptr_of(qsizes), ptr_of(ksizes)
    assert np.array_equal(got["qbounds"].cpu().numpy().reshape(-1, 2), other_side_bounds(eq, ek))
    assert np.array_equal(got["kbounds"].cpu().numpy().reshape(-1, 2), other_side_bounds(ek, eq))
    within(got, ref64, bound, f"form {form} {batch} h={h} f={f}")
    assert all(torch.equal(a, b) for a, b in zip(run_pair(x, qsizes, ksizes, form).values(), got.values())), "two calls, two results"
    assert torch.equal(run_pair(x, qsizes, ksizes, form, stats=False)["out"], got["out"]), "inference differs from the training forward"


@pytest.mark.parametrize("h,f", S.SHAPES)
def test_square_equals_the_self_pair(h, f):
    """seg_ptr_q == seg_ptr_k and the same arrays on both sides: WIDE returns the self pair's bits, SPLIT stays in the bound."""
    x, ref64, bound = S.case("boundary", h, f)
    sizes = S.BATCHES["boundary"]
    self_pair = S.run_pair("boundary", h, f)
    wide = run_pair(x, sizes, sizes, WIDE)
    assert torch.equal(wide["qbounds"], self_pair["bounds"]) and torch.equal(wide["kbounds"], self_pair["bounds"])
    assert all(torch.equal(wide[k], self_pair[k]) for k in OUTPUTS + ("delta",))
    within(run_pair(x, sizes, sizes, SPLIT), ref64, bound, f"split, square h={h} f={f}")


@pytest.mark.parametrize("form", (WIDE, SPLIT))
def test_guarded_buffers(form):
    """Every output element written -- the zero rows of dK / dV under empty query segments too --, no guard touched, no input
    modified (tests/guarded.py)."""
    from guarded import Arena
    x, _, _ = case("boundary", 2, 64)
    a = Arena("cuda")
    o = run_pair(x, *BATCHES["boundary"], form, alloc=a)
    a.verify()
    assert bool(torch.isfinite(o["delta"]).all())


def _plain(eq, ek, q, k, v, scale):
    outs = []
    for a, b, lo, hi in zip(eq[:-1], eq[1:], ek[:-1], ek[1:]):
        s = torch.einsum("ihf,jhf->hij", q[a:b], k[lo:hi]) * scale
        outs.append(torch.einsum("hij,jhf->ihf", torch.softmax(s, dim=-1), v[lo:hi]) if hi > lo else torch.zeros_like(q[a:b]))
    return torch.cat(outs)


def test_autograd_round_trip_and_layers():
    from DFGNN.layers import AttentionReadout, CrossMHA
    from DFGNN.operators.fused_gtconv import SegmentCrossMHAFuse
    dev = torch.device("cuda")
    torch.manual_seed(5)
    qs, ks = torch.tensor([3, 0, 17, 2, 130]), torch.tensor([40, 9, 0, 1, 23])
    eq, ek = ([0] + torch.cumsum(s, 0).tolist() for s in (qs, ks))
    sq, sk = (torch.tensor(e, dtype=torch.int32, device=dev) for e in (eq, ek))
    h, f = 4, 32
    leaves = [torch.randn(n, h, f, device=dev, requires_grad=True) for n in (eq[-1], ek[-1], ek[-1])]
    w = torch.randn(eq[-1], h, f, device=dev)
    for form in (0, WIDE, SPLIT):
        grads = []
        for fn in (lambda q, k, v: SegmentCrossMHAFuse(sq, sk, q, k, v, 0.25, form), lambda q, k, v: _plain(eq, ek, q, k, v, 0.25)):
            out = fn(*leaves)
            grads.append([out.detach()] + list(torch.autograd.grad((out * w).sum(), leaves)))
        assert all(S._close(a, b) for a, b in zip(*grads))
        with torch.no_grad():
            assert torch.equal(SegmentCrossMHAFuse(sq, sk, *leaves, 0.25, form), grads[0][0])   # (the inference forward)

    hq, hk = torch.randn(eq[-1], 48, device=dev), torch.randn(ek[-1], 64, device=dev)
    for heads, out_size, fused in ((4, 128, True), (2, 96, False)):    # head width 32; 48: the torch branch, silently
        cross, readout = CrossMHA(48, 64, out_size, heads).to(dev), AttentionReadout(64, out_size, heads, num_seeds=3).to(dev)
        for layer, run in ((cross, lambda fuse: cross(hq, hk, qs if fuse else sq, sk, fuse=fuse)),
                           (readout, lambda fuse: readout(hk, ks if fuse else sk, fuse=fuse))):
            res = []
            for fuse in (True, False):
                layer.zero_grad()
                y = run(fuse)
                y.square().sum().backward()
                res.append([y.detach()] + [p.grad.clone() for p in layer.parameters()])
            assert all(S._close(a, b) for a, b in zip(*res))
            assert fused != all(torch.equal(a, b) for a, b in zip(*res))
        y = readout(hk, sk)
        assert y.shape == (5, 3 * out_size) and not bool(y[2].any()) and bool(y[3].any())   # the graph without nodes: zeros


@pytest.mark.parametrize("n_seg,m_q,m_k", ((0, 0, 0), (3, 0, 0), (3, 0, 5), (3, 5, 0)))
def test_empty_sides(n_seg, m_q, m_k):
    """No rows on one side or on both: full-shape outputs, zeros where something is written."""
    import fused_gtconv as G
    dev = torch.device("cuda")
    sq, sk = (torch.tensor([0] * n_seg + [m], dtype=torch.int32, device=dev) for m in (m_q, m_k))
    q, k = torch.randn(m_q, 2, 32, device=dev), torch.randn(m_k, 2, 32, device=dev)
    qb, kb = G.segment_cross_bounds(sq, sk, m_q, m_k)
    for form in (WIDE, SPLIT):
        out, row_max, row_sum = G.segment_mha_cross_forward(qb, q, k, k, form=form)
        dQ, dK, dV = G.segment_mha_cross_backward(qb, kb, q, k, k, row_max, row_sum, q, form=form)
        assert out.shape == dQ.shape == q.shape and dK.shape == dV.shape == k.shape
        assert not any(bool(t.any()) for t in (out, row_sum, dQ, dK, dV)) and bool((row_max == -1e38).all())
