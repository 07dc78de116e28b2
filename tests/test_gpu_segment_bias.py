"""GPU: the segment attention pair with a pair bias (include/dfgnn_segment_bias.h) against a plain per-segment torch loop in
float64 with the bias added.  Batches, shapes, inputs and the bound are those of tests/test_gpu_segment_mha.py (MARGIN x the
same loop in float32 against float64; nothing of the kernel enters it), bias ~ N(0, 1).  dbias [h, n_pairs] is measured like
attn_edge, grouped by pair row.
Measured on MI355X: the worst shares of the bound are dQ 0.70, row_max 0.41 and dbias 0.38 (long batch, h=8 f=16); every
other output of every case is below 0.33."""
import functools

import numpy as np
import pytest
import torch

import parity_cases as P
from conftest import has_gpu
from test_gpu_segment_mha import BATCHES, SHAPES, _close, seg_ptr_of

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]
OUTPUTS = ("out", "row_max", "row_sum", "dQ", "dK", "dV", "dbias")


def pair_rows_of(sizes):
    n = np.asarray(sizes, dtype=np.int64)
    pair_ptr = np.concatenate([[0], np.cumsum(n * n)])
    row_off = np.concatenate([pair_ptr[g] + np.arange(k) * k for g, k in enumerate(n)] + [np.zeros(0, dtype=np.int64)])
    return pair_ptr, row_off.astype(np.int64)


def reference(sizes, x, dtype):
    """Every output of the biased pair by a loop over the segments in `dtype` on the CPU (scale 1)."""
    Q, K, V, dO, bias = (torch.from_numpy(x[k]).to(dtype) for k in ("Q", "K", "V", "dO", "bias"))
    m, h, _ = Q.shape
    r = {k: torch.zeros_like(Q) for k in ("out", "dQ", "dK", "dV")}
    r["row_max"], r["row_sum"], r["dbias"] = torch.zeros(m, h, dtype=dtype), torch.zeros(m, h, dtype=dtype), torch.zeros_like(bias)
    ends, pair_ptr = seg_ptr_of(sizes).tolist(), pair_rows_of(sizes)[0].tolist()
    for lo, hi, at in zip(ends[:-1], ends[1:], pair_ptr):
        n = hi - lo
        if n == 0:
            continue
        q, k, v, g = (a[lo:hi].transpose(0, 1) for a in (Q, K, V, dO))      # [h, n, f]
        s = q @ k.transpose(1, 2) + bias[:, at:at + n * n].reshape(h, n, n)
        mx = s.max(dim=2, keepdim=True).values
        e = torch.exp(s - mx)
        sm = e.sum(dim=2, keepdim=True)
        p = e / sm
        dp = g @ v.transpose(1, 2)
        ds = p * (dp - (p * dp).sum(dim=2, keepdim=True))
        for name, val in (("out", p @ v), ("dQ", ds @ k), ("dK", ds.transpose(1, 2) @ q), ("dV", p.transpose(1, 2) @ g)):
            r[name][lo:hi] = val.transpose(0, 1)
        r["row_max"][lo:hi], r["row_sum"][lo:hi] = mx[:, :, 0].T, sm[:, :, 0].T
        r["dbias"][:, at:at + n * n] = ds.reshape(h, n * n)
    return {k: v.numpy() for k, v in r.items()}


@functools.lru_cache(maxsize=None)
def case(batch, h, f):
    """-> (inputs float32, ref64, bounds per output, pair-row starts int64[m + 1]); computed once, nobody writes to it."""
    sizes = BATCHES[batch]
    m = int(sum(sizes))
    rng = np.random.default_rng(2000 * h + f + len(sizes))
    x = {k: rng.standard_normal((m, h, f)) * (f ** -0.25 if k in "QK" else 1.0) for k in ("Q", "K", "V", "dO")}
    ends = seg_ptr_of(sizes)
    for lo in ends[:-1][np.diff(ends) == 1]:     # (1-node segments: dQ = dK = 0 exactly, test_gpu_segment_mha.py says why)
        v = x["V"][lo]
        x["dO"][lo] -= (x["dO"][lo] * v).sum(-1, keepdims=True) / (v * v).sum(-1, keepdims=True) * v
    pair_ptr, row_off = pair_rows_of(sizes)
    x["bias"] = rng.standard_normal((h, int(pair_ptr[-1])))
    x = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in x.items()}
    starts = np.concatenate([row_off, pair_ptr[-1:]])
    ref64, ref32 = reference(sizes, x, torch.float64), reference(sizes, x, torch.float32)
    rows = {k: starts if k == "dbias" else None for k in OUTPUTS}     # dbias [h, n_pairs] is grouped by pair row
    return x, ref64, {k: P.MARGIN * P.worst(ref32[k], ref64[k], row_ptr=rows[k]) for k in OUTPUTS}, starts


def run_pair(sizes, x, stats=True, dbias=True, alloc=None):
    """The C entries -> dict of outputs made by alloc(name, shape, dtype) (default: NaN / -7 filled tensors)."""
    from _binding_util import call
    dev = torch.device("cuda")
    t = {k: v if isinstance(v, torch.Tensor) else torch.from_numpy(v).to(dev) for k, v in x.items()}
    m, h, f = t["Q"].shape
    n_pairs = t["bias"].size(1)
    seg_ptr = t["seg_ptr"] if "seg_ptr" in t else torch.from_numpy(seg_ptr_of(sizes)).to(dev)
    n_seg = seg_ptr.numel() - 1
    if alloc is None:
        alloc = lambda name, shape, dtype=torch.float32: torch.full(  # noqa: E731
            shape, float("nan") if dtype == torch.float32 else -7, dtype=dtype, device=dev)
    o = dict(bounds=alloc("bounds", (2 * m,), torch.int32), pair_ptr=alloc("pair_ptr", (2 * (n_seg + 1),), torch.int32),
             row_off=alloc("row_off", (2 * m,), torch.int32), out=alloc("out", (m, h, f)))    # (int64 as pairs of int32)
    call("dfgnn_segment_bounds", "bounds", dev, m, n_seg, seg_ptr, o["bounds"])
    call("dfgnn_segment_pair_rows", "pair_rows", dev, m, n_seg, seg_ptr, o["pair_ptr"], o["row_off"])
    head = (m, h, f, 1.0, o["bounds"], o["row_off"], n_pairs, t["bias"], t["Q"], t["K"], t["V"])
    if not stats:
        call("dfgnn_segment_mha_bias_fwd", "fwd", dev, *head, o["out"], None, None)
        return o
    o.update({k: alloc(k, (m, h)) for k in ("row_max", "row_sum", "delta")})
    o.update({k: alloc(k, (m, h, f)) for k in ("dQ", "dK", "dV")})
    if dbias:
        o["dbias"] = alloc("dbias", (h, n_pairs))
    call("dfgnn_segment_mha_bias_fwd", "fwd", dev, *head, o["out"], o["row_max"], o["row_sum"])
    call("dfgnn_segment_mha_bias_bwd", "bwd", dev, *head, o["row_max"], o["row_sum"], t["dO"], o["dQ"], o["dK"], o["dV"],
         o.get("dbias"), o["delta"])
    return o


@pytest.mark.parametrize("h,f", SHAPES)
@pytest.mark.parametrize("batch", BATCHES)
def test_pair_at_fp32_level(batch, h, f):
    sizes = BATCHES[batch]
    x, ref64, bound, starts = case(batch, h, f)
    got = run_pair(sizes, x)
    pair_ptr, row_off = pair_rows_of(sizes)
    assert np.array_equal(got["pair_ptr"].view(torch.int64).cpu().numpy(), pair_ptr)
    assert np.array_equal(got["row_off"].view(torch.int64).cpu().numpy(), row_off)
    errs = {k: P.worst(got[k].cpu().numpy(), ref64[k], row_ptr=starts if k == "dbias" else None) for k in OUTPUTS}
    print(f"{batch} h={h} f={f}: " + ", ".join(f"{k} {errs[k] / bound[k]:.3f}" for k in OUTPUTS) + " of the bound")
    for k in OUTPUTS:
        assert errs[k] <= bound[k], (k, errs[k], bound[k])
    assert all(torch.equal(a, b) for a, b in zip(run_pair(sizes, x).values(), got.values())), "two calls, two results"
    assert torch.equal(run_pair(sizes, x, stats=False)["out"], got["out"]), "inference differs from the training forward"
    without = run_pair(sizes, x, dbias=False)
    assert all(torch.equal(without[k], got[k]) for k in ("dQ", "dK", "dV")), "dbias = NULL changes the other gradients"


@pytest.mark.parametrize("n", (129, 640))
def test_a_bias_that_decides(n):
    """Rows whose bias is -1e30 on all keys but one, the first and the last key of the graph: out is that key's V row and
    dbias is 0 on the masked pairs (P = 0 there).  With P = 1 the only error of out is that of V's two-half fp16 image,
    2^-22 of its power-of-two scale, which is below twice the largest |V|: 2^-21 < 1e-6."""
    h, f = 2, 32
    rng = np.random.default_rng(n)
    x = {k: rng.standard_normal((n, h, f)).astype(np.float32) for k in ("Q", "K", "V", "dO")}
    bias = rng.standard_normal((h, n, n)).astype(np.float32)
    rows, keys = np.array([0, 1, n // 2, n - 1]), np.array([0, n - 1, n - 1, 0])
    bias[:, rows] = -1e30
    bias[:, rows, keys] = 0.5
    x["bias"] = bias.reshape(h, n * n)
    got = run_pair((n,), x)
    want = torch.from_numpy(x["V"][keys]).cuda()
    assert float((got["out"][rows] - want).abs().max()) <= 1e-6 * float(np.abs(x["V"]).max())
    db = got["dbias"].reshape(h, n, n)[:, rows].cpu().numpy()
    assert (db == 0).all()       # masked pairs: P = 0 exactly; the surviving pair: dS = 1 (dP - dP) = 0
    assert bool(torch.isfinite(got["dbias"]).all())


def test_guarded_buffers():
    """Every output -- dbias, pair_ptr and row_off included -- between sentinel-filled guards (tests/guarded.py): all of it
    written and finite, no guard touched, no input modified."""
    from guarded import Arena
    batch, h, f = "boundary", 2, 64
    x, _, _, _ = case(batch, h, f)
    a = Arena("cuda")
    t = {k: a.input(k, v) for k, v in x.items()}
    t["seg_ptr"] = a.input("seg_ptr", seg_ptr_of(BATCHES[batch]))
    scratch = lambda name, shape, dtype=torch.float32: (  # noqa: E731
        a.scratch(name, int(np.prod(shape))) if name == "delta" else a.output(name, shape, dtype=dtype))
    o = run_pair(BATCHES[batch], t, alloc=scratch)
    a.verify()
    assert bool(torch.isfinite(o["delta"]).all())


def test_autograd_round_trip_and_layer():
    from DFGNN.layers import GlobalMHA, PairBias
    from DFGNN.operators.fused_gtconv import SegmentMHABiasFuse
    dev = torch.device("cuda")
    torch.manual_seed(4)
    sizes = torch.tensor([0, 40, 1, 130, 0, 23])
    ends = [0] + torch.cumsum(sizes, 0).tolist()
    seg_ptr = torch.tensor(ends, dtype=torch.int32, device=dev)
    m, h, f, n_pairs = ends[-1], 4, 32, int((sizes * sizes).sum())
    plain = GlobalMHA(h * f, h * f, h)            # (forward_plain only: scaling 32^-0.5)
    leaves = [torch.randn(m, h, f, device=dev, requires_grad=True) for _ in range(3)]
    leaves.append(torch.randn(h, n_pairs, device=dev, requires_grad=True))
    w = torch.randn(m, h, f, device=dev)
    grads = []
    for fn in (lambda q, k, v, b: SegmentMHABiasFuse(seg_ptr, q, k, v, b, plain.scaling),
               lambda q, k, v, b: plain.forward_plain(seg_ptr, q, k, v, b)):
        out = fn(*leaves)
        grads.append([out.detach()] + list(torch.autograd.grad((out * w).sum(), leaves)))
    assert all(_close(a, b) for a, b in zip(*grads))
    q, k, v, b = leaves
    out = SegmentMHABiasFuse(seg_ptr, q, k, v, b.detach(), plain.scaling)      # no gradient asked for the bias: NULL
    assert all(torch.equal(x, y) for x, y in zip(torch.autograd.grad((out * w).sum(), (q, k, v)), grads[0][1:4]))

    x = torch.randn(m, 64, device=dev)
    types = torch.randint(0, 6, (n_pairs,), device=dev)
    for heads, out_size, fused in ((4, 128, True), (2, 96, False)):    # head width 32; 48: the torch branch, silently
        layer, enc = GlobalMHA(64, out_size, heads).to(dev), PairBias(6, heads).to(dev)
        res = []
        for fuse, segments in ((True, sizes), (False, seg_ptr)):
            layer.zero_grad()
            enc.zero_grad()
            y = layer(x, segments, fuse=fuse, bias=enc(types))
            y.square().sum().backward()
            res.append([y.detach(), enc.table.grad.clone()] + [p.grad.clone() for p in layer.parameters()])
        assert all(_close(a, b) for a, b in zip(*res))
        assert fused != torch.equal(res[0][0], res[1][0])
