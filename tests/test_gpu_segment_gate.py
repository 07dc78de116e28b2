"""GPU: the segment attention pair with pair gates and a logit output (include/dfgnn_segment_gate.h) against a plain
per-segment torch loop in float64.  Batches, shapes, inputs and the bound are those of tests/test_gpu_segment_bias.py (MARGIN x
the same loop in float32 against float64; nothing of the kernel enters it), gate ~ N(0, 1), dlogits ~ N(0, 1); the three output
planes [h, n_pairs] are measured grouped by pair row, as dbias is.
Measured on MI355X: the worst shares of the bound are dgate 0.42 (boundary batch, h=8 f=16) and row_max 0.41 (long batch,
h=8 f=16); every other output of every case is below 0.33."""
import functools

import numpy as np
import pytest
import torch

import parity_cases as P
from conftest import has_gpu
from test_gpu_segment_bias import pair_rows_of
from test_gpu_segment_bias import run_pair as run_bias_pair
from test_gpu_segment_mha import BATCHES, SHAPES, _close, seg_ptr_of

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]
PLANES = ("logits", "dbias", "dgate")
OUTPUTS = ("out", "row_max", "row_sum", "dQ", "dK", "dV") + PLANES


def reference(sizes, x, dtype):
    """Every output of the gated pair by a loop over the segments in `dtype` on the CPU (scale 1)."""
    Q, K, V, dO, bias, gate, dlogits = (torch.from_numpy(x[k]).to(dtype) for k in ("Q", "K", "V", "dO", "bias", "gate", "dlogits"))
    m, h, _ = Q.shape
    r = {k: torch.zeros_like(Q) for k in ("out", "dQ", "dK", "dV")}
    r.update({k: torch.zeros(m, h, dtype=dtype) for k in ("row_max", "row_sum")})
    r.update({k: torch.zeros_like(bias) for k in PLANES})
    ends, pair_ptr = seg_ptr_of(sizes).tolist(), pair_rows_of(sizes)[0].tolist()
    for lo, hi, at in zip(ends[:-1], ends[1:], pair_ptr):
        n = hi - lo
        if n == 0:
            continue
        q, k, v, g = (a[lo:hi].transpose(0, 1) for a in (Q, K, V, dO))      # [h, n, f]
        block = lambda a: a[:, at:at + n * n].reshape(h, n, n)  # noqa: E731
        s = q @ k.transpose(1, 2) + block(bias)
        mx = s.max(dim=2, keepdim=True).values
        e = torch.exp(s - mx)
        sm = e.sum(dim=2, keepdim=True)
        p, sg = e / sm, 1 / (1 + torch.exp(-block(gate)))
        da = g @ v.transpose(1, 2)
        ds = p * (sg * da - (p * sg * da).sum(dim=2, keepdim=True)) + block(dlogits)
        for name, val in (("out", (p * sg) @ v), ("dQ", ds @ k), ("dK", ds.transpose(1, 2) @ q), ("dV", (p * sg).transpose(1, 2) @ g)):
            r[name][lo:hi] = val.transpose(0, 1)
        r["row_max"][lo:hi], r["row_sum"][lo:hi] = mx[:, :, 0].T, sm[:, :, 0].T
        for name, val in (("logits", s), ("dbias", ds), ("dgate", da * p * sg * (1 - sg))):
            r[name][:, at:at + n * n] = val.reshape(h, n * n)
    return {k: v.numpy() for k, v in r.items()}


@functools.lru_cache(maxsize=None)
def case(batch, h, f):
    """-> (inputs float32, ref64, bounds per output, pair-row starts int64[m + 1]); computed once, nobody writes to it."""
    sizes, m = BATCHES[batch], int(sum(BATCHES[batch]))
    rng = np.random.default_rng(2000 * h + f + len(sizes))
    x = {k: rng.standard_normal((m, h, f)) * (f ** -0.25 if k in "QK" else 1.0) for k in ("Q", "K", "V", "dO")}
    ends = seg_ptr_of(sizes)
    for lo in ends[:-1][np.diff(ends) == 1]:     # (1-node segments, as in the bias test: dQ = dK = 0 when dlogits is NULL)
        v = x["V"][lo]
        x["dO"][lo] -= (x["dO"][lo] * v).sum(-1, keepdims=True) / (v * v).sum(-1, keepdims=True) * v
    pair_ptr, row_off = pair_rows_of(sizes)
    for k in ("bias", "gate", "dlogits"):
        x[k] = rng.standard_normal((h, int(pair_ptr[-1])))
    x = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in x.items()}
    starts = np.concatenate([row_off, pair_ptr[-1:]])
    ref64, ref32 = reference(sizes, x, torch.float64), reference(sizes, x, torch.float32)
    rows = {k: starts if k in PLANES else None for k in OUTPUTS}
    return x, ref64, {k: P.MARGIN * P.worst(ref32[k], ref64[k], row_ptr=rows[k]) for k in OUTPUTS}, starts


def run_pair(sizes, x, stats=True, skip=(), alloc=None):
    """run_pair of the bias test for the gated entries; the optional planes named in `skip` are passed as NULL."""
    from _binding_util import call
    dev = torch.device("cuda")
    t = {k: v if isinstance(v, torch.Tensor) else torch.from_numpy(v).to(dev) for k, v in x.items()}
    (m, h, f), n_pairs = t["Q"].shape, t["bias"].size(1)
    seg_ptr = t["seg_ptr"] if "seg_ptr" in t else torch.from_numpy(seg_ptr_of(sizes)).to(dev)
    n_seg = seg_ptr.numel() - 1
    if alloc is None:
        alloc = lambda name, shape, dtype=torch.float32: torch.full(  # noqa: E731
            shape, float("nan") if dtype == torch.float32 else -7, dtype=dtype, device=dev)
    o = dict(bounds=alloc("bounds", (2 * m,), torch.int32), pair_ptr=alloc("pair_ptr", (2 * (n_seg + 1),), torch.int32),
             row_off=alloc("row_off", (2 * m,), torch.int32), out=alloc("out", (m, h, f)))    # (int64 as pairs of int32)
    call("dfgnn_segment_bounds", "bounds", dev, m, n_seg, seg_ptr, o["bounds"])
    call("dfgnn_segment_pair_rows", "pair_rows", dev, m, n_seg, seg_ptr, o["pair_ptr"], o["row_off"])
    gate = None if "gate" in skip else t["gate"]
    head = (m, h, f, 1.0, o["bounds"], o["row_off"], n_pairs, t["bias"], gate, t["Q"], t["K"], t["V"])
    if not stats:
        call("dfgnn_segment_mha_gate_fwd", "fwd", dev, *head, o["out"], None, None, None)
        return o
    o.update({k: alloc(k, (m, h)) for k in ("row_max", "row_sum", "delta")})
    o.update({k: alloc(k, (m, h, f)) for k in ("dQ", "dK", "dV")})
    o.update({k: alloc(k, (h, n_pairs)) for k in PLANES if k not in skip and not (k == "dgate" and gate is None)})
    call("dfgnn_segment_mha_gate_fwd", "fwd", dev, *head, o["out"], o["row_max"], o["row_sum"], o.get("logits"))
    call("dfgnn_segment_mha_gate_bwd", "bwd", dev, *head, o["row_max"], o["row_sum"], t["dO"],
         None if "dlogits" in skip else t["dlogits"], o["dQ"], o["dK"], o["dV"], o.get("dbias"), o.get("dgate"), o["delta"])
    return o


@pytest.mark.parametrize("h,f", SHAPES)
@pytest.mark.parametrize("batch", BATCHES)
def test_pair_at_fp32_level(batch, h, f):
    sizes = BATCHES[batch]
    x, ref64, bound, starts = case(batch, h, f)
    got = run_pair(sizes, x)
    errs = {k: P.worst(got[k].cpu().numpy(), ref64[k], row_ptr=starts if k in PLANES else None) for k in OUTPUTS}
    print(f"{batch} h={h} f={f}: " + ", ".join(f"{k} {errs[k] / bound[k]:.3f}" for k in OUTPUTS) + " of the bound")
    for k in OUTPUTS:
        assert errs[k] <= bound[k], (k, errs[k], bound[k])
    same = lambda a, b, keys: all(torch.equal(a[k], b[k]) for k in keys)  # noqa: E731
    assert same(run_pair(sizes, x), got, got), "two calls, two results"
    assert torch.equal(run_pair(sizes, x, stats=False)["out"], got["out"]), "inference differs from the training forward"
    for name in ("logits", "dbias", "dgate"):            # an output passed as NULL changes no other output's bits
        less = run_pair(sizes, x, skip=(name,))
        assert name not in less and same(less, got, less), name
    zeros = dict(x, dlogits=np.zeros_like(x["dlogits"]))
    assert same(run_pair(sizes, x, skip=("dlogits",)), run_pair(sizes, zeros), got), "dlogits = NULL is not dlogits = 0"
    plain, bias = run_pair(sizes, x, skip=("gate", "logits", "dlogits")), run_bias_pair(sizes, x)
    assert same(plain, bias, ("out", "row_max", "row_sum", "dQ", "dK", "dV", "dbias")), "without gate: not the bias pair's bits"


def test_guarded_buffers():
    """Every output and the delta scratch between sentinel-filled guards (tests/guarded.py), as in the bias test."""
    from guarded import Arena
    batch, a = "boundary", Arena("cuda")
    x = case(batch, 2, 64)[0]
    t = {k: a.input(k, v) for k, v in x.items()}
    t["seg_ptr"] = a.input("seg_ptr", seg_ptr_of(BATCHES[batch]))
    scratch = lambda name, shape, dtype=torch.float32: (  # noqa: E731
        a.scratch(name, int(np.prod(shape))) if name == "delta" else a.output(name, shape, dtype=dtype))
    o = run_pair(BATCHES[batch], t, alloc=scratch)
    a.verify()
    assert bool(torch.isfinite(o["delta"]).all())


def test_autograd_round_trip_and_layer():
    from DFGNN.layers import EGTAttention, GlobalMHA
    from DFGNN.operators.fused_gtconv import SegmentMHAGateFuse
    dev = torch.device("cuda")
    sizes = torch.tensor([0, 40, 1, 130, 0, 23])
    ends = [0] + torch.cumsum(sizes, 0).tolist()
    seg_ptr = torch.tensor(ends, dtype=torch.int32, device=dev)
    m, h, f, n_pairs = ends[-1], 4, 32, int((sizes * sizes).sum())
    torch.manual_seed(5)
    plain = GlobalMHA(h * f, h * f, h)            # (forward_plain only: scaling 32^-0.5)
    leaves = [torch.randn(m, h, f, device=dev, requires_grad=True) for _ in range(3)]
    leaves += [torch.randn(h, n_pairs, device=dev, requires_grad=True) for _ in range(2)]
    w, u = torch.randn(m, h, f, device=dev), torch.randn(h, n_pairs, device=dev)
    loss = lambda out, logits: (out * w).sum() + (logits * u).sum()  # noqa: E731
    fused = lambda q, k, v, b, g: SegmentMHAGateFuse(seg_ptr, q, k, v, b, g, plain.scaling, return_logits=True)  # noqa: E731
    grads = []
    for fn in (fused, lambda q, k, v, b, g: plain.forward_plain(seg_ptr, q, k, v, b, g, return_logits=True)):
        out, logits = fn(*leaves)
        grads.append([out.detach(), logits.detach()] + list(torch.autograd.grad(loss(out, logits), leaves)))
    assert all(_close(a, b) for a, b in zip(*grads))
    (q, k, v, b, g), pair_feat = leaves, torch.randn(n_pairs, 8, device=dev)
    for args, kept in (((q, k, v, b.detach(), g), (0, 1, 2, 4)), ((q, k, v, b, g.detach()), (0, 1, 2, 3))):   # NULL dbias / dgate
        got = torch.autograd.grad(loss(*fused(*args)), [leaves[i] for i in kept])
        assert all(torch.equal(a, grads[0][2 + i]) for a, i in zip(got, kept))
    for heads, dim, is_fused in ((2, 64, True), (2, 96, False)):    # head width 32; 48: the torch branch, silently
        layer, xin, res = EGTAttention(dim, 8, heads).to(dev), torch.randn(m, dim, device=dev), []
        for fuse, segments in ((True, sizes), (False, seg_ptr)):
            layer.zero_grad()
            node, pair = layer(xin, pair_feat, segments, fuse=fuse)
            (node.square().sum() + pair.square().sum()).backward()
            res.append([node.detach(), pair.detach()] + [p.grad.clone() for p in layer.parameters()])
        assert all(_close(a, b) for a, b in zip(*res))
        assert is_fused != torch.equal(res[0][0], res[1][0])
