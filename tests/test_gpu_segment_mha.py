"""GPU: the segment multi-head attention pair (include/dfgnn_segment.h) against a plain per-segment torch loop in float64.

The bound is the project's fp32-level bar (parity_cases: MARGIN x the error of the same loop in float32 against float64, on
the same inputs); nothing of the kernel enters it.  Inputs as parity_cases.gt_inputs: Q, K ~ N(0, 1) f^-1/4, V, dO ~ N(0, 1),
scale 1.  In a 1-node segment P = 1 and dQ = dK = 0 exactly, so dO is made orthogonal to that node's V in float64 before
the cast: rounding noise on an exact zero does not decide the test (tests/dense_cases.py says the same of its inputs)."""
import functools

import numpy as np
import pytest
import torch

import parity_cases as P
from conftest import has_gpu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]

# segment ends on, before and after strip (16) and window (128) edges, several small graphs in one window, empty
# segments at the front, inside and at the end; then multi-tile rows, windows inside one segment, a window that straddles
# two large segments with a small one between them
BATCHES = {"boundary": (0, 1, 2, 3, 15, 16, 17, 0, 63, 64, 65, 127, 128, 129, 0), "long": (257, 5, 300, 640)}
SHAPES = ((1, 128), (2, 64), (4, 32), (8, 16))
OUTPUTS = ("out", "row_max", "row_sum", "dQ", "dK", "dV")


def seg_ptr_of(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)


def reference(sizes, x, dtype):
    """Every output of the pair by a loop over the segments in `dtype` on the CPU (scale 1)."""
    Q, K, V, dO = (torch.from_numpy(x[k]).to(dtype) for k in ("Q", "K", "V", "dO"))
    m, h, _ = Q.shape
    r = {k: torch.zeros_like(Q) for k in ("out", "dQ", "dK", "dV")}
    r["row_max"], r["row_sum"] = torch.zeros(m, h, dtype=dtype), torch.zeros(m, h, dtype=dtype)
    ends = seg_ptr_of(sizes).tolist()
    for lo, hi in zip(ends[:-1], ends[1:]):
        if hi == lo:
            continue
        q, k, v, g = (a[lo:hi].transpose(0, 1) for a in (Q, K, V, dO))      # [h, n, f]
        s = q @ k.transpose(1, 2)
        mx = s.max(dim=2, keepdim=True).values
        e = torch.exp(s - mx)
        sm = e.sum(dim=2, keepdim=True)
        p = e / sm
        dp = g @ v.transpose(1, 2)
        ds = p * (dp - (p * dp).sum(dim=2, keepdim=True))
        for name, val in (("out", p @ v), ("dQ", ds @ k), ("dK", ds.transpose(1, 2) @ q), ("dV", p.transpose(1, 2) @ g)):
            r[name][lo:hi] = val.transpose(0, 1)
        r["row_max"][lo:hi], r["row_sum"][lo:hi] = mx[:, :, 0].T, sm[:, :, 0].T
    return {k: v.numpy() for k, v in r.items()}


@functools.lru_cache(maxsize=None)
def case(batch, h, f):
    """-> (inputs float32, ref64, bounds per output); computed once, nobody writes to it."""
    sizes = BATCHES[batch]
    m = int(sum(sizes))
    rng = np.random.default_rng(1000 * h + f + len(sizes))
    x = {k: rng.standard_normal((m, h, f)) * (f ** -0.25 if k in "QK" else 1.0) for k in ("Q", "K", "V", "dO")}
    ends = seg_ptr_of(sizes)
    for lo in ends[:-1][np.diff(ends) == 1]:
        v = x["V"][lo]
        x["dO"][lo] -= (x["dO"][lo] * v).sum(-1, keepdims=True) / (v * v).sum(-1, keepdims=True) * v
    x = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in x.items()}
    ref64, ref32 = reference(sizes, x, torch.float64), reference(sizes, x, torch.float32)
    return x, ref64, {k: P.MARGIN * P.worst(ref32[k], ref64[k]) for k in OUTPUTS}


def run_pair(batch, h, f, stats=True):
    """The C entries on NaN-filled outputs -> dict of tensors (bounds, the six outputs, delta)."""
    from _binding_util import call
    x, _, _ = case(batch, h, f)
    dev = torch.device("cuda")
    t = {k: torch.from_numpy(v).to(dev) for k, v in x.items()}
    m = t["Q"].size(0)
    seg_ptr = torch.from_numpy(seg_ptr_of(BATCHES[batch])).to(dev)
    nan = lambda *shape: torch.full(shape, float("nan"), device=dev)  # noqa: E731
    o = dict(bounds=torch.full((2 * m,), -7, dtype=torch.int32, device=dev), out=nan(m, h, f))
    call("dfgnn_segment_bounds", "bounds", dev, m, seg_ptr.numel() - 1, seg_ptr, o["bounds"])
    if not stats:
        call("dfgnn_segment_mha_fwd", "fwd", dev, m, h, f, 1.0, o["bounds"], t["Q"], t["K"], t["V"], o["out"], None, None)
        return o
    o.update(row_max=nan(m, h), row_sum=nan(m, h), delta=nan(m, h), dQ=nan(m, h, f), dK=nan(m, h, f), dV=nan(m, h, f))
    call("dfgnn_segment_mha_fwd", "fwd", dev, m, h, f, 1.0, o["bounds"], t["Q"], t["K"], t["V"], o["out"], o["row_max"], o["row_sum"])
    call("dfgnn_segment_mha_bwd", "bwd", dev, m, h, f, 1.0, o["bounds"], t["Q"], t["K"], t["V"], o["out"], o["row_max"], o["row_sum"],
         t["dO"], o["dQ"], o["dK"], o["dV"], o["delta"])
    return o


@pytest.mark.parametrize("h,f", SHAPES)
@pytest.mark.parametrize("batch", BATCHES)
def test_pair_at_fp32_level(batch, h, f):
    _, ref64, bound = case(batch, h, f)
    got = run_pair(batch, h, f)
    ends = seg_ptr_of(BATCHES[batch])
    seg = np.searchsorted(ends, np.arange(ends[-1]), side="right") - 1
    assert np.array_equal(got["bounds"].cpu().numpy().reshape(-1, 2), np.stack([ends[seg], ends[seg + 1]], axis=1))
    errs = {k: P.worst(got[k].cpu().numpy(), ref64[k]) for k in OUTPUTS}
    print(f"{batch} h={h} f={f}: " + ", ".join(f"{k} {errs[k] / bound[k]:.3f}" for k in OUTPUTS) + " of the bound")
    for k in OUTPUTS:
        assert errs[k] <= bound[k], (k, errs[k], bound[k])
    assert all(torch.equal(a, b) for a, b in zip(run_pair(batch, h, f).values(), got.values())), "two calls, two results"
    assert torch.equal(run_pair(batch, h, f, stats=False)["out"], got["out"]), "inference differs from the training forward"


def _plain(seg_ptr, q, k, v, scale):
    outs = []
    for lo, hi in zip(seg_ptr[:-1], seg_ptr[1:]):
        s = torch.einsum("ihf,jhf->hij", q[lo:hi], k[lo:hi]) * scale
        outs.append(torch.einsum("hij,jhf->ihf", torch.softmax(s, dim=-1), v[lo:hi]))
    return torch.cat(outs)


def _close(a, b):
    return float((a - b).abs().max()) < 1e-3 * max(1.0, float(b.abs().max()))


def test_autograd_round_trip_and_layer():
    from DFGNN.layers import GlobalMHA
    from DFGNN.operators.fused_gtconv import SegmentMHAFuse
    dev = torch.device("cuda")
    torch.manual_seed(3)
    sizes = torch.tensor([0, 40, 1, 130, 0, 23])
    ends = [0] + torch.cumsum(sizes, 0).tolist()
    seg_ptr = torch.tensor(ends, dtype=torch.int32, device=dev)
    m, h, f = ends[-1], 4, 32
    leaves = [torch.randn(m, h, f, device=dev, requires_grad=True) for _ in range(3)]
    w = torch.randn(m, h, f, device=dev)
    grads = []
    for fn in (lambda q, k, v: SegmentMHAFuse(seg_ptr, q, k, v, 0.25), lambda q, k, v: _plain(ends, q, k, v, 0.25)):
        out = fn(*leaves)
        grads.append([out.detach()] + list(torch.autograd.grad((out * w).sum(), leaves)))
    assert all(_close(a, b) for a, b in zip(*grads))
    with torch.no_grad():
        assert torch.equal(SegmentMHAFuse(seg_ptr, *leaves, 0.25), grads[0][0])   # (the inference forward)

    x = torch.randn(m, 64, device=dev)
    for heads, out_size, fused in ((4, 128, True), (2, 96, False)):    # head width 32; 48: the torch branch, silently
        layer = GlobalMHA(64, out_size, heads).to(dev)
        res = []
        for fuse, segments in ((True, sizes), (False, seg_ptr)):
            layer.zero_grad()
            y = layer(x, segments, fuse=fuse)
            y.square().sum().backward()
            res.append([y.detach()] + [p.grad.clone() for p in layer.parameters()])
        assert all(_close(a, b) for a, b in zip(*res))
        assert fused != all(torch.equal(a, b) for a, b in zip(*res))


def test_guarded_buffers():
    """Outputs and the delta scratch between sentinel-filled guards (tests/guarded.py): every output element written, no
    guard touched, no input modified."""
    from _binding_util import call
    from guarded import Arena
    batch, h, f = "boundary", 2, 64
    x, _, _ = case(batch, h, f)
    m = x["Q"].shape[0]
    seg_ptr = seg_ptr_of(BATCHES[batch])
    a = Arena("cuda")
    t = {k: a.input(k, x[k]) for k in ("Q", "K", "V", "dO")}
    sp = a.input("seg_ptr", seg_ptr)
    bounds = a.output("bounds", (2 * m,), dtype=torch.int32)
    o = {k: a.output(k, (m, h, f)) for k in ("out", "dQ", "dK", "dV")}
    st = {k: a.output(k, (m, h)) for k in ("row_max", "row_sum")}
    delta = a.scratch("delta", m * h)
    dev = torch.device("cuda")
    call("dfgnn_segment_bounds", "bounds", dev, m, len(seg_ptr) - 1, sp, bounds)
    call("dfgnn_segment_mha_fwd", "fwd", dev, m, h, f, 1.0, bounds, t["Q"], t["K"], t["V"], o["out"], st["row_max"], st["row_sum"])
    call("dfgnn_segment_mha_bwd", "bwd", dev, m, h, f, 1.0, bounds, t["Q"], t["K"], t["V"], o["out"], st["row_max"], st["row_sum"],
         t["dO"], o["dQ"], o["dK"], o["dV"], delta)
    a.verify()
    assert bool(torch.isfinite(delta).all())


@pytest.mark.parametrize("n_seg", (0, 3))
def test_no_nodes_is_a_no_op(n_seg):
    import fused_gtconv as G
    dev = torch.device("cuda")
    seg_ptr = torch.zeros(n_seg + 1, dtype=torch.int32, device=dev)
    e = torch.empty(0, 2, 32, device=dev)
    bounds = G.segment_bounds(seg_ptr, 0)
    out, row_max, row_sum = G.segment_mha_forward(bounds, e, e, e)
    grads = G.segment_mha_backward(bounds, e, e, e, out, row_max, row_sum, e)
    assert bounds.numel() == 0 and out.shape == e.shape and all(g.shape == e.shape for g in grads)
    torch.cuda.synchronize()
