"""GPU: the segment attention pair with a TYPED pair bias (include/dfgnn_segment_tbias.h) against the float64 loop of
tests/test_gpu_segment_bias.py on the materialised bias table.t()[:, types], dB = index_add of its dbias.  Bounds: MARGIN x
the same loop in float32 against float64 (dB [T, h]: every (type, head) a row of its own); nothing of the kernel enters them.
Everything but dB must also equal the plane-biased pair on the materialised fp32 bias to the bit.  The T of the cases are 1,
256 and both sides of every threshold of the dB tables' slot count (csrc/dfgnn_segment.hpp: seg_tbias_slots: 48, 96, 192)."""
import functools

import numpy as np
import pytest
import torch

import parity_cases as P
from conftest import has_gpu
from test_gpu_segment_bias import pair_rows_of, reference, run_pair
from test_gpu_segment_mha import BATCHES, SHAPES, _close, seg_ptr_of

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not has_gpu(), reason="needs a GPU")]
PLANE = ("out", "row_max", "row_sum", "dQ", "dK", "dV")
OUTPUTS = PLANE + ("dB",)
CASES = [(b, h, f, 20) for b in BATCHES for h, f in SHAPES] + [
    ("boundary", 8, 16, 1), ("long", 4, 32, 48), ("boundary", 2, 64, 49), ("long", 1, 128, 96), ("boundary", 4, 32, 97),
    ("long", 2, 64, 192), ("boundary", 4, 32, 193), ("long", 8, 16, 256)]


def table_grad(dbias, types, T):
    """dB[t, hd] = sum of dbias[hd, p] over the pairs of type t, in dbias's precision."""
    dB = np.zeros((T, dbias.shape[0]), dtype=dbias.dtype)
    np.add.at(dB, types, dbias.T)
    return dB


@functools.lru_cache(maxsize=None)
def case(batch, h, f, T):
    """-> (inputs with the fp32 `table`, uint8 `types` and the materialised `bias`, ref64, bound per output)."""
    sizes = BATCHES[batch]
    m = int(sum(sizes))
    rng = np.random.default_rng(3000 * h + f + 7 * T + len(sizes))
    x = {k: rng.standard_normal((m, h, f)) * (f ** -0.25 if k in "QK" else 1.0) for k in ("Q", "K", "V", "dO")}
    ends = seg_ptr_of(sizes)
    for lo in ends[:-1][np.diff(ends) == 1]:     # (1-node segments: dQ = dK = 0 exactly, test_gpu_segment_mha.py says why)
        v = x["V"][lo]
        x["dO"][lo] -= (x["dO"][lo] * v).sum(-1, keepdims=True) / (v * v).sum(-1, keepdims=True) * v
    x = {k: np.ascontiguousarray(v, dtype=np.float32) for k, v in x.items()}
    x["types"] = rng.integers(0, T, int(pair_rows_of(sizes)[0][-1])).astype(np.uint8)
    x["table"] = rng.standard_normal((T, h)).astype(np.float32)
    x["bias"] = np.ascontiguousarray(x["table"].T[:, x["types"]])
    refs = []
    for dtype in (torch.float64, torch.float32):
        r = reference(sizes, x, dtype)
        r["dB"] = table_grad(r["dbias"], x["types"], T)
        refs.append(r)
    return x, refs[0], {k: P.MARGIN * P.worst(refs[1][k], refs[0][k]) for k in OUTPUTS}


def run_tpair(sizes, x, stats=True, dB=True, alloc=None):
    """The C entries -> dict of outputs made by alloc(name, shape, dtype) (default: NaN / -7 filled tensors)."""
    import dfgnn_native as N
    from _binding_util import call
    dev = torch.device("cuda")
    t = {k: v if isinstance(v, torch.Tensor) else torch.from_numpy(v).to(dev) for k, v in x.items()}
    (m, h, f), T = t["Q"].shape, t["table"].size(0)
    seg_ptr = t["seg_ptr"] if "seg_ptr" in t else torch.from_numpy(seg_ptr_of(sizes)).to(dev)
    n_seg = seg_ptr.numel() - 1
    if alloc is None:
        alloc = lambda name, shape, dtype=torch.float32: torch.full(  # noqa: E731
            shape, float("nan") if dtype == torch.float32 else -7, dtype=dtype, device=dev)
    o = dict(bounds=alloc("bounds", (2 * m,), torch.int32), pair_ptr=alloc("pair_ptr", (2 * (n_seg + 1),), torch.int32),
             row_off=alloc("row_off", (2 * m,), torch.int32), out=alloc("out", (m, h, f)))    # (int64 as pairs of int32)
    call("dfgnn_segment_bounds", "bounds", dev, m, n_seg, seg_ptr, o["bounds"])
    call("dfgnn_segment_pair_rows", "pair_rows", dev, m, n_seg, seg_ptr, o["pair_ptr"], o["row_off"])
    head = (m, h, f, 1.0, o["bounds"], o["row_off"], t["types"].numel(), t["types"], T, t["table"], t["Q"], t["K"], t["V"])
    if not stats:
        call("dfgnn_segment_mha_tbias_fwd", "fwd", dev, *head, o["out"], None, None)
        return o
    o.update({k: alloc(k, (m, h)) for k in ("row_max", "row_sum", "delta")})
    o.update({k: alloc(k, (m, h, f)) for k in ("dQ", "dK", "dV")})
    if dB:
        o["dB"] = alloc("dB", (T, h))
        o["ws"] = alloc("ws", (N.lib().dfgnn_segment_mha_tbias_ws_floats(m, h, T),))
    call("dfgnn_segment_mha_tbias_fwd", "fwd", dev, *head, o["out"], o["row_max"], o["row_sum"])
    call("dfgnn_segment_mha_tbias_bwd", "bwd", dev, *head, o["row_max"], o["row_sum"], t["dO"], o["dQ"], o["dK"], o["dV"],
         o.get("dB"), o.get("ws"), o["delta"])
    return o


@pytest.mark.parametrize("batch,h,f,T", CASES)
def test_pair_at_fp32_level(batch, h, f, T):
    sizes = BATCHES[batch]
    x, ref64, bound = case(batch, h, f, T)
    got = run_tpair(sizes, x)
    errs = {k: P.worst(got[k].cpu().numpy(), ref64[k]) for k in OUTPUTS}
    print(f"{batch} h={h} f={f} T={T}: " + ", ".join(f"{k} {errs[k] / bound[k]:.3f}" for k in OUTPUTS) + " of the bound")
    for k in OUTPUTS:
        assert errs[k] <= bound[k], (k, errs[k], bound[k])
    plane = run_pair(sizes, {k: v for k, v in x.items() if k not in ("types", "table")}, dbias=False)
    assert all(torch.equal(plane[k], got[k]) for k in PLANE), "not the plane-biased pair's bits"
    again = run_tpair(sizes, x)
    assert all(torch.equal(again[k], got[k]) for k in OUTPUTS), "two calls, two results"
    assert torch.equal(run_tpair(sizes, x, stats=False)["out"], got["out"]), "inference differs from the training forward"
    frozen = run_tpair(sizes, x, dB=False)
    assert all(torch.equal(frozen[k], got[k]) for k in ("dQ", "dK", "dV")), "dB = NULL changes the other gradients"


@pytest.mark.parametrize("n", (129, 640))
def test_a_type_that_decides(n):
    """Type 1 is -1e30 in the table and covers all keys but one of four rows: out is the surviving key's V row (the argument
    of test_a_bias_that_decides: 2^-21 < 1e-6), dB of the masked type is exactly 0 (P = 0 on its pairs; the other rows avoid
    it).  Types past the table clamp to its last row."""
    h, f, T = 2, 32, 3
    rng = np.random.default_rng(n)
    x = {k: rng.standard_normal((n, h, f)).astype(np.float32) for k in ("Q", "K", "V", "dO")}
    types = 2 * rng.integers(0, 2, (n, n)).astype(np.uint8)           # types 0 and 2 elsewhere
    rows, keys = np.array([0, 1, n // 2, n - 1]), np.array([0, n - 1, n - 1, 0])
    types[rows] = 1
    types[rows, keys] = 0
    x["types"], x["table"] = types.reshape(-1), rng.standard_normal((T, h)).astype(np.float32)
    x["table"][1] = -1e30
    got = run_tpair((n,), x)
    want = torch.from_numpy(x["V"][keys]).cuda()
    assert float((got["out"][rows] - want).abs().max()) <= 1e-6 * float(np.abs(x["V"]).max())
    assert bool((got["dB"][1] == 0).all())
    assert all(bool(torch.isfinite(got[k]).all()) for k in OUTPUTS)
    a, b = (run_tpair((n,), dict(x, types=np.full(n * n, v, dtype=np.uint8))) for v in (255, 2))
    assert all(torch.equal(a[k], b[k]) for k in OUTPUTS), "a type past the table is not its last row"


def test_guarded_buffers():
    """types and the table are guarded inputs, ws and delta scratch, dB and every other output between sentinel-filled guards
    (tests/guarded.py): all of each output written and finite, no guard touched, no input modified."""
    from guarded import Arena
    batch, h, f, T = "boundary", 2, 64, 20
    x, _, _ = case(batch, h, f, T)
    a = Arena("cuda")
    t = {k: a.input(k, v) for k, v in x.items() if k != "bias"}
    t["seg_ptr"] = a.input("seg_ptr", seg_ptr_of(BATCHES[batch]))
    alloc = lambda name, shape, dtype=torch.float32: (  # noqa: E731
        a.scratch(name, int(np.prod(shape))) if name in ("delta", "ws") else a.output(name, shape, dtype=dtype))
    o = run_tpair(BATCHES[batch], t, alloc=alloc)
    a.verify()
    assert bool(torch.isfinite(o["delta"]).all()) and bool(torch.isfinite(o["ws"]).all())


def test_autograd_round_trip_and_layer():
    from DFGNN.layers import GlobalMHA, PairBias
    from DFGNN.operators.fused_gtconv import SegmentMHATBiasFuse
    dev = torch.device("cuda")
    torch.manual_seed(5)
    sizes = torch.tensor([0, 40, 1, 130, 0, 23])
    ends = [0] + torch.cumsum(sizes, 0).tolist()
    seg_ptr = torch.tensor(ends, dtype=torch.int32, device=dev)
    m, h, f, n_pairs = ends[-1], 4, 32, int((sizes * sizes).sum())
    plain = GlobalMHA(h * f, h * f, h)            # (forward_plain only: scaling 32^-0.5)
    w = torch.randn(m, h, f, device=dev)
    for T, dtype in ((6, torch.uint8), (300, torch.int64)):       # 300 types: the materialised fallback
        types = torch.randint(0, T, (n_pairs,), device=dev).to(dtype)
        leaves = [torch.randn(m, h, f, device=dev, requires_grad=True) for _ in range(3)]
        leaves.append(torch.randn(T, h, device=dev, requires_grad=True))
        grads = []
        for fn in (lambda q, k, v, tb: SegmentMHATBiasFuse(seg_ptr, q, k, v, types, tb, plain.scaling),
                   lambda q, k, v, tb: plain.forward_plain(seg_ptr, q, k, v, tb.t()[:, types.long()])):
            out = fn(*leaves)
            grads.append([out.detach()] + list(torch.autograd.grad((out * w).sum(), leaves)))
        assert all(_close(a, b) for a, b in zip(*grads)), T
        q, k, v, tb = leaves
        out = SegmentMHATBiasFuse(seg_ptr, q, k, v, types, tb.detach(), plain.scaling)     # a frozen table: dB = NULL
        assert all(torch.equal(x, y) for x, y in zip(torch.autograd.grad((out * w).sum(), (q, k, v)), grads[0][1:4]))

    x = torch.randn(m, 64, device=dev)
    types = torch.randint(0, 6, (n_pairs,), device=dev)              # int64: the layer converts
    layer, enc = GlobalMHA(64, 128, 4).to(dev), PairBias(6, 4).to(dev)
    res = []
    for fuse in (True, False):
        layer.zero_grad()
        enc.zero_grad()
        y = layer(x, seg_ptr, fuse=fuse, pair_types=types, pair_table=enc.table)
        y.square().sum().backward()
        res.append([y.detach(), enc.table.grad.clone()] + [p.grad.clone() for p in layer.parameters()])
    assert all(_close(a, b) for a, b in zip(*res))
    assert not torch.equal(res[0][0], res[1][0])
    with pytest.raises(ValueError):
        layer(x, seg_ptr, bias=enc(types), pair_types=types, pair_table=enc.table)
