"""GPU tests of the GT conv with a typed attention bias (include/dfgnn.h: dfgnn_gt_fwd_tbias / dfgnn_gt_bwd_tbias;
csrc/gt_tbias_train.hip): inference, the training pair that saves two floats per (row, head), the reduction of dB, masks,
the autograd Function and the layer.  The reference is tests/gt_tbias_cases.reference on the CPU -- the bias pair's
float64 formulation on the materialised B[etype].T, masked edges removed, dB by a float64 index_add --; the bar is the
project's own, max abs error < 1e-3 * max(1, max |ref|), all finite.  Everything the bias pair has too -- out, the
statistics, dQ, dK, dV -- must equal the bias pair's on the materialised bias BIT FOR BIT, also on the 32 boundary-degree
graphs: tests/test_gpu_gt_bias.py proves there that the bias pair loses no edge, and equal bits carry that proof over
without a new tolerance.  The graphs are those of tests/test_gpu_gt_typed.py."""
import functools

import numpy as np
import pytest
import torch

import gt_bias_cases as bc
import gt_tbias_cases as zc
import parity_cases as pc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BAR = 1e-3
SENTINEL = np.float32(-1e38)
PAIR_OUTPUTS = zc.PAIR_OUTPUTS


def _np(t):
    return t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t.to(dtype) if dtype is not None else t).to(DEV)


def _check(got, ref, what):
    """The parity bar; prints the measured figure first (pytest -s / a failing run shows it)."""
    got, ref = _np(got).astype(np.float64), _np(ref).astype(np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    bound = BAR * max(1.0, float(np.abs(ref).max()) if ref.size else 0.0)
    print(f"gt_tbias {what}: max abs err {err:.3e} (bound {bound:.3e})")
    assert np.isfinite(got).all(), what
    assert err < bound, (what, err, bound)


# ---- graphs and inputs ------------------------------------------------------------------------------------------------
def _graph(kind):
    from test_gpu_gt_typed import _graph as base
    return base(kind)


def _types(rng, nnz, T):
    from test_gpu_gt_typed import _types as base
    return base(rng, nnz, T)


def _inputs(g, h, f, weighted, etype, T, seed=0):
    """float32 host inputs on graph g with the given types; B ~ N(0, 1)."""
    m, n, nnz = g["m"], g["n_cols"], g["nnz"]
    rng = np.random.default_rng(1000 * h + f + 7 * weighted + 13 * seed)
    val = rng.uniform(0.5, 1.5, nnz) if weighted else np.ones(nnz)
    Q, K = rng.standard_normal((m, h, f)) * f ** -0.25, rng.standard_normal((n, h, f)) * f ** -0.25
    V, dO = rng.standard_normal((n, h, f)), rng.standard_normal((m, h, f))
    B = rng.standard_normal((T, h))
    x = {k: np.ascontiguousarray(a, dtype=np.float32) for k, a in dict(val=val, B=B, Q=Q, K=K, V=V, dO=dO).items()}
    x["etype"] = np.ascontiguousarray(etype, dtype=np.int32)
    x["etype_csc"] = np.ascontiguousarray(x["etype"][g["val_idx_np"]])
    return x


def _reference(g, x):
    return zc.reference(g["row_ptr_np"], g["col_ind_np"], g["n_cols"], x["val"], x["etype"], x["B"], x["Q"], x["K"], x["V"],
                        x["dO"])


@functools.lru_cache(maxsize=None)
def _case(kind, h, f, weighted, T):
    """-> (host inputs dict, float64 reference dict); computed once per case and shared, nobody writes to it."""
    g = _graph(kind)
    x = _inputs(g, h, f, weighted, _types(np.random.default_rng(T), g["nnz"], T), T)
    return x, _reference(g, x)


def _on_device(x):
    return {k: _dev(a) for k, a in x.items()}


def _pair(g, d, need_dB=True):
    import fused_gtconv as gt
    out, mx, sm = gt.gt_forward_tbias(g["row_ptr"], g["col_ind"], d["val"], d["etype"], d["B"], d["Q"], d["K"], d["V"])
    dQ, dK, dV, dB = gt.gt_backward_tbias(g["row_ptr"], g["col_ind"], d["val"], d["etype"], g["col_ptr"], g["row_ind"],
                                          g["val_idx"], d["etype_csc"], d["B"], d["Q"], d["K"], d["V"], out, mx, sm, d["dO"],
                                          need_dB=need_dB)
    torch.cuda.synchronize()
    return dict(out=out, row_max=mx, row_sum=sm, dQ=dQ, dK=dK, dV=dV, dB=dB)


def _bias_pair(g, d, need_dbias=False):
    """The bias pair on the materialised bias[h, nnz] = B[etype].t()."""
    import fused_gtconv as gt
    bias = d["B"][d["etype"].long()].t().contiguous()
    out, mx, sm = gt.gt_forward_bias(g["row_ptr"], g["col_ind"], d["val"], bias, d["Q"], d["K"], d["V"])
    dQ, dK, dV, dbias = gt.gt_backward_bias(g["row_ptr"], g["col_ind"], d["val"], bias, g["col_ptr"], g["row_ind"],
                                            g["val_idx"], d["Q"], d["K"], d["V"], out, mx, sm, d["dO"], need_dbias=need_dbias)
    torch.cuda.synchronize()
    return dict(out=out, row_max=mx, row_sum=sm, dQ=dQ, dK=dK, dV=dV, dbias=dbias)


def _against_reference(res, ref, what, names=("out", "row_sum", "dQ", "dK", "dV", "dB")):
    """Everything at the bar; row_max where the (row, head) has an unmasked edge, the sentinel exactly elsewhere."""
    live = ref["row_max"] != zc.SENTINEL_MAX
    for name in names:
        _check(res[name], ref[name], f"{what} {name}")
    mx = _np(res["row_max"])
    _check(mx[live], ref["row_max"][live], f"{what} row_max")
    assert (mx[~live] == SENTINEL).all(), what
    return live


def _exact_zeros(g, res):
    er, ecol = g["empty_rows"], g["empty_cols"]
    assert (_np(res["out"])[er] == 0).all() and (_np(res["dQ"])[er] == 0).all()
    assert (_np(res["dK"])[ecol] == 0).all() and (_np(res["dV"])[ecol] == 0).all()
    assert (_np(res["row_max"])[er] == SENTINEL).all() and (_np(res["row_sum"])[er] == 0).all()


def _same_bits(res, other, names=PAIR_OUTPUTS):
    for name in names:
        assert torch.equal(res[name], other[name]), name


# ---- 1. the pair against the reference, 2. the bias pair's bits ---------------------------------------------------------
CASES = [("lane", 3, 7), ("lane", 2, 20), ("wave", 1, 128), ("wave", 8, 16), ("wave", 2, 260)]


@pytest.mark.parametrize("T", [1, 5, 64])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind,h,f", CASES)
def test_pair_against_reference(kind, h, f, weighted, T):
    """Both forms, float4 and scalar lane layouts, f > 256, several heads, a table of one row, of a few and of 64: every
    output at the bar; exact zeros and sentinels where a row / column has no edge; the dB row of the type without an edge is
    exactly 0; inference equals the training forward's out, need_dB=False leaves dQ, dK, dV as they are; and at T = 5 out,
    the statistics, dQ, dK, dV equal the bias pair's on B[etype].t() bit for bit."""
    import fused_gtconv as gt
    g = _graph(kind)
    x, ref = _case(kind, h, f, weighted, T)
    d = _on_device(x)
    assert gt.gt_tbias_dB_supported(T, h)
    res = _pair(g, d)
    _against_reference(res, ref, f"{kind} h{h} f{f} val={weighted} T={T}")
    _exact_zeros(g, res)
    assert res["dB"].shape == (T, h)
    if T > 1:
        assert (x["etype"] != T // 2).all() and (_np(res["dB"])[T // 2] == 0).all() and (ref["dB"][T // 2] == 0).all()
        assert np.abs(ref["dB"]).max() > 0.01
    plain = gt.gt_inference_tbias(g["row_ptr"], g["col_ind"], d["val"], d["etype"], d["B"], d["Q"], d["K"], d["V"])
    assert torch.equal(plain, res["out"])
    without = _pair(g, d, need_dB=False)
    assert without["dB"] is None
    _same_bits(res, without)
    if T == 5:
        _same_bits(res, _bias_pair(g, d))


@pytest.mark.parametrize("case", pc.case_ids("gt"), ids=str)
def test_boundary_degrees_have_the_bias_pairs_bits(case):
    """The 32 boundary-degree graphs with the bias pair's Q, K, V, dO and val (gt_bias_cases.boundary_inputs), a random
    B[304, h] and etype = col_ind: out, row_max, row_sum, dQ, dK, dV equal the bias pair's on B[etype].t() bit for bit."""
    g = pc.graph(case[0], case[1])
    x = bc.boundary_inputs(case)
    h, T = case[3], 304
    assert g["col_ind"].max() < T
    rng = np.random.default_rng(304)
    dg = {k: _dev(g[k], torch.int32) for k in ("row_ptr", "col_ind", "col_ptr", "row_ind", "val_idx")}
    d = _on_device({k: x[k] for k in ("val", "Q", "K", "V", "dO")})
    d["B"] = _dev(rng.standard_normal((T, h)).astype(np.float32))
    d["etype"] = dg["col_ind"]
    d["etype_csc"] = dg["col_ind"][dg["val_idx"].long()].contiguous()
    res = _pair(dg, d)
    _same_bits(res, _bias_pair(dg, d))
    assert torch.isfinite(res["dB"]).all() and res["dB"].shape == (T, h)


# ---- 3. one type per edge ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f,T", [("lane", 3, 7, None), ("w16", 2, 32, None), ("w16", 8, 16, None), ("w4", 1, 128, None),
                                        ("lane", 3, 7, 4096)])
def test_one_type_per_edge(kind, h, f, T):
    """etype = arange(nnz), T = nnz (or the table padded to T = 4096 exactly, the limit): every slot of dB receives exactly
    one edge's dS, so dB[:nnz] must equal the bias pair's dbias.t() bit for bit -- a contribution that is lost, misrouted or
    added twice cannot hide -- and the slots above nnz are exactly 0."""
    import fused_gtconv as gt
    g = _graph(kind)
    nnz = g["nnz"]
    T = nnz if T is None else T
    assert nnz <= T and gt.gt_tbias_dB_supported(T, h)
    x = _inputs(g, h, f, True, np.arange(nnz), T)
    d = _on_device(x)
    res, bias = _pair(g, d), _bias_pair(g, d, need_dbias=True)
    assert res["dB"].shape == (T, h) and bias["dbias"].shape == (h, nnz)
    assert torch.equal(res["dB"][:nnz], bias["dbias"].t())
    assert (res["dB"][nnz:] == 0).all() and float(res["dB"].abs().max()) > 0
    _same_bits(res, bias)


# ---- 4. masks ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f", [("lane", 3, 7), ("wave", 8, 16)])
def test_masked_type(kind, h, f):
    """B[3, head] = -inf with T = 5; one row's edges are all of type 3, so that (row, head) is fully masked and other rows
    partly.  Everything is finite and at the bar against the reference, which removes the masked edges; the fully masked
    (row, head) is exactly an empty row; dB[3, head] is exactly 0; the other heads equal the unmasked run bit for bit; and
    the bits are the bias pair's."""
    g, T, head = _graph(kind), 5, h - 2
    deg = np.diff(g["row_ptr_np"])
    row = int(np.nonzero(deg >= 3)[0][1])
    etype = _types(np.random.default_rng(T), g["nnz"], T)
    etype[g["row_ptr_np"][row]:g["row_ptr_np"][row + 1]] = 3
    plain = _inputs(g, h, f, True, etype, T)
    masked = dict(plain, B=plain["B"].copy())
    masked["B"][3, head] = -np.inf
    rows_with_3 = np.unique(g["rows_np"][etype == 3])
    assert len(rows_with_3) > 5                                                # partly masked rows exist
    ref = _reference(g, masked)
    base, res = _pair(g, _on_device(plain)), _pair(g, _on_device(masked))
    for name in zc.OUTPUTS:
        assert np.isfinite(_np(res[name])).all(), name
    live = _against_reference(res, ref, f"masked type {kind}")
    assert not live[row, head] and live[row, [hd for hd in range(h) if hd != head]].all()
    assert (_np(res["out"])[row, head] == 0).all() and (_np(res["dQ"])[row, head] == 0).all()
    assert _np(res["row_max"])[row, head] == SENTINEL and _np(res["row_sum"])[row, head] == 0
    assert _np(res["dB"])[3, head] == 0 and ref["dB"][3, head] == 0 and _np(base["dB"])[3, head] != 0
    others = [hd for hd in range(h) if hd != head]
    for name in zc.OUTPUTS:
        assert torch.equal(res[name][:, others], base[name][:, others]), name
        assert not torch.equal(res[name][:, head], base[name][:, head]), name
    _same_bits(res, _bias_pair(g, _on_device(masked)))


# ---- 5. determinism ---------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits():
    g = _graph("wave")
    d = _on_device(_case("wave", 8, 16, True, 64)[0])
    first, second = _pair(g, d), _pair(g, d)
    assert torch.equal(first["dB"], second["dB"]) and float(first["dB"].abs().max()) > 0
    _same_bits(first, second)


# ---- 6. dB == NULL and the limit ----------------------------------------------------------------------------------------
def _op(g, d, q, k, v, b):
    from DFGNN.operators.fused_gtconv import GTConvFuse_tbias
    return GTConvFuse_tbias(None, g["row_ptr"], g["col_ind"], d["val"], g["col_ptr"], g["row_ind"], g["val_idx"], 0, q, k, v, b,
                            d["etype"], d["etype_csc"])


def test_above_the_limit():
    """T = 5000 on the wave graph (types spread over the whole table).  Without dB the pair runs and has the bias pair's
    bits; with dB the raw backward raises the library's "unsupported" RuntimeError before any launch; the operator still
    returns every gradient at the bar, through GTConvFuse_bias on B[etype].t()."""
    import fused_gtconv as gt
    g, h, f, T = _graph("wave"), 8, 16, 5000
    assert not gt.gt_tbias_dB_supported(T, h)
    x = _inputs(g, h, f, True, np.random.default_rng(T).integers(0, T, g["nnz"]), T)
    d, ref = _on_device(x), _reference(g, x)
    with pytest.raises(RuntimeError, match="unsupported"):
        _pair(g, d)
    res = _pair(g, d, need_dB=False)
    assert res["dB"] is None
    _same_bits(res, _bias_pair(g, d))
    _against_reference(res, ref, "above the limit, raw without dB", names=("out", "row_sum", "dQ", "dK", "dV"))
    q, k, v, b = (d[n].clone().requires_grad_(True) for n in ("Q", "K", "V", "B"))
    out = _op(g, d, q, k, v, b)
    grads = torch.autograd.grad(out, (q, k, v, b), d["dO"])
    _check(out, ref["out"], "fallback out")
    for got, name in zip(grads, ("dQ", "dK", "dV", "dB")):
        _check(got, ref[name], f"fallback {name}")
    assert grads[3].shape == (T, h)


# ---- 7. rectangular graphs --------------------------------------------------------------------------------------------
def _raw(g, d, T, h, f, rect):
    """The C entries through ctypes: the square ones, or the _rect ones with n_cols given."""
    import dfgnn_native
    from _binding_util import call
    m, nnz = g["m"], g["nnz"]
    E = lambda *s: torch.empty(s, dtype=torch.float32, device=DEV)  # noqa: E731
    ws = E(int(dfgnn_native.lib().dfgnn_gt_tbias_bwd_ws_floats(T, h)))
    out, mx, sm, delta = E(m, h, f), E(m, h), E(m, h), E(m, h)
    dQ, dK, dV, dB = E(m, h, f), E(g["n_cols"], h, f), E(g["n_cols"], h, f), E(T, h)
    dims = (m, g["n_cols"], nnz, h, f, T) if rect else (m, nnz, h, f, T)
    sfx = "_rect" if rect else ""
    call("dfgnn_gt_fwd_tbias" + sfx, "fwd", d["Q"].device, *dims, g["row_ptr"], g["col_ind"], d["val"], d["etype"], d["B"],
         d["Q"], d["K"], d["V"], mx, sm, out)
    call("dfgnn_gt_bwd_tbias" + sfx, "bwd", d["Q"].device, *dims, g["row_ptr"], g["col_ind"], d["val"], d["etype"],
         g["col_ptr"], g["row_ind"], g["val_idx"], d["etype_csc"], d["B"], d["Q"], d["K"], d["V"], out, mx, sm, d["dO"], delta,
         ws, dQ, dK, dV, dB)
    torch.cuda.synchronize()
    return dict(out=out, row_max=mx, row_sum=sm, dQ=dQ, dK=dK, dV=dV, dB=dB)


@pytest.mark.parametrize("kind,h,f", [("tall", 2, 20), ("wide", 1, 128), ("wide", 3, 7)])
def test_rectangular(kind, h, f):
    """150 x 96 (a lane group per row, a wave per column) and 96 x 150 (the reverse), empty rows and columns: every output
    at the bar against the reference, exact zeros where nothing arrives, and the bias pair's bits."""
    g, T = _graph(kind), 5
    x = _inputs(g, h, f, True, _types(np.random.default_rng(5), g["nnz"], T), T)
    d = _on_device(x)
    res = _pair(g, d)
    assert res["out"].shape == res["dQ"].shape == (g["m"], h, f) and res["dK"].shape == res["dV"].shape == (g["n_cols"], h, f)
    _against_reference(res, _reference(g, x), f"rect {kind} h{h} f{f}")
    _exact_zeros(g, res)
    _same_bits(res, _bias_pair(g, d))


def test_square_entry_is_the_rect_entry():
    """dfgnn_gt_*_tbias and dfgnn_gt_*_tbias_rect with n_cols = m: the same bits; and without rows (m = 0, n_cols > 0) the
    backward writes dK = dV = dB = 0 in full."""
    import fused_gtconv as gt
    h, f, T = 2, 20, 5
    g = _graph("lane")
    d = _on_device(_case("lane", h, f, True, T)[0])
    sq, rect = _raw(g, d, T, h, f, False), _raw(g, d, T, h, f, True)
    _same_bits(sq, rect, zc.OUTPUTS)
    _same_bits(sq, _pair(g, d), zc.OUTPUTS)
    i32 = dict(dtype=torch.int32, device=DEV)
    none, n = torch.zeros(0, **i32), 7
    Q, KV, B = torch.zeros(0, h, f, device=DEV), torch.randn(n, h, f, device=DEV), torch.randn(T, h, device=DEV)
    out, mx, sm = gt.gt_forward_tbias(torch.zeros(1, **i32), none, None, none, B, Q, KV, KV)
    dQ, dK, dV, dB = gt.gt_backward_tbias(torch.zeros(1, **i32), none, None, none, torch.zeros(n + 1, **i32), none, none, none,
                                          B, Q, KV, KV, out, mx, sm, Q)
    torch.cuda.synchronize()
    assert dK.shape == dV.shape == (n, h, f) and dB.shape == (T, h) and dQ.shape == (0, h, f)
    assert (dK == 0).all() and (dV == 0).all() and (dB == 0).all()


# ---- 8. surface -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,h,f,weighted", [("lane", 2, 20, True), ("wave", 8, 16, False)])
def test_operator_equals_raw_calls(kind, h, f, weighted):
    """GTConvFuse_tbias + autograd.grad equals the raw binding calls bit for bit; `val` is saved only when it is not all
    ones; with B.requires_grad == False its gradient is None and the others are the same bits."""
    from DFGNN.operators.fused_gtconv import GTConvFuse_inference_tbias
    g = _graph(kind)
    d = _on_device(_case(kind, h, f, weighted, 5)[0])
    raw = _pair(g, d)
    q, k, v, b = (d[n].clone().requires_grad_(True) for n in ("Q", "K", "V", "B"))
    out = _op(g, d, q, k, v, b)
    assert any(t.data_ptr() == d["val"].data_ptr() for t in out.grad_fn.saved_tensors) == weighted
    grads = torch.autograd.grad(out, (q, k, v, b), d["dO"])
    assert torch.equal(out, raw["out"])
    for got, name in zip(grads, ("dQ", "dK", "dV", "dB")):
        assert torch.equal(got, raw[name]), name
    assert torch.equal(GTConvFuse_inference_tbias(g["row_ptr"], g["col_ind"], d["val"], d["Q"], d["K"], d["V"], d["B"],
                                                  d["etype"]), raw["out"])
    out = _op(g, d, q, k, v, d["B"])
    out.backward(d["dO"])
    assert d["B"].grad is None
    for t, name in zip((q, k, v), ("dQ", "dK", "dV")):
        assert torch.equal(t.grad, raw[name]), name


def test_layer_against_its_torch_branch():
    """SparseMHA_tbias(fuse=True) in training mode at two heads against its own fuse=False branch on the cora-like graph: the
    output and the gradients of the q / k / v projection weights and of rel_bias; in .eval() the inference operator gives
    the same output; --conv gt --format forward_tbias runs."""
    import argparse

    from DFGNN.layers import SparseMHA_tbias, load_graphconv_layer, preprocess_Hyper_fw_bw, preprocess_types
    from DFGNN.utils import synthetic as S
    torch.manual_seed(1)
    g = S.cora_like().to(DEV)
    params = preprocess_Hyper_fw_bw(g)
    nnz, T = params[3].numel(), 9
    types = preprocess_types(params, torch.randint(0, T, (nnz,), device=DEV), T)
    layer = SparseMHA_tbias(64, 64, 2, T).to(DEV).train()
    x = torch.randn(g.num_nodes(), 64, device=DEV)
    weights = (layer.q_proj.weight, layer.k_proj.weight, layer.v_proj.weight, layer.rel_bias)
    outs, grads = [], []
    for fuse in (False, True):
        layer.zero_grad()
        out = layer(params, x, types, fuse=fuse)
        (out * torch.linspace(-1, 1, out.numel(), device=DEV).reshape(out.shape)).sum().backward()
        outs.append(out.detach())
        grads.append([p.grad.clone() for p in weights])
    _check(outs[1], outs[0], "layer out")
    for name, a, b in zip(("q_proj.weight", "k_proj.weight", "v_proj.weight", "rel_bias"), *grads):
        _check(b, a, f"layer d{name}")
    assert float(grads[0][3].abs().max()) > 0
    with torch.no_grad():
        _check(layer.eval()(params, x, types, fuse=True), outs[0], "layer eval out")
    args = argparse.Namespace(conv="gt", format="forward_tbias", dim=64, heads=2)
    out, ms = load_graphconv_layer(args).to(DEV).train()(params, x, fuse=True)
    assert out.shape == (g.num_nodes(), 64) and ms > 0


def _empty_problem(m):
    import fused_gtconv as gt
    h, f, T = 2, 12, 3
    i32 = dict(dtype=torch.int32, device=DEV)
    gen = torch.Generator(device=DEV).manual_seed(m)
    row_ptr, none = torch.zeros(m + 1, **i32), torch.zeros(0, **i32)
    x, dO = torch.randn(m, h, f, device=DEV, generator=gen), torch.randn(m, h, f, device=DEV, generator=gen)
    B = torch.randn(T, h, device=DEV, generator=gen)
    out, mx, sm = gt.gt_forward_tbias(row_ptr, none, None, none, B, x, x, x)
    dQ, dK, dV, dB = gt.gt_backward_tbias(row_ptr, none, None, none, row_ptr, none, none, none, B, x, x, x, out, mx, sm, dO)
    torch.cuda.synchronize()
    assert out.shape == dQ.shape == dK.shape == dV.shape == (m, h, f) and mx.shape == sm.shape == (m, h)
    assert dB.shape == (T, h) and (dB == 0).all()
    if m:      # (m == 0 launches nothing but the reduction)
        for t in (out, dQ, dK, dV, sm):
            assert (t == 0).all()
        assert (mx == -1e38).all()
    return [out, mx, sm, dQ, dK, dV, dB]


def test_bindings_agree_and_empty_problems():
    """The torch C++ extension and the ctypes transport give bit-identical results for gt_inference_tbias, gt_forward_tbias
    and gt_backward_tbias (with and without dB), also on empty problems (m == 0, and m == 5 without an edge: zero outputs,
    sentinels, dB = 0), and the same RuntimeError words for a bad argument."""
    import dfgnn_native
    import fused_gtconv as gt
    assert dfgnn_native.ext() is not None and hasattr(dfgnn_native.ext(), "gt_bwd_tbias")
    cases = [(_graph(kind), _on_device(_case(kind, h, f, w, T)[0])) for kind, h, f, w, T in
             (("lane", 2, 20, True, 5), ("wave", 8, 16, False, 64), ("wave", 2, 260, True, 1))]

    def run():
        res = []
        for g, d in cases:
            both = _pair(g, d)
            res += [both[k] for k in zc.OUTPUTS]
            res += [_pair(g, d, need_dB=False)[k] for k in ("dQ", "dK", "dV")]
            res.append(gt.gt_inference_tbias(g["row_ptr"], g["col_ind"], d["val"], d["etype"], d["B"], d["Q"], d["K"], d["V"]))
        res += _empty_problem(0) + _empty_problem(5)
        g, d = cases[0]
        first = _pair(g, d)
        errs = []
        for bad in (dict(row_ptr=g["row_ptr"].long()), dict(etype=d["etype"][:-1].contiguous()),
                    dict(B=d["B"].t().contiguous()), dict(B=d["B"].reshape(-1)), dict(B=d["B"][:0])):
            a = dict(row_ptr=g["row_ptr"], etype=d["etype"], B=d["B"])
            a.update(bad)
            try:
                gt.gt_forward_tbias(a["row_ptr"], g["col_ind"], d["val"], a["etype"], a["B"], d["Q"], d["K"], d["V"])
                errs.append(None)
            except RuntimeError as e:
                errs.append(str(e))
        try:
            gt.gt_backward_tbias(g["row_ptr"], g["col_ind"], d["val"], d["etype"], g["col_ptr"], g["row_ind"], g["val_idx"],
                                 d["etype_csc"][:-1].contiguous(), d["B"], d["Q"], d["K"], d["V"], first["out"], first["row_max"],
                                 first["row_sum"], d["dO"])
            errs.append(None)
        except RuntimeError as e:
            errs.append(str(e))
        return res, errs

    via_ext, err_ext = run()
    saved = dfgnn_native._ext
    dfgnn_native._ext = None                      # force the ctypes path
    try:
        via_ctypes, err_ctypes = run()
    finally:
        dfgnn_native._ext = saved
    assert len(via_ext) == len(via_ctypes) == 3 * 11 + 14
    for a, b in zip(via_ext, via_ctypes):
        assert torch.equal(a, b)
    words = ("int32", "etype must have", "B must have", "B must have", "B must have", "etype_csc must have")
    for e1, e2, word in zip(err_ext, err_ctypes, words):
        assert e1 and e2 and word in e1 and word in e2, (e1, e2)


@pytest.mark.parametrize("kind,h,f,T,warmup", [("lane", 2, 20, 5, 3), ("wave", 1, 128, 4096, 0)])
def test_hipgraph_capture(kind, h, f, T, warmup):
    """fwd + bwd (with dB: CSR pass, CSC pass, reduction) recorded into a HIP graph (one stream, no parallel branches)
    replays bit-identically, also after Q and B were overwritten in place.  T = 4096 on the wave graph: four wave tables of
    64 KB together, the default limit of dynamic LDS, so no launch sets a function attribute -- that step is captured with
    no warm-up and no earlier eager run of its shape (only a step of ANOTHER shape runs first, so that the library and its
    code object are loaded), and the eager step that it is compared with runs after the capture."""
    import fused_gtconv as gt
    from DFGNN.utils import GraphedStep
    g = _graph(kind)
    if T == 4096:
        x = _inputs(g, h, f, True, np.random.default_rng(T).integers(0, T, g["nnz"]), T)
        _pair(_graph("lane"), _on_device(_case("lane", 2, 20, True, 5)[0]))
    else:
        x = _case(kind, h, f, True, T)[0]
    d = _on_device(x)
    gt.val_ptr(d["val"])        # (the all-ones test of `val`, a host synchronisation, is cached here: it launches no kernel of the pair)

    def step():
        out, mx, sm = gt.gt_forward_tbias(g["row_ptr"], g["col_ind"], d["val"], d["etype"], d["B"], d["Q"], d["K"], d["V"])
        return [out] + list(gt.gt_backward_tbias(g["row_ptr"], g["col_ind"], d["val"], d["etype"], g["col_ptr"], g["row_ind"],
                                                 g["val_idx"], d["etype_csc"], d["B"], d["Q"], d["K"], d["V"], out, mx, sm,
                                                 d["dO"]))

    graphed = GraphedStep(step, warmup=warmup)
    first = [t.clone() for t in graphed.replay()]
    for a, b in zip(step(), first):
        assert torch.equal(a, b)
    d["Q"].mul_(0.5)                                       # next "batch" of features, same structure
    d["B"].add_(0.25)
    again = [t.clone() for t in graphed.replay()]
    for a, b in zip(step(), again):
        assert torch.equal(a, b)
    assert not torch.equal(again[0], first[0])
    _check(first[-1], _reference(g, x)["dB"], f"graphed {kind} T={T} dB")


# ---- 9. memory --------------------------------------------------------------------------------------------------------
def test_memory_of_one_step():
    """The wave graph at h = 2, f = 16, T = 16.  The fused step allocates out, dQ, dK, dV (4 bytes(Q)), the statistics and
    delta (3 [m, h] arrays), the partials ws and dB -- nothing of h nnz floats.  Its peak over the inputs stays below
    bytes(ws) + 4 bytes(Q) + 3 bytes([m, h]) + bytes(B) + a slack of 8 KB: 16 allocations rounded up to the caching
    allocator's 512-byte blocks.  The slack is below 4 h nnz bytes, so one array of that size could not hide in it; the
    bias-pair step on the materialised B[etype].t() is above two such arrays (bias and dbias)."""
    import dfgnn_native
    from DFGNN.operators.fused_gtconv import GTConvFuse_bias
    g, h, f, T = _graph("wave"), 2, 16, 16
    d = _on_device(_case("wave", h, f, True, T)[0])
    bytes_q, bytes_mh, bytes_b, bytes_hnnz = 4 * g["m"] * h * f, 4 * g["m"] * h, 4 * T * h, 4 * h * g["nnz"]
    ws_floats = int(dfgnn_native.lib().dfgnn_gt_tbias_bwd_ws_floats(T, h))
    slack = 16 * 512
    assert ws_floats == 1024 * T * h and slack < bytes_hnnz

    def peak(fused):
        q, k, v, b = (d[n].clone().requires_grad_(True) for n in ("Q", "K", "V", "B"))

        def step():
            if fused:
                o = _op(g, d, q, k, v, b)
            else:
                o = GTConvFuse_bias(None, g["row_ptr"], g["col_ind"], d["val"], g["col_ptr"], g["row_ind"], g["val_idx"], 0,
                                    q, k, v, b[d["etype"].long()].t().contiguous())
            return torch.autograd.grad(o, (q, k, v, b), d["dO"])

        step()                                                   # (the all-ones test of `val` is cached here)
        torch.cuda.synchronize()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        res = step()
        torch.cuda.synchronize()
        assert len(res) == 4
        return torch.cuda.max_memory_allocated() - base

    p_tbias, p_bias = peak(True), peak(False)
    bound = 4 * ws_floats + 4 * bytes_q + 3 * bytes_mh + bytes_b + slack
    print(f"gt_tbias peak of one fwd+bwd: tbias {p_tbias} B (bound {bound} B, of which ws {4 * ws_floats} B, slack {slack} B), "
          f"bias pair on B[etype].t() {p_bias} B; 4 h nnz = {bytes_hnnz} B, bytes(Q) = {bytes_q} B")
    assert p_tbias <= bound
    assert p_bias > 2 * bytes_hnnz
