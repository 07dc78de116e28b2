"""One-head GT backward of 161 .. 192-node ranges (csrc/dfgnn_dense_wide.hpp: dense_bwd_wide2_body -- two row blocks of <= 96
rows against all columns) and the order `gt_dense_bwd_kernel` takes the ranges in (csrc/gt_dense.hip: bwd_reverse_keep,
bwd_order_tail).  Sizes at the edges of the class (161, 176, 177 = a second row block of one strip plus one row, 192), the
neighbours 160 and 193 that keep their bodies, and a mixed batch that sends every class through the remapped order.

The accuracy bound is the parent commit's own error: PARENT_ERR holds, per (features, batch), the largest error relative to
the largest element of each array that commit abe8225 reached against the float64 oracle on exactly these inputs (measured
once on an MI355X; both call paths agree to the bit there).  The new body changes the order of summation and nothing else,
so it may reach at most 2 x that (a lost term shows as orders of magnitude), and never more than FP32_BAR, the bar of
test_gpu_parity.py::test_dense_kernels_are_fp32_equivalent."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
FP32_BAR = 2e-4
P_EDGE = 0.43
CLASS_SIZES = (161, 176, 177, 192)
NEIGHBOURS = (160, 193)
MIXED = (186, 50, 128, 161, 140)
BATCHES = {**{str(n): (n,) for n in CLASS_SIZES + NEIGHBOURS}, "mixed": MIXED}
ARRAYS = ("out", "dQ", "dK", "dV")

# commit abe8225, MI355X: max |got - oracle| / max |oracle| per array, (features, batch) -> (out, dQ, dK, dV)
PARENT_ERR = {
    (128, "161"): (5.754e-07, 5.101e-07, 5.199e-07, 3.308e-07),
    (128, "176"): (5.417e-07, 4.809e-07, 2.957e-07, 3.916e-07),
    (128, "177"): (5.146e-07, 3.678e-07, 2.585e-07, 6.149e-07),
    (128, "192"): (7.253e-07, 1.035e-06, 5.730e-07, 5.791e-07),
    (128, "160"): (3.366e-07, 3.994e-07, 2.675e-07, 3.850e-07),
    (128, "193"): (6.183e-07, 6.310e-07, 4.081e-07, 7.093e-07),
    (128, "mixed"): (4.975e-07, 6.071e-07, 6.212e-07, 5.226e-07),
    (64, "161"): (6.648e-07, 3.311e-07, 4.545e-07, 4.100e-07),
    (64, "176"): (5.768e-07, 3.603e-07, 6.792e-07, 4.291e-07),
    (64, "177"): (2.554e-07, 4.194e-07, 3.341e-07, 1.821e-07),
    (64, "192"): (7.302e-07, 7.693e-07, 5.573e-07, 8.525e-07),
    (64, "160"): (5.389e-07, 4.920e-07, 4.068e-07, 4.691e-07),
    (64, "193"): (5.744e-07, 4.429e-07, 6.084e-07, 5.141e-07),
    (64, "mixed"): (2.999e-07, 4.178e-07, 6.369e-07, 2.951e-07),
}


def _sym_graph(rng, n, lonely=(), single=None):
    """Symmetric Erdos-Renyi graph, p = 0.43; nodes in `lonely` lose all edges; `single` = (node, partner): that node keeps
    exactly the edge pair with its partner (one out-edge, one in-edge)."""
    from DFGNN.utils import Graph
    iu, ju = np.triu_indices(n, k=1)
    keep = rng.random(len(iu)) < P_EDGE
    gone = list(lonely) + ([single[0]] if single else [])
    keep &= ~np.isin(iu, gone) & ~np.isin(ju, gone)
    s, d = iu[keep], ju[keep]
    if single:
        s, d = np.append(s, min(single)), np.append(d, max(single))
    return Graph(np.concatenate([s, d]), np.concatenate([d, s]), n)


def _inputs(sizes, f, seed, **kw):
    from DFGNN.layers import preprocess_Hyper_fw_bw
    from DFGNN.utils import batch
    from DFGNN.utils import synthetic as S
    rng = np.random.default_rng(seed)
    g = batch([_sym_graph(rng, n, **kw) for n in sizes]).to(DEV)
    A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem = preprocess_Hyper_fw_bw(g)
    m = g.num_nodes()
    Q, K, V = S.gt_features(m, 1, f, seed=seed + 1, device=DEV)
    dO = torch.randn(m, 1, f, generator=torch.Generator().manual_seed(seed + 2)).to(DEV)
    return dict(rows=rows, row_ptr=row_ptr, col_ind=col_ind, val=val, col_ptr=col_ptr, row_ind=row_ind, val_idx=val_idx,
                smem=smem, Q=Q, K=K, V=V, dO=dO)


def _autograd_path(x):
    """GTConvFuse_hyper + autograd.grad: the rank-ordered attn_edge pair at one head."""
    import fused_gtconv as gt
    from DFGNN.operators.fused_gtconv import GTConvFuse_hyper
    assert gt.gt_ranked_pair_chosen(x["row_ptr"], x["col_ind"], x["val"], x["Q"]) is not None
    Q, K, V = (x[k].clone().requires_grad_(True) for k in "QKV")
    out = GTConvFuse_hyper(x["rows"], x["row_ptr"], x["col_ind"], x["val"], x["col_ptr"], x["row_ind"], x["val_idx"], x["smem"],
                           Q, K, V)
    dQ, dK, dV = torch.autograd.grad(out, (Q, K, V), x["dO"])
    return out.detach(), dQ, dK, dV


def _csr_path(x):
    """dfgnn_gt_hyper_fwd / dfgnn_gt_bwd: attention values and coordinates in CSR order."""
    import fused_gtconv as gt
    args = (x["row_ptr"], x["col_ind"], x["rows"], x["val"], x["col_ptr"], x["row_ind"], x["val_idx"], x["smem"], x["Q"],
            x["K"], x["V"])
    out, attn = gt.gt_hyper_forward(*args)
    return (out,) + tuple(gt.gt_backward(*args, attn, x["dO"]))


def _oracle(oracle_mod, x):
    n_ = lambda t: t.detach().cpu().numpy()  # noqa: E731
    a = (n_(x["row_ptr"]), n_(x["col_ind"]), n_(x["val"]), n_(x["Q"]), n_(x["K"]), n_(x["V"]))
    return (oracle_mod.gt_forward(*a),) + tuple(oracle_mod.gt_backward(*a, n_(x["dO"])))


def _rel_to_max(got, want):
    got = got.detach().cpu().double().numpy()
    want = np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))


_CASES = {}


def case_errors(oracle_mod, f, name):
    """(inputs, oracle arrays, {path: (out, dQ, dK, dV)}, {path: errors}) of one batch, computed once per session."""
    if (f, name) not in _CASES:
        x = _inputs(BATCHES[name], f, seed=1000 + 7 * len(name) + sum(BATCHES[name]) + f)
        want = _oracle(oracle_mod, x)
        got = {"autograd": _autograd_path(x), "csr": _csr_path(x)}
        err = {p: tuple(_rel_to_max(a, w) for a, w in zip(arrs, want)) for p, arrs in got.items()}
        _CASES[(f, name)] = (x, want, got, err)
    return _CASES[(f, name)]


@pytest.mark.parametrize("name", list(BATCHES))
@pytest.mark.parametrize("f", [128, 64])
def test_accuracy_against_the_parent_commits_own_error(oracle_mod, f, name):
    _, _, got, err = case_errors(oracle_mod, f, name)
    for path, errs in err.items():
        print(f"f={f} batch={name} {path}: " + " ".join(f"{w}={e:.3e}" for w, e in zip(ARRAYS, errs)))
    for path, errs in err.items():
        for what, arr, e, parent in zip(ARRAYS, got[path], errs, PARENT_ERR[(f, name)]):
            assert torch.isfinite(arr).all(), (path, what)
            assert e <= 2 * parent, f"{path} {what}: {e:.3e} against the parent commit's {parent:.3e}"
            assert e <= FP32_BAR, f"{path} {what}: {e:.3e}"


_CHILD = r"""
import sys
sys.path[:0] = [%(root)r, %(root)r + "/df-gnn_amd", %(root)r + "/tests"]
import numpy as np
import test_gpu_bwd_192 as T
x = T._inputs(T.MIXED, int(sys.argv[1]), seed=int(sys.argv[2]))
np.savez(sys.argv[3], **{p: np.stack([a.cpu().numpy() for a in fn(x)[1:]]) for p, fn in
                         (("autograd", T._autograd_path), ("csr", T._csr_path))})
"""


@pytest.mark.parametrize("f", [128, 64])
def test_gradients_do_not_depend_on_the_range_order(tmp_path, f):
    """dQ, dK, dV of the mixed batch, bit for bit, in plan order (DFGNN_BWD_REVERSE=0, read once: a fresh process) and in the
    default order (largest eighth, middle reversed, smallest quarter last)."""
    seed = 77
    x = _inputs(MIXED, f, seed=seed)
    here = {"autograd": _autograd_path(x)[1:], "csr": _csr_path(x)[1:]}
    dump = str(tmp_path / "plan_order.npz")
    env = dict(os.environ, DFGNN_BWD_REVERSE="0")
    env.pop("DFGNN_BWD_TAIL", None)
    run = subprocess.run([sys.executable, "-c", _CHILD % {"root": ROOT}, str(f), str(seed), dump], env=env,
                         capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, run.stderr[-3000:]
    there = np.load(dump)
    for path, arrs in here.items():
        for k, what in enumerate(("dQ", "dK", "dV")):
            assert np.array_equal(arrs[k].cpu().numpy(), there[path][k]), (path, what)


@pytest.mark.parametrize("f", [128, 64])
def test_every_edge_is_counted(oracle_mod, f):
    """177 nodes: the last node (the one row of the second row block's second strip) has exactly one out-edge and one
    in-edge -- its dK and dV rows are non-zero and the oracle's (its dQ row is zero in exact arithmetic: a softmax over one
    edge has no gradient, so that row is held to the oracle's zero); a node without edges gets exact zeros."""
    n, last, partner, lonely = 177, 176, 5, 100
    x = _inputs((n,), f, seed=31 + f, lonely=(lonely,), single=(last, partner))
    rp, ci = x["row_ptr"].cpu().numpy(), x["col_ind"].cpu().numpy()
    assert rp[last + 1] - rp[last] == 1 and int((ci == last).sum()) == 1 and rp[lonely + 1] == rp[lonely]
    assert int((ci == lonely).sum()) == 0
    want = _oracle(oracle_mod, x)
    for path, fn in (("autograd", _autograd_path), ("csr", _csr_path)):
        got = fn(x)
        for what, a, w in zip(ARRAYS, got, want):
            assert _rel_to_max(a, w) <= FP32_BAR, (path, what)
            if what == "out":
                continue
            row, wrow = a[last].detach().cpu().double().numpy(), np.asarray(w, dtype=np.float64)[last]
            if what == "dQ":  # (softmax over ONE edge: P = 1, dS = 0 -- the oracle's row is zero, and so must this one be)
                assert np.abs(wrow).max() <= 1e-12 and np.abs(row).max() <= FP32_BAR * np.abs(np.asarray(w)).max(), (path, what)
            else:
                assert np.abs(row).max() > 0 and np.abs(wrow).max() > 0, (path, what)
                assert np.abs(row - wrow).max() <= FP32_BAR * np.abs(wrow).max(), (path, what)
            assert not a[lonely].any(), (path, what)
