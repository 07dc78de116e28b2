"""Reference and fp32-level cases of the GT conv with a per-edge multiplicative gate on the keys and an edge output
(dfgnn_gt_fwd_gate / dfgnn_gt_bwd_gate), shared by tests/test_gt_gate_host.py and tests/test_gpu_gt_gate.py.

The reference is a torch formulation on the CPU -- index ops over the edge list, W_e = val_e Q_i (.) (K_j (.) E_e),
s_e = sum_d W_e[d], gradients from torch.autograd.grad of (out, W) with (dO, G) -- in float64 (or, for the bounds, the same
formulation in float32).  An empty row has out = 0, row_sum = 0, dQ = 0, row_max = -1e38 (the statistics pairs' sentinel).

The fp32-level cases are those of parity_cases.case_ids("gt") with E_e[d] = 2^c_d, c_d cycling through -1, 0, 1 over the
dimensions (the same row for every edge and head), and Q'[:, :, d] = Q[:, :, d] 2^-c_d.  Both are exact in fp32, and so is
every product K_j[d] E_e[d]; Q'[d] (K_j[d] E_e[d]) is the real number Q[d] K_j[d], so every fused multiply-add of the dot
product rounds what it rounds in the proven case: the logits are those of the proven case EXACTLY and the sentinels keep
their weight.  boundary_inputs asserts the exactness.

G, the gradient of the edge output, is seeded N(0, 1) x G_SCALE with G_SCALE = 1 / 32.  Why that scale: g_e[d] = dS_e +
G_e[d], and dS_e = P_e (dP_e - delta_i) -- dP of the size of sqrt(f), P_e of the size of 1 / degree -- lies between a few
hundredths (the rows of 250 and more edges) and a few units (the short ones).  dE is measured relative to the largest
|dE| of its ROW, and G, unlike every term of the additive pairs' dE, does not shrink with P_e: a G above the dS of the long
rows sets that norm there, the fp32 error of dE becomes relative to |G|, and what the loss of an edge does to the dE of the
edges that stay (it moves dS only) falls below POWER x bound -- at G_SCALE = 1 / 4 the least move of dE is 17 x the
float32 error where 32 x are required (figures of the float64 and float32 references alone; no kernel is involved).  At
1 / 32, the dS of the long rows, the least move is 200 x; and G is still at least a hundredth of g on every edge, 1000 x
the bounds, so a kernel that reads G through a wrong slot or not at all fails every case.  tests/test_gt_gate_host.py proves
the power condition with this scale.

Bounds are parity_cases.MARGIN x the float32 formulation's error against the float64 one in parity_cases.row_errors'
measure; W and dE [nnz, h, f] are grouped by CSR row (all f values of all edges of a row form the row's vector), like dE of
tests/gt_edge_cases.py.  One output has a wider bound, dK: MARGIN x gt_bias_cases.DK_FACTOR, for the reason derived in
tests/gt_bias_cases.py: this pair, too, takes delta_i = <dO_i, out_i> from the forward's output as it was stored, in fp32,
and dK of a column of in-degree 1 is a single edge's dS (times val Q (.) E)."""
import functools

import numpy as np
import torch

import parity_cases as pc
from gt_bias_cases import DK_FACTOR, SENTINEL_MAX
from gt_edge_cases import edge_rows

OUTPUTS = ("out", "W", "row_max", "row_sum", "dQ", "dK", "dV", "dE")
ROW_SIDE = ("out", "W", "row_sum", "dQ", "dE")      # moved by a dropped CSR edge of a test row (row_max: no sum, see
COL_SIDE = ("dK", "dV")                             # test_parity_cases_host.py); by a dropped CSC entry of a test column
PER_EDGE = ("W", "dE")                              # [nnz, h, f], grouped by CSR row
G_SCALE = 1.0 / 32                                  # the module's docstring says why
GATE_EXPONENTS = (-1, 0, 1)


def _head(rows, cols, m, val, e, g, q, k, v, dO):
    """One head on the edges (rows, cols): -> out, w, row_max, row_sum, (dq, dk, dv, de), all detached.  g: the gradient
    of w, or None (zero)."""
    q, k, v, e = (t.clone().requires_grad_(True) for t in (q, k, v, e))
    w = q[rows] * (k[cols] * e) * val[:, None]
    s = w.sum(-1)
    mx = torch.full((m,), float("-inf"), dtype=s.dtype).scatter_reduce(0, rows, s.detach(), reduce="amax", include_self=True)
    p = torch.exp(s - mx[rows])
    den = torch.zeros(m, dtype=s.dtype).index_add_(0, rows, p)
    out = torch.zeros((m,) + tuple(v.shape[1:]), dtype=v.dtype).index_add_(0, rows, v[cols] * (p / den[rows])[:, None])
    if len(rows):
        outs, seeds = ((out, w), (dO, g)) if g is not None else ((out,), (dO,))
        grads = torch.autograd.grad(outs, (q, k, v, e), seeds)
    else:
        grads = [torch.zeros_like(t) for t in (q, k, v, e)]
    mx = torch.where(torch.isinf(mx), torch.full_like(mx, SENTINEL_MAX), mx)
    return out.detach(), w.detach(), mx, den.detach(), [t.detach() for t in grads]


def reference(row_ptr, col_ind, val, E, G, Q, K, V, dO, acc="f64"):
    """Every output of the pair as numpy arrays in precision `acc` ("f64" / "f32").  E, G: [nnz, h, f]; G None: zero.
    Q, dO: [m, h, f]; K, V: [n_cols, h, f] (a square graph: n_cols = m)."""
    dt = torch.float64 if acc == "f64" else torch.float32
    m, h, f = Q.shape
    n_cols, nnz = K.shape[0], len(col_ind)
    rows = torch.from_numpy(np.repeat(np.arange(m), np.diff(row_ptr)).astype(np.int64))
    cols = torch.from_numpy(np.asarray(col_ind).astype(np.int64))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt)  # noqa: E731
    val_t, dOt = t(val), t(dO)
    res = dict(out=np.zeros((m, h, f)), dQ=np.zeros((m, h, f)), dK=np.zeros((n_cols, h, f)), dV=np.zeros((n_cols, h, f)))
    res.update(row_max=np.zeros((m, h)), row_sum=np.zeros((m, h)), W=np.zeros((nnz, h, f)), dE=np.zeros((nnz, h, f)))
    for hd in range(h):
        out, w, mx, den, (dq, dk, dv, de) = _head(rows, cols, m, val_t, t(E[:, hd]), None if G is None else t(G[:, hd]),
                                                  t(Q[:, hd]), t(K[:, hd]), t(V[:, hd]), dOt[:, hd])
        for name, a in (("out", out), ("W", w), ("dQ", dq), ("dK", dk), ("dV", dv), ("dE", de)):
            res[name][:, hd] = a.numpy()
        res["row_max"][:, hd], res["row_sum"][:, hd] = mx.numpy(), den.numpy()
    return res


def error_of(g, name, got, ref64, where=False):
    """parity_cases.error_of with W and dE grouped by CSR row and row_max compared on rows with edges only."""
    if name in PER_EDGE:
        a, rp = edge_rows(got, g["row_ptr"])
        return pc.worst(a, edge_rows(ref64, g["row_ptr"])[0], row_ptr=rp, where=where)
    if name == "row_max":                       # (rows without edges hold the sentinel: out of the measure and of its floor)
        valid = np.diff(g["row_ptr"]) > 0
        got, ref64 = (np.where(valid[:, None], np.asarray(a, dtype=np.float64), 0.0) for a in (got, ref64))
        return pc.worst(got, ref64, valid=valid, where=where)
    return pc.worst(got, ref64, where=where)


def boundary_inputs(case):
    """-> dict(val, E, G [nnz, h, f], Q, K, V, dO) float32 of one fp32-level case (fresh arrays; see the module's
    docstring)."""
    g = pc.graph(case[0], case[1])
    x = pc.gt_inputs(*case)
    m, h, f = x["Q"].shape
    c = np.asarray(GATE_EXPONENTS)[np.arange(f) % len(GATE_EXPONENTS)]
    gate = np.exp2(c).astype(np.float32)                                         # [f]: 0.5, 1, 2, 0.5, ...
    Q = np.ascontiguousarray(x["Q"] * np.exp2(-c).astype(np.float32))
    E = np.ascontiguousarray(np.broadcast_to(gate, (g["nnz"], h, f)))
    K64 = x["K"].astype(np.float64)
    assert (Q.astype(np.float64) * gate.astype(np.float64) == x["Q"].astype(np.float64)).all()      # Q' E = Q, exactly
    assert ((x["K"] * gate).astype(np.float64) == K64 * gate.astype(np.float64)).all()              # K E is exact in fp32
    assert np.isfinite(Q).all() and (np.abs(Q[x["Q"] != 0]) > 1e-30).all()                           # (nothing underflowed)
    rng = np.random.default_rng(77 + 100 * f + 10 * h + int(case[4]) + (1000 if case[0] else 0) + (5000 if case[1] else 0))
    G = np.ascontiguousarray((rng.standard_normal((g["nnz"], h, f)) * G_SCALE).astype(np.float32))
    return dict(val=x["val"].copy(), E=E, G=G, Q=Q, K=x["K"].copy(), V=x["V"].copy(), dO=x["dO"].copy())


def _run(row_ptr, col_ind, x, acc):
    return reference(row_ptr, col_ind, x["val"], x["E"], x["G"], x["Q"], x["K"], x["V"], x["dO"], acc)


@functools.lru_cache(maxsize=2)
def boundary_references(case):
    """-> (inputs, ref64, bounds): bounds[name] = MARGIN x the float32 formulation's worst error in output `name`."""
    g = pc.graph(case[0], case[1])
    x = boundary_inputs(case)
    ref64 = _run(g["row_ptr"], g["col_ind"], x, "f64")
    ref32 = _run(g["row_ptr"], g["col_ind"], x, "f32")
    bounds = {k: pc.MARGIN * (DK_FACTOR if k == "dK" else 1.0) * error_of(g, k, ref32[k], ref64[k]) for k in OUTPUTS}
    return x, ref64, bounds


def mutated_reference(case, x, keep, row_ptr, col_ind):
    """The float64 reference of the case's inputs on the graph without the edges where keep is False."""
    y = dict(x)
    y["val"] = x["val"][keep]
    y["E"], y["G"] = np.ascontiguousarray(x["E"][keep]), np.ascontiguousarray(x["G"][keep])
    return _run(row_ptr, col_ind, y, "f64")
