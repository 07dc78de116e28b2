"""Reference and fp32-level cases of the GT conv with per-edge feature vectors in keys and values (dfgnn_gt_fwd_edge /
dfgnn_gt_bwd_edge), shared by tests/test_gt_edge_host.py and tests/test_gpu_gt_edge.py.

The reference is a torch formulation on the CPU -- index ops over the edge list, k~_e = K_j + E_e, v~_e = V_j + E_e,
gradients from torch.autograd.grad -- in float64 (or, for the bounds, the same formulation in float32).  An empty row has
out = 0, row_sum = 0, dQ = 0, row_max = -1e38 (the statistics pairs' sentinel).

The fp32-level cases are those of parity_cases.case_ids("gt") with K' = K / 2 (exact in fp32), E_e = K'_j and
V' = fp32(V - K'): K'_j + E_e = K_j exactly, so the logits are those of the proven case, and V'_j + E_e = V_j to one
rounding, so the messages are those of the proven case and the sentinels keep their weight.  Bounds are
parity_cases.MARGIN x the float32 formulation's error against the float64 one in parity_cases.row_errors' measure; dE
[nnz, h, f] is grouped by CSR row like attn_edge and dbias (all f values of all edges of a row form the row's vector).

One output has a wider bound, dK: MARGIN x gt_bias_cases.DK_FACTOR, for the reason derived in tests/gt_bias_cases.py: this
pair, too, takes delta_i = <dO_i, out_i> from the forward's output as it was stored, in fp32, and dK of a column of
in-degree 1 is a single edge's dS.  tests/test_gt_edge_host.py proves the power condition with that bound."""
import functools

import numpy as np
import torch

import parity_cases as pc
from gt_bias_cases import DK_FACTOR, SENTINEL_MAX

OUTPUTS = ("out", "row_max", "row_sum", "dQ", "dK", "dV", "dE")
ROW_SIDE = ("out", "row_sum", "dQ", "dE")           # moved by a dropped CSR edge of a test row (row_max: no sum, see
COL_SIDE = ("dK", "dV")                             # test_parity_cases_host.py); by a dropped CSC entry of a test column


def _head(rows, cols, m, val, e, q, k, v, dO):
    """One head on the edges (rows, cols): -> out, row_max, row_sum, (dq, dk, dv, de), all detached."""
    q, k, v, e = (t.clone().requires_grad_(True) for t in (q, k, v, e))
    s = (q[rows] * (k[cols] + e)).sum(-1) * val
    mx = torch.full((m,), float("-inf"), dtype=s.dtype).scatter_reduce(0, rows, s.detach(), reduce="amax", include_self=True)
    p = torch.exp(s - mx[rows])
    den = torch.zeros(m, dtype=s.dtype).index_add_(0, rows, p)
    out = torch.zeros_like(v).index_add_(0, rows, (v[cols] + e) * (p / den[rows])[:, None])
    grads = torch.autograd.grad(out, (q, k, v, e), dO) if len(rows) else [torch.zeros_like(t) for t in (q, k, v, e)]
    mx = torch.where(torch.isinf(mx), torch.full_like(mx, SENTINEL_MAX), mx)
    return out.detach(), mx, den.detach(), [t.detach() for t in grads]


def reference(row_ptr, col_ind, val, E, Q, K, V, dO, acc="f64"):
    """Every output of the pair as numpy arrays in precision `acc` ("f64" / "f32").  E: [nnz, h, f]."""
    dt = torch.float64 if acc == "f64" else torch.float32
    m, h, f = Q.shape
    nnz = len(col_ind)
    rows = torch.from_numpy(np.repeat(np.arange(m), np.diff(row_ptr)).astype(np.int64))
    cols = torch.from_numpy(np.asarray(col_ind).astype(np.int64))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt)  # noqa: E731
    val_t, dOt = t(val), t(dO)
    res = {k: np.zeros((m, h, f)) for k in ("out", "dQ", "dK", "dV")}
    res.update(row_max=np.zeros((m, h)), row_sum=np.zeros((m, h)), dE=np.zeros((nnz, h, f)))
    for hd in range(h):
        out, mx, den, (dq, dk, dv, de) = _head(rows, cols, m, val_t, t(E[:, hd]), t(Q[:, hd]), t(K[:, hd]), t(V[:, hd]),
                                               dOt[:, hd])
        for name, a in (("out", out), ("dQ", dq), ("dK", dk), ("dV", dv), ("dE", de)):
            res[name][:, hd] = a.numpy()
        res["row_max"][:, hd], res["row_sum"][:, hd] = mx.numpy(), den.numpy()
    return res


def edge_rows(a, row_ptr):
    """dE [nnz, h, f] -> ([h, nnz f], row_ptr f): the layout parity_cases' measure groups by CSR row."""
    a = np.asarray(a)
    return np.ascontiguousarray(a.transpose(1, 0, 2)).reshape(a.shape[1], -1), np.asarray(row_ptr, dtype=np.int64) * a.shape[2]


def error_of(g, name, got, ref64, where=False):
    """parity_cases.error_of with dE grouped by CSR row and row_max compared on rows with edges only."""
    if name == "dE":
        a, rp = edge_rows(got, g["row_ptr"])
        return pc.worst(a, edge_rows(ref64, g["row_ptr"])[0], row_ptr=rp, where=where)
    if name == "row_max":                       # (rows without edges hold the sentinel: out of the measure and of its floor)
        valid = np.diff(g["row_ptr"]) > 0
        got, ref64 = (np.where(valid[:, None], np.asarray(a, dtype=np.float64), 0.0) for a in (got, ref64))
        return pc.worst(got, ref64, valid=valid, where=where)
    return pc.worst(got, ref64, where=where)


def boundary_inputs(case):
    """-> dict(val, E [nnz, h, f], Q, K, V, dO) float32 of one fp32-level case (fresh arrays; see the module's docstring)."""
    g = pc.graph(case[0], case[1])
    x = pc.gt_inputs(*case)
    K = np.ascontiguousarray(x["K"] * np.float32(0.5))
    assert (K.astype(np.float64) * 2 == x["K"].astype(np.float64)).all()
    E = np.ascontiguousarray(K[g["col_ind"].astype(np.int64)])
    assert (E + K[g["col_ind"].astype(np.int64)] == x["K"][g["col_ind"].astype(np.int64)]).all()
    V = np.ascontiguousarray((x["V"].astype(np.float64) - K.astype(np.float64)).astype(np.float32))
    return dict(val=x["val"].copy(), E=E, Q=x["Q"].copy(), K=K, V=V, dO=x["dO"].copy())


def _run(row_ptr, col_ind, x, acc):
    return reference(row_ptr, col_ind, x["val"], x["E"], x["Q"], x["K"], x["V"], x["dO"], acc)


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
    y["val"], y["E"] = x["val"][keep], np.ascontiguousarray(x["E"][keep])
    return _run(row_ptr, col_ind, y, "f64")
