"""Reference and fp32-level cases of the GT conv with typed edges (dfgnn_gt_fwd_typed / dfgnn_gt_bwd_typed), shared by
tests/test_gt_typed_host.py and tests/test_gpu_gt_typed.py.

The reference is the torch index-op formulation on the CPU: it materialises E = R[etype], runs the arithmetic of
tests/gt_edge_cases.py on it (k~_e = K_j + E_e, v~_e = V_j + E_e, gradients from torch.autograd.grad) and reduces dE to dR
with index_add -- in float64 or, for the bounds, in float32.  out, dQ and the statistics have m rows, K, V, dK, dV n_cols
rows: the graph may be rectangular.

The fp32-level cases reuse gt_edge_cases.boundary_inputs(case) verbatim with the table R = K'[:304] (the halved keys) and
etype = col_ind, T = 304: every edge of all four parity_cases.graph variants has a column below 304 (the padded graphs only
add isolated nodes above), so R[etype[e]] = K'[col_ind[e]] = E_e exactly and the references, the bounds and the power
condition proven in tests/test_gt_edge_host.py carry over unchanged for out, row_max, row_sum, dQ, dK, dV.  The bound of dR
is parity_cases.MARGIN x the float32 formulation's error against the float64 one in parity_cases.worst's measure over
[T, h, f] -- the treatment GATv2's dattn gets."""
import functools

import numpy as np
import torch

import gt_edge_cases as ec
import parity_cases as pc
from gt_bias_cases import SENTINEL_MAX

OUTPUTS = ("out", "row_max", "row_sum", "dQ", "dK", "dV", "dR")
BOUNDARY_T = 304


def _head(rows, cols, m, val, etype, r, q, k, v, dO):
    """One head on the edges (rows, cols) of an m x len(k) graph: -> out, row_max, row_sum, (dq, dk, dv, dr), detached."""
    q, k, v, r = (t.clone().requires_grad_(True) for t in (q, k, v, r))
    e = r[etype]                                                        # the materialised [nnz, f]
    s = (q[rows] * (k[cols] + e)).sum(-1) * val
    mx = torch.full((m,), float("-inf"), dtype=s.dtype).scatter_reduce(0, rows, s.detach(), reduce="amax", include_self=True)
    p = torch.exp(s - mx[rows])
    den = torch.zeros(m, dtype=s.dtype).index_add_(0, rows, p)
    out = torch.zeros_like(q).index_add_(0, rows, (v[cols] + e) * (p / den[rows])[:, None])
    if len(rows):
        dq, dk, dv, de = torch.autograd.grad(out, (q, k, v, e), dO)
        dr = torch.zeros_like(r).index_add_(0, etype, de)
    else:
        dq, dk, dv, dr = (torch.zeros_like(t) for t in (q, k, v, r))
    mx = torch.where(torch.isinf(mx), torch.full_like(mx, SENTINEL_MAX), mx)
    return out.detach(), mx, den.detach(), [t.detach() for t in (dq, dk, dv, dr)]


def reference(row_ptr, col_ind, n_cols, val, etype, R, Q, K, V, dO, acc="f64"):
    """Every output of the pair as numpy arrays in precision `acc` ("f64" / "f32").  R: [T, h, f]; Q, dO: [m, h, f]; K, V:
    [n_cols, h, f]."""
    dt = torch.float64 if acc == "f64" else torch.float32
    m, h, f = Q.shape
    assert K.shape == V.shape == (n_cols, h, f)
    rows = torch.from_numpy(np.repeat(np.arange(m), np.diff(row_ptr)).astype(np.int64))
    cols = torch.from_numpy(np.asarray(col_ind).astype(np.int64))
    types = torch.from_numpy(np.asarray(etype).astype(np.int64))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt)  # noqa: E731
    val_t, dOt = t(val), t(dO)
    res = dict(out=np.zeros((m, h, f)), dQ=np.zeros((m, h, f)), dK=np.zeros((n_cols, h, f)), dV=np.zeros((n_cols, h, f)),
               row_max=np.zeros((m, h)), row_sum=np.zeros((m, h)), dR=np.zeros(np.shape(R)))
    for hd in range(h):
        out, mx, den, (dq, dk, dv, dr) = _head(rows, cols, m, val_t, types, t(R[:, hd]), t(Q[:, hd]), t(K[:, hd]),
                                               t(V[:, hd]), dOt[:, hd])
        for name, a in (("out", out), ("dQ", dq), ("dK", dk), ("dV", dv), ("dR", dr)):
            res[name][:, hd] = a.numpy()
        res["row_max"][:, hd], res["row_sum"][:, hd] = mx.numpy(), den.numpy()
    return res


def error_of(g, name, got, ref64, where=False):
    """gt_edge_cases.error_of; dR [T, h, f] in parity_cases.worst's measure, a (type, head) per row."""
    if name == "dR":
        return pc.worst(got, ref64, where=where)
    return ec.error_of(g, name, got, ref64, where=where)


def boundary_inputs(case):
    """-> dict(val, etype, R [304, h, f], Q, K, V, dO, E): gt_edge_cases.boundary_inputs(case) and the table / types that
    give R[etype] == E exactly."""
    g = pc.graph(case[0], case[1])
    x = ec.boundary_inputs(case)
    assert int(g["col_ind"].max()) < BOUNDARY_T <= x["K"].shape[0]
    x["R"] = np.ascontiguousarray(x["K"][:BOUNDARY_T])
    x["etype"] = g["col_ind"].astype(np.int32)
    return x


def _dR(dE, etype, T, dt):
    """index_add of dE [nnz, h, f] by type, sequentially in precision dt."""
    out = torch.zeros((T,) + dE.shape[1:], dtype=dt)
    out.index_add_(0, torch.from_numpy(np.asarray(etype).astype(np.int64)), torch.from_numpy(np.ascontiguousarray(dE)).to(dt))
    return out.numpy()


@functools.lru_cache(maxsize=2)
def boundary_references(case):
    """-> (inputs, ref64, bounds): gt_edge_cases.boundary_references(case) -- the same inputs, references and bounds for out,
    row_max, row_sum, dQ, dK, dV -- plus dR: the float64 / float32 formulation's dE reduced by index_add in its own
    precision, bound = MARGIN x the float32 one's worst error."""
    g = pc.graph(case[0], case[1])
    x = boundary_inputs(case)
    xe, ref64e, bounds_e = ec.boundary_references(case)
    for k in ("val", "Q", "K", "V", "dO", "E"):
        assert np.array_equal(x[k], xe[k]), k
    ref64 = {k: ref64e[k] for k in OUTPUTS if k != "dR"}
    bounds = {k: bounds_e[k] for k in OUTPUTS if k != "dR"}
    ref32_dE = ec.reference(g["row_ptr"], g["col_ind"], x["val"], x["E"], x["Q"], x["K"], x["V"], x["dO"], "f32")["dE"]
    ref64["dR"] = _dR(ref64e["dE"], x["etype"], BOUNDARY_T, torch.float64)
    bounds["dR"] = pc.MARGIN * error_of(g, "dR", _dR(ref32_dE, x["etype"], BOUNDARY_T, torch.float32), ref64["dR"])
    return x, ref64, bounds
