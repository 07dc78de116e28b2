"""Reference and fp32-level cases of the GatedGCN conv (dfgnn_gatedgcn_fwd / dfgnn_gatedgcn_bwd), shared by
tests/test_gatedgcn_host.py and tests/test_gpu_gatedgcn.py.

The reference is a torch formulation on the CPU -- index ops over the edge list, z_e = X_row_i + X_col_j + E_e, sg_e =
sigmoid(z_e), den_i = sum sg_e, out_i = sum sg_e (.) V_j [/ (den_i + eps)], Z = z, gradients from torch.autograd.grad of
(out, Z) with (dO, G) -- in float64 (or, for the bounds, the same formulation in float32).  An empty row has out = 0, den = 0,
dX_row = 0; an empty column dX_col = dV = 0.

The fp32-level cases are those of parity_cases.case_ids("gt") -- widths 32, 128, 7 x 2 and 260, both kernel forms, both
orientations -- with X_row = Q, X_col = K, V and dO of parity_cases.gt_inputs, E ~ N(0, 1) and G ~ N(0, 1) x G_SCALE, seeded,
float32 (G_SCALE = 1 / 32 as in tests/gt_gate_cases.py, for the reason given there: G does not shrink with the degree, and a
G above the gradient of a long row's edges would set the norm its dE is measured against).  The gates need no construction:
every edge carries a gate of the size of 1/2 in every dimension, so a lost edge moves den by 1 / degree of itself -- 0.4 %
at 257 edges, thousands of float32 roundings -- and everything downstream with it.  tests/test_gatedgcn_host.py proves the
power condition on exactly these inputs, in both modes.

Bounds are parity_cases.MARGIN x the float32 formulation's error against the float64 one in parity_cases.row_errors'
measure; Z and dE [nnz, h, f] are grouped by CSR row (all f values of all edges of a row form the row's vector), like dE of
tests/gt_edge_cases.py.  No output has a wider factor."""
import functools

import numpy as np
import torch

import parity_cases as pc
from gt_edge_cases import edge_rows

OUTPUTS = ("out", "den", "Z", "dX_row", "dX_col", "dV", "dE")
ROW_SIDE = ("out", "den", "dX_row", "Z", "dE")      # moved by a dropped CSR edge of a test row
COL_SIDE = ("dX_col", "dV")                         # ... by a dropped CSC entry of a test column
PER_EDGE = ("Z", "dE")                              # [nnz, h, f], grouped by CSR row
G_SCALE = 1.0 / 32
EPS = 1e-6
MODES = (1, 0)                                      # normalize


def reference(row_ptr, col_ind, E, G, X_row, X_col, V, dO, normalize=1, eps=EPS, acc="f64"):
    """Every output of the pair as numpy arrays in precision `acc` ("f64" / "f32").  E, G: [nnz, h, f] or None (zero).
    X_row, dO: [m, h, f]; X_col, V: [n_cols, h, f] (a square graph: n_cols = m)."""
    dt = torch.float64 if acc == "f64" else torch.float32
    m, nnz = X_row.shape[0], len(col_ind)
    rows = torch.from_numpy(np.repeat(np.arange(m), np.diff(row_ptr)).astype(np.int64))
    cols = torch.from_numpy(np.asarray(col_ind).astype(np.int64))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt)  # noqa: E731
    xr, xc, v = (t(a).requires_grad_(True) for a in (X_row, X_col, V))
    e = t(E if E is not None else np.zeros((nnz,) + X_row.shape[1:])).requires_grad_(True)
    z = (xr[rows] + xc[cols]) + e
    sg = torch.sigmoid(z)
    den = torch.zeros_like(xr).index_add_(0, rows, sg)
    out = torch.zeros_like(xr).index_add_(0, rows, sg * v[cols])
    if normalize:
        out = out / (den + eps)
    outs, seeds = ((out, z), (t(dO), t(G))) if G is not None else ((out,), (t(dO),))
    grads = torch.autograd.grad(outs, (xr, xc, v, e), seeds, allow_unused=True)
    grads = [torch.zeros_like(x) if gr is None else gr for gr, x in zip(grads, (xr, xc, v, e))]
    names = ("out", "den", "Z", "dX_row", "dX_col", "dV", "dE")
    return {k: a.detach().numpy() for k, a in zip(names, (out, den, z) + tuple(grads))}


def error_of(g, name, got, ref64, where=False):
    """parity_cases.worst with Z and dE grouped by CSR row."""
    if name in PER_EDGE:
        a, rp = edge_rows(got, g["row_ptr"])
        return pc.worst(a, edge_rows(ref64, g["row_ptr"])[0], row_ptr=rp, where=where)
    return pc.worst(got, ref64, where=where)


def boundary_inputs(case):
    """-> dict(E, G [nnz, h, f], X_row, X_col, V, dO) float32 of one fp32-level case (fresh arrays)."""
    g = pc.graph(case[0], case[1])
    x = pc.gt_inputs(*case)
    m, h, f = x["Q"].shape
    rng = np.random.default_rng(31 + 100 * f + 10 * h + int(case[4]) + (1000 if case[0] else 0) + (5000 if case[1] else 0))
    E = np.ascontiguousarray(rng.standard_normal((g["nnz"], h, f)).astype(np.float32))
    G = np.ascontiguousarray((rng.standard_normal((g["nnz"], h, f)) * G_SCALE).astype(np.float32))
    return dict(E=E, G=G, X_row=x["Q"].copy(), X_col=x["K"].copy(), V=x["V"].copy(), dO=x["dO"].copy())


def _run(row_ptr, col_ind, x, normalize, acc):
    return reference(row_ptr, col_ind, x["E"], x["G"], x["X_row"], x["X_col"], x["V"], x["dO"], normalize, EPS, acc)


@functools.lru_cache(maxsize=2)
def boundary_references(case, normalize):
    """-> (inputs, ref64, bounds): bounds[name] = MARGIN x the float32 formulation's worst error in output `name`."""
    g = pc.graph(case[0], case[1])
    x = boundary_inputs(case)
    ref64 = _run(g["row_ptr"], g["col_ind"], x, normalize, "f64")
    ref32 = _run(g["row_ptr"], g["col_ind"], x, normalize, "f32")
    bounds = {k: pc.MARGIN * error_of(g, k, ref32[k], ref64[k]) for k in OUTPUTS}
    return x, ref64, bounds


def mutated_reference(case, x, keep, row_ptr, col_ind, normalize):
    """The float64 reference of the case's inputs on the graph without the edges where keep is False."""
    y = dict(x)
    y["E"], y["G"] = np.ascontiguousarray(x["E"][keep]), np.ascontiguousarray(x["G"][keep])
    return _run(row_ptr, col_ind, y, normalize, "f64")
