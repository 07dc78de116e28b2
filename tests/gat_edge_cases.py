"""Reference and fp32-level cases of the any-graph GAT pair with a per-edge attention term (dfgnn_gat_fwd_edge /
dfgnn_gat_bwd_edge), shared by tests/test_gat_edge_host.py and tests/test_gpu_gat_edge.py.

The reference is a torch formulation on the CPU -- index ops over the edge list, pre_e = (attn_row_i + attn_col_j) +
score_e, s_e = LeakyReLU(pre_e), P_e = exp(s_e - max_i) / sum_i over ALL edges of the row, out_i = sum k_e P_e X_j with k_e
= (mask_e > attn_drop) / (1 - attn_drop), gradients from torch.autograd.grad of out with dO -- in float64 (or, for the
bounds, the same formulation in float32).  An empty row -- and a (row, head) whose scores are all -inf -- has out = 0,
edge_max = -1e38, edge_sum = 0, grad_attn_row = 0; an empty column grad_feat = 0, grad_attn_col = 0.

The fp32-level cases are those of parity_cases.case_ids("gat") -- widths 32, 128, 7 x 2 and 260, both kernel forms, both
orientations -- with parity_cases.gat_inputs, a seeded score ~ N(0, 1/4) [h, nnz] and the sentinels re-aimed so that their
pre_e is still +3 with the score included: as built attn_col of the sentinel column (it has that one edge), transposed
attn_row of the sentinel row (for its edge into the test column) and then its attn_col (for its self-loop).
tests/test_gat_edge_host.py proves the power condition on exactly these inputs.

Bounds are parity_cases.MARGIN x the float32 formulation's error against the float64 one in parity_cases.row_errors'
measure; grad_score [h, nnz] is grouped by CSR row like attn_edge; edge_max / edge_sum are measured on rows with edges.  No
output has a wider factor."""
import functools

import numpy as np
import torch

import parity_cases as pc

OUTPUTS = ("out", "edge_max", "edge_sum", "grad_feat", "grad_attn_row", "grad_attn_col", "grad_score")
ROW_SIDE = ("out", "edge_max", "edge_sum", "grad_attn_row", "grad_score")     # moved by a dropped CSR edge of a test row
COL_SIDE = ("grad_feat", "grad_attn_col")                                     # ... by a dropped CSC entry of a test column
SCORE_STD = 0.5
EMPTY_MAX = -1e38


def reference(row_ptr, col_ind, attn_row, attn_col, score, X, dO, slope=pc.SLOPE, mask=None, attn_drop=0.0, acc="f64"):
    """Every output of the pair as numpy arrays in precision `acc` ("f64" / "f32").  attn_row, dO rows: m; attn_col, X rows:
    n_cols (a square graph: n_cols = m); score: [h, nnz] in CSR order or None (zeros); mask: [nnz, h] or None."""
    dt = torch.float64 if acc == "f64" else torch.float32
    m, nnz, h = attn_row.shape[0], len(col_ind), attn_row.shape[1]
    rows = torch.from_numpy(np.repeat(np.arange(m), np.diff(row_ptr)).astype(np.int64))
    cols = torch.from_numpy(np.asarray(col_ind).astype(np.int64))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt)  # noqa: E731
    ar, ac, x = (t(a).requires_grad_(True) for a in (attn_row, attn_col, X))
    sc = t(np.asarray(score).T if score is not None else np.zeros((nnz, h))).requires_grad_(True)      # [nnz, h]
    pre = (ar[rows] + ac[cols]) + sc
    s = torch.where(torch.isinf(pre), pre, torch.nn.functional.leaky_relu(pre, slope))
    mx = torch.full((m, h), float("-inf"), dtype=dt)
    mx = mx.scatter_reduce(0, rows[:, None].expand_as(s), s.detach(), reduce="amax", include_self=True)
    shift = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)                 # empty or fully masked row
    p = torch.exp(s - shift[rows])
    den = torch.zeros((m, h), dtype=dt).index_add_(0, rows, p)
    p = p / torch.where(den == 0, torch.ones_like(den), den)[rows]
    if mask is not None:
        p = p * (t(mask) > attn_drop).to(dt) / (1.0 - attn_drop)
    out = torch.zeros((m,) + tuple(x.shape[1:]), dtype=dt).index_add_(0, rows, x[cols] * p[:, :, None])
    leaves = (x, ar, ac, sc)
    grads = torch.autograd.grad(out, leaves, t(dO), allow_unused=True) if out.requires_grad else [None] * 4
    gx, gar, gac, gsc = (torch.zeros_like(l) if gr is None else gr for gr, l in zip(grads, leaves))
    n = lambda a: a.detach().numpy()  # noqa: E731
    emax = n(mx).copy()
    emax[np.isinf(emax)] = EMPTY_MAX
    gsc = n(gsc).copy()
    gsc[np.isinf(n(pre))] = 0.0                                                    # (a masked edge: 0, whatever autograd makes of -inf)
    return dict(out=n(out), edge_max=emax, edge_sum=n(den), grad_feat=n(gx), grad_attn_row=n(gar), grad_attn_col=n(gac),
                grad_score=np.ascontiguousarray(gsc.T))


def error_of(g, name, got, ref64, where=False):
    """parity_cases.worst with grad_score grouped by CSR row and the statistics on rows with edges."""
    if name == "grad_score":
        return pc.worst(got, ref64, row_ptr=g["row_ptr"], where=where)
    if name in pc.STATS:
        return pc.worst(got, ref64, valid=np.diff(g["row_ptr"]) > 0, where=where)
    return pc.worst(got, ref64, where=where)


def boundary_inputs(case):
    """-> dict(attn_row, attn_col [m, h], score [h, nnz], X, dO) float32 of one fp32-level case (fresh arrays)."""
    transposed, low, f, h = case
    g = pc.graph(transposed, low)
    x = pc.gat_inputs(*case)
    rng = np.random.default_rng(41 + 100 * f + 10 * h + (1000 if transposed else 0) + (5000 if low else 0))
    score = (rng.standard_normal((h, g["nnz"])) * SCORE_STD).astype(np.float32)
    ar, ac = x["attn_row"].astype(np.float64), x["attn_col"].astype(np.float64)
    if transposed:      # the sentinel row's two edges: slot e into the test column, slot e + 1 its self-loop
        s, a, e = pc._sentinels(g)
        ar[s] = pc.SENTINEL_LOGIT - ac[a] - score[:, e].T
        ar = ar.astype(np.float32).astype(np.float64)
        ac[s] = pc.SENTINEL_LOGIT - ar[s] - score[:, e + 1].T
    else:               # the sentinel column's one edge (those of gat_inputs: test rows of degree >= 3)
        s, a, e = pc._sentinels(g, 3)
        ac[s] = pc.SENTINEL_LOGIT - ar[a] - score[:, e].T
    f32 = lambda v: np.ascontiguousarray(v, dtype=np.float32)  # noqa: E731
    return dict(attn_row=f32(ar), attn_col=f32(ac), score=np.ascontiguousarray(score), X=x["X"].copy(), dO=x["dO"].copy())


def _run(row_ptr, col_ind, x, acc):
    return reference(row_ptr, col_ind, x["attn_row"], x["attn_col"], x["score"], x["X"], x["dO"], pc.SLOPE, acc=acc)


@functools.lru_cache(maxsize=2)
def boundary_references(case):
    """-> (inputs, ref64, bounds): bounds[name] = MARGIN x the float32 formulation's worst error in output `name`."""
    g = pc.graph(case[0], case[1])
    x = boundary_inputs(case)
    ref64 = _run(g["row_ptr"], g["col_ind"], x, "f64")
    ref32 = _run(g["row_ptr"], g["col_ind"], x, "f32")
    bounds = {k: pc.MARGIN * error_of(g, k, ref32[k], ref64[k]) for k in OUTPUTS}
    return x, ref64, bounds


def mutated_reference(x, keep, row_ptr, col_ind):
    """The float64 reference of a case's inputs on the graph without the edges where keep is False."""
    y = dict(x)
    y["score"] = np.ascontiguousarray(x["score"][:, keep])
    return _run(row_ptr, col_ind, y, "f64")
