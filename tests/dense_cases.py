"""Cases, inputs and references for the fp32-level tests of the matrix-core ("dense") kernels
(tests/test_dense_cases_host.py, tests/test_gpu_dense_exact.py).  Measure, MARGIN and POWER are those of
tests/parity_cases.py: bound = MARGIN x the plain-fp32 reference's own error against the float64 one, per
output, in the per-row measure; nothing about the kernel under test enters a bound.

Batches.  Block-diagonal batches of DIRECTED member graphs (the out-edge bitmap differs from the in-edge bitmap), no
duplicate edge, every member one dense range of the plan:
  narrow   one range of every size in NARROW_SIZES (<= 128 nodes: one head at f = 64 / 128 takes the 256-thread forward),
           ordered so that two neighbours always hold more than 128 nodes -- the plan merges nothing;
  wide     one range of every size in WIDE_SIZES (129 .. 255), the sizes 16, 64 and 128 in between, and the hole copies.
Every range holds Erdos-Renyi edges (out-degree about 25 - 50, p = 0.6 for the small ones) and the full probe grid
B(n) x B(n), B(n) = {0, n - 1} + {b - 1, b : b in (16, 32, 64, 96, 128, 160, 192), b < n}: the edges at the corners of
every strip, k-block, 64-column image, bitmap word and row block, self-loops included.  CSR rows are NOT sorted by column.

Hole copies (HOLE_SIZES, appended to `wide`).  Node n - 1 keeps exactly one out-edge and one in-edge, both with
HOLE_PARTNER, and one boundary node has no edge at all: 177 -> 96 and 255 -> 128; where the boundary node of the size is
n - 1 itself (17, 128, 160, 192) a node cannot both be isolated and hold an edge, and an isolated LAST node would shorten
the range by one, so there the isolated node is the next probe node below: 17 -> 15, 128 -> 96, 160 -> 128, 192 -> 160.

Inputs.  Q, K ~ N(0, 1) f^-1/4, V, dO ~ N(0, 1) as parity_cases.gt_inputs, then aimed at the probe grid:
  * Q and K of the probe nodes get the common component PROBE_LOGIT^1/2 u_head (their random parts made orthogonal to u
    and scaled by PROBE_NOISE), so a probe edge's logit is val (PROBE_LOGIT + N(0, 1) / 4): no probe edge holds a
    vanishing share of its row;
  * dK_j loses dS_ij val Q_i with the edge (i, j), and dS_ij = P_ij <dO_i, V_j - out_i> is a scalar that a random dO_i
    makes arbitrarily small for one of a hundred thousand probe edges.  dO_i of every probe row is therefore a N(0, 1) draw
    corrected (_best_draw) so that |<dO_i, z>| / |z| is AIM_DP standard deviations for every probe edge of the row
    (z = V_j - out_i), as parity_cases aims its sentinels; the row's norm stays within about twice a random row's.  GAT:
    the same with z = X_j - out_i, and GAT_ROW_DAMP of dO_i's component along the gradient of grad_attn_row_i is taken
    out, so that one probe edge's share of that scalar is large; the branch of the LeakyReLU an edge sits on is decided
    by its column (gat_inputs), so that no row has grad_attn_row = 0 exactly.
  * node n - 1 of a hole copy has one edge, P = 1 and dQ = dS val K = 0 exactly.  The statistics pair recomputes the logit in
    the backward (K Q^T where the forward had Q K^T), gets P = 1 + 1e-7 and with it dS = dP x 1e-7: rounding noise on an
    exact zero, in proportion to dP = <dO, V_partner> -- measured on the MI355X as 7.9e-7 absolute at |dP| = 7.5
    ((h, f) = (8, 16), edge values), 8.4 x the fp32 reference's worst row once divided by the measure's floor.  As
    parity_cases does for its rows of one and two edges, the inputs keep that noise out: dO of node n - 1 is made orthogonal
    to V of its partner (dP = 0); dV of the partner still receives P dO.
Only float64 numpy on the inputs decides this; the draws are seeded."""
import functools

import numpy as np

import parity_cases as pc
from conftest import csc_of

MARGIN, POWER, SLOPE = pc.MARGIN, pc.POWER, pc.SLOPE
NARROW_SIZES = (2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96, 97, 111, 112, 113, 127, 128)
WIDE_SIZES = (129, 130, 143, 144, 145, 159, 160, 161, 162, 175, 176, 177, 191, 192, 193, 207, 208, 209, 223, 224, 225, 239,
              240, 241, 254, 255)
WIDE_BETWEEN = ((5, 16), (13, 64), (20, 128))        # (after how many wide ranges, size): one-tile ranges between wide ones
HOLE_SIZES = (17, 128, 160, 177, 192, 255)
HOLE_ISOLATED = {17: 15, 128: 96, 160: 128, 177: 96, 192: 160, 255: 128}
HOLE_PARTNER = 5
BOUNDARIES = (16, 32, 64, 96, 128, 160, 192)
BATCHES = ("narrow", "wide")
# (h, f): one head at every dense width; heads bodies (walked backward); h f no multiple of 64 (per-head MULTI body);
# MULTI at F = 128
WIDTHS = ((1, 128), (1, 64), (1, 32), (1, 16), (1, 8), (2, 64), (4, 32), (8, 16), (3, 32), (2, 128))
TARGET_DEGREE = 38
P_SMALL = 0.6
PROBE_LOGIT = 2.0               # <Q_i, K_j> of a probe edge: PROBE_LOGIT + PROBE_NOISE^2 N(0, 1)
PROBE_NOISE = 0.5
GAT_PROBE_COL = 3.0             # attn_col of the probe nodes: GAT_PROBE_COL + U(-0.5, 0.5)
GAT_PROBE_ROW = -1.5            # attn_row of the probe nodes: GAT_PROBE_ROW + U(-0.25, 0.25)
GAT_ROW_DAMP = 0.7              # share of dO_i's component along the gradient of grad_attn_row_i that is taken out (more
#                                 makes the probe rows' own grad_attn_row small and the fp32 reference's error in them the bound)
AIM_DRAWS = 64
AIM_DP = 2.5                    # |<dO_i, z>| / |z| of a probe edge is brought up to this many standard deviations
GT_NAMES = ("out", "attn_edge", "row_max", "row_sum", "dQ", "dK", "dV")
GAT_NAMES = ("out", "inference", "edge_max", "edge_sum", "grad_feat", "grad_attn_row", "grad_attn_col")


def probe_nodes(n):
    """B(n), ascending."""
    b = {0, n - 1}
    for x in BOUNDARIES:
        if x < n:
            b.update((x - 1, x))
    return np.asarray(sorted(b), dtype=np.int64)


def edge_probability(n):
    return min(P_SMALL, TARGET_DEGREE / n)


def batch_layout(name):
    """-> list of (size, is_hole_copy) in batch order."""
    if name == "narrow":
        small, large = NARROW_SIZES[:12], NARROW_SIZES[12:][::-1]
        return [(n, False) for pair in zip(small, large) for n in pair]
    assert name == "wide"
    out, between = [], dict(WIDE_BETWEEN)
    for k, n in enumerate(WIDE_SIZES):
        if k in between:
            out.append((between[k], False))
        out.append((n, False))
    return out + [(n, True) for n in HOLE_SIZES]


def _member(rng, n, hole):
    """-> (src, dst) of one member graph in CSR order (rows ascending, the columns of a row shuffled)."""
    adj = rng.random((n, n)) < edge_probability(n)
    b = probe_nodes(n)
    adj[np.ix_(b, b)] = True
    if hole:
        last, iso = n - 1, HOLE_ISOLATED[n]
        for node in (last, iso):
            adj[node, :] = False
            adj[:, node] = False
        adj[last, HOLE_PARTNER] = adj[HOLE_PARTNER, last] = True
    src, dst = [], []
    for i in range(n):
        cols = rng.permutation(np.nonzero(adj[i])[0])
        src.append(np.full(len(cols), i, dtype=np.int64))
        dst.append(cols.astype(np.int64))
    return np.concatenate(src), np.concatenate(dst)


@functools.lru_cache(maxsize=None)
def graph(name):
    """-> dict: int32 CSR / CSC arrays of the batch, `ranges` (one dict per member: n0, n, hole, probes, and for a hole copy
    last / isolated / partner as global node ids), `members` ((src, dst, n) in local ids, for the public preprocessing),
    `probe` (global (row, column, CSR slot) of every probe edge, with the index of its range).  Nobody writes to it."""
    rng = np.random.default_rng({"narrow": 4101, "wide": 4102}[name])
    ranges, members, src, dst, n0 = [], [], [], [], 0
    for n, hole in batch_layout(name):
        s, d = _member(rng, n, hole)
        members.append((s, d, n))
        src.append(s + n0)
        dst.append(d + n0)
        r = dict(n0=n0, n=n, hole=hole, probes=probe_nodes(n) + n0)
        if hole:
            r.update(last=n0 + n - 1, isolated=n0 + HOLE_ISOLATED[n], partner=n0 + HOLE_PARTNER)
            r["probes"] = r["probes"][~np.isin(r["probes"], (r["last"], r["isolated"]))]
        ranges.append(r)
        n0 += n
    m, src, dst = n0, np.concatenate(src), np.concatenate(dst)
    assert (np.diff(src) >= 0).all()
    nnz = len(src)
    rows, col_ind = src.astype(np.int32), dst.astype(np.int32)
    row_ptr = np.zeros(m + 1, dtype=np.int64)
    np.add.at(row_ptr, src + 1, 1)
    row_ptr = np.cumsum(row_ptr).astype(np.int32)
    col_ptr, row_ind, val_idx = csc_of(row_ptr, col_ind, rows, m)
    probe = []
    for k, r in enumerate(ranges):
        lo, hi = row_ptr[r["n0"]], row_ptr[r["n0"] + r["n"]]
        key = src[lo:hi] * m + dst[lo:hi]
        order = np.argsort(key)
        want = (r["probes"][:, None] * m + r["probes"][None, :]).reshape(-1)
        at = np.searchsorted(key[order], want)
        assert (key[order][at] == want).all()
        slots = lo + order[at]
        probe.append(np.stack([want // m, want % m, slots, np.full(len(want), k)], axis=1))
    probe = np.concatenate(probe).astype(np.int64)
    return dict(name=name, m=m, nnz=nnz, row_ptr=row_ptr, col_ind=col_ind, rows=rows, col_ptr=col_ptr, row_ind=row_ind,
                val_idx=val_idx, ranges=ranges, members=members, probe=probe)


def padded_rows(g):
    """The rows of the ranges whose size is no multiple of 16: their last strip holds padding rows and columns."""
    return np.concatenate([np.arange(r["n0"], r["n0"] + r["n"]) for r in g["ranges"] if r["n"] % 16])


def probe_node_ids(g):
    return np.concatenate([r["probes"] for r in g["ranges"]])


# ---- float64 evaluation of single rows (the aim of the inputs; the moves of the power condition) -----------------------
def _row(g, i):
    lo, hi = int(g["row_ptr"][i]), int(g["row_ptr"][i + 1])
    return lo, hi, g["col_ind"][lo:hi].astype(np.int64)


def gt_row(Qi, Kc, Vc, v, dOi):
    """One row of the GT pair in float64: Qi, dOi [h, f]; Kc, Vc [deg, h, f]; v [deg] -> dict with out, dQ [h, f]; attn
    [h, deg]; row_max, row_sum [h]; dK, dV [deg, h, f]: what this row adds to the rows of its columns."""
    s = np.einsum("dhf,hf->hd", Kc, Qi) * v
    mx = s.max(axis=1)
    e = np.exp(s - mx[:, None])
    sm = e.sum(axis=1)
    P = e / sm[:, None]
    out = np.einsum("hd,dhf->hf", P, Vc)
    dP = np.einsum("dhf,hf->hd", Vc, dOi)
    dS = P * (dP - (P * dP).sum(axis=1, keepdims=True))
    return dict(out=out, attn=P, row_max=mx, row_sum=sm, dQ=np.einsum("hd,dhf->hf", dS * v, Kc),
                dK=np.einsum("hd,hf->dhf", dS * v, Qi), dV=np.einsum("hd,hf->dhf", P, dOi))


def gat_row(ari, acc_, Xc, dOi):
    """One row of the GAT pair (no dropout) in float64: ari, [h]; acc_ [deg, h]; Xc [deg, h, f]; dOi [h, f] -> out [h, f],
    edge_max, edge_sum, grad_attn_row [h]; grad_feat [deg, h, f] and grad_attn_col [deg, h]: this row's terms."""
    pre = (ari[None, :] + acc_).T                                       # [h, deg]
    SLOPE = float(np.float32(pc.SLOPE))                                 # (the oracle takes the slope as a float)
    s = np.where(pre > 0, pre, SLOPE * pre)
    mx = s.max(axis=1)
    e = np.exp(s - mx[:, None])
    sm = e.sum(axis=1)
    P = e / sm[:, None]
    out = np.einsum("hd,dhf->hf", P, Xc)
    dP = np.einsum("dhf,hf->hd", Xc, dOi)
    G = P * (dP - (P * dP).sum(axis=1, keepdims=True)) * np.where(pre > 0, 1.0, SLOPE)
    return dict(out=out, edge_max=mx, edge_sum=sm, grad_attn_row=G.sum(axis=1), grad_feat=np.einsum("hd,hf->dhf", P, dOi),
                grad_attn_col=G.T, attn=P, slope=np.where(pre > 0, 1.0, SLOPE))


def _unit_rows(a):
    return a / np.maximum(np.linalg.norm(a, axis=-1, keepdims=True), 1e-300)


def _best_draw(rng, F, damp=None, also=None):
    """F [h, k, f]: vectors z.  -> dO [h, f].  Every one of AIM_DRAWS N(0, 1) rows d gets the least-norm (least-squares,
    where k > f) correction that brings each |<d, z>| / |z| up to AIM_DP with the sign it had -- and, with damp [h, f], takes
    GAT_ROW_DAMP of d's component along damp out; per head the corrected draw wins whose least |<d, z>| / |z| (over F and
    `also` [h, k2, f]) relative to |d| / f^1/2 is largest."""
    h, _, f = F.shape
    F = _unit_rows(F)
    D = rng.standard_normal((h, AIM_DRAWS, f))
    x = np.einsum("hcf,hkf->hck", D, F)
    miss = np.where(x < 0, -1.0, 1.0) * np.maximum(np.abs(x), AIM_DP) - x
    A = F
    if damp is not None:
        r = _unit_rows(damp)[:, None, :]
        A = np.concatenate([F, r], axis=1)
        miss = np.concatenate([miss, -GAT_ROW_DAMP * np.einsum("hcf,hkf->hck", D, r)], axis=2)
    D = D + np.einsum("hck,hfk->hcf", miss, np.linalg.pinv(A, rcond=1e-6))     # (two-node ranges: collinear z)
    S = F if also is None else np.concatenate([F, _unit_rows(also)], axis=1)
    score = np.abs(np.einsum("hcf,hkf->hck", D, S)).min(axis=2) / (np.linalg.norm(D, axis=-1) / f ** 0.5)
    return D[np.arange(h), score.argmax(axis=1)]


def _f32(*arrays):
    return tuple(np.ascontiguousarray(a, dtype=np.float32) for a in arrays)


@functools.lru_cache(maxsize=2)
def gt_inputs(name, h, f, unit_val):
    """-> dict(val, Q, K, V, dO) float32 (module docstring: the aim)."""
    g = graph(name)
    m = g["m"]
    rng = np.random.default_rng(1000 * f + 10 * h + int(unit_val) + (500 if name == "wide" else 0))
    val = np.ones(g["nnz"]) if unit_val else rng.uniform(0.5, 1.5, g["nnz"])
    val = val.astype(np.float32).astype(np.float64)
    Q, K = (rng.standard_normal((m, h, f)) * f ** -0.25 for _ in range(2))
    V, dO = (rng.standard_normal((m, h, f)) for _ in range(2))
    u = rng.standard_normal((h, f))
    u /= np.linalg.norm(u, axis=-1, keepdims=True)
    b = probe_node_ids(g)
    for A in (Q, K):
        A[b] = PROBE_NOISE * (A[b] - (A[b] * u).sum(axis=-1, keepdims=True) * u) + PROBE_LOGIT ** 0.5 * u
    Q, K, V = (a.astype(np.float32).astype(np.float64) for a in (Q, K, V))
    for r in g["ranges"]:
        for i in r["probes"]:
            lo, hi, cols = _row(g, i)
            row = gt_row(Q[i], K[cols], V[cols], val[lo:hi], dO[i])
            z = V[cols[np.isin(cols, r["probes"])]] - row["out"][None]          # [k, h, f]
            dO[i] = _best_draw(rng, z.transpose(1, 0, 2))
        if r["hole"]:     # the one-edge row: dO across V of its partner (module docstring)
            last, v = r["last"], V[r["partner"]]
            dO[last] -= (dO[last] * v).sum(axis=-1, keepdims=True) / (v * v).sum(axis=-1, keepdims=True) * v
    val, Q, K, V, dO = _f32(val, Q, K, V, dO)
    return dict(val=val, Q=Q, K=K, V=V, dO=dO)


@functools.lru_cache(maxsize=2)
def gat_inputs(name, h, f):
    """-> dict(attn_row, attn_col [m, h], X, dO) float32 as parity_cases.gat_inputs; the probe edges sit on the
    positive branch of the LeakyReLU at the top of their rows, most other edges of a probe row on the negative one (with one
    branch only, grad_attn_row is an exact 0); dO of the probe rows is aimed (module docstring)."""
    g = graph(name)
    m = g["m"]
    rng = np.random.default_rng(1000 * f + 10 * h + 7 + (500 if name == "wide" else 0))
    # a row whose edges all sit on one branch of the LeakyReLU has grad_attn_row = slope x sum dS = 0 exactly, which every fp32
    # evaluation fills with its own rounding noise -- measured against the floor that is the worst row of the whole batch and
    # sets the bound (1.8e-3 with N(0, 1) terms: 30 x what the other rows reach).  So |attn_row| <= 0.5 < 0.6 <= |attn_col|:
    # the branch of an edge is decided by its column, and the columns alternate.
    ar = rng.uniform(-0.5, 0.5, (m, h))
    ac = np.where(np.arange(m) % 2 == 0, 1.0, -1.0)[:, None] * (0.6 + np.abs(rng.standard_normal((m, h))))
    X, dO = (rng.standard_normal((m, h, f)) for _ in range(2))
    for r in g["ranges"]:
        b = r["probes"]
        if len(b) == r["n"]:      # (two nodes, four probe edges: a row's two edges on different branches of the LeakyReLU)
            ac[b] = np.where(np.arange(len(b)) % 2 == 0, 2.0, -2.0)[:, None] + rng.uniform(-0.25, 0.25, (len(b), h))
            ar[b] = rng.uniform(-0.5, 0.5, (len(b), h))
        else:
            ac[b] = GAT_PROBE_COL + rng.uniform(-0.5, 0.5, (len(b), h))
            ar[b] = GAT_PROBE_ROW + rng.uniform(-0.25, 0.25, (len(b), h))
    ar, ac, X = (a.astype(np.float32).astype(np.float64) for a in (ar, ac, X))
    for r in g["ranges"]:
        for i in r["probes"]:
            lo, hi, cols = _row(g, i)
            row = gat_row(ar[i], ac[cols], X[cols], dO[i])
            P, sl, out = row["attn"], row["slope"], row["out"]                  # [h, deg], [h, deg], [h, f]
            at = np.nonzero(np.isin(cols, r["probes"]))[0]
            z = X[cols[at]] - out[None]                                         # dS of the probe edges: [k, h, f]
            # grad_attn_row = <dO_i, S1 - S0 out>, S1 = sum P slope X, S0 = sum P slope; without edge j the same over the
            # renormalised rest: w_j = the difference of the two vectors
            S1, S0 = np.einsum("hd,dhf->hf", P * sl, X[cols]), (P * sl).sum(axis=1)
            p, gp = P[:, at].T[..., None], (P * sl)[:, at].T[..., None]        # [k, h, 1]
            out_j = (out[None] - p * X[cols[at]]) / (1 - p)
            w = (S1 - S0[:, None] * out)[None] - ((S1[None] - gp * X[cols[at]]) - (S0[None, :, None] - gp) * out_j) / (1 - p)
            dO[i] = _best_draw(rng, z.transpose(1, 0, 2), damp=S1 - S0[:, None] * out, also=w.transpose(1, 0, 2))
    ar, ac, X, dO = _f32(ar, ac, X, dO)
    return dict(attn_row=ar, attn_col=ac, X=X, dO=dO)


# ---- references and bounds --------------------------------------------------------------------------------------------
def bounds_of(g, ref32, ref64):
    return {k: MARGIN * pc.error_of(g, k, ref32[k], ref64[k]) for k in ref64}


@functools.lru_cache(maxsize=2)
def gt_references(name, h, f, unit_val):
    """-> (inputs, ref64, ref32, bounds): bounds[output] = MARGIN x the fp32 reference's worst row error."""
    g, x = graph(name), gt_inputs(name, h, f, unit_val)
    ref64 = pc.gt_reference(g["row_ptr"], g["col_ind"], x, "f64")
    ref32 = pc.gt_reference(g["row_ptr"], g["col_ind"], x, "f32")
    return x, ref64, ref32, bounds_of(g, ref32, ref64)


@functools.lru_cache(maxsize=2)
def gat_references(name, h, f):
    g, x = graph(name), gat_inputs(name, h, f)
    ref64 = pc.gat_reference(g["row_ptr"], g["col_ind"], x, "f64")
    ref32 = pc.gat_reference(g["row_ptr"], g["col_ind"], x, "f32")
    return x, ref64, ref32, bounds_of(g, ref32, ref64)


# ---- the density threshold ---------------------------------------------------------------------------------------------
THRESHOLD_SIZES = (64, 160, 255)
THRESHOLD_COMPANION = 100            # nodes of the well-connected ranges on either side (p = 0.5: nnz >= 8 m for the batch)


def dense_rule(n, edges):
    """The plan's rule for a range of n nodes without duplicate edges (csrc/plan.hip: fit_entry)."""
    return n <= 255 and 32 * edges >= n * n


@functools.lru_cache(maxsize=None)
def threshold_graph(n, short):
    """A batch companion | test range | companion; the test range holds exactly ceil(n^2 / 32) - short edges, among them
    (0, n - 1) and (n - 1, 0), which keep it one range.  -> dict like graph(), `test` = (n0, n, edges)."""
    rng = np.random.default_rng(900 + n)              # (the same draw for short = 0 and 1: the last edge goes)
    edges = -(-n * n // 32)
    pick = rng.permutation(n * n)
    pick = pick[~np.isin(pick, (n - 1, (n - 1) * n))][:edges - 2]
    pairs = np.concatenate([[n - 1, (n - 1) * n], pick])[:edges - short]
    test = np.zeros((n, n), dtype=bool)
    test[pairs // n, pairs % n] = True
    assert test.sum() == edges - short
    members, src, dst, n0, at = [], [], [], 0, None
    for k, size in enumerate((THRESHOLD_COMPANION, n, THRESHOLD_COMPANION)):
        adj = test if k == 1 else rng.random((size, size)) < 0.5
        if k != 1:
            adj[0, size - 1] = adj[size - 1, 0] = True
        else:
            at = n0
        s, d = np.nonzero(adj)
        members.append((s.astype(np.int64), d.astype(np.int64), size))
        src.append(s + n0)
        dst.append(d + n0)
        n0 += size
    m, src, dst = n0, np.concatenate(src).astype(np.int64), np.concatenate(dst).astype(np.int64)
    rows, col_ind = src.astype(np.int32), dst.astype(np.int32)
    row_ptr = np.zeros(m + 1, dtype=np.int64)
    np.add.at(row_ptr, src + 1, 1)
    row_ptr = np.cumsum(row_ptr).astype(np.int32)
    col_ptr, row_ind, val_idx = csc_of(row_ptr, col_ind, rows, m)
    return dict(m=m, nnz=len(src), row_ptr=row_ptr, col_ind=col_ind, rows=rows, col_ptr=col_ptr, row_ind=row_ind,
                val_idx=val_idx, members=members, test=(at, n, edges - short))


@functools.lru_cache(maxsize=2)
def threshold_references(n, short, h, f):
    """Plain random inputs (parity_cases' scales) on threshold_graph -> (inputs, ref64, ref32, bounds)."""
    g = threshold_graph(n, short)
    rng = np.random.default_rng(31 * n + f)
    Q, K = (rng.standard_normal((g["m"], h, f)) * f ** -0.25 for _ in range(2))
    V, dO = (rng.standard_normal((g["m"], h, f)) for _ in range(2))
    x = dict(zip(("val", "Q", "K", "V", "dO"), _f32(np.ones(g["nnz"]), Q, K, V, dO)))
    ref64 = pc.gt_reference(g["row_ptr"], g["col_ind"], x, "f64")
    ref32 = pc.gt_reference(g["row_ptr"], g["col_ind"], x, "f32")
    return x, ref64, ref32, bounds_of(g, ref32, ref64)
