"""Cases and measures for fp32-level parity tests (tests/test_parity_cases_host.py, tests/test_gpu_edge_exact.py).

The bound.  For a result with feature rows [n, h, k] the error of row (i, head) is
    ||got - ref64||_inf / max(||ref64||_inf, floor),      floor = 1e-2 x median of the non-zero row norms of ref64,
a statistic [n, h] is k = 1, attn_edge [h, nnz] is grouped by CSR row.  The bound of one output of one case is
MARGIN x the worst such error of the plain-fp32 reference (oracle acc="f32": sequential sums, expf; GATv2: the torch
formulation in float32) against the float64 one on the same inputs.  Nothing is hard-coded and the kernel under test is
not involved.

The power condition.  The inputs are built so that the single edge at either end of a long row carries weight (a
sentinel: logit +3, a value row aimed along the row's dO so that its dP is three standard deviations, a column of its
own; as built from degree SENTINEL_DEGREE on, see _sentinels), and
tests/test_parity_cases_host.py proves on the CPU that dropping that one edge moves every checked output of the row by
at least POWER x bound.  A kernel that loses a tile tail, a remainder-loop element or the edge at an LDS cap therefore
cannot pass.

Node layout of every graph: test nodes 0..R-1, the R sentinels of the first edges, a pool of POOL ordinary nodes, the R
sentinels of the last edges, then (lane-group form only) isolated nodes.  As built the test nodes are the rows;
transposed they are the columns, whose CSC segments then start with the first sentinel's entry and end with the last
one's (CSC order is by row id).  There every sentinel row gets a second edge, a self-loop with the same logit +3, and a
dO row that tells its two value rows apart, so that its softmax is balanced and the dS of its edge into the test column
is large, not zero.
"""
import functools
import os
import re

import numpy as np

from conftest import ROOT, csc_of

MARGIN = 8.0            # bound = MARGIN x (fp32 reference against the float64 reference); DESIGN.md 5.1 says why not 4
POWER = 4.0             # a lost boundary edge moves every checked output by >= POWER x bound
SLOPE = 0.2
POOL = 64
FILLER_DEGREE = 5
SENTINEL_LOGIT = 3.0
SENTINEL_DP = 3.0
SENTINEL_DEGREE = 15    # as built, test rows from this degree on get sentinel features (see _sentinels)
WIDTHS = ((32, 1), (128, 1), (7, 2), (260, 1))        # (f, h): float4 EPW 8 / EPW 2 / scalar path / f > 256
FIXED_DEGREES = (1, 2, 3, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257)
CAP_NAMES = ("kGroupMaxDegree", "kRowCap", "kCsrRowCap", "kHyperCap")
CSRC = os.path.join(ROOT, "df-gnn_amd", "csrc")


@functools.lru_cache(maxsize=None)
def caps():
    """The four degree caps at which a kernel changes its code path, read from the sources they are defined in."""
    found = {}
    for fn in sorted(os.listdir(CSRC)):
        if fn.endswith((".hip", ".hpp")):
            text = open(os.path.join(CSRC, fn)).read()
            for name in CAP_NAMES:
                for hit in re.finditer(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text):
                    assert name not in found, f"{name} is defined twice"
                    found[name] = int(hit.group(1))
    assert sorted(found) == sorted(CAP_NAMES), found
    return found


def degree_list():
    """The fixed boundary degrees and cap - 1, cap, cap + 1 of each cap."""
    deg = set(FIXED_DEGREES)
    for c in caps().values():
        deg.update((c - 1, c, c + 1))
    return sorted(deg)


def block_rows():
    """(first row, degrees) of the two aligned 16-row blocks: one sums to kHyperCap (the workgroup's LDS path), the next
    to kHyperCap + 1 (the online fallback)."""
    cap = caps()["kHyperCap"]
    start = -(-len(degree_list()) // 16) * 16
    out = []
    for k, total in enumerate((cap, cap + 1)):
        base, rem = divmod(total, 16)
        out.append((start + 16 * k, [base + 1] * rem + [base] * (16 - rem)))
    return out


def node_degrees():
    """Degree of every test node: the degree list, filler rows up to the next multiple of 16, the two blocks."""
    deg = list(degree_list())
    blocks = block_rows()
    deg += [FILLER_DEGREE] * (blocks[0][0] - len(deg))
    for _, d in blocks:
        deg += d
    return np.asarray(deg, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def graph(transposed=False, low=False):
    """-> dict of int32 CSR / CSC arrays and the bookkeeping of the test nodes; shared by the tests, nobody writes to it.
    low: padded with isolated nodes until nnz < 8 m (the kernels' lane-group form; long rows taken cooperatively)."""
    rng = np.random.default_rng(2024)
    deg = node_degrees()
    R = len(deg)
    first0, pool0, last0, end0 = R, 2 * R, 2 * R + POOL, 3 * R + POOL
    src, dst = [], []
    for i, d in enumerate(deg):
        cols = pool0 + rng.integers(0, POOL, d)
        cols[0] = first0 + i                      # (degree 1: the one edge is a sentinel, degree 2: both are)
        if d >= 2:
            cols[-1] = last0 + i
        src.append(np.full(d, i, dtype=np.int64))
        dst.append(cols.astype(np.int64))
    src, dst = np.concatenate(src), np.concatenate(dst)
    hf, hl = np.arange(R), np.nonzero(deg >= 2)[0]
    sent = np.concatenate([first0 + hf, last0 + hl])
    if transposed:
        src, dst = np.concatenate([dst, sent]), np.concatenate([src, sent])      # transpose + self-loops
    nnz = len(src)
    m = end0
    if low:
        m = max(m, nnz // 8 + 1)
    order = np.argsort(src, kind="stable")
    rows, col_ind = src[order].astype(np.int32), dst[order].astype(np.int32)
    row_ptr = np.zeros(m + 1, dtype=np.int64)
    np.add.at(row_ptr, src + 1, 1)
    row_ptr = np.cumsum(row_ptr).astype(np.int32)
    col_ptr, row_ind, val_idx = csc_of(row_ptr, col_ind, rows, m)
    test = np.arange(R)
    if transposed:
        # CSR slot of the first / last CSC entry of every test column
        first_slot, last_slot = val_idx[col_ptr[test]], val_idx[col_ptr[test + 1] - 1]
        mutate = test                                                      # every test column
        sent_slot = np.concatenate([first_slot[hf], last_slot[hl]])
        sent_node = rows[sent_slot].astype(np.int64)
        assert (sent_node == sent).all()
        assert (np.diff(row_ptr)[sent_node] == 2).all() and (sent_slot == row_ptr[sent_node]).all()
        assert (col_ind[sent_slot + 1] == sent_node).all()                 # the self-loop follows in CSR slot + 1
        assert (np.bincount(col_ind, minlength=m)[:R] == deg).all()
    else:
        first_slot, last_slot = row_ptr[test], row_ptr[test + 1] - 1
        mutate = np.nonzero(deg >= 3)[0]                                   # test rows of degree >= 3
        sent_slot = np.concatenate([first_slot[hf], last_slot[hl]])
        sent_node = col_ind[sent_slot].astype(np.int64)
        assert (sent_node == sent).all()
        assert (np.bincount(col_ind, minlength=m)[sent_node] == 1).all()
        assert (np.diff(row_ptr)[:R] == deg).all()
    return dict(m=m, nnz=nnz, R=R, transposed=transposed, low=low, row_ptr=row_ptr, col_ind=col_ind, rows=rows,
                col_ptr=col_ptr, row_ind=row_ind, val_idx=val_idx, deg=deg, test=test, mutate=mutate,
                first_slot=np.asarray(first_slot)[mutate], last_slot=np.asarray(last_slot)[mutate],
                sent_slot=sent_slot, sent_node=sent_node, sent_anchor=np.concatenate([hf, hl]),
                pool=np.arange(pool0, pool0 + POOL))


def drop_slots(g, slots):
    """The CSR arrays of g without the edges in CSR slots `slots` -> (row_ptr, col_ind, keep mask over the old slots)."""
    keep = np.ones(g["nnz"], dtype=bool)
    keep[slots] = False
    rows = g["rows"][keep]
    row_ptr = np.zeros(g["m"] + 1, dtype=np.int64)
    np.add.at(row_ptr, rows.astype(np.int64) + 1, 1)
    return np.cumsum(row_ptr).astype(np.int32), g["col_ind"][keep], keep


def mutations(g):
    """name -> CSR slots to drop: the last / first CSR edge of every test row of degree >= 3, or (transposed) the last /
    first CSC entry of every test column."""
    side = "csc" if g["transposed"] else "csr"
    return {f"last_{side}": g["last_slot"], f"first_{side}": g["first_slot"]}


# ---- the error measure ------------------------------------------------------------------------------------------------
def _row_norms(a, row_ptr=None):
    """||.||_inf per (node, head): a is [n, h, k], [n, h], or -- with row_ptr -- attn_edge [h, nnz] grouped by CSR row."""
    a = np.abs(np.asarray(a, dtype=np.float64))
    if row_ptr is None:
        return a.reshape(a.shape[0], a.shape[1], -1).max(axis=2) if a.size else np.zeros(a.shape[:2])
    n = len(row_ptr) - 1
    out = np.zeros((n, a.shape[0]))
    nonempty = np.diff(row_ptr) > 0
    if nonempty.any():
        out[nonempty] = np.maximum.reduceat(a, row_ptr[:-1][nonempty].astype(np.int64), axis=1).T
    return out


def floor_of(ref64, row_ptr=None):
    norms = _row_norms(ref64, row_ptr)
    nz = norms[norms > 0]
    return 1e-2 * float(np.median(nz)) if nz.size else 1.0


def row_errors(got, ref64, row_ptr=None, floor=None):
    """-> [n, h]: the error of every (node, head) of `got` in the measure of this module."""
    got, ref64 = np.asarray(got, dtype=np.float64), np.asarray(ref64, dtype=np.float64)
    assert got.shape == ref64.shape, (got.shape, ref64.shape)
    if floor is None:
        floor = floor_of(ref64, row_ptr)
    return _row_norms(got - ref64, row_ptr) / np.maximum(_row_norms(ref64, row_ptr), floor)


def worst(got, ref64, row_ptr=None, valid=None, where=False):
    """The worst row error; where=True: -> (error, (node, head) of that row)."""
    e = row_errors(got, ref64, row_ptr)
    if valid is not None:
        e = np.where(np.asarray(valid)[:, None], e, 0.0)
    at = np.unravel_index(int(e.argmax()), e.shape) if e.size else (0, 0)
    err = float(e[at]) if e.size else 0.0
    return (err, (int(at[0]), int(at[1]))) if where else err


# ---- inputs -----------------------------------------------------------------------------------------------------------
def _f32(*arrays):
    return tuple(np.ascontiguousarray(a, dtype=np.float32) for a in arrays)


def _sentinels(g, degree=SENTINEL_DEGREE):
    """(node, test node, CSR slot) of the sentinels that get their features.  As built those of test rows of at least
    `degree` edges: a row of a few edges needs none to notice a lost edge, and there the two sentinels hold nearly all the
    mass with the same val K (GATv2: the same X_col).  In a row of two edges dQ (dX_row) is then an exact 0 that every fp32
    evaluation order fills with different rounding noise, and in a row of three or five, delta = <dO_i, out_i> (what
    the row-statistics backward computes) and delta = sum P dP (the oracle) differ by rounding that the aligned sentinel
    rows carry straight into dQ and dK: 6 x the fp32 reference's error at degree 3, which says nothing about a lost edge.
    Transposed all of them, the columns of in-degree 1 and 2 included."""
    keep = np.ones(len(g["sent_node"]), dtype=bool) if g["transposed"] else g["deg"][g["sent_anchor"]] >= degree
    return g["sent_node"][keep], g["sent_anchor"][keep], g["sent_slot"][keep]


def _aim_sentinel_rows(W, D, g):
    """The value row W_s of the sentinels of _sentinels(g) keeps its random part across D_i, the dO row of its test row,
    and gets the component SENTINEL_DP along it: dP_s = <D_i, W_s> = 3 |D_i|, three standard deviations of an ordinary
    edge's dP, so the sentinel's dS is large by construction and not by the luck of a random dot product."""
    s, a, _ = _sentinels(g)
    d = D[a] / np.linalg.norm(D[a], axis=-1, keepdims=True)
    W[s] += (SENTINEL_DP - (W[s] * d).sum(axis=-1, keepdims=True)) * d


@functools.lru_cache(maxsize=2)
def gt_inputs(transposed, low, f, h, unit_val):
    """-> dict(val, Q, K, V, dO) float32.  The anchor side (Q of the test rows; transposed: K of the test columns) has
    norm f^(1/4) per head; the sentinel's other operand is 3 anchor / (val_e |anchor|^2), so its logit is +3; the row the
    sentinel contributes is aimed (as built: V_s, _aim_sentinel_rows; transposed: dO_s = 2 V of the test column)."""
    g = graph(transposed, low)
    m = g["m"]
    rng = np.random.default_rng(100 * f + 10 * h + int(unit_val) + (1000 if transposed else 0))
    val = np.ones(g["nnz"]) if unit_val else rng.uniform(0.5, 1.5, g["nnz"])
    val = val.astype(np.float32).astype(np.float64)
    Q, K = (rng.standard_normal((m, h, f)) * f ** -0.25 for _ in range(2))
    V, dO = (rng.standard_normal((m, h, f)) for _ in range(2))
    A, B = (K, Q) if transposed else (Q, K)
    t = g["test"]
    A[t] *= f ** 0.25 / np.linalg.norm(A[t], axis=-1, keepdims=True)
    s, a, e = _sentinels(g)
    B[s] = SENTINEL_LOGIT * A[a] / (val[e][:, None, None] * f ** 0.5)
    if transposed:        # the self-loop's logit is +3 as well; dO_s along V of the test column: <dO_s, V_i - V_s> is large
        # ... on top of a random part across Q_s: with val K_s parallel to val K_i, dQ_s = dS (val K_i - val K_s) would be
        # an exact 0 that every fp32 evaluation order fills with different rounding noise
        q2 = (Q[s] ** 2).sum(axis=-1, keepdims=True)
        K[s] += (SENTINEL_LOGIT / val[e + 1][:, None, None] - (K[s] * Q[s]).sum(axis=-1, keepdims=True)) * Q[s] / q2
        dO[s] = 2 * V[a]
    else:
        _aim_sentinel_rows(V, dO, g)
    val, Q, K, V, dO = _f32(val, Q, K, V, dO)
    return dict(val=val, Q=Q, K=K, V=V, dO=dO)


@functools.lru_cache(maxsize=2)
def gat_inputs(transposed, low, f, h):
    """-> dict(attn_row, attn_col [m, h], X, dO) float32; the sentinel's LeakyReLU logit is +3, its X row is aimed
    (_aim_sentinel_rows; transposed: dO_s = 2 X of the test column)."""
    g = graph(transposed, low)
    m = g["m"]
    rng = np.random.default_rng(100 * f + 10 * h + (1000 if transposed else 0) + 7)
    ar, ac = (rng.standard_normal((m, h)) for _ in range(2))
    X, dO = (rng.standard_normal((m, h, f)) for _ in range(2))
    s, a, _ = _sentinels(g)
    if transposed:        # (self-loop: the same logit; dO_s along X of the test column)
        ar[s] = SENTINEL_LOGIT - ac[a]
        ac[s] = ac[a]
        dO[s] = 2 * X[a]
    else:
        # attn_row of the test rows around -3: every pool edge is on LeakyReLU's negative branch, the sentinels on the
        # positive one at the row's top (with one branch only, grad_attn_row is an exact 0: sum dS = 0)
        t = g["test"]
        ar[t] = -3 + rng.uniform(-0.5, 0.5, (len(t), h))
        s, a, _ = _sentinels(g, 3)          # (the rank-one logits have no aligned K: every mutated row keeps both branches)
        ac[s] = SENTINEL_LOGIT - ar[a]
        _aim_sentinel_rows(X, dO, g)
    ar, ac, X, dO = _f32(ar, ac, X, dO)
    return dict(attn_row=ar, attn_col=ac, X=X, dO=dO)


@functools.lru_cache(maxsize=2)
def gatv2_inputs(transposed, low, f, h):
    """-> dict(attn [h, f], X_row, X_col, dO) float32.  The sentinel's operand is -anchor + t sign(attn), which makes
    its logit t (sum of attn > 0 + SLOPE x sum of |attn < 0|) = +3."""
    g = graph(transposed, low)
    m = g["m"]
    rng = np.random.default_rng(100 * f + 10 * h + (1000 if transposed else 0) + 13)
    attn = rng.standard_normal((h, f)) * f ** -0.5
    xr, xc, dO = (rng.standard_normal((m, h, f)) for _ in range(3))
    t = SENTINEL_LOGIT / (np.where(attn > 0, attn, -SLOPE * attn)).sum(axis=1, keepdims=True)      # [h, 1]
    s, a, _ = _sentinels(g)
    if transposed:        # self-loop: logit +3 from the first half of the features alone, so X_col[s] != X_col[anchor];
        half = np.arange(f) < (f + 1) // 2                             # dO_s along the difference of the two value rows
        w = np.where(attn > 0, attn, -SLOPE * attn)
        z, z2 = t * np.sign(attn), SENTINEL_LOGIT / (w * half).sum(axis=1, keepdims=True) * np.sign(attn) * half
        xr[s] = -xc[a] + z
        xc[s] = -xr[s] + z2
        d = xc[a] - xc[s]
        dO[s] = 2 * f ** 0.5 * d / np.linalg.norm(d, axis=-1, keepdims=True)
    else:
        xc[s] = -xr[a] + t * np.sign(attn)
    attn, xr, xc, dO = _f32(attn, xr, xc, dO)
    return dict(attn=attn, X_row=xr, X_col=xc, dO=dO)


# ---- references -------------------------------------------------------------------------------------------------------
def gt_row_stats(row_ptr, col_ind, val, Q, K, dtype):
    """Logit maximum and sum of exponentials per (row, head) in `dtype`: sequential sums; rows without edges: 0, 0."""
    m, h, _ = Q.shape
    Q, K, val = Q.astype(dtype), K.astype(dtype), val.astype(dtype)
    mx, sm = np.zeros((m, h), dtype=dtype), np.zeros((m, h), dtype=dtype)
    for i in np.nonzero(np.diff(row_ptr))[0]:
        lo, hi = row_ptr[i], row_ptr[i + 1]
        s = np.cumsum(K[col_ind[lo:hi]] * Q[i], axis=-1, dtype=dtype)[..., -1] * val[lo:hi, None]
        mx[i] = s.max(axis=0)
        sm[i] = np.cumsum(np.exp(s - mx[i]), axis=0, dtype=dtype)[-1]
    return mx, sm


def gt_reference(row_ptr, col_ind, x, acc):
    """Every GT output on inputs x (gt_inputs) from the oracle in precision `acc` ("f64" / "f32")."""
    import oracle
    args = (row_ptr, col_ind, x["val"], x["Q"], x["K"], x["V"])
    out, attn = oracle.gt_forward(*args, want_attn=True, acc=acc)
    dQ, dK, dV = oracle.gt_backward(*args, x["dO"], acc=acc)
    mx, sm = gt_row_stats(row_ptr, col_ind, x["val"], x["Q"], x["K"], np.float64 if acc == "f64" else np.float32)
    return dict(out=out, attn_edge=attn, row_max=mx, row_sum=sm, dQ=dQ, dK=dK, dV=dV)


def gat_reference(row_ptr, col_ind, x, acc, mask=None, attn_drop=0.0):
    import oracle
    args = (row_ptr, col_ind, x["attn_row"], x["attn_col"], SLOPE, x["X"])
    out, emax, esum = oracle.gat_train_forward(*args, mask, attn_drop, acc=acc)
    gf, gr, gc = oracle.gat_backward(*args, x["dO"], mask, attn_drop, acc=acc)
    res = dict(out=out, edge_max=emax, edge_sum=esum, grad_feat=gf, grad_attn_row=gr, grad_attn_col=gc)
    if mask is None:
        res["inference"] = oracle.gat_forward(*args, acc=acc)
    return res


def gatv2_reference(row_ptr, col_ind, x, acc):
    """The torch formulation of tests/test_gpu_gatv2.py in float64 / float32 on the CPU."""
    import torch
    from test_gpu_gatv2 import _ref_conv
    dt = torch.float64 if acc == "f64" else torch.float32
    m = len(row_ptr) - 1
    rows = torch.from_numpy(np.repeat(np.arange(m), np.diff(row_ptr)).astype(np.int64))
    cols = torch.from_numpy(np.asarray(col_ind).astype(np.int64))
    a, xr, xc = (torch.from_numpy(x[k]).to(dt).requires_grad_(True) for k in ("attn", "X_row", "X_col"))
    out, mx, den = _ref_conv(rows, cols, m, a, xr, xc)
    gxr, gxc, ga = torch.autograd.grad(out, (xr, xc, a), torch.from_numpy(x["dO"]).to(dt))
    n = lambda t: t.detach().numpy()  # noqa: E731
    mx = n(mx).copy()
    mx[np.diff(row_ptr) == 0] = 0
    return dict(out=n(out), row_max=mx, row_sum=n(den), dX_row=n(gxr), dX_col=n(gxc), dattn=n(ga)[None])


# which outputs live on the rows (moved by a dropped CSR edge of a test row), which on the columns (moved by a dropped CSC
# entry of a test column), and dattn, one vector per head summed over every edge
ROW_SIDE = dict(gt=("out", "attn_edge", "row_max", "row_sum", "dQ"), gat=("out", "inference", "edge_max", "edge_sum",
                                                                           "grad_attn_row"),
                gatv2=("out", "row_max", "row_sum", "dX_row", "dattn"))
COL_SIDE = dict(gt=("dK", "dV"), gat=("grad_feat", "grad_attn_col"), gatv2=("dX_col", "dattn"))
STATS = ("row_max", "row_sum", "edge_max", "edge_sum")      # defined on rows with edges only (sentinels elsewhere)

_INPUTS = dict(gt=gt_inputs, gat=gat_inputs, gatv2=gatv2_inputs)
_REFERENCE = dict(gt=gt_reference, gat=gat_reference, gatv2=gatv2_reference)


def case_ids(op):
    """Every case of `op` as the argument tuple of its *_inputs function."""
    out = []
    for f, h in WIDTHS:
        for transposed in (False, True):
            for low in (False, True):
                out += [(transposed, low, f, h, u) for u in (True, False)] if op == "gt" else [(transposed, low, f, h)]
    return out


@functools.lru_cache(maxsize=2)
def references(op, *case):
    """-> (inputs, ref64, ref32, bounds): bounds[name] = MARGIN x the fp32 reference's worst error in output `name`."""
    g = graph(case[0], case[1])
    x = _INPUTS[op](*case)
    ref64 = _REFERENCE[op](g["row_ptr"], g["col_ind"], x, "f64")
    ref32 = _REFERENCE[op](g["row_ptr"], g["col_ind"], x, "f32")
    bounds = {k: MARGIN * error_of(g, k, ref32[k], ref64[k]) for k in ref64}
    return x, ref64, ref32, bounds


def error_of(g, name, got, ref64, where=False):
    """The worst row error of output `name` of a case on graph g (where=True: and its (node, head))."""
    if name == "attn_edge":
        return worst(got, ref64, row_ptr=g["row_ptr"], where=where)
    if name in STATS:
        return worst(got, ref64, valid=np.diff(g["row_ptr"]) > 0, where=where)
    return worst(got, ref64, where=where)


# ---- peaked and ordered softmax (one graph) ---------------------------------------------------------------------------
# Twelve test rows: {ascending, descending, constant, large} x degree {65, 200, 1500}.  Ascending / descending rows walk a
# ladder of columns whose logit rises by PEAKED_STEP per column, so every 64-edge tile's maximum exceeds the previous
# tile's by 128: the online-softmax rescale factor exp(-128) is 0 in fp32, the "previous maximum was -inf" and "nothing
# survives the rescale" branches run, and a sweep without the max subtraction overflows (logits up to 3000).  Constant rows
# send every edge to ONE column: all logits equal, every exponential is exp(0).  Large rows draw from a pool whose logits
# are about +-60.  The mass of such rows sits on few edges, so the power condition of the boundary cases does not apply;
# dQ, dK and the attention gradients of GAT / GATv2 cancel almost completely on one-hot rows (the fp32 reference's own
# relative error there is of order 10) and are held to the absolute bar 1e-3 max(1, max |ref|) instead.
PEAKED_DEGREES = (65, 200, 1500)
PEAKED_PATTERNS = ("ascending", "descending", "constant", "large")
PEAKED_WIDTHS = (32, 128)
PEAKED_STEP = 2.0
PEAKED_LARGE = 60.0
PEAKED_V2_ATTN = 8.0         # GATv2: standard deviation of an attn element (see peaked_inputs)
PEAKED_FILL = 4                # out-edges per ladder node in the wave form (nnz >= 8 m)
PEAKED_LOOSE = dict(gt=("dQ", "dK"), gat=("grad_attn_row", "grad_attn_col"), gatv2=("dX_row", "dX_col", "dattn"))


@functools.lru_cache(maxsize=None)
def peaked_graph(wave):
    """-> dict like graph(); rows 0..11 are the test rows (pattern-major), then the ladder, the constant column, the large
    pool; every ladder node has a self-loop.  wave: every ladder node also has PEAKED_FILL edges into the large pool, which
    makes nnz >= 8 m."""
    rng = np.random.default_rng(77)
    R, L = len(PEAKED_PATTERNS) * len(PEAKED_DEGREES), max(PEAKED_DEGREES)
    ladder0, const0, large0 = R, R + L, R + L + 1
    m = large0 + POOL
    src, dst, pattern = [], [], []
    for p in PEAKED_PATTERNS:
        for d in PEAKED_DEGREES:
            i = len(pattern)
            pattern.append(p)
            cols = {"ascending": ladder0 + np.arange(d), "descending": ladder0 + np.arange(d)[::-1],
                    "constant": np.full(d, const0), "large": large0 + rng.integers(0, POOL, d)}[p]
            src.append(np.full(d, i, dtype=np.int64))
            dst.append(cols.astype(np.int64))
    # a self-loop on every ladder node: its dV / dK row gets an ordinary O(1) term, so that the measure's floor (a median
    # over rows) is not set by the columns whose only mass underflows
    src.append(ladder0 + np.arange(L))
    dst.append(ladder0 + np.arange(L))
    if wave:
        src.append(np.repeat(ladder0 + np.arange(L), PEAKED_FILL))
        dst.append(large0 + rng.integers(0, POOL, L * PEAKED_FILL))
    src, dst = np.concatenate(src), np.concatenate(dst)
    nnz = len(src)
    assert (nnz >= 8 * m) == wave
    order = np.argsort(src, kind="stable")
    src, dst = src[order], dst[order]
    rows, col_ind = src.astype(np.int32), dst.astype(np.int32)
    row_ptr = np.zeros(m + 1, dtype=np.int64)
    np.add.at(row_ptr, src + 1, 1)
    row_ptr = np.cumsum(row_ptr).astype(np.int32)
    col_ptr, row_ind, val_idx = csc_of(row_ptr, col_ind, rows, m)
    deg = np.asarray(PEAKED_DEGREES * len(PEAKED_PATTERNS))
    assert (np.diff(row_ptr)[:R] == deg).all()
    return dict(m=m, nnz=nnz, R=R, row_ptr=row_ptr, col_ind=col_ind, rows=rows, col_ptr=col_ptr, row_ind=row_ind,
                val_idx=val_idx, deg=deg, pattern=np.asarray(pattern), ladder=np.arange(ladder0, const0), const=const0,
                large=np.arange(large0, m))


def _unit(rng, f):
    u = rng.standard_normal(f)
    return u / np.linalg.norm(u)


def peaked_inputs(op, wave, f):
    """float32 inputs (one head) that give the logits of peaked_graph's patterns."""
    g = peaked_graph(wave)
    m, R = g["m"], g["R"]
    rng = np.random.default_rng(500 + f)
    ladder, large = g["ladder"], g["large"]
    step = PEAKED_STEP * np.arange(len(ladder))
    big = PEAKED_LARGE * rng.choice([-1.0, 1.0], len(large)) + rng.standard_normal(len(large))
    dO = rng.standard_normal((m, 1, f))
    if op == "gt":      # Q of a test row = a u, K of a ladder / large column = (logit / a) u + noise orthogonal to u
        u, a = _unit(rng, f), f ** 0.25
        Q, K = (rng.standard_normal((m, 1, f)) * f ** -0.25 for _ in range(2))
        V = rng.standard_normal((m, 1, f))
        Q[:R, 0] = a * u
        for nodes, logit in ((ladder, step), (large, big)):
            K[nodes, 0] += ((logit / a) - K[nodes, 0] @ u)[:, None] * u
        return dict(zip(("val", "Q", "K", "V", "dO"), _f32(np.ones(g["nnz"]), Q, K, V, dO)))
    if op == "gat":     # attn_row of a test row ~ 0.5, attn_col of a ladder / large column = logit - 0.5
        ar, ac = (rng.standard_normal((m, 1)) for _ in range(2))
        ar[:R, 0] = 0.5 + rng.uniform(-0.1, 0.1, R)
        ac[ladder, 0], ac[large, 0] = step - 0.25, big - 0.5
        return dict(zip(("attn_row", "attn_col", "X", "dO"), _f32(ar, ac, rng.standard_normal((m, 1, f)), dO)))
    # GATv2: X_row of a test row = 0, X_col of a ladder / large column = b sign(attn) / sum |attn| + small noise; a
    # positive b gives the logit b k with k = (sum of attn > 0 + SLOPE x sum of |attn < 0|) / sum |attn|.  A logit of 3000
    # carries ~5e-4 of fp32 rounding whoever computes it, and so does every dS of such a row; dattn multiplies dS by
    # LeakyReLU(z) ~ 3000 / sum |attn| and dX by attn, so one of them misses the absolute bar even in the fp32 reference
    # unless |attn| and |z| are balanced: with attn elements of standard deviation PEAKED_V2_ATTN the fp32 reference is
    # inside the bar for dX_row, dX_col and dattn at both widths (by 1.4x at the least).
    attn = rng.standard_normal((1, f)) * PEAKED_V2_ATTN
    xr, xc = (rng.standard_normal((m, 1, f)) for _ in range(2))
    w = np.sign(attn[0]) / np.abs(attn[0]).sum()
    k = np.where(attn[0] > 0, attn[0], -SLOPE * attn[0]).sum() / np.abs(attn[0]).sum()
    xr[:R] = 0
    xc[ladder, 0] = (step / k)[:, None] * w + 0.1 / PEAKED_V2_ATTN * rng.standard_normal((len(ladder), f))
    xc[large, 0] = (big / k)[:, None] * w + 0.1 / PEAKED_V2_ATTN * rng.standard_normal((len(large), f))
    return dict(zip(("attn", "X_row", "X_col", "dO"), _f32(attn, xr, xc, dO)))


@functools.lru_cache(maxsize=2)
def peaked_references(op, wave, f):
    """-> (inputs, ref64, ref32, bounds) as references()."""
    g = peaked_graph(wave)
    x = peaked_inputs(op, wave, f)
    ref64 = _REFERENCE[op](g["row_ptr"], g["col_ind"], x, "f64")
    ref32 = _REFERENCE[op](g["row_ptr"], g["col_ind"], x, "f32")
    bounds = {k: MARGIN * error_of(g, k, ref32[k], ref64[k]) for k in ref64}
    return x, ref64, ref32, bounds
