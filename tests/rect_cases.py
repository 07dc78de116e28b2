"""Rectangular (m rows x n_cols columns) cases of the four any-graph pairs -- GT row statistics, GT with an attention bias,
GT with edge features, GATv2 -- shared by tests/test_rect_host.py and tests/test_gpu_rect.py.

The reference.  A torch formulation on the CPU with separate extents: index ops over the edge list (rows[e] < m,
cols[e] < n_cols), gradients from torch.autograd.grad, in float64 (acc="f32": the same formulation in float32).  Empty-row
conventions as tests/gt_edge_cases.py: out = 0, row_sum = 0, dQ = 0, row_max = -1e38.

The graphs.  graph(kind) builds the edge lists of tests/test_gpu_rect.py with numpy under fixed seeds: each has duplicate
edges, an edge into column n_cols - 1 and (where its shape allows) an empty row and an empty column, and sits on a known
side of the kernels' form thresholds, which thresholds() reads from csrc the way parity_cases.caps() reads its caps.

The embedding.  embed_* move a SQUARE case into a rectangle: column j becomes j + col_shift, col_pad empty columns and
row_pad empty rows follow.  No edge's arithmetic changes and no order inside a row or a column does, so the square case's
float64 reference, its fp32-level bounds and its proven power (parity_cases) carry over as they are; restrict_* maps the
rectangle's outputs back and reports whether everything outside the image is an exact zero (row_max: the sentinel)."""
import functools
import os
import re

import numpy as np
import torch

from conftest import ROOT, csc_of

SENTINEL_MAX = -1e38
SLOPE = 0.2
WIDTHS = ((1, 128), (2, 20), (3, 7), (8, 16))            # (h, f): float4 two chunks / float4 / scalar lanes / many heads
PAIRS = ("rowstats", "bias", "edge", "gatv2")
ROW_OUTPUTS = dict(rowstats=("out", "dQ"), bias=("out", "dQ"), edge=("out", "dQ"), gatv2=("out", "dX_row"))
COL_OUTPUTS = dict(rowstats=("dK", "dV"), bias=("dK", "dV"), edge=("dK", "dV"), gatv2=("dX_col",))
CSRC = os.path.join(ROOT, "df-gnn_amd", "csrc")


@functools.lru_cache(maxsize=None)
def thresholds():
    """The constants that decide a pass's kernel form, read from the sources: a pass over n rows / columns of a graph of
    nnz edges takes the lane-group form when nnz < kBlockMinAvgDegree n; inside it a wave whose rows include one of more
    than k*GroupMaxDegree entries takes them cooperatively."""
    found = {}
    for fn, names in (("dfgnn_launch.hpp", ("kBlockMinAvgDegree",)), ("gt_train.hip", ("kGtGroupMaxDegree",)),
                      ("gt_bias_train.hip", ("kGtBiasGroupMaxDegree",)), ("gt_edge_train.hip", ("kGtEdgeGroupMaxDegree",)),
                      ("gatv2_train.hip", ("kGatv2GroupMaxDegree",))):
        text = open(os.path.join(CSRC, fn)).read()
        for name in names:
            hits = re.findall(r"constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text)
            assert len(hits) == 1, (fn, name, hits)
            found[name] = int(hits[0])
    return found


def lane_form(n, nnz):
    """low_degree(n, nnz) of csrc/dfgnn_launch.hpp."""
    return nnz < thresholds()["kBlockMinAvgDegree"] * n


# ---- graphs -----------------------------------------------------------------------------------------------------------
def _finish(src, dst, m, n_cols):
    """COO (row, column) in any order -> dict of int32 CSR / CSC arrays (stable sorts, as the preprocessing)."""
    src, dst = np.asarray(src, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    order = np.argsort(src, kind="stable")
    rows, col_ind = src[order].astype(np.int32), dst[order].astype(np.int32)
    row_ptr = np.zeros(m + 1, dtype=np.int64)
    np.add.at(row_ptr, src + 1, 1)
    row_ptr = np.cumsum(row_ptr).astype(np.int32)
    col_ptr, row_ind, val_idx = csc_of(row_ptr, col_ind, rows, n_cols)
    return dict(m=m, n_cols=n_cols, nnz=len(src), src=src, dst=dst, row_ptr=row_ptr, col_ind=col_ind, rows=rows,
                col_ptr=col_ptr, row_ind=row_ind, val_idx=val_idx, deg=np.diff(row_ptr), indeg=np.diff(col_ptr))


def _random_rect(rng, m, n_cols, avg, empty_rows, empty_cols, heavy_row=None, heavy_col=None):
    deg = np.maximum(rng.poisson(avg, m), 1)
    deg[list(empty_rows)] = 0
    if heavy_row is not None:
        deg[heavy_row[0]] = heavy_row[1]
    src = np.repeat(np.arange(m), deg)
    allowed = np.setdiff1d(np.arange(n_cols), list(empty_cols))
    dst = allowed[rng.integers(0, len(allowed), len(src))]
    dup = np.nonzero(src[1:] == src[:-1])[0][::7] + 1            # duplicate edges: the edge before it, again
    dst[dup] = dst[dup - 1]
    if heavy_col is not None:                                    # one edge of each of the first rows with edges -> that column
        first = np.nonzero(np.r_[True, src[1:] != src[:-1]])[0][:heavy_col[1]]
        dst[first] = heavy_col[0]
    dst[-1] = n_cols - 1
    return _finish(src, dst, m, n_cols)


def _block_parent():
    """The parent graph of `block`: 400 nodes; seeds 0..95 -- 90 of ten edges each (with duplicates) that together reach
    every node of 96..256, four of thirty edges (the fanout cuts them to ten), two without edges."""
    rng = np.random.default_rng(96257)
    src, dst = [], []
    pool = np.arange(96, 257)
    for i in range(90):
        cols = list(pool[i::90])                                 # every pool node is somebody's neighbour
        cols += list(rng.choice(np.r_[np.arange(3, 96), pool], 10 - len(cols) - 1))
        cols.append(cols[0])                                     # a duplicate edge
        src += [i] * 10
        dst += cols
    for i in range(90, 94):
        src += [i] * 30
        dst += list(rng.choice(pool, 30))
    for i in range(96, 400):                                     # the rest of the parent graph: never sampled from
        src += [i] * 2
        dst += list(rng.integers(0, 400, 2))
    g = _finish(src, dst, 400, 400)
    return g


@functools.lru_cache(maxsize=None)
def graph(kind):
    """tall 600 x 40 | wide 40 x 600 | block 96 x 257 (sample_block, fanout 10) | line_row 1 x 300 | line_col 300 x 1 |
    no_rows 0 x 5 | no_cols 5 x 0.  Shared by the tests; nobody writes to it."""
    t = thresholds()
    if kind == "tall":
        g = _random_rect(np.random.default_rng(60040), 600, 40, 3, empty_rows=(5, 599), empty_cols=(13,), heavy_col=(7, 80))
        assert lane_form(g["m"], g["nnz"]) and not lane_form(g["n_cols"], g["nnz"]) and g["indeg"].max() > 64
    elif kind == "wide":
        g = _random_rect(np.random.default_rng(40600), 40, 600, 40, empty_rows=(11,), empty_cols=(77,), heavy_row=(3, 200),
                         heavy_col=(500, 30))
        assert not lane_form(g["m"], g["nnz"]) and lane_form(g["n_cols"], g["nnz"]) and g["deg"].max() == 200
        assert g["indeg"].max() > max(v for k, v in t.items() if k.endswith("GroupMaxDegree"))   # the cooperative branch, all four files
        assert (g["dst"] >= g["m"]).mean() > 0.5
    elif kind == "block":
        from DFGNN.utils.graph import sample_block
        p = _block_parent()
        gen = torch.Generator().manual_seed(10)
        block, col_nodes = sample_block(torch.from_numpy(p["row_ptr"]), torch.from_numpy(p["col_ind"]), torch.arange(96), 10, gen)
        s, d = (x.numpy() for x in block.edges())
        g = _finish(s, d, block.num_rows(), block.num_cols())
        g["col_nodes"], g["parent"] = col_nodes.numpy(), p
        assert (g["m"], g["n_cols"]) == (96, 257) and g["deg"].max() == 10
        assert not lane_form(g["m"], g["nnz"]) and lane_form(g["n_cols"], g["nnz"])          # a wave per row, a lane group per column
    elif kind == "line_row":
        rng = np.random.default_rng(1300)
        dst = rng.integers(0, 299, 300)
        dst[-1], dst[5] = 299, dst[4]
        g = _finish(np.zeros(300, dtype=np.int64), dst, 1, 300)
    elif kind == "line_col":
        src = np.r_[np.arange(0, 300, 2), np.arange(1, 300, 6), [8, 8]]                       # rows 3, 5, ... stay empty
        g = _finish(src, np.zeros(len(src), dtype=np.int64), 300, 1)
    elif kind in ("no_rows", "no_cols"):
        return _finish([], [], *((0, 5) if kind == "no_rows" else (5, 0)))
    else:
        raise KeyError(kind)
    if kind not in ("line_row", "line_col"):
        assert (g["deg"] == 0).any() and (g["indeg"] == 0).any()
    assert g["indeg"][-1] > 0 and (np.diff(g["col_ind"].astype(np.int64)) == 0)[np.diff(g["rows"]) == 0].any()   # duplicates
    return g


def inputs(pair, g, h, f, unit_val, seed=0):
    """float32 numpy inputs of `pair` on graph g: row side [m, h, f], column side [n_cols, h, f], per-edge arrays in CSR order."""
    rng = np.random.default_rng(1000 * h + f + 7 * seed + (0 if unit_val else 1))
    m, n, nnz = g["m"], g["n_cols"], g["nnz"]
    r = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    if pair == "gatv2":
        return dict(attn=r(h, f) * np.float32(f ** -0.5), X_row=r(m, h, f), X_col=r(n, h, f), dO=r(m, h, f))
    x = dict(val=np.ones(nnz, dtype=np.float32) if unit_val else rng.uniform(0.5, 1.5, nnz).astype(np.float32),
             Q=r(m, h, f) * np.float32(f ** -0.25), K=r(n, h, f) * np.float32(f ** -0.25), V=r(n, h, f), dO=r(m, h, f))
    if pair == "bias":
        x["bias"] = r(h, nnz)
    if pair == "edge":
        x["E"] = r(nnz, h, f) * np.float32(0.5)
    return x


# ---- the reference ----------------------------------------------------------------------------------------------------
def reference(pair, m, n_cols, rows, cols, x, acc="f64"):
    """Every output of `pair` on the m x n_cols graph with the edges (rows[e], cols[e]) in CSR order, as numpy arrays in
    precision `acc`.  x: inputs() (bias [h, nnz], E [nnz, h, f])."""
    dt = torch.float64 if acc == "f64" else torch.float32
    rows, cols = (torch.from_numpy(np.asarray(a).astype(np.int64)) for a in (rows, cols))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dt).requires_grad_(True)  # noqa: E731
    dO = torch.from_numpy(x["dO"]).to(dt)
    if pair == "gatv2":
        names, leaves = ("dX_row", "dX_col", "dattn"), [t(x["X_row"]), t(x["X_col"]), t(x["attn"])]
        xr, xc, a = leaves
        s = (torch.nn.functional.leaky_relu(xr[rows] + xc[cols], SLOPE) * a).sum(-1)                 # [nnz, h]
        msg = xc[cols]
    else:
        names, leaves = ["dQ", "dK", "dV"], [t(x["Q"]), t(x["K"]), t(x["V"])]
        q, k, v = leaves
        ke, msg = k[cols], v[cols]
        if pair == "edge":
            e = t(x["E"])
            ke, msg = ke + e, msg + e
            names.append("dE"), leaves.append(e)
        s = (q[rows] * ke).sum(-1) * torch.from_numpy(x["val"]).to(dt)[:, None]
        if pair == "bias":
            b = t(x["bias"])
            s = s + b.t()
            names.append("dbias"), leaves.append(b)
    h = s.size(1)
    mx = torch.full((m, h), float("-inf"), dtype=dt).scatter_reduce(0, rows[:, None].expand_as(s), s.detach(), reduce="amax",
                                                                    include_self=True)
    p = torch.exp(s - mx[rows])
    den = torch.zeros((m, h), dtype=dt).index_add_(0, rows, p)
    out = torch.zeros((m,) + tuple(msg.shape[1:]), dtype=dt).index_add_(0, rows, msg * (p / den[rows])[:, :, None])
    grads = torch.autograd.grad(out, leaves, dO) if len(rows) and m else [torch.zeros_like(l) for l in leaves]
    mx = torch.where(torch.isinf(mx), torch.full_like(mx, SENTINEL_MAX), mx)
    res = dict(out=out.detach().numpy(), row_max=mx.numpy(), row_sum=den.detach().numpy())
    res.update({k: g.detach().numpy() for k, g in zip(names, grads)})
    return res


def reference_on(pair, g, x, acc="f64"):
    return reference(pair, g["m"], g["n_cols"], g["rows"], g["col_ind"], x, acc)


# ---- the embedding of a square case -------------------------------------------------------------------------------------
def embed_graph(row_ptr, col_ind, col_shift=0, col_pad=0, row_pad=0):
    """The square CSR graph (m nodes) as an (m + row_pad) x (m + col_shift + col_pad) one: column j -> j + col_shift."""
    m = len(row_ptr) - 1
    row_ptr = np.r_[row_ptr, np.full(row_pad, row_ptr[-1])].astype(np.int32)
    col_ind = (np.asarray(col_ind, dtype=np.int64) + col_shift).astype(np.int32)
    rows = np.repeat(np.arange(m + row_pad, dtype=np.int32), np.diff(row_ptr))
    n_cols = m + col_shift + col_pad
    col_ptr, row_ind, val_idx = csc_of(row_ptr, col_ind, rows, n_cols)
    return dict(m=m + row_pad, n_cols=n_cols, nnz=len(col_ind), row_ptr=row_ptr, col_ind=col_ind, rows=rows, col_ptr=col_ptr,
                row_ind=row_ind, val_idx=val_idx, m0=m, col_shift=col_shift)


def embed_rows(a, row_pad, fill=None, seed=1):
    """A row-side array [m, ...] of the square case with row_pad trailing rows: of noise (inputs: the rows have no edge, so
    nothing may depend on them) or of `fill` (expected outputs)."""
    a = np.asarray(a)
    shape = (row_pad,) + a.shape[1:]
    pad = np.full(shape, fill, dtype=a.dtype) if fill is not None else \
        np.random.default_rng(seed).standard_normal(shape).astype(a.dtype)
    return np.ascontiguousarray(np.concatenate([a, pad]))


def embed_cols(a, col_shift, col_pad, fill=None, seed=2):
    """A column-side array [m, ...] moved to rows col_shift .. col_shift + m of [m + col_shift + col_pad, ...]."""
    a = np.asarray(a)
    n = a.shape[0] + col_shift + col_pad
    out = np.full((n,) + a.shape[1:], fill, dtype=a.dtype) if fill is not None else \
        np.random.default_rng(seed).standard_normal((n,) + a.shape[1:]).astype(a.dtype)
    out[col_shift:col_shift + a.shape[0]] = a
    return np.ascontiguousarray(out)


def restrict_rows(a, m0, fill=0.0):
    """-> (the first m0 rows, whether every other row holds exactly `fill`)."""
    a = np.asarray(a)
    return a[:m0], bool((a[m0:] == np.asarray(fill, dtype=a.dtype)).all())


def restrict_cols(a, m0, col_shift):
    a = np.asarray(a)
    rest = np.r_[a[:col_shift].ravel(), a[col_shift + m0:].ravel()]
    return a[col_shift:col_shift + m0], bool((rest == 0).all())
