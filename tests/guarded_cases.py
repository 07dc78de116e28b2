"""The table, the cases and the argument builder of the guarded-buffer run of the C ABI (tests/test_gpu_guarded.py; the
host-side checks of all three are tests/test_guarded_host.py).  Nothing here needs a GPU.

The table.  TABLE maps every entry of include/dfgnn.h that takes a stream to the family whose test calls it; EXCLUDED names
the two entries whose guard test lives elsewhere.  The argument list of an entry is not written down a second time: it is
built from the header's own prototype (guarded.prototypes), parameter by parameter (Call) --
    int / float / size_t      the case's scalar of that name
    const T *                 an input: the case's array of that name in an Arena (None: NULL)
    float * / int * / void *  scratch if the name is one of SCRATCH, else an output of the shape shape_of gives its name;
                              names listed in `omit` are passed as NULL (the optional outputs)
so a parameter added to the header is a KeyError here until the table knows it.

The cases of family A (the eleven any-graph pairs).  rect_cases.graph's seven rectangles and four small square graphs of
this module, which supply what rect_cases does not (test_guarded_host.py asserts the geometry): for either pass form, a
last row / column that is empty and one that has an odd degree.  Inputs are seeded normals in the scales of rect_cases.inputs;
the float64 reference of a pair is its cases module's.  The bound on these graphs is the one every pair's own test holds on
them (tests/test_gpu_rect.py, test_gpu_gt_typed.py, ...): max abs error < BAR max(1, max |ref|), BAR = 1e-3 -- row_max /
edge_max on the rows that have an edge, the sentinel exactly elsewhere.  The fp32-level bounds (MARGIN x the float32
formulation's error) belong to the constructed cases of tests/parity_cases.py, whose docstring says why they say nothing
on rows of two or three random edges (the delta of the row-statistics backward): boundary() below puts every pair on four
of those constructed cases, where the fp32-level bound is asserted, and family B runs on them too."""
import functools
import os

import numpy as np
import torch

import guarded
import rect_cases as rc

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "dfgnn.h")
BAR = 1e-3
SLOPE = rc.SLOPE
SENTINEL_MAX = np.float32(-1e38)
TYPES = 5                                    # T of the typed / tbias cases: T h f = 200, T h = 10 at (h, f) = (2, 20)
EPS = 1e-6
ATTN_DROP = 0.25


@functools.lru_cache(maxsize=None)
def protos():
    return guarded.prototypes(open(HEADER).read())


# ---- the table ----------------------------------------------------------------------------------------------------------
# pair -> (forward entry, backward entry); the *_rect entries are these names + "_rect"
PAIRS = dict(rowstats=("dfgnn_gt_fwd_rowstats", "dfgnn_gt_bwd_rowstats"), bias=("dfgnn_gt_fwd_bias", "dfgnn_gt_bwd_bias"),
             edge=("dfgnn_gt_fwd_edge", "dfgnn_gt_bwd_edge"), gate=("dfgnn_gt_fwd_gate", "dfgnn_gt_bwd_gate"),
             typed=("dfgnn_gt_fwd_typed", "dfgnn_gt_bwd_typed"), tbias=("dfgnn_gt_fwd_tbias", "dfgnn_gt_bwd_tbias"),
             gatv2=("dfgnn_gatv2_fwd", "dfgnn_gatv2_bwd"), gatv2_edge=("dfgnn_gatv2_fwd_edge", "dfgnn_gatv2_bwd_edge"),
             agnn=("dfgnn_agnn_fwd", "dfgnn_agnn_bwd"), gatedgcn=("dfgnn_gatedgcn_fwd", "dfgnn_gatedgcn_bwd"),
             gat_edge=("dfgnn_gat_fwd_edge", "dfgnn_gat_bwd_edge"))
TAKES_VAL = ("rowstats", "bias", "edge", "gate", "typed", "tbias")

TABLE = {}
for _pair, _entries in PAIRS.items():
    for _e in _entries:
        TABLE[_e] = TABLE[_e + "_rect"] = "pair:" + _pair
TABLE.update({e: "gt" for e in (
    "dfgnn_gt_hyper_fwd", "dfgnn_gt_bwd", "dfgnn_gt_bwd_rows", "dfgnn_gt_bwd_cols", "dfgnn_gt_tiling_fwd", "dfgnn_gt_softmax_fwd",
    "dfgnn_gt_softmax_gm_fwd", "dfgnn_gt_csr_fwd", "dfgnn_gt_csr_gm_fwd")})
TABLE.update({e: "ranked" for e in ("dfgnn_gt_hyper_fwd_ranked", "dfgnn_gt_bwd_ranked")})
TABLE.update({e: "gat" for e in (
    "dfgnn_gat_hyper_fwd", "dfgnn_gat_recompute_fwd", "dfgnn_gat_softmax_fwd", "dfgnn_gat_softmax_gm_fwd", "dfgnn_gat_tiling_fwd",
    "dfgnn_gat_tiling_chunked_fwd", "dfgnn_gat_attn_scores", "dfgnn_gat_fwd_train", "dfgnn_gat_bwd")})
TABLE.update({e: "prep" for e in ("dfgnn_preprocess_hyper", "dfgnn_preprocess_hyper_rect", "dfgnn_plan_build",
                                  "dfgnn_plan_dense_weights")})
# guard regions of their own: tests/test_gpu_stats_pair.py::test_stats_kernels_write_nothing_outside_their_outputs
EXCLUDED = ("dfgnn_gt_hyper_fwd_stats", "dfgnn_gt_bwd_stats")


def entries_of(family):
    return sorted(e for e, fam in TABLE.items() if fam == family)


# ---- the argument builder -----------------------------------------------------------------------------------------------
SCRATCH = ("delta", "ws", "grad_edge", "logits", "edge_ws")
ALIGNED = ("ws", "weights")                  # the header asks for 16 bytes: they stay aligned under shift = 1
_ROWS3, _COLS3 = ("out", "dQ", "dX_row", "den"), ("dK", "dV", "dX_col", "grad_feat")
_ROWS2, _COLS2 = ("row_max", "row_sum", "edge_max", "edge_sum", "delta", "grad_attn_row", "dbeta_rows", "attn_row"), \
    ("grad_attn_col", "attn_col")
_HEAD_EDGE, _EDGE3 = ("dbias", "grad_score", "attn_edge", "grad_edge", "logits", "edge_ws"), ("dE", "W", "Z")
_PER_EDGE_INT = ("col_ind", "rows", "edge_order", "row_ind", "val_idx")


def shape_of(name, s):
    """The extent include/dfgnn.h gives the writable array `name` at the scalars s (m, n_cols, nnz, h, f, T, ws_numel)."""
    m, n, nnz, h, f = s["m"], s.get("n_cols", s["m"]), s.get("nnz"), s.get("h"), s.get("f")
    if name in _ROWS3:
        return (m, h, f)
    if name in _COLS3:
        return (n, h, f)
    if name in _ROWS2:
        return (m, h)
    if name in _COLS2:
        return (n, h)
    if name in _HEAD_EDGE:
        return (h, nnz)
    if name in _EDGE3:
        return (nnz, h, f)
    if name in _PER_EDGE_INT:
        return (nnz,)
    return {"dR": lambda: (s["T"], h, f), "dB": lambda: (s["T"], h), "dattn": lambda: (h, f), "attn_ranked": lambda: (nnz,),
            "weights": lambda: (s["weights_numel"],), "ws": lambda: (s["ws_numel"],), "row_ptr": lambda: (m + 1,),
            "col_ptr": lambda: (n + 1,), "plan": lambda: (s["plan_numel"],)}[name]()


class Call:
    """One guarded call: the Arena, the argument list, and what verify is to check as outputs."""

    def __init__(self, entry, case, device, shift=0, omit=(), written=()):
        """case: scalars and arrays under the header's parameter names; omit: pointers to pass as NULL; written: names of
        SCRATCH that this entry writes in full (dfgnn_gt_bwd_rows' grad_edge) and that verify checks as outputs."""
        self.entry, self.arena, self.args, self.outputs, self.written = entry, guarded.Arena(device, shift=shift), [], {}, written
        for ctype, name in protos()[entry]:
            self.args.append(self._arg(ctype, name, case, omit))

    def _arg(self, ctype, name, case, omit):
        a = self.arena
        if ctype in ("int", "float", "size_t"):
            return case[name]
        if ctype == "dfgnn_stream_t":
            return case.get("stream")
        if name in omit or (ctype.startswith("const") and case.get(name) is None):
            return None
        if name in ("plan_meta", "meta_host"):               # host memory
            return case[name]
        if ctype.startswith("const"):
            v = case[name]
            if isinstance(v, int):                           # an address the caller owns (the plan of another Arena)
                return v
            return a.input(name, v, aligned=name in ALIGNED).data_ptr()
        dtype = {"float *": torch.float32, "int *": torch.int32, "void *": torch.uint8}[ctype]
        if (name in SCRATCH and name not in self.written) or name == "plan":
            return a.scratch(name, int(np.prod(shape_of(name, case))), dtype, aligned=name in ALIGNED).data_ptr()
        self.outputs[name] = a.output(name, shape_of(name, case), dtype, aligned=name in ALIGNED)
        return self.outputs[name].data_ptr()

    def run(self, lib, sync):
        """-> the entry's return code, after synchronising and verifying: on 0 everything; on an error code that nothing was
        written -- the guards are intact, the inputs unchanged and every output still holds the fill."""
        code = getattr(lib, self.entry)(*self.args)
        sync()
        self.arena.verify(outputs=list(self.outputs) if code == 0 else [])
        if code != 0:
            for name, view in self.outputs.items():
                assert bool((guarded._bits(view) == self.arena.records[name].fill).all()), f"{name}: written by a refused call"
        return code

    def numpy(self):
        return {k: v.detach().cpu().numpy().copy() for k, v in self.outputs.items()}


# ---- graphs -------------------------------------------------------------------------------------------------------------
RECT_KINDS = ("tall", "wide", "block", "line_row", "line_col", "no_rows", "no_cols")
SQUARE_KINDS = ("sq_lane_odd", "sq_lane_empty", "sq_wave_odd", "sq_wave_empty")
WIDTHS = tuple(rc.WIDTHS) + ((1, 100), (2, 130))
EXTRA_WIDTHS = ((1, 100), (2, 130))          # run wherever the entry answers 0 for them
SHIFT_KINDS, SHIFT_WIDTH = ("tall", "wide"), (2, 20)


@functools.lru_cache(maxsize=None)
def graph(kind):
    """rect_cases.graph(kind), or one of the four square circulants: n nodes, row i has the edges i -> (i + k) mod n',
    k < degree; `odd`: n' = n, every row and every column has `degree` (odd) entries; `empty`: n' = n - 1 and the last
    row has no edge, so the last row and the last column are empty.  lane: 70 nodes of degree 3; wave: 20 of degree 9."""
    if kind not in SQUARE_KINDS:
        return rc.graph(kind)
    n, deg = (70, 3) if "lane" in kind else (20, 9)
    live = n if kind.endswith("odd") else n - 1
    src = np.repeat(np.arange(live), deg)
    dst = (src + np.tile(np.arange(deg), live)) % live
    g = rc._finish(src, dst, n, n)
    assert rc.lane_form(n, g["nnz"]) == ("lane" in kind)
    return g


def geometry(g):
    """-> {(side, form, what)}: side rows / cols, form lane / wave (rect_cases.lane_form of that side's pass), what is
    "odd" (the last row / column has an odd number of entries) or "empty" (it has none)."""
    found = set()
    for side, n, deg in (("rows", g["m"], g["deg"]), ("cols", g["n_cols"], g["indeg"])):
        if n == 0:
            continue
        form = "lane" if rc.lane_form(n, g["nnz"]) else "wave"
        if deg[-1] == 0:
            found.add((side, form, "empty"))
        elif deg[-1] % 2 == 1:
            found.add((side, form, "odd"))
    return found


# ---- inputs -------------------------------------------------------------------------------------------------------------
STATS = dict(gatedgcn=("den",), gat_edge=("edge_max", "edge_sum"))       # every other pair: row_max, row_sum
MAX_NAMES = ("row_max", "edge_max")


def stats_of(pair):
    return STATS.get(pair, ("row_max", "row_sum"))


def inputs(pair, g, h, f, unit_val):
    """float32 / int32 numpy inputs of `pair` on graph g under the header's parameter names, every optional one included."""
    base = {"gate": "edge", "typed": "rowstats", "tbias": "rowstats", "gatv2_edge": "gatv2"}.get(pair, pair)
    m, n, nnz = g["m"], g["n_cols"], g["nnz"]
    rng = np.random.default_rng(77000 + 1000 * h + f + (0 if unit_val else 1) + 31 * sorted(PAIRS).index(pair))
    r = lambda *s: rng.standard_normal(s).astype(np.float32)  # noqa: E731
    if base in rc.PAIRS:
        x = dict(rc.inputs(base, g, h, f, unit_val))
        x["grad_out"] = x.pop("dO")
    elif pair == "agnn":
        x = dict(beta=rng.uniform(0.5, 4.5, h).astype(np.float32), X_row=r(m, h, f), X_col=r(n, h, f), grad_out=r(m, h, f))
    elif pair == "gatedgcn":
        x = dict(X_row=r(m, h, f), X_col=r(n, h, f), V=r(n, h, f), E=r(nnz, h, f), G=r(nnz, h, f) * np.float32(1 / 32),
                 grad_out=r(m, h, f))
    else:
        assert pair == "gat_edge"
        x = dict(attn_row=r(m, h), attn_col=r(n, h), score=r(h, nnz) * np.float32(0.5), X=r(n, h, f), grad_out=r(m, h, f),
                 edge_mask=rng.uniform(0, 1, (nnz, h)).astype(np.float32))
    if pair == "gate":
        x["E"] = (1 + 0.25 * rng.standard_normal((nnz, h, f))).astype(np.float32)
        x["G"] = r(nnz, h, f) * np.float32(1 / 32)
    if pair in ("typed", "tbias"):
        x["etype"] = rng.integers(0, TYPES, nnz).astype(np.int32)
        x["etype_csc"] = np.ascontiguousarray(x["etype"][g["val_idx"]])
        if pair == "typed":
            x["R"] = r(TYPES, h, f) * np.float32(0.5)
        else:
            x["B"] = r(TYPES, h)
    if pair == "gatv2_edge":
        x["E"] = r(nnz, h, f)
    return x


def variant(pair, which, x, f):
    """-> (inputs, scalars, forward outputs to omit, backward outputs to omit) of the `full` run (every optional argument
    given and every optional output requested) or the `min` run (every optional argument and output NULL)."""
    x, scal, fo, bo = dict(x), {}, (), ()
    full = which == "full"
    if pair in ("gatv2", "gatv2_edge", "gat_edge"):
        scal["negative_slope"] = SLOPE
    if pair == "agnn":
        scal["cosine"] = 1 if full else 0
        if not full:
            x["beta"] = x["beta"] * np.float32(f ** -0.5)
    if pair == "gatedgcn":
        scal.update(normalize=1 if full else 0, eps=EPS)
    if pair == "gat_edge":
        scal["attn_drop"] = ATTN_DROP if full else 0.0
    if pair in ("typed", "tbias"):
        scal["T"] = TYPES
    if not full:
        bo = dict(bias=("dbias",), edge=("dE",), gate=("dE",), typed=("dR", "ws"), tbias=("dB", "ws"), gatv2_edge=("dE",),
                  agnn=("dbeta_rows",), gatedgcn=("dE", "ws"), gat_edge=("grad_score",)).get(pair, ())
        fo = dict(gate=("W",), gatedgcn=("Z",)).get(pair, ())
        for name in dict(gate=("G",), gatedgcn=("E", "G"), gat_edge=("edge_mask",)).get(pair, ()):
            x[name] = None
    return x, scal, fo, bo


def has_variants(pair):
    return pair not in ("rowstats", "gatv2")


# ---- references ---------------------------------------------------------------------------------------------------------
def _degenerate(pair, g, x):
    """m == 0 or n_cols == 0 (then nnz == 0): what the header says such a call writes -- zeros, and the sentinel."""
    s = dict(m=g["m"], n_cols=g["n_cols"], nnz=0, h=x["grad_out"].shape[1], f=x["grad_out"].shape[2], T=TYPES)
    names = [n for e in PAIRS[pair] for t, n in protos()[e] if t == "float *" and n not in SCRATCH]
    return {n: np.full(shape_of(n, s), SENTINEL_MAX if n in MAX_NAMES else 0.0, dtype=np.float64) for n in names}


FP32_PAIRS = ("rowstats", "bias", "edge", "gatv2", "gate", "typed", "gatedgcn", "gat_edge")   # reference(acc="f32") exists


def reference(pair, g, x, scal, acc="f64"):
    """Every output of `pair` under the header's names, from the pair's cases module: in float64, or (FP32_PAIRS) the same
    formulation in float32.  x, scal: variant()."""
    assert acc == "f64" or pair in FP32_PAIRS
    if g["nnz"] == 0:
        return _degenerate(pair, g, x)
    rp, ci, m, n = g["row_ptr"], g["col_ind"], g["m"], g["n_cols"]
    dO = x["grad_out"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    rows, cols = t(g["rows"].astype(np.int64)), t(ci.astype(np.int64))
    if pair in rc.PAIRS:
        return rc.reference_on(pair, g, dict(x, dO=dO), acc)
    if pair == "gate":
        import gt_gate_cases as gc
        return gc.reference(rp, ci, x["val"], x["E"], x["G"], x["Q"], x["K"], x["V"], dO, acc)
    if pair == "typed":
        import gt_typed_cases as tc
        return tc.reference(rp, ci, n, x["val"], x["etype"], x["R"], x["Q"], x["K"], x["V"], dO, acc)
    if pair == "tbias":
        import gt_tbias_cases as tb
        return tb.reference(rp, ci, n, x["val"], x["etype"], x["B"], x["Q"], x["K"], x["V"], dO)
    if pair == "gatedgcn":
        import gatedgcn_cases as gg
        return gg.reference(rp, ci, x["E"], x["G"], x["X_row"], x["X_col"], x["V"], dO, scal["normalize"], scal["eps"], acc)
    if pair == "gat_edge":
        import gat_edge_cases as ge
        return ge.reference(rp, ci, x["attn_row"], x["attn_col"], x["score"], x["X"], dO, SLOPE, x["edge_mask"],
                            scal["attn_drop"], acc=acc)
    assert pair in ("gatv2_edge", "agnn")
    return _torch_reference(pair, g, x, scal, torch.float64)


def _torch_reference(pair, g, x, scal, dt):
    """GATv2-edge (gatv2_edge_cases.ref_conv) and AGNN (agnn_cases.ref_conv) in precision dt, gradients from
    torch.autograd.grad -> numpy float64 under the header's names; row_max of a row without an edge: the sentinel."""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    m = g["m"]
    rows, cols, dO = t(g["rows"].astype(np.int64)), t(g["col_ind"].astype(np.int64)), t(x["grad_out"]).to(dt)
    xr, xc = (t(x[k]).to(dt).requires_grad_(True) for k in ("X_row", "X_col"))
    if pair == "gatv2_edge":
        from gatv2_edge_cases import ref_conv
        a, e = (t(x[k]).to(dt).requires_grad_(True) for k in ("attn", "E"))
        out, mx, den = ref_conv(rows, cols, m, a, xr, xc, e)
        names, leaves = ("dX_row", "dX_col", "dattn", "dE"), (xr, xc, a, e)
    else:
        from agnn_cases import ref_conv
        # beta as one leaf per (row, head): the gradient of that leaf is the row's share dbeta_rows[i, h]
        b = t(x["beta"]).to(dt)[None].expand(m, -1).clone().requires_grad_(True)
        out, mx, den = ref_conv(rows, cols, m, b[rows], xr, xc, bool(scal["cosine"]))
        names, leaves = ("dX_row", "dX_col", "dbeta_rows"), (xr, xc, b)
    res = dict(zip(names, torch.autograd.grad(out, leaves, dO)), out=out, row_max=mx, row_sum=den)
    res = {k: v.detach().numpy().astype(np.float64) for k, v in res.items()}
    res["row_max"] = np.where(np.isinf(res["row_max"]), np.float64(SENTINEL_MAX), res["row_max"])
    return res


def error_and_bound(name, got, ref, deg):
    """-> (max abs error, bound) of output `name` at the bar; row_max / edge_max on the rows with an edge -- on the others
    the sentinel, exactly (then the error is inf)."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    if name in MAX_NAMES:
        live = np.asarray(deg) > 0
        if not (got[~live] == np.float64(SENTINEL_MAX)).all():
            return float("inf"), 0.0
        got, ref = got[live], ref[live]
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    return err, BAR * max(1.0, float(np.abs(ref).max()) if ref.size else 0.0)


# ---- block-diagonal batches (family B) ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def batch_graph(kind):
    """Block-diagonal batches of symmetric Erdos-Renyi graphs as rect_cases._finish dicts (square), with `ranges`.
    mixed: 40, 60 (with one duplicate edge), 100, 130, 180 nodes at 55 % and 400 nodes at 6 % -- ranges that run LDS-resident,
    one whose per-edge values do not fit next to its rows, one that is too large for LDS at any width (the spill path).
    dense: 40, 96, 131 nodes, no duplicates: every range on the matrix cores (the ranked pair, the dense weights)."""
    sizes = dict(mixed=((40, 0.6), (60, 0.5), (100, 0.3), (130, 0.4), (180, 0.55), (400, 0.06)),
                 dense=((40, 0.5), (96, 0.4), (131, 0.4)))[kind]
    rng = np.random.default_rng(dict(mixed=71, dense=72)[kind])
    src, dst, ranges, off = [], [], [], 0
    for k, (n, p) in enumerate(sizes):
        iu, ju = np.triu_indices(n, k=1)
        keep = rng.random(len(iu)) < p
        s, d = np.concatenate([iu[keep], ju[keep]]), np.concatenate([ju[keep], iu[keep]])
        if kind == "mixed" and k == 1:
            s, d = np.r_[s, s[:1]], np.r_[d, d[:1]]                      # the duplicate edge
        src.append(s + off), dst.append(d + off), ranges.append((off, off + n))
        off += n
    g = rc._finish(np.concatenate(src), np.concatenate(dst), off, off)
    g["ranges"] = ranges
    assert g["nnz"] >= 8 * g["m"]                                        # (a plan applies)
    return g


def fp32_level(pair, g, name, got, ref64, ref32):
    """-> (error, MARGIN x the float32 formulation's error) of output `name` in its cases module's row-wise measure
    (parity_cases.worst; dK of the GT pairs: x DK_FACTOR).  On the random graphs of family A this is a FIGURE the run prints
    next to the bar, not a bound it holds -- rows of two and three random edges and analytic zeros are where
    parity_cases._sentinels says what the measure is worth; the bound itself is held on boundary()'s constructed cases."""
    import parity_cases as pc
    mod = dict(rowstats="gt_bias_cases", bias="gt_bias_cases", edge="gt_edge_cases", gate="gt_gate_cases", typed="gt_typed_cases",
               gatedgcn="gatedgcn_cases", gat_edge="gat_edge_cases").get(pair)
    error_of = __import__(mod).error_of if mod else pc.error_of
    fix = (lambda a: np.asarray(a, dtype=np.float64)[None]) if name == "dattn" else (lambda a: np.asarray(a, dtype=np.float64))
    factor = __import__("gt_bias_cases").DK_FACTOR if name == "dK" else 1.0
    return error_of(g, name, fix(got), fix(ref64)), pc.MARGIN * factor * error_of(g, name, fix(ref32), fix(ref64))


# ---- the pairs on the constructed boundary-degree cases -------------------------------------------------------------------
# (transposed, low, f, h, unit_val) of parity_cases.case_ids("gt"): both kernel forms, both orientations, float4 and scalar
# lanes, with and without edge values; the pairs without edge values take the first four entries
BOUNDARY_CASES = ((False, False, 128, 1, True), (True, True, 7, 2, False), (False, True, 32, 1, False), (True, False, 32, 1, True))
BOUNDARY_T = 304


@functools.lru_cache(maxsize=2)
def boundary(pair, case):
    """-> (graph, inputs, scalars, ref64, bounds, error_of, backward outputs to omit) of `pair` on one boundary-degree case,
    under the header's names: the inputs, float64 reference, measure and bound = MARGIN x the float32 formulation's error of
    the pair's own cases module, where one exists (rowstats and gatv2: parity_cases; bias, edge, gate, typed, gatedgcn,
    gat_edge: *_cases.boundary_references).  The other three are built here in the same way:
      tbias       gt_bias_cases.boundary_inputs, B ~ N(0, 1) [304, h], etype = col_ind (tests/test_gpu_gt_tbias.py); the
                  float32 formulation is gt_bias_cases.reference(acc="f32") on B[etype], dB its dbias summed by type;
      gatv2_edge  X_row' = 0, E_e = X_row[row(e)] of parity_cases.gatv2_inputs: z_e has the plain pair's bits
                  (tests/test_gpu_gatv2_edge.py), so the six outputs of the plain pair keep parity_cases' references and
                  bounds; dE from gatv2_edge_cases.ref_conv in float64 / float32, grouped by CSR row;
      agnn        X_row = Q, X_col = K of parity_cases.gt_inputs, cosine = unit_val, beta = 2 (cosine) or 1 (dot product);
                  agnn_cases.ref_conv in float64 / float32.
    Shared; nobody writes to it."""
    import gt_bias_cases as bc
    import parity_cases as pc
    from gt_edge_cases import edge_rows
    g = pc.graph(case[0], case[1])
    f, h = case[2], case[3]
    scal, omit, err = {}, (), pc.error_of
    live = (np.diff(g["row_ptr"]) > 0)[:, None]             # (rows without an edge hold the sentinel: out of the measure)
    stats_valid = lambda name, a, b: pc.worst(np.where(live, a, 0.0), np.where(live, b, 0.0), valid=live[:, 0]) \
        if name in pc.STATS else pc.worst(a, b)  # noqa: E731
    if pair == "rowstats":
        x, ref, _, bounds = pc.references("gt", *case)
    elif pair in ("bias", "edge", "gate", "typed"):
        mod = __import__(f"gt_{pair}_cases")
        (x, ref, bounds), err = mod.boundary_references(case), mod.error_of
        if pair == "typed":
            x = dict(x, etype_csc=np.ascontiguousarray(x["etype"][g["val_idx"]]))
            scal["T"] = BOUNDARY_T
            omit = () if BOUNDARY_T * f <= 8192 else ("dR", "ws")                # (the LDS tables: T f <= 8192)
    elif pair == "tbias":
        import gt_tbias_cases as tb
        x = dict(bc.boundary_inputs(case))
        x["B"] = np.random.default_rng(304).standard_normal((BOUNDARY_T, h)).astype(np.float32)
        x["etype"] = g["col_ind"].astype(np.int32)
        x["etype_csc"] = np.ascontiguousarray(x["etype"][g["val_idx"]])
        scal["T"] = BOUNDARY_T
        args = (x["val"], x["Q"], x["K"], x["V"], x["dO"])
        ref = tb.reference(g["row_ptr"], g["col_ind"], g["m"], x["val"], x["etype"], x["B"], *args[1:])
        r32 = bc.reference(g["row_ptr"], g["col_ind"], x["val"], tb.materialise(x["B"], x["etype"]), *args[1:], "f32")
        dB32 = torch.zeros((BOUNDARY_T, h)).index_add_(0, torch.from_numpy(x["etype"].astype(np.int64)),
                                                       torch.from_numpy(r32["dbias"].T.astype(np.float32))).numpy()
        r32 = dict(r32, dB=dB32)
        err = lambda g_, name, a, b: pc.worst(a, b) if name == "dB" else bc.error_of(g_, name, a, b)  # noqa: E731
        bounds = {k: pc.MARGIN * (bc.DK_FACTOR if k == "dK" else 1.0) * err(g, k, r32[k], ref[k]) for k in tb.OUTPUTS}
    elif pair == "gatedgcn":
        import gatedgcn_cases as gg
        (x, ref, bounds), err = gg.boundary_references(case, 1), gg.error_of
        scal.update(normalize=1, eps=gg.EPS)
    elif pair == "gat_edge":
        import gat_edge_cases as ge
        (x, ref, bounds), err = ge.boundary_references(case[:4]), ge.error_of
        scal.update(negative_slope=pc.SLOPE, attn_drop=0.0)
        x = dict(x, edge_mask=None)
    elif pair in ("gatv2", "gatv2_edge"):
        x, ref, _, bounds = pc.references("gatv2", *case[:4])
        scal["negative_slope"] = SLOPE
        ref = dict(ref, dattn=ref["dattn"][0])
        err = lambda g_, name, a, b: pc.error_of(g_, name, np.asarray(a)[None], np.asarray(b)[None]) if name == "dattn" \
            else pc.error_of(g_, name, a, b)  # noqa: E731
        if pair == "gatv2_edge":
            x = dict(x, E=np.ascontiguousarray(x["X_row"][g["rows"]]), X_row=np.zeros_like(x["X_row"]), grad_out=x["dO"])
            dE = [_torch_reference(pair, g, x, scal, dt)["dE"] for dt in (torch.float64, torch.float32)]
            plain = err
            by_row = lambda a: edge_rows(a, g["row_ptr"])  # noqa: E731
            err = lambda g_, name, a, b: pc.worst(by_row(a)[0], by_row(b)[0], row_ptr=by_row(b)[1]) if name == "dE" \
                else plain(g_, name, a, b)  # noqa: E731
            ref, bounds = dict(ref, dE=dE[0]), dict(bounds, dE=pc.MARGIN * err(g, "dE", dE[1], dE[0]))
    else:
        assert pair == "agnn"
        gx = pc.gt_inputs(*case)
        scal["cosine"] = int(case[4])
        x = dict(X_row=gx["Q"], X_col=gx["K"], grad_out=gx["dO"], beta=np.full(h, 2.0 if case[4] else 1.0, dtype=np.float32))
        ref, r32 = (_torch_reference(pair, g, x, scal, dt) for dt in (torch.float64, torch.float32))
        err = lambda g_, name, a, b: stats_valid(name, a, b)  # noqa: E731
        bounds = {k: pc.MARGIN * err(g, k, r32[k], ref[k]) for k in ref}
    x = dict(x)
    if "dO" in x:
        x["grad_out"] = x.pop("dO")
    return g, x, scal, ref, bounds, err, omit
