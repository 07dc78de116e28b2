"""What keeps the fp32-level bounds of tests/test_gpu_dense_exact.py honest, proved on the CPU for the cases of
tests/dense_cases.py.

Structure: every range satisfies the plan's density rule with room to spare, no row holds a column twice, nnz >= 8 m, two
neighbouring ranges never fit 128 nodes together, every range holds its probe grid, the hole copies have the stated degrees.

Power: for EVERY probe edge (i, j) of every range, at every width, with and without edge values, losing that one edge moves
out, attn_edge, row_sum and dQ of row i and dK, dV of column j by at least POWER x bound in the measure of parity_cases
(GAT: out / inference, edge_sum, grad_attn_row of the row, grad_feat, grad_attn_col of the column).  An edge (i, j) enters
row i's softmax and nothing else, so the moved values of row i are one float64 evaluation of that row without the edge, and
column j loses exactly the term row i added to it; the same evaluation of the intact row must first reproduce the float64
oracle's row.  No width is left out.  The row maxima are not under the condition, for the reason given in
test_parity_cases_host.py -- with one consequence here, where the lost edge can be its row's argmax: row_sum is stored
relative to row_max, and when the maximum moves by d the sum becomes (S - 1) e^d, which equals S for one d.  The maximum
has then moved by that d, so for row_sum (edge_sum) the larger of the two moves counts, each in units of its own bound;
the GPU test holds both at their bounds.

Padding: in a range whose size is no multiple of 16 a padding column counted as an edge has logit 0 and a zero value row; it
would add exp(-row_max) to row_sum, and that is at least POWER x bound of every such row."""
import numpy as np
import pytest

import dense_cases as dc
import parity_cases as pc

ISSUE_NARROW = [2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 79, 80, 81, 95, 96, 97, 111, 112, 113, 127, 128]
ISSUE_WIDE = [129, 130, 143, 144, 145, 159, 160, 161, 162, 175, 176, 177, 191, 192, 193, 207, 208, 209, 223, 224, 225, 239,
              240, 241, 254, 255]
ISSUE_HOLES = [17, 128, 160, 177, 192, 255]
ISSUE_WIDTHS = {(1, 128), (1, 64), (1, 32), (1, 16), (1, 8), (2, 64), (4, 32), (8, 16), (3, 32), (2, 128)}
GT_CASES = [(b, h, f, u) for b in dc.BATCHES for h, f in dc.WIDTHS for u in (True, False)]
GAT_CASES = [(b, h, f) for b in dc.BATCHES for h, f in dc.WIDTHS]


def test_the_cases_are_the_ones_asked_for():
    assert set(dc.WIDTHS) == ISSUE_WIDTHS and len(dc.WIDTHS) == 10
    narrow = dc.batch_layout("narrow")
    assert sorted(n for n, _ in narrow) == ISSUE_NARROW and not any(hole for _, hole in narrow)
    wide = dc.batch_layout("wide")
    plain = [n for n, hole in wide if not hole]
    assert sorted(n for n in plain if n > 128) == ISSUE_WIDE and sorted(n for n in plain if n <= 128) == [16, 64, 128]
    assert [n for n, hole in wide if hole] == ISSUE_HOLES
    for k, n in enumerate(plain):                     # the small ones stand between wide ranges
        if n <= 128:
            assert plain[k - 1] > 128 and plain[k + 1] > 128
    assert list(dc.probe_nodes(17)) == [0, 15, 16] and list(dc.probe_nodes(2)) == [0, 1]
    assert list(dc.probe_nodes(255)) == [0, 15, 16, 31, 32, 63, 64, 95, 96, 127, 128, 159, 160, 191, 192, 254]
    assert list(dc.probe_nodes(128)) == [0, 15, 16, 31, 32, 63, 64, 95, 96, 127]


@pytest.mark.parametrize("name", dc.BATCHES)
def test_structure(name):
    g = dc.graph(name)
    m, nnz, rp, ci = g["m"], g["nnz"], g["row_ptr"], g["col_ind"]
    assert nnz >= 8 * m                                              # else make_plan refuses the plan
    assert [(r["n"], r["hole"]) for r in g["ranges"]] == dc.batch_layout(name)
    sizes = [r["n"] for r in g["ranges"]]
    assert all(a + b > 128 for a, b in zip(sizes, sizes[1:]))       # the plan merges ranges up to 128 nodes
    assert (max(sizes) <= 128) == (name == "narrow")
    deg, indeg = np.diff(rp), np.bincount(ci, minlength=m)
    rows = g["rows"].astype(np.int64)
    assert len(np.unique(rows * m + ci)) == nnz                     # no duplicate edge
    sorted_rows = 0
    for r in g["ranges"]:
        n0, n = r["n0"], r["n"]
        lo, hi = rp[n0], rp[n0 + n]
        cols = ci[lo:hi]
        assert cols.min() >= n0 and cols.max() < n0 + n            # block-diagonal
        assert dc.dense_rule(n, hi - lo) and 32 * (hi - lo) >= 4 * n * n, (n, hi - lo)    # four times the rule's edges
        if n >= 64 and not r["hole"]:
            assert 25 <= (hi - lo) / n <= 60, (n, (hi - lo) / n)    # mean out-degree
        has = np.zeros((m, ), dtype=bool)
        for i in r["probes"]:                                        # the whole grid B x B, self-loops included
            has[:] = False
            has[ci[rp[i]:rp[i + 1]]] = True
            assert has[r["probes"]].all(), (n, i)
        sorted_rows += sum(bool((np.diff(ci[rp[i]:rp[i + 1]]) > 0).all()) for i in range(n0, n0 + n) if deg[i] > 2)
        if r["hole"]:
            last, iso, partner = r["last"], r["isolated"], r["partner"]
            assert deg[last] == 1 == indeg[last] and ci[rp[last]] == partner and partner in rows[ci == last]
            assert deg[iso] == 0 == indeg[iso] and iso not in (last, partner)
            assert last == n0 + n - 1 and (iso - n0) in dc.probe_nodes(n)
            assert deg[partner] > 5 and indeg[partner] > 5      # an ordinary node
    empty = np.nonzero((deg == 0) | (indeg == 0))[0]
    assert list(empty) == [r["isolated"] for r in g["ranges"] if r["hole"]]    # (the directed graphs leave no other)
    assert sorted_rows < 0.05 * m                                   # CSR rows are not in column order (the ranked pair)
    assert not np.array_equal(                                      # directed: mask != maskT
np.sort(rows * m + ci), np.sort(ci.astype(np.int64) * m + rows))
    # the probe edges' CSR slots
    p = g["probe"]
    assert (rows[p[:, 2]] == p[:, 0]).all() and (ci[p[:, 2]] == p[:, 1]).all() and len(np.unique(p[:, 2])) == len(p)
    assert len(p) == sum(len(r["probes"]) ** 2 for r in g["ranges"])
    pad = dc.padded_rows(g)
    assert len(pad) == sum(n for n in sizes if n % 16) and len(pad) > 0


@pytest.mark.parametrize("n", dc.THRESHOLD_SIZES)
def test_threshold_graphs(n):
    for short in (0, 1):
        g = dc.threshold_graph(n, short)
        n0, nn, edges = g["test"]
        assert nn == n and edges == -(-n * n // 32) - short
        assert g["row_ptr"][n0 + n] - g["row_ptr"][n0] == edges
        assert dc.dense_rule(n, edges) == (short == 0)              # exactly at the rule / one edge short of it
        assert g["nnz"] >= 8 * g["m"]
        rows = g["rows"].astype(np.int64)
        assert len(np.unique(rows * g["m"] + g["col_ind"])) == g["nnz"]
        assert n + dc.THRESHOLD_COMPANION > 128


# ---- the power condition -------------------------------------------------------------------------------------------------
def _norm(a):
    """||.||_inf over the last axis of [h, k]."""
    return np.abs(a).max(axis=-1)


class _Report:
    def __init__(self, what, bounds):
        self.what, self.bounds, self.least = what, bounds, {}

    def add(self, size, name, move, with_max=None):
        """with_max = (name of the maximum, its move): the sum is stored relative to the maximum, so the two count together
        (module docstring) -- the larger of the two moves, each in units of its own bound."""
        if with_max is not None:
            move = np.maximum(move, with_max[1] * self.bounds[name] / self.bounds[with_max[0]])
        key = (size, name)
        self.least[key] = min(self.least.get(key, np.inf), float(np.min(move)))

    def done(self):
        for (size, name), move in sorted(self.least.items()):
            print(f"power {self.what} range of {size} nodes {name}: least move {move:.3e}, bound {self.bounds[name]:.3e}, "
                  f"ratio {move / self.bounds[name]:.1f}")
        bad = [(k, v, self.bounds[k[1]]) for k, v in self.least.items() if not v >= pc.POWER * self.bounds[k[1]]]
        assert not bad, (self.what, bad)
        return min(v / self.bounds[k[1]] for k, v in self.least.items())


def _same(a, b, what):
    assert np.allclose(a, b, rtol=1e-9, atol=1e-12), what


def _power_gt(name, h, f, unit_val):
    g = dc.graph(name)
    x, ref64, _, bounds = dc.gt_references(name, h, f, unit_val)
    assert all(bounds[k] > 0 for k in dc.GT_NAMES)
    val, Q, K, V, dO = (x[k].astype(np.float64) for k in ("val", "Q", "K", "V", "dO"))
    floor = {k: pc.floor_of(ref64[k], g["row_ptr"] if k == "attn_edge" else None) for k in ref64}
    rep = _Report(f"gt {name} h={h} f={f} unit_val={unit_val}", bounds)
    for r in g["ranges"]:
        probes = r["probes"]
        for i in probes:
            lo, hi, cols = dc._row(g, i)
            full = dc.gt_row(Q[i], K[cols], V[cols], val[lo:hi], dO[i])
            _same(full["out"], ref64["out"][i], "out")
            _same(full["attn"], ref64["attn_edge"][:, lo:hi], "attn_edge")
            _same(full["row_sum"], ref64["row_sum"][i], "row_sum")
            _same(full["dQ"], ref64["dQ"][i], "dQ")
            for at in np.nonzero(np.isin(cols, probes))[0]:
                keep = np.arange(hi - lo) != at
                c = cols[keep]
                less = dc.gt_row(Q[i], K[c], V[c], val[lo:hi][keep], dO[i])
                j = cols[at]
                rep.add(r["n"], "out", _norm(less["out"] - full["out"]) / np.maximum(_norm(ref64["out"][i]), floor["out"]))
                rep.add(r["n"], "attn_edge", _norm(less["attn"] - full["attn"][:, keep])
                        / np.maximum(_norm(full["attn"]), floor["attn_edge"]))
                rep.add(r["n"], "row_sum", np.abs(less["row_sum"] - full["row_sum"])
                        / np.maximum(np.abs(full["row_sum"]), floor["row_sum"]),
                        with_max=("row_max", np.abs(less["row_max"] - full["row_max"])
                                  / np.maximum(np.abs(full["row_max"]), floor["row_max"])))
                rep.add(r["n"], "dQ", _norm(less["dQ"] - full["dQ"]) / np.maximum(_norm(ref64["dQ"][i]), floor["dQ"]))
                for nm in ("dK", "dV"):                   # column j loses the term row i added to it
                    rep.add(r["n"], nm, _norm(full[nm][at]) / np.maximum(_norm(ref64[nm][j]), floor[nm]))
    return rep.done()


def _power_gat(name, h, f):
    g = dc.graph(name)
    x, ref64, _, bounds = dc.gat_references(name, h, f)
    assert all(bounds[k] > 0 for k in dc.GAT_NAMES)
    ar, ac, X, dO = (x[k].astype(np.float64) for k in ("attn_row", "attn_col", "X", "dO"))
    floor = {k: pc.floor_of(ref64[k]) for k in ref64}
    rep = _Report(f"gat {name} h={h} f={f}", bounds)
    for r in g["ranges"]:
        probes = r["probes"]
        for i in probes:
            lo, hi, cols = dc._row(g, i)
            full = dc.gat_row(ar[i], ac[cols], X[cols], dO[i])
            for nm, ref in (("out", "out"), ("out", "inference"), ("edge_sum", "edge_sum"), ("grad_attn_row", "grad_attn_row")):
                _same(full[nm], ref64[ref][i], ref)
            for at in np.nonzero(np.isin(cols, probes))[0]:
                c = cols[np.arange(hi - lo) != at]
                less = dc.gat_row(ar[i], ac[c], X[c], dO[i])
                j = cols[at]
                for nm in ("out", "inference"):
                    rep.add(r["n"], nm, _norm(less["out"] - full["out"]) / np.maximum(_norm(ref64[nm][i]), floor[nm]))
                mx = np.abs(less["edge_max"] - full["edge_max"]) / np.maximum(np.abs(full["edge_max"]), floor["edge_max"])
                rep.add(r["n"], "edge_sum", np.abs(less["edge_sum"] - full["edge_sum"])
                        / np.maximum(np.abs(full["edge_sum"]), floor["edge_sum"]), with_max=("edge_max", mx))
                rep.add(r["n"], "grad_attn_row", np.abs(less["grad_attn_row"] - full["grad_attn_row"])
                        / np.maximum(np.abs(ref64["grad_attn_row"][i]), floor["grad_attn_row"]))
                rep.add(r["n"], "grad_feat", _norm(full["grad_feat"][at])
                        / np.maximum(_norm(ref64["grad_feat"][j]), floor["grad_feat"]))
                rep.add(r["n"], "grad_attn_col", np.abs(full["grad_attn_col"][at])
                        / np.maximum(np.abs(ref64["grad_attn_col"][j]), floor["grad_attn_col"]))
    return rep.done()


def _padding(g, row_max, row_sum, bound, what):
    rows = dc.padded_rows(g)
    rows = rows[np.diff(g["row_ptr"])[rows] > 0]
    share = np.exp(-row_max[rows]) / row_sum[rows]
    print(f"padding {what}: least exp(-max) / sum {share.min():.3e}, bound {bound:.3e}, ratio {share.min() / bound:.0f}")
    assert (share >= pc.POWER * bound).all(), (what, float(share.min()), bound)


@pytest.mark.parametrize("name,h,f,unit_val", GT_CASES, ids=str)
def test_power_and_padding_gt(oracle_mod, name, h, f, unit_val):
    _power_gt(name, h, f, unit_val)
    _, ref64, _, bounds = dc.gt_references(name, h, f, unit_val)
    _padding(dc.graph(name), ref64["row_max"], ref64["row_sum"], bounds["row_sum"], f"gt {name} h={h} f={f} unit_val={unit_val}")


@pytest.mark.parametrize("name,h,f", GAT_CASES, ids=str)
def test_power_and_padding_gat(oracle_mod, name, h, f):
    _power_gat(name, h, f)
    _, ref64, _, bounds = dc.gat_references(name, h, f)
    _padding(dc.graph(name), ref64["edge_max"], ref64["edge_sum"], bounds["edge_sum"], f"gat {name} h={h} f={f}")
