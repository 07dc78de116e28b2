"""The condition that keeps the fp32-level bound of tests/parity_cases.py honest, proved on the CPU for every case that
tests/test_gpu_edge_exact.py runs: losing ONE boundary edge -- the last or the first CSR edge of every test row, on the
transposed cases the last or the first CSC entry of every test column -- moves every checked output of every affected
row or column by at least POWER x bound in the measure of parity_cases, where bound = MARGIN x the plain-fp32
reference's own error.  A case that does not meet it needs other inputs, not another factor.

Not under the condition: the row maxima (row_max / edge_max).  A maximum is no sum -- a lost edge moves it only when it
was the row's argmax, and both ends of a row cannot be that at once; the sums and `out` taken relative to it are under
the condition.  The structural facts the GPU cases rely on (form, degree list, aligned blocks, sentinels) are asserted
here as well."""
import numpy as np
import pytest

import parity_cases as pc

ISSUE_DEGREES = [1, 2, 3, 15, 16, 17, 23, 24, 25, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1023,
                 1024, 1025, 2047, 2048, 2049, 4095, 4096, 4097]
NOT_UNDER_CONDITION = ("row_max", "edge_max")
SEEN = set()


def test_caps_and_degree_list():
    caps = pc.caps()
    assert caps == dict(kGroupMaxDegree=24, kRowCap=1024, kCsrRowCap=2048, kHyperCap=4096)   # else: the list below moves
    assert pc.degree_list() == ISSUE_DEGREES
    for c in caps.values():
        assert {c - 1, c, c + 1} <= set(pc.degree_list())


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("low", [False, True])
def test_structure(transposed, low):
    g = pc.graph(transposed, low)
    m, nnz, R = g["m"], g["nnz"], g["R"]
    assert (nnz < 8 * m) == low                                     # the form the kernels take
    assert 8 * (m - 1) <= nnz if low else m < 400                   # padded no further than needed / a few hundred nodes
    assert nnz <= 60_000
    deg = np.diff(g["row_ptr"]).astype(np.int64)
    indeg = np.bincount(g["col_ind"], minlength=m)
    mine = indeg if transposed else deg
    assert list(mine[:len(ISSUE_DEGREES)]) == ISSUE_DEGREES         # the exact degree list, in order, from node 0
    cap = pc.caps()["kHyperCap"]
    (a0, da), (b0, db) = pc.block_rows()
    assert a0 % 16 == 0 and b0 == a0 + 16 and R == b0 + 16
    assert mine[a0:a0 + 16].sum() == cap == sum(da) and mine[b0:b0 + 16].sum() == cap + 1 == sum(db)
    # sentinels: one column (transposed: row) of their own per end of every test row (degree 1: its one edge)
    has = np.nonzero(g["deg"] >= 2)[0]
    assert len(g["sent_node"]) == R + len(has) == len(set(g["sent_node"])) and len(has) == R - 1
    assert len(g["mutate"]) == (R if transposed else R - 2)
    if transposed:
        assert (deg[g["sent_node"]] == 2).all() and (deg[:R] == 0).all()
        # CSC order: the first sentinel's entry opens the column's segment, the last one's closes it
        first = g["row_ind"][g["col_ptr"][has]]
        last = g["row_ind"][g["col_ptr"][has + 1] - 1]
        assert (first == R + has).all() and (last == 2 * R + pc.POOL + has).all()
    else:
        assert (indeg[g["sent_node"]] == 1).all()
        assert (g["col_ind"][g["row_ptr"][has]] == R + has).all()
        assert (g["col_ind"][g["row_ptr"][has + 1] - 1] == 2 * R + pc.POOL + has).all()
    assert (deg[m - 1] == 0 and indeg[m - 1] == 0) if low else True
    lo, hi = g["pool"][0], g["pool"][-1]
    assert lo < 192 <= hi                                           # chunk_rows = 192 (chunked GAT tiling) splits the pool


def _mutated_inputs(op, x, keep):
    if op != "gt":
        return x
    y = dict(x)
    y["val"] = x["val"][keep]
    return y


def _power(op, case):
    g = pc.graph(case[0], case[1])
    x, ref64, ref32, bounds = pc.references(op, *case)
    names = (pc.COL_SIDE if g["transposed"] else pc.ROW_SIDE)[op]
    report = {}
    for mut, slots in pc.mutations(g).items():
        assert len(slots) == len(g["mutate"]) > 0
        row_ptr, col_ind, keep = pc.drop_slots(g, slots)
        assert keep.sum() == g["nnz"] - len(slots)
        moved = pc._REFERENCE[op](row_ptr, col_ind, _mutated_inputs(op, x, keep), "f64")
        for name in names:
            if name in NOT_UNDER_CONDITION:
                continue
            if name == "attn_edge":              # the edges that stay, grouped by the rows of the mutated graph
                e = pc.row_errors(moved[name], ref64[name][:, keep], row_ptr, floor=pc.floor_of(ref64[name], g["row_ptr"]))
            else:
                e = pc.row_errors(moved[name], ref64[name])
            e = e if name == "dattn" else e[g["mutate"]]
            fp32 = bounds[name] / pc.MARGIN
            assert fp32 > 0, (op, case, name)
            report[(mut, name)] = (float(e.min()), bounds[name], float(e.min()) / fp32)
    for (mut, name), (move, bound, ratio) in report.items():
        print(f"power {op} {case} {mut} {name}: least move {move:.3e}, bound {bound:.3e}, move / fp32 error {ratio:.1f}")
    for (mut, name), (move, bound, ratio) in report.items():
        assert move >= pc.POWER * bound, (op, case, mut, name, move, bound)


@pytest.mark.parametrize("case", pc.case_ids("gt"), ids=str)
def test_power_gt(oracle_mod, case):
    _power("gt", case)
    SEEN.add(("gt", case))


@pytest.mark.parametrize("case", pc.case_ids("gat"), ids=str)
def test_power_gat(oracle_mod, case):
    _power("gat", case)
    SEEN.add(("gat", case))


@pytest.mark.parametrize("case", pc.case_ids("gatv2"), ids=str)
def test_power_gatv2(case):
    _power("gatv2", case)
    SEEN.add(("gatv2", case))


def test_zz_no_case_was_skipped(request):
    """Runs last in this module: every case of every operator went through the condition (when the whole module ran)."""
    wanted = {(op, c) for op in ("gt", "gat", "gatv2") for c in pc.case_ids(op)}
    assert len(wanted) == 32 + 16 + 16        # 4 widths x {as built, transposed} x {wave, lane-group form} (GT: x 2 val)
    selected = [i.name for i in request.session.items if i.module is request.module and i.name.startswith("test_power")]
    if len(selected) == len(wanted):           # (a -k selection of single cases is not a skipped case)
        assert SEEN == wanted, sorted(wanted - SEEN)
