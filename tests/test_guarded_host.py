"""Host tests of the guarded-buffer run (tests/guarded.py, tests/guarded_cases.py; the run itself is tests/test_gpu_guarded.py):
the helper catches each planted fault on CPU tensors and names the buffer; every stream-taking entry of include/dfgnn.h is in
the table; the case set has the geometry at which a grid cap or a tail loop goes wrong; the argument builder produces an
argument list for every entry of the pairs' table that agrees with the ctypes signature."""
import os

import numpy as np
import pytest
import torch

import guarded
import guarded_cases as gc
import rect_cases as rc

CPU = "cpu"


# ---- 1. the helper, on stand-in kernels -----------------------------------------------------------------------------------
def _setup(shift=0):
    """out[i] = 2 x[idx[i]] on guarded buffers -> (arena, x, idx, out)."""
    a = guarded.Arena(CPU, shift=shift)
    x = a.input("x", np.arange(1, 41, dtype=np.float32).reshape(10, 4))
    idx = a.input("idx", np.array([3, 0, 9, 9, 1], dtype=np.int32))
    out = a.output("out", (5, 4))
    a.scratch("ws", 33, aligned=True)
    return a, x, idx, out


def _correct(x, idx, out):
    out.copy_(2 * x[idx.long()])


def _flat(a, name):
    """The buffer around view `name` and the view's first offset in it (what a kernel with a wrong index reaches)."""
    r = a.records[name]
    return r.buf, r.lo, r.n


@pytest.mark.parametrize("shift", [0, 1])
def test_correct_stand_in_passes(shift):
    a, x, idx, out = _setup(shift)
    _correct(x, idx, out)
    assert a.verify(outputs=["out"], scratch=["ws"], inputs=["x", "idx"]) == 4 == len(a)
    assert a.verify() == 4
    assert torch.equal(out, 2 * x[idx.long()])
    assert x.data_ptr() % 16 == out.data_ptr() % 16 == 4 * shift and a["ws"].data_ptr() % 16 == 0 and idx.data_ptr() % 16 == 0


def _write_before(a, x, idx, out):
    _correct(x, idx, out)
    buf, lo, n = _flat(a, "out")
    buf[lo - 1] = 1.0


def _write_after(a, x, idx, out):
    _correct(x, idx, out)
    buf, lo, n = _flat(a, "out")
    buf[lo + n] = 0.0


def _slot_unwritten(a, x, idx, out):
    out[:4].copy_(2 * x[idx.long()[:4]])
    out[4, :3].copy_(2 * x[1, :3])                         # the last element of the last row is never stored


def _accumulate(a, x, idx, out):
    out.add_(2 * x[idx.long()])                            # += into memory nobody zeroed


def _modify_input(a, x, idx, out):
    _correct(x, idx, out)
    x[9, 3] = -x[9, 3]


def _leak_input_guard(a, x, idx, out):
    _correct(x, idx, out)
    buf, lo, n = _flat(a, "x")
    out[2, 0] = 2 * x[9, 3] + 0 * buf[lo + n]              # a masked lane: one element past x, times zero


def _scratch_overrun(a, x, idx, out):
    _correct(x, idx, out)
    buf, lo, n = _flat(a, "ws")
    buf[lo + n + 5] = 0.0


def _int_output_unwritten(a, x, idx, out):
    _correct(x, idx, out)
    a.output("count", (3,), torch.int32)[:2] = 7


FAULTS = [(_write_before, r"^out: guard before the output written at offset -1$"),
          (_write_after, r"^out: guard after the output written at offset 20 "),
          (_slot_unwritten, r"^out: output element at offset 19 of 20 still carries the fill \(1 unwritten\)$"),
          (_accumulate, r"^out: output element at offset 0 of 20 (still carries the fill|is not finite)"),
          (_modify_input, r"^x: input modified at offset 39 of 40$"),
          (_leak_input_guard, r"^out: output element at offset 8 of 20 (still carries the fill|is not finite)"),
          (_scratch_overrun, r"^ws: guard after the scratch written at offset 38 "),
          (_int_output_unwritten, r"^count: output element at offset 2 of 3 still carries the fill")]


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("fault,message", FAULTS, ids=[f.__name__[1:] for f, _ in FAULTS])
def test_planted_fault_is_caught_and_named(fault, message, shift):
    a, x, idx, out = _setup(shift)
    fault(a, x, idx, out)
    with pytest.raises(AssertionError, match=message):
        a.verify()


def test_fill_is_told_from_a_computed_nan_and_integer_guards_are_zero():
    """A NaN the stand-in computes is reported as not finite, not as unwritten; the guards of an integer input hold 0 (a
    leaked index gathers row 0), those of a float input the fill; an optional output passed as NULL is not listed."""
    a, x, idx, out = _setup()
    _correct(x, idx, out)
    out[1, 1] = float("nan")
    with pytest.raises(AssertionError, match=r"^out: output element at offset 5 of 20 is not finite"):
        a.verify()
    out[1, 1] = -1e38                                      # the operators' sentinel is finite
    a.verify()
    buf, lo, n = _flat(a, "idx")
    assert buf.dtype == torch.int32 and int(buf[:lo].abs().max()) == 0 == int(buf[lo + n:].abs().max()) and lo >= guarded.GUARD
    buf, lo, n = _flat(a, "x")
    assert (buf.view(torch.int32)[:lo] == guarded.FILL_BITS).all() and torch.isnan(buf[:lo]).all() and lo >= guarded.GUARD
    a.output("optional", (7,))
    a.verify(outputs=["out"])
    with pytest.raises(AssertionError, match="^optional: output element at offset 0 of 7 still carries the fill"):
        a.verify()
    with pytest.raises(AssertionError, match="ws is recorded as scratch"):
        a.verify(outputs=["ws"])


# ---- 2. completeness ------------------------------------------------------------------------------------------------------
def test_every_stream_taking_entry_is_in_the_table():
    """include/dfgnn.h's entries whose last parameter is `dfgnn_stream_t stream` = the GPU test's table + the two entries of
    tests/test_gpu_stats_pair.py's guard test.  A new C entry fails here until a family's test calls it."""
    import dfgnn_native
    launching = guarded.stream_entries(gc.protos())
    assert len(launching) == 70, len(launching)
    assert set(gc.EXCLUDED) == {"dfgnn_gt_hyper_fwd_stats", "dfgnn_gt_bwd_stats"}
    assert not set(gc.EXCLUDED) & set(gc.TABLE)
    assert sorted(set(gc.TABLE) | set(gc.EXCLUDED)) == launching, sorted(set(launching) ^ (set(gc.TABLE) | set(gc.EXCLUDED)))
    for entry in launching:                                 # the parsed prototype agrees with the ctypes signature
        assert len(gc.protos()[entry]) == len(dfgnn_native.SIGNATURES[entry]), entry
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_stats_pair.py")).read()
    assert "def test_stats_kernels_write_nothing_outside_their_outputs" in src
    assert all(e in src for e in gc.EXCLUDED)


def test_a_new_prototype_or_a_dropped_row_is_noticed():
    text = open(gc.HEADER).read()
    more = text.replace("#ifdef __cplusplus\n}", "int dfgnn_new_conv(int m, const float *X, float *out,\n"
                        "                   dfgnn_stream_t stream);\n#ifdef __cplusplus\n}", 1)
    assert "dfgnn_new_conv" in guarded.stream_entries(guarded.prototypes(more))
    assert guarded.prototypes(more)["dfgnn_new_conv"][1:3] == [("const float *", "X"), ("float *", "out")]
    fewer = dict(gc.TABLE)
    del fewer["dfgnn_gat_attn_scores"]
    assert sorted(set(fewer) | set(gc.EXCLUDED)) != guarded.stream_entries(gc.protos())


# ---- 3. case geometry -----------------------------------------------------------------------------------------------------
def test_case_geometry():
    """For a lane group per row (column) and for a wave per row (column): a graph whose last row (column) has an odd number
    of entries and one whose last row (column) is empty.  The typed cases have T h f, the tbias cases T h, off a multiple of
    64 at one width at least."""
    found = {}
    for kind in gc.RECT_KINDS + gc.SQUARE_KINDS:
        for key in gc.geometry(gc.graph(kind)):
            found.setdefault(key, []).append(kind)
    want = {(side, form, what) for side in ("rows", "cols") for form in ("lane", "wave") for what in ("odd", "empty")}
    assert want <= set(found), sorted(want - set(found))
    for kind in gc.SQUARE_KINDS:
        g = gc.graph(kind)
        assert g["m"] == g["n_cols"]
    assert any((gc.TYPES * h * f) % 64 for h, f in gc.WIDTHS) and any((gc.TYPES * h) % 64 for h, f in gc.WIDTHS)
    assert set(rc.WIDTHS) | {(1, 100), (2, 130)} == set(gc.WIDTHS) and gc.SHIFT_WIDTH in gc.WIDTHS


# ---- 4. the argument builder ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", sorted(gc.PAIRS))
def test_argument_lists_of_the_pairs(pair):
    """On CPU tensors: for each of the pair's four entries and both variants the builder fills every parameter of the
    header's prototype -- pointers for what is given, NULL for what is omitted -- and a stand-in that writes every output
    in full passes verify; the float64 reference has every output under the header's name and shape."""
    g = gc.graph("sq_wave_empty")
    h, f = 2, 20
    for which in ("full", "min") if gc.has_variants(pair) else ("full",):
        x, scal, fo, bo = gc.variant(pair, which, gc.inputs(pair, g, h, f, False), f)
        ref = gc.reference(pair, g, x, scal)
        base = dict(m=g["m"], n_cols=g["n_cols"], nnz=g["nnz"], h=h, f=f, stream=None, ws_numel=64, **scal)
        base.update({k: g[k] for k in ("row_ptr", "col_ind", "col_ptr", "row_ind", "val_idx")})
        base.update(x)
        stats = {k: ref[k].astype(np.float32) for k in ("out",) + gc.stats_of(pair)}
        for rect in (False, True):
            for entry, omit, extra in ((gc.PAIRS[pair][0], fo, {}), (gc.PAIRS[pair][1], bo, stats)):
                entry += "_rect" if rect else ""
                call = gc.Call(entry, dict(base, **extra), CPU, shift=1, omit=omit)
                assert len(call.args) == len(gc.protos()[entry])
                for (ctype, name), arg in zip(gc.protos()[entry], call.args):
                    if name in omit or name == "stream" or (name in x and x[name] is None):
                        assert arg is None, (entry, name)
                    else:
                        assert arg is not None, (entry, name)
                for name, view in call.outputs.items():
                    assert tuple(view.shape) == ref[name].shape, (entry, name)
                    view.copy_(torch.from_numpy(ref[name]).float())
                assert call.arena.verify(outputs=list(call.outputs)) == len(call.arena)
                assert set(call.outputs).isdisjoint(omit)
