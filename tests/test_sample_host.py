"""CPU: the neighbour sampler's definition (DFGNN.utils.graph.sample_block_reference = include/dfgnn_sample.h), its
conventions, the quality of its key function, its header and loader, and the hand-over to preprocess_block."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import sample_cases as C
from conftest import ROOT, csc_of
from DFGNN.layers import preprocess_block
from DFGNN.utils import Block, sample_block, sample_block_fused, sample_block_reference
from DFGNN.utils.graph import mix32, sample_keys

HEADER = os.path.join(ROOT, "include", "dfgnn_sample.h")


def _ref(row_ptr, col_ind, seeds, fanout, seed):
    return {k: v.numpy() for k, v in sample_block_reference(torch.from_numpy(row_ptr), torch.from_numpy(col_ind),
                                                            torch.from_numpy(seeds), fanout, seed).items()}


# ---- the definition -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fanout", C.FANOUTS)
def test_reference_equals_the_per_row_loop(fanout):
    row_ptr, col_ind = C.boundary_graph()
    seeds = C.seeds_for(C.N)
    want = C.loop_reference(row_ptr, col_ind, seeds, fanout, 1)
    got = _ref(row_ptr, col_ind, seeds, fanout, 1)
    assert sorted(got) == sorted(C.ARRAYS)
    for name in C.ARRAYS:
        assert got[name].dtype == np.int32 and np.array_equal(got[name], want[name]), name


@pytest.mark.parametrize("m", (1, 65, 777))
@pytest.mark.parametrize("fanout", C.FANOUTS)
def test_conventions(m, fanout):
    row_ptr, col_ind = C.boundary_graph()
    seeds = C.seeds_for(m)
    b = _ref(row_ptr, col_ind, seeds, fanout, 0xFFFFFFFF)
    deg = (row_ptr[seeds.astype(np.int64) + 1] - row_ptr[seeds]).astype(np.int64)
    assert np.array_equal(np.diff(b["row_ptr"]), np.minimum(deg, fanout)) and b["row_ptr"][0] == 0
    nnz = int(b["row_ptr"][-1])
    assert all(b[k].shape == (nnz,) for k in ("parent_edge", "col_ind", "rows", "row_ind", "val_idx"))
    assert np.array_equal(b["col_nodes"][:m], seeds)
    rest = b["col_nodes"][m:]
    assert np.all(np.diff(rest) > 0) and not np.intersect1d(rest, seeds).size
    assert np.array_equal(b["col_nodes"][b["col_ind"]], col_ind[b["parent_edge"]])
    assert np.array_equal(b["rows"], np.repeat(np.arange(m), np.diff(b["row_ptr"])))
    node = seeds[b["rows"]].astype(np.int64)
    assert np.all(b["parent_edge"] >= row_ptr[node]) and np.all(b["parent_edge"] < row_ptr[node + 1])
    same_row = b["rows"][1:] == b["rows"][:-1]
    assert np.all(np.diff(b["parent_edge"])[same_row] > 0)
    if m > 1:
        assert C.N - 1 in seeds and C.N - 1 in col_ind[b["parent_edge"]]      # the last bit of both bitmaps
    col_ptr, row_ind, val_idx = csc_of(b["row_ptr"], b["col_ind"], b["rows"], len(b["col_nodes"]))
    assert np.array_equal(b["col_ptr"], col_ptr) and np.array_equal(b["row_ind"], row_ind)
    assert np.array_equal(b["val_idx"], val_idx)


def test_ties_to_sample_block_when_every_edge_is_kept():
    row_ptr, col_ind = (torch.from_numpy(a) for a in C.boundary_graph())
    seeds = torch.from_numpy(C.seeds_for(257)).long()
    for fanout in (4097, 10 ** 6):
        old, old_nodes = sample_block(row_ptr, col_ind, seeds, fanout, torch.Generator().manual_seed(5))
        new, new_nodes = sample_block_fused(row_ptr, col_ind, seeds, fanout, seed=7)
        assert torch.equal(new_nodes, old_nodes) and new_nodes.dtype == torch.int64
        for a, b in zip(new.edges(), old.edges()):
            assert a.dtype == torch.int64 and torch.equal(a, b)
        assert (new.num_rows(), new.num_cols(), new.num_edges()) == (old.num_rows(), old.num_cols(), old.num_edges())


def test_seed_comes_from_the_generator():
    row_ptr, col_ind = (torch.from_numpy(a) for a in C.boundary_graph())
    seeds = torch.from_numpy(C.seeds_for(65))
    draw = lambda s: sample_block_fused(row_ptr, col_ind, seeds, 5, generator=torch.Generator().manual_seed(s))[0]  # noqa: E731
    a, b, c = draw(3), draw(3), draw(4)
    assert torch.equal(a.parent_edge, b.parent_edge) and not torch.equal(a.parent_edge, c.parent_edge)
    assert a.parent_edge.dtype == torch.int32


# ---- the key function -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("start", (0, 12345, 2 ** 31 - 100))
def test_spread_of_one_row(start):
    """One row of degree 20 at fanout 5 under seeds 0..3999: every edge is kept 1000 times +- 5 sigma, every pair of edges
    together 210.5 times +- 6 sigma."""
    d, fanout, trials = 20, 5, 4000
    keys = np.stack([sample_keys(start + np.arange(d), s) for s in range(trials)])
    kept = np.zeros((trials, d), dtype=np.int64)
    np.put_along_axis(kept, np.argsort(keys, axis=1)[:, :fanout], 1, axis=1)
    assert np.all(kept.sum(1) == fanout)
    edge = kept.sum(0)
    pair = (kept.T @ kept)[np.triu_indices(d, 1)]
    print(f"start {start}: edges {edge.min()}-{edge.max()}, pairs {pair.min()}-{pair.max()}")
    assert 860 <= edge.min() and edge.max() <= 1140
    assert 125 <= pair.min() and pair.max() <= 296


def test_mix_is_a_bijection_on_20_bits():
    x = np.arange(2 ** 20)
    assert np.unique(mix32(x)).size == 2 ** 20
    assert [int(v) for v in mix32(np.array([0, 1, 0xFFFFFFFF]))] == [C.mix_scalar(0), C.mix_scalar(1), C.mix_scalar(0xFFFFFFFF)]


def test_consecutive_seeds_overlap_like_independent_draws():
    d, fanout, trials = 100, 10, 2000
    keys = np.stack([sample_keys(777 + np.arange(d), s) for s in range(trials)])
    kept = np.zeros((trials, d), dtype=np.int64)
    np.put_along_axis(kept, np.argsort(keys, axis=1)[:, :fanout], 1, axis=1)
    overlap = (kept[1:] * kept[:-1]).sum(1).mean()
    print(f"mean overlap {overlap:.3f}")
    assert 0.85 <= overlap <= 1.15


# ---- header and loader ----------------------------------------------------------------------------------------------------
def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {name: [a for a in args.split(",") if a.strip() and a.strip() != "void"]
            for name, args in re.findall(r"\b(dfgnn_sample_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", text)}


def test_header_entries_are_exported_and_bound():
    import dfgnn_native
    declared = _declared()
    assert sorted(declared) == ["dfgnn_sample_abi_version", "dfgnn_sample_emit", "dfgnn_sample_select", "dfgnn_sample_ws_bytes"]
    assert sorted(dfgnn_native.SAMPLE_SIGNATURES) == sorted(declared)
    for name, args in declared.items():
        assert len(args) == len(dfgnn_native.SAMPLE_SIGNATURES[name]), name
    assert not set(dfgnn_native.SAMPLE_SIGNATURES) & set(dfgnn_native.SIGNATURES)
    hip = os.path.join(os.path.dirname(dfgnn_native.LIB_PATH), "libdfgnn_hip.so")
    for path in (dfgnn_native.LIB_PATH, hip):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        exported = {ln.split()[-1] for ln in out.splitlines()}
        assert not [n for n in declared if n not in exported], path
    needed = subprocess.run(["readelf", "-d", dfgnn_native.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert "amdhip" not in needed and "hsa" not in needed
    assert "#define DFGNN_SAMPLE_ABI_VERSION 1" in open(HEADER).read()
    assert dfgnn_native.lib().dfgnn_sample_abi_version() == 1
    assert dfgnn_native.lib().dfgnn_abi_version() == 11


def _ws_bytes(n, m, fanout):
    import dfgnn_native
    size = ctypes.c_size_t(0)
    rc = dfgnn_native.lib().dfgnn_sample_ws_bytes(n, m, fanout, ctypes.addressof(size))
    return rc, int(size.value)


def test_argument_errors():
    """Host-only calls: every check comes before the first use of the device, so NULL device pointers are enough."""
    import dfgnn_native
    L = dfgnn_native.lib()
    BAD, UNSUPPORTED = -1, -2
    assert L.dfgnn_sample_ws_bytes(10, 4, 3, None) == BAD
    for n, m, fanout in ((-1, 4, 3), (10, -1, 3), (10, 4, 0), (10, 4, -2), (0, 4, 3)):
        assert _ws_bytes(n, m, fanout)[0] == BAD, (n, m, fanout)
        assert L.dfgnn_sample_select(n, m, fanout, 0, *[None] * 6, 0, None) == BAD, (n, m, fanout)
        assert L.dfgnn_sample_emit(n, m, fanout, 0, max(m, 0), *[None] * 12, 0, None) == BAD, (n, m, fanout)
    for m, fanout in ((2 ** 16, 2 ** 15), (2 ** 30, 2), (1, 2 ** 31 - 1), (3, 2 ** 30)):
        want = UNSUPPORTED if m * fanout >= 2 ** 31 else BAD       # below the limit: on to the pointers, which are NULL
        assert _ws_bytes(2 ** 18, m, fanout)[0] == (UNSUPPORTED if want == UNSUPPORTED else 0), (m, fanout)
        assert L.dfgnn_sample_select(2 ** 18, m, fanout, 0, *[None] * 6, 0, None) == want, (m, fanout)
        assert L.dfgnn_sample_emit(2 ** 18, m, fanout, 0, m, *[None] * 12, 0, None) == want, (m, fanout)
    assert _ws_bytes(1000, 64, 5)[0] == 0 and _ws_bytes(1000, 2 ** 16, 2 ** 15 - 1)[0] == 0
    assert _ws_bytes(1000, 2 ** 31 - 1, 1)[0] == UNSUPPORTED       # m + 1 must be an int
    # NULL required pointers (valid extents), a negative output size, sizes select cannot have reported
    assert L.dfgnn_sample_select(10, 4, 3, 0, *[None] * 6, 0, None) == BAD
    assert L.dfgnn_sample_select(10, 0, 3, 0, *[None] * 6, 0, None) == BAD      # m == 0 still writes blk_row_ptr and counts
    assert L.dfgnn_sample_emit(10, 4, 3, 0, 4, *[None] * 12, 0, None) == BAD
    assert L.dfgnn_sample_emit(10, 4, 3, -1, 4, *[None] * 12, 0, None) == BAD
    assert L.dfgnn_sample_emit(10, 4, 3, 13, 4, *[None] * 12, 0, None) == BAD   # nnz_b > m * fanout
    assert L.dfgnn_sample_emit(10, 4, 3, 2, 3, *[None] * 12, 0, None) == BAD    # n_cols_b < m
    assert L.dfgnn_sample_emit(10, 4, 3, 2, 7, *[None] * 12, 0, None) == BAD    # n_cols_b > m + nnz_b
    assert L.dfgnn_sample_emit(10, 0, 3, 0, 0, *[None] * 12, 0, None) == 0      # m == 0, no CSC: nothing to write
    assert b"bad argument" in L.dfgnn_error_string(BAD) and b"unsupported" in L.dfgnn_error_string(UNSUPPORTED)


def test_ws_bytes_is_monotone():
    base = (20000, 4096, 25)
    rc, last = _ws_bytes(*base)
    assert rc == 0 and last >= 2 * 4 * ((base[0] + 31) // 32) + 4 * base[0] + 4 * base[1] + 4 * base[1] * base[2]
    assert _ws_bytes(10, 0, 3) == (0, 256)
    for axis in range(3):
        prev = 0
        for scale in (1, 2, 3, 5, 8, 13, 40):
            args = list(base)
            args[axis] = base[axis] * scale // 2 + 1
            rc, size = _ws_bytes(*args)
            assert rc == 0 and size >= prev and size % 256 == 0, (args, size, prev)
            prev = size


# ---- the hand-over to the layers ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fanout", (5, 300))
def test_preprocess_block_hands_the_arrays_on(fanout):
    row_ptr, col_ind = (torch.from_numpy(a) for a in C.boundary_graph())
    seeds = torch.from_numpy(C.seeds_for(257))
    block, col_nodes = sample_block_fused(row_ptr, col_ind, seeds, fanout, seed=11)
    src, dst = block.edges()
    got = preprocess_block(block)
    want = preprocess_block(Block(src, dst, block.num_rows(), block.num_cols()))
    assert len(got) == len(want) == 9 and got[8] == want[8]
    for a, b in ((got[0].row, want[0].row), (got[0].col, want[0].col), (got[0].val, want[0].val)):
        assert a.dtype == b.dtype and torch.equal(a, b)
    assert got[0].shape == want[0].shape == (257, col_nodes.numel())
    for k in range(1, 8):
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    assert got[2] is block.row_ptr and got[7] is block.val_idx      # handed on, not rebuilt
    ref = sample_block_reference(row_ptr, col_ind, seeds, fanout, 11)
    assert torch.equal(block.parent_edge, ref["parent_edge"]) and torch.equal(col_nodes, ref["col_nodes"].long())
