"""GPU: the native neighbour sampler (include/dfgnn_sample.h, csrc/sample.hip) against its definition
(DFGNN.utils.graph.sample_block_reference).  Every array is an integer array and must be torch.equal to the reference: no
tolerances.  Every call runs on a stream that is not the default one."""
import ctypes
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import sample_cases as C
from conftest import ROOT
from guarded import Arena

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EDGE = ("parent_edge", "col_ind", "rows", "row_ind", "val_idx")


@functools.lru_cache(maxsize=None)
def _boundary_on_device():
    return tuple(torch.from_numpy(a).to(DEV) for a in C.boundary_graph())


def _reference(row_ptr, col_ind, seeds, fanout, seed):
    from DFGNN.utils import sample_block_reference
    return sample_block_reference(torch.as_tensor(row_ptr), torch.as_tensor(col_ind), torch.as_tensor(seeds), fanout, seed)


def _native(row_ptr, col_ind, seeds, fanout, seed, csc=True):
    """dfgnn_preprocess.sample_hop on a side stream -> dict of CPU tensors."""
    import dfgnn_preprocess
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    with torch.cuda.stream(side):
        out = dfgnn_preprocess.sample_hop(row_ptr, col_ind, seeds, fanout, seed, csc=csc)
    side.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _compare(got, want, csc, what):
    names = [n for n in C.ARRAYS if csc or n not in ("col_ptr", "row_ind", "val_idx")]
    assert sorted(got) == sorted(names), what
    for name in names:
        assert got[name].dtype == torch.int32 and got[name].shape == want[name].shape, (what, name, got[name].shape)
        assert torch.equal(got[name], want[name]), (what, name)


# ---- the boundary graph ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", C.MS)
def test_boundary_graph(m):
    """Degrees on both sides of every fanout of the list and of the wave width, m on both sides of a workgroup's 32 rows and
    of the bitmap words; every fanout x every seed, with the CSC half and without."""
    row_ptr, col_ind = _boundary_on_device()
    host = C.boundary_graph()
    seeds = C.seeds_for(m)
    dseeds = torch.from_numpy(seeds).to(DEV)
    for fanout in C.FANOUTS:
        for seed in C.SEEDS:
            want = _reference(*host, seeds, fanout, seed)
            for csc in (True, False):
                _compare(_native(row_ptr, col_ind, dseeds, fanout, seed, csc), want, csc, (m, fanout, seed, csc))


def test_boundary_graph_matches_the_loop():
    """One case straight against the plain per-row loop, so that the device does not only agree with the vectorised code."""
    row_ptr, col_ind = _boundary_on_device()
    seeds = C.seeds_for(257)
    want = C.loop_reference(*C.boundary_graph(), seeds, 25, 1)
    got = _native(row_ptr, col_ind, torch.from_numpy(seeds).to(DEV), 25, 1)
    for name in C.ARRAYS:
        assert np.array_equal(got[name].numpy(), want[name]), name


# ---- degenerate graphs ----------------------------------------------------------------------------------------------------
def test_every_seed_of_degree_zero():
    n, m = 100, 37
    row_ptr = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    col_ind = torch.zeros(0, dtype=torch.int32, device=DEV)
    seeds = torch.from_numpy(C.seeds_for(m, n)).to(DEV)
    got = _native(row_ptr, col_ind, seeds, 5, 3)
    assert all(got[k].numel() == 0 for k in EDGE)
    assert torch.equal(got["row_ptr"], torch.zeros(m + 1, dtype=torch.int32))
    assert torch.equal(got["col_nodes"], seeds.cpu()) and torch.equal(got["col_ptr"], torch.zeros(m + 1, dtype=torch.int32))
    # ... and in a graph that does have edges, none of them at the seeds
    row_ptr, col_ind = _boundary_on_device()
    host = C.boundary_graph()
    empty = np.flatnonzero(np.diff(host[0]) == 0).astype(np.int32)
    got = _native(row_ptr, col_ind, torch.from_numpy(empty).to(DEV), 5, 3)
    _compare(got, _reference(*host, empty, 5, 3), True, "empty rows")
    assert got["col_ind"].numel() == 0 and got["col_nodes"].numel() == empty.size and int(got["col_ptr"].abs().sum()) == 0


def test_one_node_with_a_self_loop():
    row_ptr = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    col_ind = torch.tensor([0], dtype=torch.int32, device=DEV)
    seeds = torch.tensor([0], dtype=torch.int32, device=DEV)
    for csc in (True, False):
        got = _native(row_ptr, col_ind, seeds, 1, 9, csc)
        _compare(got, _reference(row_ptr.cpu(), col_ind.cpu(), seeds.cpu(), 1, 9), csc, "n = 1")
        assert got["col_nodes"].tolist() == [0] and got["col_ind"].tolist() == [0] and got["parent_edge"].tolist() == [0]


def test_no_seeds():
    row_ptr, col_ind = _boundary_on_device()
    got = _native(row_ptr, col_ind, torch.zeros(0, dtype=torch.int32, device=DEV), 5, 1)
    assert got["row_ptr"].tolist() == [0] and got["col_ptr"].tolist() == [0]
    assert all(got[k].numel() == 0 for k in EDGE + ("col_nodes",))
    from DFGNN.utils import sample_block_fused
    block, nodes = sample_block_fused(row_ptr, col_ind, torch.zeros(0, dtype=torch.int64, device=DEV), 5, seed=1)
    assert (block.num_rows(), block.num_cols(), block.num_edges(), nodes.numel()) == (0, 0, 0, 0)


# ---- two hops, a mid-size graph -------------------------------------------------------------------------------------------
def test_two_hops():
    row_ptr, col_ind = _boundary_on_device()
    host = C.boundary_graph()
    seeds = C.seeds_for(63)
    first = _native(row_ptr, col_ind, torch.from_numpy(seeds).to(DEV), 5, 21)
    _compare(first, _reference(*host, seeds, 5, 21), True, "hop 1")
    nodes = first["col_nodes"]
    assert nodes.numel() > 63
    second = _native(row_ptr, col_ind, nodes.to(DEV), 25, 22)
    _compare(second, _reference(*host, nodes, 25, 22), True, "hop 2")
    assert torch.equal(second["col_nodes"][:nodes.numel()], nodes)


def test_mid_size():
    """n = 20000, mean degree 200, m = 4096, fanout 25: thousands of workgroups of either row form (the Poisson degrees put
    rows on both sides of the fanout only at a larger one, so 190 runs too)."""
    host = C.random_graph(20000, 200, 7)
    row_ptr, col_ind = (torch.from_numpy(a).to(DEV) for a in host)
    seeds = C.seeds_for(4096, 20000)
    for fanout, seed in ((25, 5), (190, 6)):
        deg = np.diff(host[0])[seeds]
        assert (deg > fanout).any() and (fanout == 25 or (deg <= fanout).any())
        got = _native(row_ptr, col_ind, torch.from_numpy(seeds).to(DEV), fanout, seed)
        _compare(got, _reference(*host, seeds, fanout, seed), True, ("mid", fanout))


# ---- guarded buffers ------------------------------------------------------------------------------------------------------
def _ints(a):
    """int32 values in a float32 tensor, bit for bit: the arena shifts float views one element off a 16-byte boundary."""
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).view(torch.float32)


@pytest.mark.parametrize("csc", (True, False))
@pytest.mark.parametrize("case", ("boundary", "no_edges"))
def test_guarded_buffers(case, csc):
    """The two entries on arenas: every output written in full and only there, inputs unchanged, the workspace exactly
    dfgnn_sample_ws_bytes large, shared by the two calls and not refilled between them; every int array starts one element
    after a 16-byte boundary."""
    import dfgnn_native
    L = dfgnn_native.lib()
    fanout, seed = 25, 0xFFFFFFFF
    if case == "boundary":
        row_ptr, col_ind = C.boundary_graph()
        seeds = C.seeds_for(257)
    else:
        row_ptr, col_ind = np.zeros(778, dtype=np.int32), np.zeros(0, dtype=np.int32)
        seeds = C.seeds_for(65)
    n, m = row_ptr.size - 1, seeds.size
    want = _reference(row_ptr, col_ind, seeds, fanout, seed)
    size = ctypes.c_size_t(0)
    assert L.dfgnn_sample_ws_bytes(n, m, fanout, ctypes.addressof(size)) == 0
    arena = Arena(DEV, shift=1)
    # (an empty array has no address to guard: a parent without edges passes col_ind = NULL, a block without edges its
    # per-edge outputs)
    rp = arena.input("parent_row_ptr", _ints(row_ptr))
    ci = arena.input("parent_col_ind", _ints(col_ind)) if col_ind.size else None
    sd = arena.input("seeds", _ints(seeds))
    ws = arena.scratch("ws", size.value, dtype=torch.uint8, aligned=True)
    brp, counts = arena.output("blk_row_ptr", (m + 1,)), arena.output("counts", (2,))
    assert rp.data_ptr() % 16 == 4 and brp.data_ptr() % 16 == 4 and ws.data_ptr() % 256 == 0
    side = torch.cuda.Stream(DEV)
    side.wait_stream(torch.cuda.current_stream(DEV))
    ptr = lambda t: t.data_ptr() if t is not None else None  # noqa: E731
    with torch.cuda.device(DEV):
        rc = L.dfgnn_sample_select(n, m, fanout, seed, rp.data_ptr(), ptr(ci), sd.data_ptr(), brp.data_ptr(), counts.data_ptr(),
                                   ws.data_ptr(), size.value, side.cuda_stream)
    assert rc == 0
    side.synchronize()
    arena.verify()
    nnz_b, n_cols_b = counts.view(torch.int32).tolist()
    assert (nnz_b, n_cols_b) == (want["col_ind"].numel(), want["col_nodes"].numel())
    per_edge = (lambda k: arena.output(k, (nnz_b,))) if nnz_b else (lambda k: None)  # noqa: E731
    outs = {k: per_edge(k) for k in EDGE[:3]}
    outs["col_nodes"] = arena.output("col_nodes", (n_cols_b,))
    if csc:
        outs["col_ptr"] = arena.output("col_ptr", (n_cols_b + 1,))
        outs.update({k: per_edge(k) for k in EDGE[3:]})
    arg = lambda k: ptr(outs.get(k))  # noqa: E731
    with torch.cuda.device(DEV):
        rc = L.dfgnn_sample_emit(n, m, fanout, nnz_b, n_cols_b, rp.data_ptr(), ptr(ci), sd.data_ptr(), brp.data_ptr(),
                                 arg("parent_edge"), arg("col_ind"), arg("rows"), arg("col_nodes"), arg("col_ptr"),
                                 arg("row_ind"), arg("val_idx"), ws.data_ptr(), size.value, side.cuda_stream)
    assert rc == 0
    side.synchronize()
    arena.verify()
    got = {k: v.view(torch.int32).cpu() if v is not None else torch.zeros(0, dtype=torch.int32) for k, v in outs.items()}
    got["row_ptr"] = brp.view(torch.int32).cpu()
    _compare(got, want, csc, (case, csc))


# ---- through the layers ---------------------------------------------------------------------------------------------------
def test_through_the_layers():
    """sample_block_fused -> preprocess_block -> SparseMHA_rowstats, forward and backward, against the same layer on
    preprocess_block(Block(src, dst, m, n_cols)) of the same edges: the same arrays into the same kernels, so equal bits."""
    from DFGNN.layers import SparseMHA_rowstats, preprocess_block
    from DFGNN.utils import Block, SampledBlock, sample_block_fused
    row_ptr, col_ind = _boundary_on_device()
    seeds = torch.from_numpy(C.seeds_for(257)).to(DEV).long()
    block, col_nodes = sample_block_fused(row_ptr, col_ind, seeds, 25, generator=torch.Generator().manual_seed(1))
    assert isinstance(block, SampledBlock) and col_nodes.dtype == torch.int64 and col_nodes.is_cuda
    assert torch.equal(col_nodes[:257], seeds)
    src, dst = block.edges()
    mine = preprocess_block(block)
    theirs = preprocess_block(Block(src, dst, block.num_rows(), block.num_cols()).to(DEV))
    assert mine[8] == theirs[8] and mine[0].shape == theirs[0].shape
    assert torch.equal(mine[0].row, theirs[0].row) and torch.equal(mine[0].col, theirs[0].col)
    for k in range(1, 8):
        assert mine[k].dtype == theirs[k].dtype and torch.equal(mine[k], theirs[k]), k
    torch.manual_seed(0)
    layer = SparseMHA_rowstats(16, 24, 1).to(DEV).train()
    h0 = torch.randn(block.num_cols(), 16, device=DEV)
    results = []
    for params in (mine, theirs):
        h = h0.clone().requires_grad_(True)
        layer.zero_grad()
        out = layer(params, (h, h[:257]), fuse=True)
        out.square().sum().backward()
        results.append([out.detach(), h.grad] + [p.grad.clone() for p in layer.parameters()])
    torch.cuda.synchronize()
    assert results[0][0].shape == (257, 24) and bool(results[0][1].abs().sum() > 0)
    for a, b in zip(*results):
        assert torch.equal(a, b)


def test_train_sampled_with_the_native_sampler():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "train_sampled.py"), "--sampler", "native", "--steps", "2",
                          "--warmup", "1", "--iters", "2", "--repeats", "1", "--scale", "0.02"], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert [ln["what"] for ln in lines] == ["losses", "sampling", "preprocessing", "step", "conv_pairs"]
    assert all(ln["sampler"] == "native" for ln in lines)
    losses = lines[0]
    assert np.isfinite(losses["fused"]) and losses["fused"] == losses["index_ops"], losses
