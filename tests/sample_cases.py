"""Shared cases of the neighbour-sampler tests (tests/test_sample_host.py on the CPU, tests/test_gpu_sample.py on the GPU):
the boundary graph, the seed sets, and a plain per-row restatement of include/dfgnn_sample.h's definition that shares no
code with DFGNN.utils.graph.sample_block_reference."""
import functools

import numpy as np

N = 777                      # a multiple of neither 32 nor 64
DEGREES = (0, 1, 2, 4, 5, 6, 24, 25, 26, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4097)
FANOUTS = (1, 5, 25, 64, 65, 300)
MS = (1, 63, 64, 65, 257, 777)
SEEDS = (0, 1, 0xFFFFFFFF)
ARRAYS = ("row_ptr", "parent_edge", "col_ind", "rows", "col_nodes", "col_ptr", "row_ind", "val_idx")
_SHIFT = 5                   # node i has degree DEGREES[(i + 5) % 20]: the last node has degree 1, its edge a self loop


@functools.lru_cache(maxsize=None)
def boundary_graph():
    """-> (row_ptr, col_ind) int32: degrees cycle through DEGREES; columns are random, with a self loop in every third row
    that has an edge, the first edge repeated in every fourth row of two edges or more, and plenty of columns that are other
    seeds (every node can be one).  Node N - 1 has one edge, to itself: whenever it is a seed -- seeds_for always makes it
    one -- it is a sampled neighbour too, the last bit of both bitmaps."""
    rng = np.random.default_rng(20251)
    deg = np.array([DEGREES[(i + _SHIFT) % len(DEGREES)] for i in range(N)], dtype=np.int64)
    assert deg[N - 1] == 1
    row_ptr = np.zeros(N + 1, dtype=np.int64)
    row_ptr[1:] = np.cumsum(deg)
    col = rng.integers(0, N, int(row_ptr[-1]))
    for i in range(N):
        s, d = int(row_ptr[i]), int(deg[i])
        if d >= 1 and i % 3 == 0:
            col[s + int(rng.integers(d))] = i
        if d >= 2 and i % 4 == 0:
            col[s + 1] = col[s]
    col[row_ptr[N - 1]] = N - 1
    return row_ptr.astype(np.int32), col.astype(np.int32)


def seeds_for(m, n=N, salt=0):
    """m distinct nodes in shuffled order, node n - 1 among them."""
    rng = np.random.default_rng(1000 * m + salt)
    picked = np.concatenate([rng.permutation(n - 1)[:m - 1], [n - 1]])
    return rng.permutation(picked).astype(np.int32)


def mix_scalar(x):
    x &= 0xFFFFFFFF
    x ^= x >> 16
    x = (x * 0x7FEB352D) & 0xFFFFFFFF
    x ^= x >> 15
    x = (x * 0x846CA68B) & 0xFFFFFFFF
    return x ^ (x >> 16)


def loop_reference(row_ptr, col_ind, seeds, fanout, seed):
    """The definition, row by row in plain Python: compute the keys, sort, take `fanout`, restore parent order; then the
    block's conventions and a stable column sort.  -> dict of int32 arrays named as ARRAYS."""
    ms = mix_scalar(int(seed))
    n, m = len(row_ptr) - 1, len(seeds)
    blk_row_ptr, parent_edge, rows = [0], [], []
    for r, s in enumerate(int(x) for x in seeds):
        ps = list(range(int(row_ptr[s]), int(row_ptr[s + 1])))
        if len(ps) > fanout:
            ps = sorted(sorted(ps, key=lambda p: mix_scalar(p ^ ms))[:fanout])
        parent_edge += ps
        rows += [r] * len(ps)
        blk_row_ptr.append(len(parent_edge))
    seed_row = {int(s): r for r, s in enumerate(seeds)}
    reached = [int(col_ind[p]) for p in parent_edge]
    others = sorted(set(c for c in reached if c not in seed_row))
    local = dict(seed_row)
    local.update({c: m + k for k, c in enumerate(others)})
    col = [local[c] for c in reached]
    by_col = sorted(range(len(col)), key=lambda e: col[e])      # (sorted is stable)
    n_cols = m + len(others)
    col_ptr = [0] * (n_cols + 1)
    for c in col:
        col_ptr[c + 1] += 1
    for c in range(n_cols):
        col_ptr[c + 1] += col_ptr[c]
    assert n >= 0
    out = dict(row_ptr=blk_row_ptr, parent_edge=parent_edge, col_ind=col, rows=rows, col_nodes=[int(s) for s in seeds] + others,
               col_ptr=col_ptr, row_ind=[rows[e] for e in by_col], val_idx=by_col)
    return {k: np.asarray(v, dtype=np.int32) for k, v in out.items()}


def random_graph(n, mean_degree, seed):
    """-> (row_ptr, col_ind) int32 of a graph with Poisson degrees and uniform columns."""
    rng = np.random.default_rng(seed)
    deg = rng.poisson(mean_degree, n)
    row_ptr = np.zeros(n + 1, dtype=np.int64)
    row_ptr[1:] = np.cumsum(deg)
    return row_ptr.astype(np.int32), rng.integers(0, n, int(row_ptr[-1])).astype(np.int32)
