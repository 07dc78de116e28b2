"""CPU: the rectangular reference, the embedding, sample_block, the CPU preprocessing and the layers' pair input
(tests/rect_cases.py; the GPU side is tests/test_gpu_rect.py)."""
import numpy as np
import pytest
import torch

import parity_cases as pc
import rect_cases as rc


def _pad_square(g, x):
    """The padded-square workaround of a rectangular GT problem: n = max(m, n_cols) nodes, Q / dO / K / V padded with rows
    that no edge touches."""
    n = max(g["m"], g["n_cols"])
    row_ptr = np.r_[g["row_ptr"], np.full(n - g["m"], g["row_ptr"][-1])].astype(np.int32)
    pad = lambda a: np.ascontiguousarray(np.concatenate([a, np.ones((n - a.shape[0],) + a.shape[1:], dtype=a.dtype)]))  # noqa: E731
    return row_ptr, {k: (pad(v) if k in ("Q", "K", "V", "dO") else v) for k, v in x.items()}


@pytest.mark.parametrize("kind", ["tall", "wide", "block"])
def test_reference_equals_oracle_on_padded_square(oracle_mod, kind):
    """float64: the rectangular reference against the oracle run on the padded-square form, restricted to the real rows and
    columns."""
    g = rc.graph(kind)
    x = rc.inputs("rowstats", g, 2, 20, unit_val=False)
    ref = rc.reference_on("rowstats", g, x)
    row_ptr, xs = _pad_square(g, x)
    args = (row_ptr, g["col_ind"], xs["val"], xs["Q"], xs["K"], xs["V"])
    out = oracle_mod.gt_forward(*args, acc="f64")
    dQ, dK, dV = oracle_mod.gt_backward(*args, xs["dO"], acc="f64")
    m, n = g["m"], g["n_cols"]
    for name, got, want in (("out", ref["out"], out[:m]), ("dQ", ref["dQ"], dQ[:m]), ("dK", ref["dK"], dK[:n]),
                            ("dV", ref["dV"], dV[:n])):
        err = float(np.abs(got - want).max())
        print(f"rect reference {kind} {name}: max abs difference to the oracle {err:.2e}")
        assert err < 1e-12 * max(1.0, float(np.abs(want).max())), (name, err)
    for a, n_real in ((out, m), (dQ, m), (dK, n), (dV, n)):
        assert (a[n_real:] == 0).all()


def test_reference_conventions_and_empties():
    g = rc.graph("tall")
    ref = rc.reference_on("rowstats", g, rc.inputs("rowstats", g, 2, 20, True))
    er, ec = g["deg"] == 0, g["indeg"] == 0
    assert (ref["out"][er] == 0).all() and (ref["dQ"][er] == 0).all() and (ref["row_sum"][er] == 0).all()
    assert (ref["row_max"][er] == rc.SENTINEL_MAX).all() and (ref["dK"][ec] == 0).all() and (ref["dV"][ec] == 0).all()
    for kind in ("no_rows", "no_cols"):
        g = rc.graph(kind)
        for pair in rc.PAIRS:
            ref = rc.reference_on(pair, g, rc.inputs(pair, g, 2, 20, True))
            assert ref["out"].shape == (g["m"], 2, 20) and all((v == 0).all() or k == "row_max" for k, v in ref.items())
            assert (ref["row_max"] == rc.SENTINEL_MAX).all()


@pytest.mark.parametrize("case", pc.case_ids("gt"), ids=str)
def test_embedding_carries_the_square_reference(case):
    """The rectangular reference of the embedded inputs equals the square case's reference moved through the embedding: the
    same edges with the same arithmetic in the same order.  Measured: exactly equal in float64 (difference 0.0) -- index_add
    visits the edges in the same order -- for every case; asserted to 1e-13 relative to leave room for another torch
    build's summation order."""
    g0 = pc.graph(case[0], case[1])
    x = pc.gt_inputs(*case)
    m0 = g0["m"]
    sq = rc.reference("rowstats", m0, m0, g0["rows"], g0["col_ind"], x)
    worst = 0.0
    for shift, cpad, rpad in ((0, 5, 3), (m0, 0, 0), (0, 0, m0)):
        g = rc.embed_graph(g0["row_ptr"], g0["col_ind"], shift, cpad, rpad)
        y = dict(val=x["val"], Q=rc.embed_rows(x["Q"], rpad), dO=rc.embed_rows(x["dO"], rpad),
                 K=rc.embed_cols(x["K"], shift, cpad), V=rc.embed_cols(x["V"], shift, cpad))
        ref = rc.reference_on("rowstats", g, y)
        for name in ("out", "dQ", "row_sum", "row_max"):
            got, clean = rc.restrict_rows(ref[name], m0, rc.SENTINEL_MAX if name == "row_max" else 0.0)
            assert clean, name
            worst = max(worst, float(np.abs(got - sq[name]).max() / max(1.0, np.abs(sq[name]).max())))
        for name in ("dK", "dV"):
            got, clean = rc.restrict_cols(ref[name], m0, shift)
            assert clean, name
            worst = max(worst, float(np.abs(got - sq[name]).max() / max(1.0, np.abs(sq[name]).max())))
    print(f"embedding {case}: worst relative difference {worst:.1e}")
    assert worst <= 1e-13


def test_sample_block():
    from DFGNN.utils.graph import sample_block
    p = rc._block_parent()
    row_ptr, col_ind = torch.from_numpy(p["row_ptr"]), torch.from_numpy(p["col_ind"])
    seeds = torch.tensor([90, 3, 17, 95, 91, 40])
    draw = lambda s: sample_block(row_ptr, col_ind, seeds, 4, torch.Generator().manual_seed(s))  # noqa: E731
    block, col_nodes = draw(5)
    src, dst = block.edges()
    assert block.num_rows() == len(seeds) and block.num_cols() == len(col_nodes) == len(set(col_nodes.tolist()))
    assert torch.equal(col_nodes[:len(seeds)], seeds)                           # the seeds are the first columns
    assert int(dst.max()) < block.num_cols() and int(src.max()) < block.num_rows()
    parent = {}
    for i, j in zip(p["rows"].tolist(), p["col_ind"].tolist()):
        parent[(i, j)] = parent.get((i, j), 0) + 1
    mine = {}
    for r, c in zip(src.tolist(), dst.tolist()):
        e = (int(seeds[r]), int(col_nodes[c]))
        mine[e] = mine.get(e, 0) + 1
    assert all(parent.get(e, 0) >= k for e, k in mine.items())                  # every block edge is a parent edge
    deg = torch.bincount(src, minlength=len(seeds))
    want = torch.minimum(torch.from_numpy(p["deg"].astype(np.int64))[seeds], torch.tensor(4))
    assert torch.equal(deg, want)                                               # the fanout, and every edge of a short row
    again, col_again = draw(5)
    assert torch.equal(again.edges()[0], src) and torch.equal(again.edges()[1], dst) and torch.equal(col_again, col_nodes)
    other, _ = sample_block(row_ptr, col_ind, torch.arange(90, 94), 10, torch.Generator().manual_seed(6))
    first, _ = sample_block(row_ptr, col_ind, torch.arange(90, 94), 10, torch.Generator().manual_seed(7))
    assert not (torch.equal(other.edges()[1], first.edges()[1]) and other.num_cols() == first.num_cols())
    moved = block.to("cpu")
    assert moved.num_rows() == block.num_rows() and moved.num_cols() == block.num_cols()


@pytest.mark.parametrize("kind", ["tall", "wide", "block", "no_rows", "no_cols"])
def test_cpu_preprocessing_of_a_rectangle(kind):
    """preprocess_block on the CPU (DFGNN/utils/sparse.py) against a numpy construction with stable sorts."""
    from DFGNN.layers import preprocess_block
    from DFGNN.utils.graph import Block
    g = rc.graph(kind)
    perm = np.random.default_rng(3).permutation(g["nnz"])                       # hand the edges over in COO order
    src, dst = g["src"][perm], g["dst"][perm]
    want = rc._finish(src, dst, g["m"], g["n_cols"])
    A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, _ = preprocess_block(Block(src, dst, g["m"], g["n_cols"]))
    assert A.shape == (g["m"], g["n_cols"]) and row_ptr.dtype == torch.int32
    for name, got in (("rows", rows), ("row_ptr", row_ptr), ("col_ind", col_ind), ("col_ptr", col_ptr), ("row_ind", row_ind),
                      ("val_idx", val_idx)):
        assert np.array_equal(got.numpy(), want[name]), name
    assert row_ptr.numel() == g["m"] + 1 and col_ptr.numel() == g["n_cols"] + 1 and bool((val == 1).all())


def test_square_cpu_preprocessing_unchanged():
    from DFGNN.layers import preprocess_Hyper_fw_bw
    from DFGNN.utils.graph import Graph
    g = rc.graph("tall")
    n = 600
    want = rc._finish(g["src"], g["dst"], n, n)
    _, rows, row_ptr, col_ind, _, col_ptr, row_ind, val_idx, _ = preprocess_Hyper_fw_bw(Graph(g["src"], g["dst"], n))
    for name, got in (("rows", rows), ("row_ptr", row_ptr), ("col_ind", col_ind), ("col_ptr", col_ptr), ("row_ind", row_ind),
                      ("val_idx", val_idx)):
        assert np.array_equal(got.numpy(), want[name]), name


def test_layers_take_a_pair_on_the_cpu():
    """The non-fused branch of the four layers with (h_cols, h_rows) on a rectangular SparseMatrix: shape [m, heads * dim],
    and (GT, one head; bias = 0; E = 0 through a zeroed lin_edge) the rectangular reference."""
    from DFGNN.layers import GATv2Conv_forward, SparseMHA_bias, SparseMHA_edge, SparseMHA_rowstats, preprocess_block
    from DFGNN.utils.graph import Block
    g = rc.graph("block")
    block = Block(g["src"], g["dst"], g["m"], g["n_cols"])
    params = preprocess_block(block)
    torch.manual_seed(0)
    h_cols = torch.randn(g["n_cols"], 16)
    h_rows = h_cols[:g["m"]]
    for heads, make in ((1, lambda: SparseMHA_rowstats(16, 24, 1)), (3, lambda: SparseMHA_bias(16, 24, 3)),
                        (3, lambda: SparseMHA_edge(16, 24, 3)), (3, lambda: GATv2Conv_forward(16, 8, 3))):
        layer = make().train()
        extra = ()
        if isinstance(layer, SparseMHA_bias):
            extra = (torch.zeros(g["nnz"], heads),)
        if isinstance(layer, SparseMHA_edge):
            torch.nn.init.zeros_(layer.lin_edge.weight)
            extra = (torch.randn(g["nnz"], 16),)
        out = layer(params, (h_cols, h_rows), *extra, fuse=False)
        assert out.shape == (g["m"], 24) and bool(torch.isfinite(out).all())
        assert bool((out[torch.from_numpy(g["deg"] == 0)] == 0).all())
        if isinstance(layer, GATv2Conv_forward):
            x_row, x_col = layer.project((h_cols, h_rows))
            x = dict(attn=layer.attn.detach().numpy(), X_row=x_row.detach().numpy(), X_col=x_col.detach().numpy(),
                     dO=np.zeros((g["m"], 3, 8), dtype=np.float32))
            ref = rc.reference_on("gatv2", g, x)["out"].reshape(g["m"], -1)
        elif heads == 1 or not isinstance(layer, SparseMHA_rowstats):
            q, k, v = (t.detach().numpy() for t in layer._qkv_fused((h_cols, h_rows)))
            x = dict(val=np.ones(g["nnz"], dtype=np.float32), Q=q, K=k, V=v, dO=np.zeros_like(q))
            ref = rc.reference_on("rowstats", g, x)["out"].reshape(g["m"], -1)
        err = float(np.abs(out.detach().numpy() - ref).max())
        print(f"{type(layer).__name__} pair input, non-fused: max abs err {err:.2e}")
        assert err < 1e-4 * max(1.0, float(np.abs(ref).max()))
