"""Minimal graph container standing in for the DGLGraph the reference's harness passes around.

Only what the hot path's callers touch is provided: `edges()`, `num_nodes()`, `num_edges()`,
`ndata`, `to(device)` (DFGNN/layers/util.py:52-57, DFGNN/utils/util.py:239-243 in the reference),
plus `batch()` which, like `dgl.batch`, lays graphs out block-diagonally: graph g owns a
contiguous node range and all of its edges stay inside it.
A real DGLGraph duck-types to the same calls, so the preprocess functions accept either.
"""
import torch


class Graph:
    def __init__(self, src, dst, num_nodes, batch_num_nodes=None):
        self._src = torch.as_tensor(src, dtype=torch.int64)
        self._dst = torch.as_tensor(dst, dtype=torch.int64)
        self._n = int(num_nodes)
        self.ndata = {}
        # nodes per member graph (None for a single graph) -- same role as DGLGraph.batch_num_nodes()
        self._batch_num_nodes = None if batch_num_nodes is None else torch.as_tensor(batch_num_nodes, dtype=torch.int64)

    def edges(self):
        return self._src, self._dst

    def num_nodes(self):
        return self._n

    def num_edges(self):
        return int(self._src.numel())

    def batch_num_nodes(self):
        if self._batch_num_nodes is None:
            return torch.tensor([self._n], dtype=torch.int64)
        return self._batch_num_nodes

    @property
    def device(self):
        return self._src.device

    def to(self, device):
        g = Graph(self._src.to(device), self._dst.to(device), self._n, self._batch_num_nodes)
        g.ndata = {k: v.to(device) for k, v in self.ndata.items()}
        return g


def batch(graphs):
    """Block-diagonal union of graphs (node ids of graph g shifted by the nodes before it)."""
    srcs, dsts, sizes, off = [], [], [], 0
    for g in graphs:
        s, d = g.edges()
        srcs.append(s + off)
        dsts.append(d + off)
        sizes.append(g.num_nodes())
        off += g.num_nodes()
    out = Graph(torch.cat(srcs) if srcs else torch.zeros(0, dtype=torch.int64),
                torch.cat(dsts) if dsts else torch.zeros(0, dtype=torch.int64), off, sizes)
    keys = set.intersection(*[set(g.ndata) for g in graphs]) if graphs else set()
    for k in keys:
        out.ndata[k] = torch.cat([g.ndata[k] for g in graphs])
    return out


class Block:
    """A rectangular (bipartite) graph: num_rows query / output nodes x num_cols key / value nodes -- one layer's share of a
    neighbour-sampled mini-batch, or cross-attention onto another node set.  As in Graph, edges() = (src, dst) with
    src the ROW of an edge (a seed, < num_rows) and dst its COLUMN (a sampled neighbour, < num_cols): every fused
    operator normalises over rows.  DFGNN.layers.preprocess_block turns it into the operators' arrays."""

    def __init__(self, src, dst, num_rows, num_cols):
        self._src = torch.as_tensor(src, dtype=torch.int64)
        self._dst = torch.as_tensor(dst, dtype=torch.int64)
        self._rows, self._cols = int(num_rows), int(num_cols)

    def edges(self):
        return self._src, self._dst

    def num_rows(self):
        return self._rows

    def num_cols(self):
        return self._cols

    def num_edges(self):
        return int(self._src.numel())

    @property
    def device(self):
        return self._src.device

    def to(self, device):
        return Block(self._src.to(device), self._dst.to(device), self._rows, self._cols)


def sample_block(row_ptr, col_ind, seeds, fanout, generator=None):
    """One hop of uniform neighbour sampling without replacement, in torch ops on the device of the CSR arrays:
    -> (block, col_nodes).  Row r of the block is seeds[r] (distinct node ids) and keeps min(fanout, degree) of its edges in the parent graph
    (row_ptr, col_ind), drawn under `generator` (a seeded torch.Generator makes the result reproducible); duplicate parent
    edges are distinct edges.  col_nodes lists the parent ids of the block's columns and BEGINS WITH THE SEEDS (DGL's block
    convention: the output nodes are the first input nodes, so x[col_nodes][:len(seeds)] are the seeds' own features),
    followed by the other sampled neighbours in increasing id; the block's column ids index col_nodes.  A block's
    col_nodes are the seeds of the next hop outwards."""
    row_ptr, col_ind = row_ptr.long(), col_ind.long()
    dev = row_ptr.device
    seeds = torch.as_tensor(seeds, dtype=torch.int64, device=dev)
    m = seeds.numel()
    start = row_ptr[seeds]
    deg = row_ptr[seeds + 1] - start
    total = int(deg.sum())
    row = torch.repeat_interleave(torch.arange(m, device=dev), deg, output_size=total)      # block row of each candidate edge
    first = torch.cumsum(deg, 0) - deg                                                      # candidates of a row are contiguous
    pos = torch.arange(total, device=dev) - first[row]
    # a random key per candidate; sorted by (row, key), the first `fanout` of a row are a uniform sample of its edges
    key = torch.rand(total, generator=generator, device=generator.device if generator is not None else "cpu").to(dev)
    order = torch.argsort(key)
    order = order[torch.argsort(row[order], stable=True)]
    keep = order[(torch.arange(total, device=dev) - first[row]) < fanout]                   # (row is sorted: rank within the row)
    keep = torch.sort(keep).values                                                          # parent edge order inside a row
    src = row[keep]
    parent_col = col_ind[start[src] + pos[keep]]
    # columns: the seeds first, then every other sampled node by increasing id
    is_seed = torch.zeros(row_ptr.numel() - 1, dtype=torch.bool, device=dev)
    is_seed[seeds] = True
    others = torch.unique(parent_col[~is_seed[parent_col]])
    col_nodes = torch.cat([seeds, others])
    local = torch.full((row_ptr.numel() - 1,), -1, dtype=torch.int64, device=dev)
    local[others] = torch.arange(m, m + others.numel(), device=dev)
    local[seeds] = torch.arange(m, device=dev)                                              # (seeds are distinct node ids)
    return Block(src, local[parent_col], m, col_nodes.numel()), col_nodes


# ---- the native sampler's definition (include/dfgnn_sample.h) ------------------------------------------------------------
class SampledBlock(Block):
    """A Block as sample_block_fused makes it: it carries the finished int32 arrays of the sampler -- parent_edge (the parent
    CSR position of every kept edge: gather etype, score or E through it), row_ptr, col_ind, rows and the CSC half col_ptr,
    row_ind, val_idx -- so DFGNN.layers.preprocess_block has nothing left to sort.  edges() are rows / col_ind as int64."""

    ARRAYS = ("parent_edge", "row_ptr", "col_ind", "rows", "col_ptr", "row_ind", "val_idx")

    def __init__(self, arrays, num_rows, num_cols):
        self._rows, self._cols = int(num_rows), int(num_cols)
        for name in self.ARRAYS:
            setattr(self, name, arrays[name])
        self._edges = None

    @property
    def _src(self):
        return self.edges()[0]

    @property
    def _dst(self):
        return self.edges()[1]

    def edges(self):
        if self._edges is None:
            self._edges = (self.rows.long(), self.col_ind.long())
        return self._edges

    def num_edges(self):
        return int(self.col_ind.numel())

    @property
    def device(self):
        return self.col_ind.device

    def to(self, device):
        return SampledBlock({name: getattr(self, name).to(device) for name in self.ARRAYS}, self._rows, self._cols)


def mix32(x):
    """The sampler's 32-bit mixer on a numpy array (or a number) -> uint64 array of values below 2^32.  A bijection."""
    import numpy as np
    x = np.asarray(x).astype(np.uint64) & np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & np.uint64(0xFFFFFFFF)
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & np.uint64(0xFFFFFFFF)
    return x ^ (x >> np.uint64(16))


def sample_keys(pos, seed):
    """key = mix(p ^ mix(seed)) of the parent edges at CSR positions `pos` under a 32-bit seed: a row keeps its `fanout`
    smallest keys.  Distinct positions have distinct keys."""
    import numpy as np
    return mix32(mix32(int(seed) & 0xFFFFFFFF) ^ (np.asarray(pos).astype(np.uint64) & np.uint64(0xFFFFFFFF)))


def sample_block_reference(row_ptr, col_ind, seeds, fanout, seed):
    """The definition of the native sampler (include/dfgnn_sample.h) in vectorised numpy on the CPU: the CPU path of
    sample_block_fused and the tests' oracle.  -> dict of int32 CPU tensors, every array dfgnn_sample_select /
    dfgnn_sample_emit write: row_ptr (the block's, [m + 1]), parent_edge, col_ind, rows [nnz_b], col_nodes [n_cols_b],
    col_ptr [n_cols_b + 1], row_ind, val_idx [nnz_b]."""
    import numpy as np
    rp = torch.as_tensor(row_ptr).cpu().numpy().astype(np.int64)
    ci = torch.as_tensor(col_ind).cpu().numpy().astype(np.int64)
    sd = torch.as_tensor(seeds).cpu().numpy().astype(np.int64).reshape(-1)
    n, m, fanout = rp.size - 1, sd.size, int(fanout)
    if fanout < 1:
        raise ValueError("fanout must be at least 1")
    start = rp[sd]
    deg = rp[sd + 1] - start
    total = int(deg.sum())
    row = np.repeat(np.arange(m, dtype=np.int64), deg)              # block row of each candidate edge
    first = np.cumsum(deg) - deg
    within = np.arange(total, dtype=np.int64) - first[row]
    pos = start[row] + within                                       # its parent CSR position
    key = sample_keys(pos, seed)
    order = np.lexsort((key, row))                                  # by row, then by key: rank `within` in its row
    keep = np.sort(order[within < fanout])                          # back to parent order (candidates are listed in it)
    rows, parent_edge = row[keep], pos[keep]
    parent_col = ci[parent_edge]
    is_seed = np.zeros(n, dtype=bool)
    is_seed[sd] = True
    others = np.unique(parent_col[~is_seed[parent_col]])
    col_nodes = np.concatenate([sd, others])
    local = np.full(n, -1, dtype=np.int64)
    local[others] = np.arange(m, m + others.size)
    local[sd] = np.arange(m)
    blk_col = local[parent_col]
    blk_row_ptr = np.zeros(m + 1, dtype=np.int64)
    blk_row_ptr[1:] = np.cumsum(np.minimum(deg, fanout))
    by_col = np.argsort(blk_col, kind="stable")
    col_ptr = np.zeros(col_nodes.size + 1, dtype=np.int64)
    col_ptr[1:] = np.cumsum(np.bincount(blk_col, minlength=col_nodes.size))
    out = dict(row_ptr=blk_row_ptr, parent_edge=parent_edge, col_ind=blk_col, rows=rows, col_nodes=col_nodes, col_ptr=col_ptr,
               row_ind=rows[by_col], val_idx=by_col)
    return {k: torch.from_numpy(np.ascontiguousarray(v.astype(np.int32))) for k, v in out.items()}


def sample_block_fused(row_ptr, col_ind, seeds, fanout, generator=None, seed=None):
    """sample_block by the native sampler: one hop of uniform neighbour sampling without replacement -> (block, col_nodes)
    with the same conventions (row r is seeds[r], col_nodes begins with the seeds, the other sampled nodes follow in
    increasing id), but the block is a SampledBlock: parent_edge and the finished CSR and CSC arrays come with it, and
    preprocess_block only hands them on.  Which edges a row keeps is a pure function of `seed` (32 bits; drawn from
    `generator` when it is None -- on the CPU unless the generator is a device one, which costs a host read) and the edge's
    position in the parent CSR: include/dfgnn_sample.h.  Other samples than sample_block draws, the same distribution.
    CUDA arrays: dfgnn_sample_select, one read of the two output sizes, dfgnn_sample_emit.  CPU arrays:
    sample_block_reference.  `fanout` is clamped to the parent's largest degree (computed once per row_ptr and cached), so
    'every neighbour' is a large fanout, not a large workspace."""
    if seed is None:
        where = generator.device if generator is not None else "cpu"
        seed = int(torch.randint(0, 2 ** 32, (1,), generator=generator, device=where, dtype=torch.int64))
    seed = int(seed) & 0xFFFFFFFF
    row_ptr, col_ind = torch.as_tensor(row_ptr), torch.as_tensor(col_ind)
    seeds = torch.as_tensor(seeds, device=row_ptr.device)
    m = seeds.numel()
    if row_ptr.is_cuda:
        import dfgnn_preprocess
        arrays = dfgnn_preprocess.sample_hop(row_ptr, col_ind, seeds, fanout, seed)
    else:
        deg = row_ptr[1:] - row_ptr[:-1]
        fanout = max(1, min(int(fanout), int(deg.max()) if deg.numel() else 1))
        arrays = sample_block_reference(row_ptr, col_ind, seeds, fanout, seed)
    col_nodes = arrays.pop("col_nodes")
    return SampledBlock(arrays, m, col_nodes.numel()), col_nodes.long()
