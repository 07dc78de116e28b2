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
