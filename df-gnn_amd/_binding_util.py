"""What the fused_gtconv / fused_gatconv / dfgnn_preprocess binding modules share: the argument checks of the ctypes
transport by family, its call helper, the `val` and block-plan look-ups and their caches.

The checks mirror the reference's binding-level ones (DFGNN/src/fused_gtconv/fused_gtconv.cpp:7-13:
CHECK_DEVICE / CHECK_CONTIGUOUS raise RuntimeError) and turn its compiled-out dtype asserts
(fused_gtconv.cpp:103-112) into real errors.
"""
import collections
import ctypes
import os

import torch

import dfgnn_native as _n


def as_int32(t):
    """Index arrays are int32 on the device; int64 (e.g. dgl's val_idx) is narrowed once here."""
    return t if t.dtype == torch.int32 else t.to(torch.int32)


# ---- argument checks of the ctypes transport, by family (csrc/torch_ext.cpp makes the same ones for the extension) ------
# A family is a set of tensors that must agree in dtype and shape.  `ref` is the tensor whose device the call runs on (the
# first feature tensor): every family compares its members' device with it -- a pointer of another GPU must not be handed
# to a kernel of this one.
def _family(ref, dtype, shape, tensors):
    """Every tensor of {name: tensor} on ref's GPU, contiguous, of `dtype` and (unless None) of `shape`."""
    dev = ref.get_device()   # (-1: not on a GPU)
    for name, t in tensors.items():
        if dev < 0 or t.get_device() != dev:
            if not t.is_cuda:
                raise RuntimeError(f"{name} must be on CUDA")
            raise RuntimeError(f"every tensor must live on one device ({ref.device}), got {name} on {t.device}")
        if not t.is_contiguous():
            raise RuntimeError(f"{name} must be contiguous")
        if t.dtype != dtype:
            raise RuntimeError(f"{name} must have dtype {dtype}, got {t.dtype}")
        if shape is not None and t.shape != shape:
            raise RuntimeError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")


def check_family(ref, dtype, **tensors):
    """Tensors of any shape."""
    _family(ref, dtype, None, tensors)


def check_feats(**tensors):
    """fp32 feature tensors [nodes, heads, feat] of one shape, the first one being the call's `ref` -> (nodes, h, f)."""
    name, ref = next(iter(tensors.items()))
    _family(ref, torch.float32, ref.shape, tensors)
    if ref.dim() != 3:
        raise RuntimeError(f"{name} must have shape [nodes, heads, feat], got {tuple(ref.shape)}")
    return tuple(ref.shape)


def check_cols(rows_name, rows, **tensors):
    """The column side of a pair that takes an m x n_cols graph (K / V, GATv2's X_col): fp32 [n_cols, heads, feat] tensors
    of one shape with the heads and features of the row side `rows` (Q, X_row) -> n_cols."""
    name, first = next(iter(tensors.items()))
    _family(rows, torch.float32, None, {name: first})
    if first.dim() != 3 or first.shape[1:] != rows.shape[1:]:
        raise RuntimeError(f"{name} must have shape (n_cols, {rows.shape[1]}, {rows.shape[2]}): the heads and features of "
                           f"{rows_name}, got {tuple(first.shape)}")
    for other, t in list(tensors.items())[1:]:
        _family(rows, torch.float32, None, {other: t})
        if t.shape != first.shape:
            raise RuntimeError(f"{other} must have shape {tuple(first.shape)} like {name}, got {tuple(t.shape)}")
    return first.shape[0]


def check_csr(ref, m, indptr, indices):
    """The int32 CSR arrays of a graph whose `m` rows are the nodes of the feature tensors -> nnz."""
    _family(ref, torch.int32, None, {"indptr": indptr, "indices": indices})
    if indptr.dim() != 1 or indices.dim() != 1:
        raise RuntimeError("indptr / indices must be 1-D")
    if indptr.size(0) - 1 != m:
        raise RuntimeError(f"indptr describes {indptr.size(0) - 1} rows but features have {m} nodes")
    return indices.size(0)


def check_csc(ref, m, nnz, col_ptr, **per_edge):
    """The int32 CSC arrays next to a CSR structure of m rows and nnz edges: col_ptr and its per-edge arrays."""
    _family(ref, torch.int32, None, {"col_ptr": col_ptr})
    if col_ptr.shape != (m + 1,):
        raise RuntimeError(f"col_ptr must have shape ({m + 1},): the adjacency must be square")
    _family(ref, torch.int32, (nnz,), per_edge)


def check_csc_rect(ref, n_cols, nnz, col_ptr, cols_name, **per_edge):
    """check_csc for an m x n_cols graph: col_ptr has one entry per column -- per row of K / V (X_col) -- and one more."""
    _family(ref, torch.int32, None, {"col_ptr": col_ptr})
    _family(ref, torch.int32, (nnz,), per_edge)
    if col_ptr.shape != (n_cols + 1,):
        raise RuntimeError(f"col_ptr must have shape ({n_cols + 1},): one entry for each of the {n_cols} rows of {cols_name} "
                           "and one more")


def check_edges(ref, nnz, dtype, **tensors):
    """Per-edge arrays [nnz]."""
    _family(ref, dtype, (nnz,), tensors)


def check_2d(ref, n, h, **tensors):
    """fp32 arrays [n, h]: per-row statistics and scores (n = m), the dropout randoms (n = nnz)."""
    _family(ref, torch.float32, (n, h), tensors)


def check_3d(ref, n, h, f, **tensors):
    """fp32 arrays [n, h, f]: per-edge feature vectors (n = nnz)."""
    _family(ref, torch.float32, (n, h, f), tensors)


def stream_ptr(device):
    return torch.cuda.current_stream(device).cuda_stream


def call(symbol, what, device, *args):
    """The ctypes transport: dfgnn_native.lib().<symbol>(*args, stream) on `device` and on torch's current stream of it.
    Tensors go as their addresses, None as NULL, numbers as they are; a non-zero return raises the library's RuntimeError
    under the operator's name `what`."""
    with torch.cuda.device(device):
        _n.check(getattr(_n.lib(), symbol)(*[a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args],
                                           stream_ptr(device)), what)


class _KeyedCache:
    """A small LRU keyed by what a tensor IS -- (data_ptr, numel, version counter) -- rather than by the Python object that
    wraps it: a re-wrapped tensor (.detach(), a view of the same memory, a tuple rebuilt by a data loader around the same
    storages) finds the entry its first wrapper made.  Each entry keeps a reference to the tensors of its key, so the
    memory behind a key cannot be freed and handed to other data while the entry lives; the LRU bound (DFGNN_CACHE_ENTRIES,
    default 16) is what that costs."""

    def __init__(self, entries=None):
        self.entries = entries or int(os.environ.get("DFGNN_CACHE_ENTRIES", "16"))
        self.d = collections.OrderedDict()

    @staticmethod
    def key_of(*tensors, extra=()):
        return tuple((t.data_ptr(), t.numel(), t._version, t.dtype, t.device.index) for t in tensors) + tuple(extra)

    def get(self, key):
        hit = self.d.get(key)
        if hit is not None:
            self.d.move_to_end(key)
            return hit[0]
        return None

    def put(self, key, value, *keep_alive):
        self.d[key] = (value, keep_alive)
        self.d.move_to_end(key)
        while len(self.d) > self.entries:
            self.d.popitem(last=False)
        return value


_unit_cache = _KeyedCache()
_plan_cache = _KeyedCache()
_rows_cache = _KeyedCache()
_weights_cache = _KeyedCache(entries=4)   # 1 KB per node each


def plan_dense_weights(plan, row_ptr, val):
    """The edge values `val` (fp32[nnz] / [nnz, 1], CSR order) in the dense form the WEIGHTED matrix-core kernels read
    (include/dfgnn.h: dfgnn_plan_dense_weights): fp32[256 m], built once per (plan, val tensor version) and cached --
    edge weights of a dataset do not change from step to step."""
    key = _KeyedCache.key_of(val, extra=(plan.key,))
    w = _weights_cache.get(key)
    if w is not None:
        return w
    v = val.reshape(-1)
    if v.dtype != torch.float32 or not v.is_contiguous():
        raise RuntimeError("val must be contiguous float32")
    ext = _n.ext()
    if ext is not None:
        w = ext.plan_dense_weights(row_ptr, v, *plan.ptrs())
    else:
        m, nnz = plan.meta[4], plan.meta[5]
        w = torch.empty(int(_n.lib().dfgnn_plan_dense_weights_floats(m)), dtype=torch.float32, device=val.device)
        call("dfgnn_plan_dense_weights", "plan_dense_weights", val.device, m, nnz, row_ptr, v, *plan.ptrs(), w)
    return _weights_cache.put(key, w, val, plan)


def val_ptr(val):
    """Edge values for the C ABI: NULL when they are all ones (include/dfgnn.h: "NULL means all ones"), which is
    what every reference flow passes (A.val of an unweighted adjacency, DFGNN/layers/util.py:82-142) and lets the
    kernels skip the per-edge multiply.  The test runs once per tensor version (one device reduction + sync)."""
    if val is None:
        return None
    cached = getattr(val, "_dfgnn_unit", None)   # preprocessing marks the arrays it creates (DFGNN/layers/util.py:_unit_val)
    if cached is not None and cached[0] == val._version:
        return None if cached[1] else val.data_ptr()
    key = _KeyedCache.key_of(val)
    unit = _unit_cache.get(key)
    if unit is None:
        # a foreign tensor is tested once per (memory, version) -- one reduction + host sync, which cannot happen inside
        # a stream capture -- whatever Python object wraps it the next time
        if val.is_cuda and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("edge values of unknown content inside a HIP-graph capture: run the operator once before "
                               "capturing (or create `val` through DFGNN.layers.preprocess_*), so that the all-ones test "
                               "is cached")
        unit = _unit_cache.put(key, bool((val == 1).all().item()) if val.numel() else True, val)
    return None if unit else val.data_ptr()


# ---- block plan cache -----------------------------------------------------------------------------
class BlockPlan:
    """Device plan buffer + its 12 host header words (include/dfgnn.h, dfgnn_plan_build).  key: plan_key() of what it
    was built from."""
    __slots__ = ("buf", "meta", "_meta_c", "key", "_ptrs", "_stats_ok")

    def __init__(self, buf, meta_c, key):
        self.buf, self._meta_c, self.key = buf, meta_c, key
        self.meta = list(meta_c)
        self._ptrs = (buf.data_ptr(), ctypes.addressof(meta_c))
        self._stats_ok = {}

    def stats_applies(self, h):
        """dfgnn_gt_stats_applies for this plan and `h` heads (include/dfgnn.h): every range of the batch is served by
        the matrix-core kernels, so the statistics-saving training pair can run it."""
        ok = self._stats_ok.get(h)
        if ok is None:
            ok = bool(_n.lib().dfgnn_gt_stats_applies(self.meta[4], self.meta[5], h, self.meta[6], self._ptrs[1]))
            self._stats_ok[h] = ok
        return ok

    @property
    def num_fit(self):
        return self.meta[0]

    @property
    def num_spill(self):
        return self.meta[1]

    @property
    def num_edge_global(self):
        return self.meta[8]

    @property
    def num_dense(self):
        """Fit ranges marked for the matrix-core kernels (they come first in the list)."""
        return self.meta[9]

    @property
    def num_dense_wide(self):
        """... of which this many have more than 128 nodes (a batch without any takes the 256-thread forward kernels)."""
        return self.meta[10]

    def ptrs(self):
        """(plan_ptr, meta_ptr) for the C ABI."""
        return self._ptrs


def plan_ptrs(plan):
    """BlockPlan | None -> (plan_ptr, meta_ptr) as either transport takes them; 0 is NULL: no plan."""
    return plan._ptrs if plan is not None else (0, 0)


def plan_key(indptr, indices, f):
    """What a plan is a plan OF: the MEMORY of the two CSR arrays (address, length, version counter) and the feature
    width.  The key of the plan cache, the test that a plan found on a tensor object is still that tensor's, and (as
    BlockPlan.key) what plan_dense_weights tells plans apart by."""
    return (indptr.data_ptr(), indptr.size(0), indptr._version, indices.data_ptr(), indices.size(0), indices._version, f)


def build_plan(indptr, indices, f):
    """Run dfgnn_plan_build for this CSR structure and feature width (synchronises the stream once)."""
    m, nnz = indptr.size(0) - 1, indices.size(0)
    ext = _n.ext()
    if ext is not None:  # torch C++ binding: allocation + call without ctypes marshalling
        buf, meta_l = ext.plan_build(indptr, indices, int(f))
        meta = (ctypes.c_int * 12)(*meta_l)
    else:
        buf = torch.empty(int(_n.lib().dfgnn_plan_ints(m, nnz)), dtype=torch.int32, device=indptr.device)
        meta = (ctypes.c_int * 12)()
        call("dfgnn_plan_build", "dfgnn_plan_build", indptr.device, m, nnz, f, indptr, indices, buf, ctypes.addressof(meta))
    return BlockPlan(buf, meta, plan_key(indptr, indices, f))


def get_plan_obj(indptr, indices, Q, enable=True):
    """The BlockPlan of (indptr, indices, f), or None when there is none.  Q: the call's feature tensor -- only
    [nodes, heads, f] has a plan -- or f itself.  Built on first use and cached by the identity of the two arrays' MEMORY
    (plan_key; _KeyedCache) -- the reference's preprocess_* tuples keep those arrays alive across the layers / epochs that
    reuse a batch (DFGNN/layers/util.py:82-142), so the plan is built once per batch structure, also when the tensors
    reach the operator re-wrapped (.detach(), views, rebuilt tuples)."""
    f = Q if isinstance(Q, int) else (Q.size(-1) if Q.dim() == 3 else 0)
    if not enable or f <= 0 or f % 4 != 0 or indices.dim() != 1 or indptr.dim() != 1 or indices.size(0) == 0:
        return None
    if not (indptr.is_cuda and indices.is_cuda and indptr.dtype == torch.int32 and indices.dtype == torch.int32 and
            indptr.is_contiguous() and indices.is_contiguous()):
        return None  # (the binding's argument checks raise the matching error right after)
    if indices.size(0) < 8 * (indptr.size(0) - 1):
        return None  # low-degree graphs take the row-per-lane-group kernels (capi.hip:low_degree)
    # first the Python object itself (the common case: the same preprocess_* tuple call after call; a dict lookup and
    # a few cheap reads), then the memory-identity cache (a re-wrapped tensor)
    key = plan_key(indptr, indices, f)
    mine = indptr.__dict__.get("_dfgnn_plans")
    plan = mine.get(f) if mine is not None else None
    if plan is None or plan.key != key:
        plan = _plan_cache.get(key)
        if plan is None:
            plan = _plan_cache.put(key, build_plan(indptr, indices, f), indptr, indices)
        indptr.__dict__.setdefault("_dfgnn_plans", {})[f] = plan   # (mirror on the tensor object: the fast path above)
    return plan if plan.num_fit else None


def get_plan(indptr, indices, f, enable=True):
    """get_plan_obj as the C ABI's arguments: (plan_ptr, meta_ptr, needs_edge_scratch), or (None, None, False)."""
    plan = get_plan_obj(indptr, indices, f, enable)
    if plan is None:
        return None, None, False
    return plan._ptrs + (plan.num_edge_global > 0,)


def get_rows(row_ptr, nnz):
    """Sorted COO row ids of a CSR structure (the COO half of the 'hyper' format), derived once per row_ptr tensor and
    cached on it like the plan.  The reference's gat_forward / gat_backward take CSR only
    (DFGNN/src/fused_gatconv/fused_gatconv.cpp:11-14, 291-300); the matrix-core kernels walk the edges by (row, col)
    pairs, so the binding derives the row ids next to the plan -- preprocessing, once per batch structure."""
    key = _KeyedCache.key_of(row_ptr, extra=(nnz,))
    rows = _rows_cache.get(key)
    if rows is None:
        deg = (row_ptr[1:] - row_ptr[:-1]).long()
        rows = torch.repeat_interleave(torch.arange(deg.numel(), dtype=torch.int32, device=row_ptr.device), deg,
                                       output_size=nnz)
        _rows_cache.put(key, rows, row_ptr)
        try:  # (mirror on the tensor object, for tests that inspect it)
            row_ptr.__dict__["_dfgnn_rows"] = (key, rows)
        except AttributeError:
            pass
    return rows
