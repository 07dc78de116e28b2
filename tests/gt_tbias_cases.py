"""Reference of the GT conv with a typed attention bias (dfgnn_gt_fwd_tbias / dfgnn_gt_bwd_tbias), shared by
tests/test_gt_tbias_host.py and tests/test_gpu_gt_tbias.py.

The reference is tests/gt_bias_cases.reference in float64 on the materialised bias[h, nnz] = B[etype].T -- which removes
masked edges (B = -inf), head by head, before it runs -- and dB is its dbias reduced by a float64 index_add over the types:
dB[t, hd] = sum_{e : etype[e] = t} dbias[hd, e].  A rectangular m x n_cols graph is padded to the square one of
max(m, n_cols) nodes with rows / columns that have no edge (they change no sum) and the outputs are cut back."""
import numpy as np

import gt_bias_cases as bc

OUTPUTS = ("out", "row_max", "row_sum", "dQ", "dK", "dV", "dB")
PAIR_OUTPUTS = ("out", "row_max", "row_sum", "dQ", "dK", "dV")     # what the bias pair has too
SENTINEL_MAX = bc.SENTINEL_MAX


def materialise(B, etype):
    """bias[h, nnz] = B[etype].T, contiguous, in B's dtype (what the bias pair takes)."""
    return np.ascontiguousarray(np.asarray(B)[np.asarray(etype).astype(np.int64)].T)


def _pad(a, n):
    a = np.asarray(a)
    return a if a.shape[0] == n else np.concatenate([a, np.zeros((n - a.shape[0],) + a.shape[1:], dtype=a.dtype)])


def reference(row_ptr, col_ind, n_cols, val, etype, B, Q, K, V, dO):
    """Every output of the pair as float64 numpy arrays.  B: [T, h], may hold -inf; Q, dO: [m, h, f]; K, V: [n_cols, h, f]."""
    m, T = Q.shape[0], B.shape[0]
    n = max(m, n_cols)
    row_ptr = np.asarray(row_ptr)
    rp = np.concatenate([row_ptr, np.full(n - m, row_ptr[-1], dtype=row_ptr.dtype)])
    res = bc.reference(rp, col_ind, val, materialise(B, etype), _pad(Q, n), _pad(K, n), _pad(V, n), _pad(dO, n))
    out = {k: res[k][:m] for k in ("out", "row_max", "row_sum", "dQ")}
    out.update({k: res[k][:n_cols] for k in ("dK", "dV")})
    dB = np.zeros((T, B.shape[1]))
    np.add.at(dB, np.asarray(etype).astype(np.int64), res["dbias"].T.astype(np.float64))
    out["dB"], out["dbias"] = dB, res["dbias"]
    return out
