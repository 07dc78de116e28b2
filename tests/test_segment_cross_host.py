"""CPU: the header, loader and libraries of the segment cross attention pair (include/dfgnn_segment_cross.h) and the
argument errors it answers before any device call."""
import ctypes
import os
import subprocess

import pytest

import dfgnn_native as N
from conftest import ROOT
from guarded import prototypes, stream_entries

PROTOS = prototypes(open(os.path.join(ROOT, "include", "dfgnn_segment_cross.h")).read())
E_BADARG, E_UNSUPPORTED = -1, -2


def test_header_equals_loader():
    assert sorted(PROTOS) == sorted(N.SEGMENT_CROSS_SIGNATURES)
    assert stream_entries(PROTOS) == ["dfgnn_segment_cross_bounds", "dfgnn_segment_mha_cross_bwd", "dfgnn_segment_mha_cross_fwd"]
    assert {n: len(p) for n, p in PROTOS.items()} == {n: len(a) for n, a in N.SEGMENT_CROSS_SIGNATURES.items()}
    older = (N.SIGNATURES, N.SAMPLE_SIGNATURES, N.SEGMENT_SIGNATURES, N.SEGMENT_BIAS_SIGNATURES, N.SEGMENT_TBIAS_SIGNATURES)
    assert not any(set(PROTOS) & set(t) for t in older)


@pytest.mark.parametrize("name", ("libdfgnn.so", "libdfgnn_hip.so"))
def test_libraries_export_the_entries(name):
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "df-gnn_amd", name)], capture_output=True, text=True,
                        check=True).stdout
    assert set(PROTOS) <= {line.split()[-1] for line in nm.splitlines() if line.strip()}


def test_argument_errors_without_a_device():
    L = N.lib()
    assert L.dfgnn_segment_cross_abi_version() == 1
    p = ctypes.addressof(ctypes.create_string_buffer(64))    # a non-NULL pointer nothing dereferences
    bounds = lambda m_q=1, m_k=1, n_seg=1, ptrs=(p,) * 4: L.dfgnn_segment_cross_bounds(m_q, m_k, n_seg, *ptrs, None)  # noqa: E731
    fwd = lambda m_q=1, m_k=1, h=1, f=32, form=0, ptrs=(p,) * 7: L.dfgnn_segment_mha_cross_fwd(  # noqa: E731
        m_q, m_k, h, f, 1.0, form, *ptrs, None)
    bwd = lambda m_q=1, m_k=1, h=1, f=32, form=0, ptrs=(p,) * 12: L.dfgnn_segment_mha_cross_bwd(  # noqa: E731
        m_q, m_k, h, f, 1.0, form, *ptrs, None)
    assert bounds(m_q=-1) == E_BADARG and bounds(m_k=-1) == E_BADARG and bounds(n_seg=-1) == E_BADARG
    assert bounds(n_seg=0) == E_BADARG and bounds(m_q=0, n_seg=0) == E_BADARG      # a row needs a segment
    for k in range(4):                                           # seg_ptr_q, seg_ptr_k, qbounds, kbounds
        assert bounds(ptrs=(p,) * k + (None,) + (p,) * (3 - k)) == E_BADARG
    assert bounds(m_q=0, m_k=0, n_seg=0, ptrs=(None,) * 4) == 0 and bounds(m_q=0, m_k=0, n_seg=3, ptrs=(None,) * 4) == 0
    for entry, n in ((fwd, 7), (bwd, 12)):
        assert entry(m_q=-1) == E_BADARG and entry(m_k=-1) == E_BADARG and entry(h=0) == E_BADARG
        assert entry(form=-1) == E_BADARG and entry(form=3) == E_BADARG
        assert entry(f=48) == E_UNSUPPORTED and entry(h=65536) == E_UNSUPPORTED
        assert entry(f=48, form=3) == E_BADARG                   # extents and the form before the limits
        assert entry(m_q=1 << 23, h=4, f=32) == E_UNSUPPORTED    # 4 GiB of features on either side: 32-bit row offsets
        assert entry(m_k=1 << 23, h=4, f=32) == E_UNSUPPORTED
        assert entry(m_q=1 << 23, h=4, f=32, ptrs=(None,) * n) == E_UNSUPPORTED    # ... before the pointers
        assert entry(m_q=0, m_k=0, ptrs=(None,) * n) == 0
    assert fwd(m_q=0, ptrs=(None,) * 7) == 0                     # no query: nothing to write
    for k in range(5):                                           # qbounds, Q, K, V, out
        assert fwd(ptrs=(p,) * k + (None,) + (p,) * (6 - k)) == E_BADARG
    assert fwd(ptrs=(p,) * 5 + (p, None)) == E_BADARG and fwd(ptrs=(p,) * 5 + (None, p)) == E_BADARG
    assert fwd(m_q=0, ptrs=(None,) * 5 + (p, None)) == E_BADARG  # one statistic without the other, whatever the extents
    for k in range(12):                                          # every pointer
        assert bwd(ptrs=(p,) * k + (None,) + (p,) * (11 - k)) == E_BADARG
    # an array of no rows may be NULL, one with rows may not: m_k == 0 frees K, V (2, 3) of the forward, m_q == 0 / m_k == 0
    # the query side (0, 2, 5..8, 11) / the key side (1, 3, 4, 9, 10) of the backward
    assert fwd(m_k=0, ptrs=(None, p, None, None, p, p, p)) == E_BADARG and fwd(m_k=0, ptrs=(p, p, None, None, None, p, p)) == E_BADARG
    query_side = (0, 2, 5, 6, 7, 8, 11)
    for k in range(12):
        ptrs = tuple(None if j == k else p for j in range(12))
        if k in query_side:
            assert bwd(m_k=0, ptrs=ptrs) == E_BADARG
        else:
            assert bwd(m_q=0, ptrs=ptrs) == E_BADARG
