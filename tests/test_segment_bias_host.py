"""CPU: the header, loader and libraries of the segment attention pair with a pair bias (include/dfgnn_segment_bias.h) and the
argument errors it answers before any device call."""
import ctypes
import os
import subprocess

import pytest

import dfgnn_native as N
from conftest import ROOT
from guarded import prototypes, stream_entries

PROTOS = prototypes(open(os.path.join(ROOT, "include", "dfgnn_segment_bias.h")).read())
E_BADARG, E_UNSUPPORTED = -1, -2


def test_header_equals_loader():
    assert sorted(PROTOS) == sorted(N.SEGMENT_BIAS_SIGNATURES)
    assert stream_entries(PROTOS) == ["dfgnn_segment_mha_bias_bwd", "dfgnn_segment_mha_bias_fwd", "dfgnn_segment_pair_rows"]
    assert {n: len(p) for n, p in PROTOS.items()} == {n: len(a) for n, a in N.SEGMENT_BIAS_SIGNATURES.items()}
    assert not set(PROTOS) & (set(N.SIGNATURES) | set(N.SAMPLE_SIGNATURES) | set(N.SEGMENT_SIGNATURES))


@pytest.mark.parametrize("name", ("libdfgnn.so", "libdfgnn_hip.so"))
def test_libraries_export_the_entries(name):
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "df-gnn_amd", name)], capture_output=True, text=True,
                        check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert set(PROTOS) <= exported


def test_argument_errors_without_a_device():
    L = N.lib()
    assert L.dfgnn_segment_bias_abi_version() == 1
    p = ctypes.addressof(ctypes.create_string_buffer(64))    # a non-NULL pointer nothing dereferences
    rows = lambda m=1, n_seg=1, ptrs=(p,) * 3: L.dfgnn_segment_pair_rows(m, n_seg, *ptrs, None)  # noqa: E731
    fwd = lambda m=1, h=1, f=32, n_pairs=1, ptrs=(p,) * 9: L.dfgnn_segment_mha_bias_fwd(  # noqa: E731
        m, h, f, 1.0, *ptrs[:2], n_pairs, *ptrs[2:], None)
    bwd = lambda m=1, h=1, f=32, n_pairs=1, ptrs=(p,) * 14: L.dfgnn_segment_mha_bias_bwd(  # noqa: E731
        m, h, f, 1.0, *ptrs[:2], n_pairs, *ptrs[2:], None)
    assert rows(m=-1) == E_BADARG and rows(n_seg=-1) == E_BADARG and rows(n_seg=0) == E_BADARG
    assert all(rows(ptrs=(p,) * k + (None,) + (p,) * (2 - k)) == E_BADARG for k in range(3))
    assert rows(m=0, n_seg=0, ptrs=(None,) * 3) == 0
    for entry, n in ((fwd, 9), (bwd, 14)):
        assert entry(m=-1) == E_BADARG and entry(h=0) == E_BADARG and entry(f=-4) == E_BADARG and entry(n_pairs=-1) == E_BADARG
        assert entry(f=48) == E_UNSUPPORTED and entry(h=65536) == E_UNSUPPORTED
        assert entry(f=48, n_pairs=-1) == E_BADARG               # extents before limits
        assert entry(m=1 << 23, h=4, f=32) == E_UNSUPPORTED      # 4 GiB of features: 32-bit row offsets
        assert entry(m=0, ptrs=(None,) * n) == 0
    for k in range(7):                                           # bounds, row_off, bias, Q, K, V, out
        assert fwd(ptrs=(p,) * k + (None,) + (p,) * (8 - k)) == E_BADARG
    assert fwd(ptrs=(p,) * 7 + (p, None)) == E_BADARG and fwd(ptrs=(p,) * 7 + (None, p)) == E_BADARG   # one statistic alone
    for k in (*range(12), 13):      # every pointer but dbias (12): that NULL is accepted there is shown where there is a device
        assert bwd(ptrs=(p,) * k + (None,) + (p,) * (13 - k)) == E_BADARG
