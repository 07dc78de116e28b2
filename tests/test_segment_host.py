"""CPU: the header, loader and libraries of the segment attention pair (include/dfgnn_segment.h), its `applies` predicate
and the argument errors it answers before any device call."""
import ctypes
import os
import subprocess

import pytest

import dfgnn_native as N
from conftest import ROOT
from guarded import prototypes, stream_entries

PROTOS = prototypes(open(os.path.join(ROOT, "include", "dfgnn_segment.h")).read())
E_BADARG, E_UNSUPPORTED = -1, -2


def test_header_equals_loader():
    assert sorted(PROTOS) == sorted(N.SEGMENT_SIGNATURES)
    streams = stream_entries(PROTOS)       # (the loader's argtypes count the stream)
    assert streams == ["dfgnn_segment_bounds", "dfgnn_segment_mha_bwd", "dfgnn_segment_mha_fwd"]
    assert {n: len(p) for n, p in PROTOS.items()} == {n: len(a) for n, a in N.SEGMENT_SIGNATURES.items()}
    assert not set(PROTOS) & (set(N.SIGNATURES) | set(N.SAMPLE_SIGNATURES))


@pytest.mark.parametrize("name", ("libdfgnn.so", "libdfgnn_hip.so"))
def test_libraries_export_the_entries(name):
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "df-gnn_amd", name)], capture_output=True, text=True,
                        check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert set(PROTOS) <= exported


def test_applies_and_argument_errors_without_a_device():
    L = N.lib()
    assert L.dfgnn_segment_abi_version() == 1
    assert [L.dfgnn_segment_mha_applies(4, f) for f in (8, 16, 32, 48, 64, 128, 256)] == [0, 1, 1, 0, 1, 1, 0]
    assert L.dfgnn_segment_mha_applies(0, 32) == 0
    p = ctypes.addressof(ctypes.create_string_buffer(64))    # a non-NULL pointer nothing dereferences
    fwd = lambda m=1, h=1, f=32, ptrs=(p,) * 7: L.dfgnn_segment_mha_fwd(m, h, f, 1.0, *ptrs, None)  # noqa: E731
    bwd = lambda m=1, h=1, f=32, ptrs=(p,) * 12: L.dfgnn_segment_mha_bwd(m, h, f, 1.0, *ptrs, None)  # noqa: E731
    assert L.dfgnn_segment_bounds(-1, 1, p, p, None) == E_BADARG and L.dfgnn_segment_bounds(1, -1, p, p, None) == E_BADARG
    assert L.dfgnn_segment_bounds(1, 0, p, p, None) == E_BADARG
    assert L.dfgnn_segment_bounds(1, 1, None, p, None) == E_BADARG and L.dfgnn_segment_bounds(1, 1, p, None, None) == E_BADARG
    assert L.dfgnn_segment_bounds(0, 0, None, None, None) == 0
    for entry in (fwd, bwd):
        assert entry(m=-1) == E_BADARG and entry(h=0) == E_BADARG and entry(f=-4) == E_BADARG
        assert entry(f=48) == E_UNSUPPORTED and entry(h=65536) == E_UNSUPPORTED
        assert entry(m=1 << 23, h=4, f=32) == E_UNSUPPORTED      # 4 GiB of features: 32-bit row offsets
        assert entry(m=0, ptrs=(None,) * (7 if entry is fwd else 12)) == 0
    for k in range(5):                                           # bounds, Q, K, V, out
        assert fwd(ptrs=(p,) * k + (None,) + (p,) * (6 - k)) == E_BADARG
    assert fwd(ptrs=(p,) * 5 + (p, None)) == E_BADARG            # one statistic without the other
    for k in (0, 1, 2, 3, 5, 6, 7, 8, 9, 10, 11):                # every pointer but `out`
        assert bwd(ptrs=(p,) * k + (None,) + (p,) * (11 - k)) == E_BADARG
