"""CPU: the header, loader and libraries of the segment attention pair with a typed pair bias (include/dfgnn_segment_tbias.h)
and the argument errors it answers before any device call."""
import ctypes
import os
import subprocess

import pytest

import dfgnn_native as N
from conftest import ROOT
from guarded import prototypes, stream_entries

PROTOS = prototypes(open(os.path.join(ROOT, "include", "dfgnn_segment_tbias.h")).read())
E_BADARG, E_UNSUPPORTED = -1, -2


def test_header_equals_loader():
    assert sorted(PROTOS) == sorted(N.SEGMENT_TBIAS_SIGNATURES)
    assert stream_entries(PROTOS) == ["dfgnn_segment_mha_tbias_bwd", "dfgnn_segment_mha_tbias_fwd"]
    assert {n: len(p) for n, p in PROTOS.items()} == {n: len(a) for n, a in N.SEGMENT_TBIAS_SIGNATURES.items()}
    assert not set(PROTOS) & (set(N.SIGNATURES) | set(N.SAMPLE_SIGNATURES) | set(N.SEGMENT_SIGNATURES) |
                              set(N.SEGMENT_BIAS_SIGNATURES))


@pytest.mark.parametrize("name", ("libdfgnn.so", "libdfgnn_hip.so"))
def test_libraries_export_the_entries(name):
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "df-gnn_amd", name)], capture_output=True, text=True,
                        check=True).stdout
    exported = {line.split()[-1] for line in nm.splitlines() if line.strip()}
    assert set(PROTOS) <= exported


def test_argument_errors_without_a_device():
    L = N.lib()
    assert L.dfgnn_segment_tbias_abi_version() == 1
    ws = L.dfgnn_segment_mha_tbias_ws_floats
    assert ws(0, 4, 20) == 0 and all(ws(m, h, T) >= -(-m // 128) * h * T for m, h, T in ((1, 1, 1), (128, 8, 48), (129, 8, 256), (100000, 3, 97)))
    assert ws(-1, 1, 1) == E_BADARG and ws(1, 0, 1) == E_BADARG and ws(1, 1, 0) == E_BADARG and ws(1, 1, 257) == E_UNSUPPORTED
    p = ctypes.addressof(ctypes.create_string_buffer(64))    # a non-NULL pointer nothing dereferences
    fwd = lambda m=1, h=1, f=32, n_pairs=1, T=4, ptrs=(p,) * 10: L.dfgnn_segment_mha_tbias_fwd(  # noqa: E731
        m, h, f, 1.0, *ptrs[:2], n_pairs, ptrs[2], T, *ptrs[3:], None)
    bwd = lambda m=1, h=1, f=32, n_pairs=1, T=4, ptrs=(p,) * 16: L.dfgnn_segment_mha_tbias_bwd(  # noqa: E731
        m, h, f, 1.0, *ptrs[:2], n_pairs, ptrs[2], T, *ptrs[3:], None)
    for entry, n in ((fwd, 10), (bwd, 16)):
        assert entry(m=-1) == E_BADARG and entry(h=0) == E_BADARG and entry(f=-4) == E_BADARG and entry(n_pairs=-1) == E_BADARG
        assert entry(T=0) == E_BADARG and entry(T=257) == E_UNSUPPORTED and entry(T=256, ptrs=(None,) * n) == E_BADARG
        assert entry(f=48) == E_UNSUPPORTED and entry(h=65536) == E_UNSUPPORTED
        assert entry(f=48, T=0) == E_BADARG and entry(T=257, n_pairs=-1) == E_BADARG      # extents before limits
        assert entry(T=257, ptrs=(None,) * n) == E_UNSUPPORTED                           # limits before pointers
        assert entry(m=1 << 23, h=4, f=32) == E_UNSUPPORTED      # 4 GiB of features: 32-bit row offsets
        assert entry(m=0, ptrs=(None,) * n) == 0
    for k in range(8):                                           # bounds, row_off, types, B, Q, K, V, out
        assert fwd(ptrs=(p,) * k + (None,) + (p,) * (9 - k)) == E_BADARG
    assert fwd(ptrs=(p,) * 8 + (p, None)) == E_BADARG and fwd(ptrs=(p,) * 8 + (None, p)) == E_BADARG   # one statistic alone
    for k in (*range(13), 14, 15):  # every pointer but dB (13); ws (14) is required with dB.  dB = NULL: where there is a device
        assert bwd(ptrs=(p,) * k + (None,) + (p,) * (15 - k)) == E_BADARG
