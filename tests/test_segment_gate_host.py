"""CPU: header, loader and libraries of the segment attention pair with pair gates (include/dfgnn_segment_gate.h) and its
argument errors.  That an optional pointer may be NULL is shown in tests/test_gpu_segment_gate.py: a call that passes launches."""
import ctypes
import os
import subprocess

import pytest

import dfgnn_native as N
from conftest import ROOT
from guarded import prototypes, stream_entries

PROTOS = prototypes(open(os.path.join(ROOT, "include", "dfgnn_segment_gate.h")).read())
E_BADARG, E_UNSUPPORTED = -1, -2


def test_header_equals_loader():
    assert sorted(PROTOS) == sorted(N.SEGMENT_GATE_SIGNATURES)
    assert stream_entries(PROTOS) == ["dfgnn_segment_mha_gate_bwd", "dfgnn_segment_mha_gate_fwd"]
    assert {n: len(p) for n, p in PROTOS.items()} == {n: len(a) for n, a in N.SEGMENT_GATE_SIGNATURES.items()}
    assert not any(set(PROTOS) & set(t) for t in (N.SIGNATURES, N.SAMPLE_SIGNATURES, N.SEGMENT_SIGNATURES, N.SEGMENT_BIAS_SIGNATURES,
                                                  N.SEGMENT_TBIAS_SIGNATURES, N.SEGMENT_CROSS_SIGNATURES))


@pytest.mark.parametrize("name", ("libdfgnn.so", "libdfgnn_hip.so"))
def test_libraries_export_the_entries(name):
    nm = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "df-gnn_amd", name)], capture_output=True, text=True,
                        check=True).stdout
    assert set(PROTOS) <= {line.split()[-1] for line in nm.splitlines() if line.strip()}


def test_argument_errors_without_a_device():
    L = N.lib()
    assert L.dfgnn_segment_gate_abi_version() == 1
    p = ctypes.addressof(ctypes.create_string_buffer(64))    # a non-NULL pointer nothing dereferences
    fwd = lambda m=1, h=1, f=32, n_pairs=1, ptrs=(p,) * 11: L.dfgnn_segment_mha_gate_fwd(  # noqa: E731
        m, h, f, 1.0, *ptrs[:2], n_pairs, *ptrs[2:], None)
    bwd = lambda m=1, h=1, f=32, n_pairs=1, ptrs=(p,) * 17: L.dfgnn_segment_mha_gate_bwd(  # noqa: E731
        m, h, f, 1.0, *ptrs[:2], n_pairs, *ptrs[2:], None)
    hole = lambda n, *ks: tuple(None if i in ks else p for i in range(n))  # noqa: E731
    for entry, n in ((fwd, 11), (bwd, 17)):
        assert entry(m=-1) == E_BADARG and entry(h=0) == E_BADARG and entry(f=-4) == E_BADARG and entry(n_pairs=-1) == E_BADARG
        assert entry(f=48) == E_UNSUPPORTED and entry(h=65536) == E_UNSUPPORTED
        assert entry(f=48, n_pairs=-1) == E_BADARG               # extents before limits
        assert entry(m=1 << 23, h=4, f=32) == E_UNSUPPORTED      # 4 GiB of features: 32-bit row offsets
        assert entry(f=48, ptrs=(None,) * n) == E_UNSUPPORTED    # limits before pointers
        assert entry(m=0, ptrs=(None,) * n) == 0
    # fwd: bounds, row_off, bias, gate (3, optional), Q, K, V, out, row_max, row_sum, logits (10, optional)
    for k in (0, 1, 2, 4, 5, 6, 7):
        assert fwd(ptrs=hole(11, k)) == E_BADARG
    assert fwd(ptrs=hole(11, 8)) == E_BADARG and fwd(ptrs=hole(11, 9)) == E_BADARG      # one statistic alone
    # bwd: bounds, row_off, bias, gate (3), Q, K, V, row_max, row_sum, dO, dlogits (10), dQ, dK, dV, dbias (14), dgate (15), delta
    for k in (0, 1, 2, 4, 5, 6, 7, 8, 9, 11, 12, 13, 16):
        assert bwd(ptrs=hole(17, k)) == E_BADARG
    assert bwd(ptrs=hole(17, 3)) == E_BADARG                     # dgate without gate
    assert bwd(ptrs=hole(17, 0, 3, 10, 14, 15)) == E_BADARG      # bounds missing; every optional one NULL changes nothing
