"""CPU: the general statistics pair (dfgnn_gt_fwd_rowstats / dfgnn_gt_bwd_rowstats) is declared, exported, bound and
validates its arguments before any GPU call; the operator and the layers import."""
import ctypes
import os
import re

from conftest import ROOT

NAMES = ("dfgnn_gt_fwd_rowstats", "dfgnn_gt_bwd_rowstats")


def test_symbols_declared_exported_and_bound():
    import dfgnn_native
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dfgnn.h")).read(), flags=re.S)
    raw = ctypes.CDLL(dfgnn_native.LIB_PATH)
    for n in NAMES:
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), n
        assert hasattr(raw, n), n
        assert n in dfgnn_native.SIGNATURES
    assert len(dfgnn_native.SIGNATURES["dfgnn_gt_fwd_rowstats"]) == 14
    assert len(dfgnn_native.SIGNATURES["dfgnn_gt_bwd_rowstats"]) == 22
    assert dfgnn_native.lib().dfgnn_abi_version() == 11


def test_argument_checks_need_no_gpu():
    """A missing pointer is DFGNN_E_BADARG, an empty problem succeeds: both answered before any launch."""
    import dfgnn_native
    L = dfgnn_native.lib()
    buf = (ctypes.c_float * 64)()
    idx = (ctypes.c_int * 8)(0, 1, 2, 2, 0, 0, 0, 0)
    p, i = ctypes.addressof(buf), ctypes.addressof(idx)
    fwd = lambda m, Q, mx=p, sm=p: L.dfgnn_gt_fwd_rowstats(m, 2, 1, 4, i, i, None, Q, p, p, mx, sm, p, None)  # noqa: E731
    bwd = lambda m, Q, delta=p: L.dfgnn_gt_bwd_rowstats(m, 2, 1, 4, i, i, None, i, i, None, Q, p, p, p, p, p, p, delta, p,  # noqa: E731
                                                        p, p, None)
    assert fwd(3, None) == -1 and bwd(3, None) == -1
    assert fwd(3, p, mx=None) == -1                    # one statistic without the other
    assert bwd(3, p, delta=None) == -1
    assert fwd(-1, p) == -1 and bwd(-1, p) == -1
    assert fwd(0, p) == 0 and bwd(0, p) == 0
    assert fwd(0, None) == 0 and bwd(0, None) == 0
    assert L.dfgnn_gt_fwd_rowstats(3, 2, 70000, 4, i, i, None, p, p, p, p, p, p, None) == -2   # h > 65535


def test_operator_and_layers_import():
    import argparse

    import fused_gtconv
    from DFGNN.layers import SparseMHA_rowstats, load_graphconv_layer, load_prepfunc, preprocess_Hyper_fw_bw
    from DFGNN.layers.GT import SparseMHA_rowstats_timing
    from DFGNN.operators.fused_gtconv import FusedGTFunction_rowstats, GTConvFuse_rowstats
    assert callable(fused_gtconv.gt_forward_rowstats) and callable(fused_gtconv.gt_backward_rowstats)
    assert callable(GTConvFuse_rowstats) and hasattr(FusedGTFunction_rowstats, "apply")
    args = argparse.Namespace(conv="gt", format="forward_rowstats", dim=64, heads=2)
    assert isinstance(load_graphconv_layer(args), SparseMHA_rowstats_timing)
    assert load_prepfunc(args) is preprocess_Hyper_fw_bw
    assert SparseMHA_rowstats(64, 64, 2).head_dim == 32
