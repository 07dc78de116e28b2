#!/usr/bin/env python3
"""Diagnostic (stamp builds): how long a workgroup of the one-head dense pair spends between kernel entry and the start of
its body (DFGNN_DSTAMP(0)) -- the chain of dependent scalar loads that fetches the range's description -- per workgroup, in
cycles and as a share of the workgroup's residency (entry -> exit), inside the autograd step of the headline batch.
The two kernels live in two translation units and each stamp build arms one of them:
  bwd : tools/diag/build_variant.sh   stamps -DDFGNN_STAMPS                      (gt_dense_bwd_kernel)
  fwd : tools/diag/build_w_variant.sh wst    -DDFGNN_STAMPS -DDFGNN_STAMPS_TU    (gt_dense_fwd_ranked_kernel)
usage: DFGNN_LIB=libdfgnn_stamps.so desc_chain.py bwd [repeats]   |   DFGNN_LIB=libdfgnn_wst.so desc_chain.py fwd [repeats]"""
import os, sys, ctypes
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
for p in (ROOT, os.path.join(ROOT, "df-gnn_amd")):
    sys.path.insert(0, p)
import numpy as np, torch
os.environ["DFGNN_BINDING"] = "ctypes"
import dfgnn_native
from DFGNN.layers import preprocess_Hyper_fw_bw
from DFGNN.operators.fused_gtconv import GTConvFuse_hyper
from DFGNN.utils import synthetic as S
which = sys.argv[1] if len(sys.argv) > 1 else "bwd"
repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
dev = "cuda:0"
g = S.pattern_like(batch_size=1024, seed=1).to(dev)
A, rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem = preprocess_Hyper_fw_bw(g)
Q, K, V = (t.requires_grad_(True) for t in S.gt_features(g.num_nodes(), 1, 128, seed=100, device=dev))
dO = torch.randn_like(Q)
L = dfgnn_native.lib()
L.dfgnn_debug_set_dense_stamps.argtypes = [ctypes.c_void_p]


def step():
    o = GTConvFuse_hyper(rows, row_ptr, col_ind, val, col_ptr, row_ind, val_idx, smem, Q, K, V)
    torch.autograd.grad(o, (Q, K, V), dO)


for _ in range(20):
    step()
nwg = row_ptr._dfgnn_plans[128].num_dense
chain, share, resid = [], [], []
for _ in range(repeats):
    st = torch.zeros(nwg * 16, dtype=torch.int64, device=dev)
    for _ in range(3):  # (steady state: the armed step has steps ahead of it in the queue)
        step()
    torch.cuda.synchronize()
    assert L.dfgnn_debug_set_dense_stamps(st.data_ptr()) == 0
    step()
    torch.cuda.synchronize()
    assert L.dfgnn_debug_set_dense_stamps(None) == 0
    s = st.cpu().numpy().reshape(nwg, 16)
    s = s[(s[:, 0] != 0) & (s[:, 13] != 0) & (s[:, 14] != 0)]   # (bodies without a DSTAMP(0) are left out)
    c = (s[:, 0] - s[:, 14]).astype(np.float64)
    r = (s[:, 13] - s[:, 14]).astype(np.float64)
    ok = (c >= 0) & (r > 0)
    chain.append(c[ok]); resid.append(r[ok]); share.append(c[ok] / r[ok])
    print(f"{which} run: {ok.sum()} of {nwg} workgroups stamped; entry->body cycles p10 {np.percentile(c[ok], 10):.0f} "
          f"p50 {np.median(c[ok]):.0f} p90 {np.percentile(c[ok], 90):.0f} max {c[ok].max():.0f}; residency p50 {np.median(r[ok]):.0f}; "
          f"share p50 {np.median(c[ok] / r[ok]) * 100:.2f} % p90 {np.percentile(c[ok] / r[ok], 90) * 100:.2f} %")
c, r, sh = np.concatenate(chain), np.concatenate(resid), np.concatenate(share)
print(f"{which} all {repeats} runs: entry->body cycles mean {c.mean():.0f} p10 {np.percentile(c, 10):.0f} p50 {np.median(c):.0f} "
      f"p90 {np.percentile(c, 90):.0f} p99 {np.percentile(c, 99):.0f}; residency cycles p50 {np.median(r):.0f} mean {r.mean():.0f}; "
      f"share of residency p50 {np.median(sh) * 100:.2f} % p90 {np.percentile(sh, 90) * 100:.2f} % mean {sh.mean() * 100:.2f} %")
