#!/usr/bin/env python3
"""Full-graph GT training on the synthetic stand-ins (the pattern of the reference's full-graph trainer,
DFGNN/script/train/train_full_graph_timing.py: one graph, preprocessing once, N attention layers sharing it, Adam),
with the fused convolution of choice:
  --op hyper      GTConvFuse_hyper     (a full graph takes its attn_edge form: 8 h nnz bytes alive per layer)
  --op rowstats   GTConvFuse_rowstats  (row statistics instead, the attention recomputed in the backward)
Prints one JSON line: ms per epoch (forward + backward + update), the final loss and the peak of allocated device memory.
usage: python3 tools/train_full_graph.py --dataset reddit --scale 0.1 --op rowstats [--layers 2] [--heads 1] [--dim 128]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "df-gnn_amd")):
    sys.path.insert(0, p)
import torch  # noqa: E402
from torch import nn  # noqa: E402

from DFGNN.layers import SparseMHA_forward, SparseMHA_rowstats, preprocess_Hyper_fw_bw  # noqa: E402
from DFGNN.utils import load_data_full_graph  # noqa: E402

LAYER = {"hyper": SparseMHA_forward, "rowstats": SparseMHA_rowstats}


class Net(nn.Module):
    def __init__(self, op, layers, in_dim, dim, heads, classes):
        super().__init__()
        self.inproj = nn.Linear(in_dim, dim)
        self.layers = nn.ModuleList(LAYER[op](dim, dim, heads) for _ in range(layers))
        self.out = nn.Linear(dim, classes)

    def forward(self, params, x):
        h = self.inproj(x)
        for layer in self.layers:
            h = layer(params, h, fuse=True)
        return self.out(h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dataset", default="cora", choices=["cora", "reddit"])
    ap.add_argument("--scale", type=float, default=None, help="reddit only: fraction of the full-size graph")
    ap.add_argument("--op", default="rowstats", choices=sorted(LAYER))
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--heads", type=int, default=1)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    g = load_data_full_graph(args.dataset, scale=args.scale)
    x = g.ndata["feat"][:, :args.dim].to(dev)
    labels = torch.randint(args.classes, (g.num_nodes(),), generator=torch.Generator().manual_seed(1)).to(dev)
    params = preprocess_Hyper_fw_bw(g.to(dev), True)
    model = Net(args.op, args.layers, x.shape[1], args.dim, args.heads, args.classes).to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    loss_fn = nn.CrossEntropyLoss()

    def epoch():
        loss = loss_fn(model(params, x), labels)
        opt.zero_grad()
        loss.backward()
        opt.step()
        return loss

    for _ in range(args.warmup):
        epoch()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    t0 = time.perf_counter()
    for _ in range(args.epochs):
        loss = epoch()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / max(args.epochs, 1) * 1e3
    print(json.dumps({"tool": "train_full_graph", "dataset": args.dataset, "scale": args.scale, "op": args.op,
                      "layers": args.layers, "heads": args.heads, "dim": args.dim, "nodes": g.num_nodes(),
                      "edges": g.num_edges(), "epochs": args.epochs, "ms_per_epoch": round(ms, 3),
                      "final_loss": round(float(loss), 6), "max_memory_allocated": torch.cuda.max_memory_allocated()}))


if __name__ == "__main__":
    main()
