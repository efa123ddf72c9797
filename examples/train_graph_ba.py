#!/usr/bin/env python3
"""Graph classification with the graph-task loaders: the shape of the reference's run/configs/IDGNN/graph.yaml (1 pre / 3
message-passing / 3 post layers of width 128, add aggregation and add pooling, l2norm, batch size 64, an 80/20 inductive
split) on synthetic BA(n, m) graphs from graphgen instead of the bundled ba500 set.  Label: the balanced class (10 bins)
of a graph's average shortest path length, computed on the device (structure.augment, label="graph_path_len"); features:
a constant 1 and log(1 + degree) per node (a constant column alone is what the first BatchNorm maps to zero).  Two
models on the same split: idconv on ego batches (dataset.transform: ego) and generalconv on plain batches.  Train and
validation accuracy are printed per eval period.

    python examples/train_graph_ba.py --graphs 512 --epochs 60
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graphgym_amd.graphgym_plugin  # noqa: E402,F401  (registers the layer keys)
from graphgym_amd import graph_loader as GL, graphgen, harness as H, structure  # noqa: E402
from graphgym_amd.config import cfg  # noqa: E402


def accuracy(model, loader):
    model.eval()
    hit = total = 0
    with torch.no_grad():
        for batch in loader:
            pred, true = model(batch)
            hit += int((pred.argmax(1) == true).sum())
            total += true.numel()
    return hit / max(total, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=512)
    ap.add_argument("--min-nodes", type=int, default=20)
    ap.add_argument("--max-nodes", type=int, default=60)
    ap.add_argument("--epochs", type=int, default=60)
    ap.add_argument("--eval-period", type=int, default=20)
    ap.add_argument("--batch-size", type=int, default=64)
    ap.add_argument("--lr", type=float, default=0.01)
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")

    cfg.gnn.layers_pre_mp, cfg.gnn.layers_mp, cfg.gnn.layers_post_mp, cfg.gnn.dim_inner = 1, 3, 3, 128
    cfg.gnn.stage_type, cfg.gnn.batchnorm, cfg.gnn.act, cfg.gnn.dropout = "stack", True, "relu", 0.0
    cfg.gnn.agg, cfg.gnn.normalize_adj, cfg.gnn.l2norm = "add", False, True
    cfg.model.graph_pooling = "add"
    cfg.dataset.task, cfg.dataset.split, cfg.dataset.shuffle_split = "graph", [0.8, 0.2], True
    cfg.train.batch_size = args.batch_size

    rng = np.random.RandomState(args.seed)
    graphs = []
    for i in range(args.graphs):
        n, m = int(rng.randint(args.min_nodes, args.max_nodes + 1)), int(rng.randint(1, 4))
        ei = graphgen.connected_ba_edge_index(n, m, seed=1000 + i)
        deg = torch.bincount(ei[1], minlength=n).float()
        graphs.append((ei, torch.stack([torch.ones(n), deg.log1p()], 1), torch.tensor(0)))
    ds = GL.GraphDataset.from_graphs(graphs, dev)
    tensors, _, classes = structure.augment(ds.base, torch.from_numpy(ds.graph_ptr), [], [], label="graph_path_len",
                                            label_dim=10)
    ds.graph_label = tensors["graph_path_len_label"].to(dev).long()

    for layer_type, transform in (("idconv", "ego"), ("generalconv", "none")):
        cfg.gnn.layer_type, cfg.dataset.transform = layer_type, transform
        train, val = GL.graph_loaders_from_cfg(cfg, ds, seed=args.seed)
        train_eval = GL.GraphLoader(ds, train.ids, args.batch_size, shuffle=False, transform=transform,
                                    radius=cfg.gnn.layers_mp)
        torch.manual_seed(args.seed)
        model = H.GNN(2, classes).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=args.lr)
        for epoch in range(args.epochs):
            model.train()
            torch.cuda.synchronize()
            t0, losses = time.time(), []
            for batch in train:
                def loss_fn(batch=batch):
                    pred, true = model(batch)
                    return F.cross_entropy(pred, true)
                losses.append(H.train_step(model, opt, loss_fn))
            torch.cuda.synchronize()
            seconds = time.time() - t0
            if (epoch + 1) % args.eval_period == 0 or epoch == args.epochs - 1:
                print(json.dumps({"layer_type": layer_type, "transform": transform, "epoch": epoch,
                                  "train_loss": round(float(torch.stack(losses).mean()), 4),
                                  "train_acc": round(accuracy(model, train_eval), 4),
                                  "val_acc": round(accuracy(model, val), 4), "classes": classes,
                                  "batches": len(train), "epoch_seconds": round(seconds, 3)}), flush=True)


if __name__ == "__main__":
    main()
