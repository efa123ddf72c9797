#!/usr/bin/env python3
"""Mini-batch training on one graph with a sampled-subgraph loader: the model of the reference's
run/configs/pyg/example_node.yaml (sageconv + skipsum, 1 pre / 3 message-passing / 1 post layer, prelu, dropout 0.1,
mean aggregation) with train.sampler: saint_rw, on a BA(n, 5) graph from graphgen instead of ogbn-arxiv (the dataset is
not bundled).  Task: a synthetic one — the balanced degree class of a node (graphgym_amd.structure.augment bins the
degrees on the device) from a noisy copy of its log-degree.  Validation runs on the whole graph (val.sampler: full_batch).

    python examples/train_sampled_ba.py --nodes 200000 --epochs 5 --sampler saint_rw
    python examples/train_sampled_ba.py --nodes 200000 --epochs 5 --sampler neighbor_subgraph --batch-size 1024

neighbor_subgraph (graphgym_amd/neighbor.py) trains on the sampled tree of --batch-size seed nodes under the fanouts
cfg.train.neighbor_sizes[:3] = [20, 15, 10], with the loss on the seeds; an epoch visits every training node once.
"""
import argparse
import json
import os
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import graphgym_amd as ga  # noqa: E402
import graphgym_amd.graphgym_plugin  # noqa: E402,F401  (registers the layer keys)
from graphgym_amd import graphgen, harness as H, samplers, structure  # noqa: E402
from graphgym_amd.config import cfg  # noqa: E402


def main(argv=None):
    """one JSON line per epoch; returns the records"""
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=200000)
    ap.add_argument("--epochs", type=int, default=5)
    ap.add_argument("--sampler", default="saint_rw", choices=samplers.KINDS + ("full_batch", "neighbor_subgraph"))
    ap.add_argument("--batch-size", type=int, default=2000,
                    help="roots / draws per batch (saint_*), seeds per batch (neighbor_subgraph)")
    ap.add_argument("--parts", type=int, default=16, help="train.train_parts (random_node)")
    ap.add_argument("--seed", type=int, default=0)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    n, classes = args.nodes, 10

    cfg.gnn.layers_pre_mp, cfg.gnn.layers_mp, cfg.gnn.layers_post_mp, cfg.gnn.dim_inner = 1, 3, 1, 128
    cfg.gnn.layer_type, cfg.gnn.stage_type, cfg.gnn.batchnorm, cfg.gnn.act = "sageconv", "skipsum", True, "prelu"
    cfg.gnn.dropout, cfg.gnn.agg, cfg.gnn.normalize_adj = 0.1, "mean", False
    cfg.dataset.task = "node"
    cfg.train.sampler, cfg.train.batch_size, cfg.train.walk_length = args.sampler, args.batch_size, 4
    cfg.train.iter_per_epoch, cfg.train.train_parts = 32, args.parts

    base = ga.CSRGraph.from_edge_index(graphgen.ba_edge_index(n, 5, seed=1, device=dev), n)
    tensors, _, classes = structure.augment(base, torch.tensor([0, n]), [], [], label="node_degree", label_dim=classes)
    y = tensors["node_degree_label"].to(dev).long()
    deg = (base.rowptr[1:] - base.rowptr[:-1]).float()
    noise = torch.randn(n, generator=torch.Generator().manual_seed(args.seed + 1)).to(dev)
    x = torch.stack([torch.ones(n, device=dev), deg.log1p() + 0.5 * noise], 1)
    gen = torch.Generator().manual_seed(args.seed)
    train_mask = (torch.rand(n, generator=gen) < 0.8).to(dev)

    torch.manual_seed(args.seed)
    model = H.GNN(x.size(1), classes).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=cfg.optim.base_lr)
    train = samplers.loader_from_cfg(cfg, base, x, y, train_mask, "train", seed=args.seed)
    val = samplers.loader_from_cfg(cfg, base, x, y, ~train_mask, "val")
    records = []
    for epoch in range(args.epochs):
        model.train()
        torch.cuda.synchronize()
        t0, losses, nodes = time.time(), [], 0
        for batch in train:
            def loss_fn(batch=batch):
                pred, true = model(batch)
                return F.cross_entropy(pred, true)
            losses.append(H.train_step(model, opt, loss_fn))
            nodes += batch.num_nodes
        torch.cuda.synchronize()
        seconds = time.time() - t0
        model.eval()
        with torch.no_grad():
            pred, true = model(next(iter(val)))
        records.append({"epoch": epoch, "sampler": args.sampler, "batches": len(train),
                        "nodes_per_batch": nodes // len(train), "train_loss": float(torch.stack(losses).mean()),
                        "val_acc": float((pred.argmax(1) == true).float().mean()), "seconds": round(seconds, 3)})
        print(json.dumps(records[-1]), flush=True)
    return records


if __name__ == "__main__":
    main()
