"""The neighbour sampler on the device (csrc/neighbor.hip, graphgym_amd.neighbor): every hand-made base under five fanout
lists and every kind of seed set against the NumPy restatement, tensor for tensor; the batch's CSR against
CSRGraph.from_edge_index; a hub row at the fanouts around the 16-lane group and at the largest one, as a seed and as a
hop-1 node, on a star and on the star with every link stored twice; a side stream; a 2-layer harness.GNN on a batch of
whole rows against the model on the full base; and examples/train_sampled_ba.py --sampler neighbor_subgraph, scaled down."""
import importlib.util
import math
import os

import pytest
import torch

import _sampler_graphs as SG
from _tol import both, close
from graphgym_amd import CSRGraph
from graphgym_amd import neighbor as NB
from graphgym_amd.link_pred import _on_cpu
from test_neighbor_host import SIZES, seed_sets

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_cache = {}


def _base(name, dev):
    """(device base, the same base on the CPU), built once per session"""
    if name not in _cache:
        g = SG.build(name, dev)
        _cache[name] = (g, _on_cpu(g))
    return _cache[name]


def _same_batch(a, b):
    assert a.num_nodes == b.num_nodes and a.graph.nnz == b.graph.nnz and a.graph.num_nodes == b.graph.num_nodes
    assert a.graph.symmetric is False and b.graph.symmetric is False
    for f in ("orig_node", "edge_index", "base_entry", "hop", "seed_index"):
        x, y = getattr(a, f), getattr(b, f)
        assert x.dtype == y.dtype and torch.equal(x.cpu(), y.cpu()), f
    for f in ("rowptr", "col", "eid"):
        x, y = getattr(a.graph, f), getattr(b.graph, f)
        assert x.dtype == y.dtype and torch.equal(x.cpu(), y.cpu()), f


@pytest.mark.parametrize("name", sorted(SG.CASES))
def test_device_batch_equals_the_host_restatement(dev, name):
    g, h = _base(name, dev)
    for sizes in SIZES:
        plan, host = NB.plan_neighbor(g, sizes, 3), NB.plan_neighbor(h, sizes, 3)
        for seeds in seed_sets(name):
            for seed, step in ((1, 0), (2 ** 40 + 3, 5)):
                got = NB.neighbor_batch_nodes(plan, torch.tensor(seeds, device=dev), seed, step)
                assert got.orig_node.is_cuda and got.hop.dtype == torch.int32
                _same_batch(got, NB.neighbor_batch_host(host, seed, step, torch.tensor(seeds)))
        for step in (0, plan.num_batches - 1, plan.num_batches + 1):
            s = NB.seeds(plan, 7, step)
            assert s.dtype == torch.int32 and s.is_cuda and torch.equal(s.cpu(), NB.seeds_host(host, 7, step))
            _same_batch(NB.neighbor_batch(plan, 7, step), NB.neighbor_batch_host(host, 7, step))
    pool = torch.arange(g.num_nodes - 1, -1, -2)                                  # a pool of its own, descending
    plan, host = NB.plan_neighbor(g, [2, 2], 2, pool.to(dev)), NB.plan_neighbor(h, [2, 2], 2, pool)
    for step in range(plan.num_batches):
        _same_batch(NB.neighbor_batch(plan, 3, step), NB.neighbor_batch_host(host, 3, step))


@pytest.mark.parametrize("name", sorted(SG.CASES))
def test_batch_graph_is_what_from_edge_index_builds(dev, name):
    g, _ = _base(name, dev)
    for sizes in SIZES:
        b = NB.neighbor_batch(NB.plan_neighbor(g, sizes, 3), 3, 0)              # (every case holds at least three nodes)
        n = b.num_nodes
        assert b.edge_index.dtype == torch.int64 and tuple(b.edge_index.shape) == (2, b.graph.nnz)
        assert b.orig_node.dtype == torch.int64 and b.orig_node.numel() == n and n >= 3
        ref = CSRGraph.from_edge_index(b.edge_index, n)
        assert torch.equal(ref.rowptr, b.graph.rowptr) and torch.equal(ref.col, b.graph.col)
        assert torch.equal(ref.eid, b.graph.eid)
        assert torch.equal(b.graph.eid, torch.arange(b.graph.nnz, dtype=torch.int32, device=dev))
        # base_entry names the base's entry of every kept edge
        assert torch.equal(g.col.long()[b.base_entry.long()], b.orig_node[b.edge_index[0]])
        assert torch.equal(g.row_ids().long()[b.base_entry.long()], b.orig_node[b.edge_index[1]])


@pytest.mark.parametrize("twice", [False, True], ids=["star5000", "star5000_twice"])
def test_a_hub_row_as_a_seed_and_as_a_hop_1_node(dev, twice):
    """node 0 is linked to 1 .. 5000 (N = 5001, no multiple of 32): its row holds 5000 entries (10000 with every link
    stored twice) and is drawn by one 16-lane group at the fanouts 1, 16, 17, 256 and as a whole"""
    n = 5001
    leaves = torch.arange(1, n)
    star = torch.stack([torch.zeros(n - 1, dtype=torch.int64), leaves])
    ei = torch.cat([star, star.flip(0)] * (2 if twice else 1), 1)
    g = CSRGraph.from_edge_index(ei.to(dev), n)
    h = _on_cpu(g)
    deg0 = (n - 1) * (2 if twice else 1)
    assert int(g.rowptr[1]) == deg0
    for fanout in (1, 16, 17, 256, -1):
        k = deg0 if fanout < 0 else fanout
        for sizes, seeds in (([fanout], [0, 4097]), ([1, fanout], [77]), ([fanout, fanout], [0])):
            plan, host = NB.plan_neighbor(g, sizes, 1), NB.plan_neighbor(h, sizes, 1)
            got = NB.neighbor_batch_nodes(plan, torch.tensor(seeds, device=dev), 13, 2)
            _same_batch(got, NB.neighbor_batch_host(host, 13, 2, torch.tensor(seeds)))
            assert int(got.orig_node[0]) == 0 and int(got.graph.rowptr[1]) == k            # the hub's row
            row = got.base_entry[:k].long()
            assert bool((row[1:] > row[:-1]).all()) and int(row[-1]) < deg0
            assert int(got.hop[0]) == (0 if seeds[0] == 0 else 1)


def test_a_side_stream_builds_the_same_batch(dev):
    g, _ = _base("ring65", dev)
    plan = NB.plan_neighbor(g, [3, -1, 2], 9)
    a = NB.neighbor_batch(plan, 9, 2)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        b = NB.neighbor_batch(plan, 9, 2)
        c = NB.neighbor_batch_nodes(plan, NB.seeds(plan, 9, 2), 9, 2)
    side.synchronize()
    _same_batch(a, b)
    _same_batch(a, c)


@pytest.fixture()
def gcfg():
    from graphgym_amd.config import cfg
    import graphgym_amd.graphgym_plugin  # noqa: F401  (registers the layer keys)
    keys = ("gnn", "dataset", "bn", "mem", "train", "val", "model")
    saved = {k: dict(vars(getattr(cfg, k))) for k in keys}
    yield cfg
    for k, v in saved.items():
        ns = getattr(cfg, k)
        for name in list(vars(ns)):
            if name not in v:
                delattr(ns, name)
        for name, val in v.items():
            setattr(ns, name, val)


def _oracle(layer_type, state, x, ei):
    """the 2-layer stack (layer -> ReLU, twice) and the head's Linear on the CPU, in float64 and in float32"""
    from oracle import ref_layers as RL

    def run(c):
        t = lambda k: c(state[k].detach().cpu())
        h = c(x)
        for i in range(2):
            p = f"mp.layer{i}.layer.model."
            if layer_type == "sageconv":
                h = RL.pyg_sage_conv(h, ei, t(p + "lin_l.weight"), t(p + "lin_l.bias"), t(p + "lin_r.weight"))
            else:
                def nn_fn(z, p=p):
                    z = torch.relu(z @ t(p + "nn.0.weight").t() + t(p + "nn.0.bias"))
                    return z @ t(p + "nn.2.weight").t() + t(p + "nn.2.bias")
                h = RL.pyg_gin_conv(h, ei, nn_fn, float(state[p + "eps"]))
            h = torch.relu(h)
        return h @ t("post_mp.layer_post_mp.model.0.model.weight").t() + t("post_mp.layer_post_mp.model.0.model.bias")
    return both(run)


@pytest.mark.parametrize("layer_type", ["sageconv", "ginconv"])
def test_whole_rows_give_the_full_graph_prediction_at_the_seeds(dev, gcfg, layer_type):
    """sizes [-1, -1]: every row a 2-layer model reads on the way to a seed is a whole base row, so the prediction at the
    seeds is the full-graph model's.  Both are held to a float64 evaluation of the full-graph model, 1e-5 per row."""
    from graphgym_amd import harness as H
    c = gcfg
    c.gnn.layers_pre_mp, c.gnn.layers_mp, c.gnn.layers_post_mp, c.gnn.dim_inner = 0, 2, 1, 16
    c.gnn.layer_type, c.gnn.stage_type, c.gnn.batchnorm, c.gnn.act, c.gnn.dropout = layer_type, "stack", False, "relu", 0.0
    c.gnn.agg, c.gnn.normalize_adj, c.gnn.l2norm = "mean", False, False
    c.dataset.task, c.dataset.transform = "node", "none"
    g, _ = _base("ring65", dev)
    N = 65
    gen = torch.Generator().manual_seed(12)
    x, y = torch.randn(N, 8, generator=gen), torch.randint(0, 3, (N,), generator=gen)
    torch.manual_seed(5)
    model = H.GNN(8, 3).to(dev).eval()
    ei, _ = SG.edge_index("ring65")
    ref64, ref32 = _oracle(layer_type, model.state_dict(), x, ei)
    mask = torch.arange(N) % 4 == 1
    loader = NB.NeighborLoader(g, x.to(dev), y.to(dev), mask.to(dev), NB.plan_neighbor(g, [-1, -1], 5), seed=3)
    full = H.Batch(node_feature=x.to(dev), node_label=y.to(dev), node_label_index=torch.arange(N, device=dev),
                   edge_index=ei.to(dev), num_nodes=N)
    with torch.no_grad():
        pred_full, _ = model(full)
        close(pred_full, (ref64, ref32), what=f"{layer_type} on the full base")
        seen = []
        for batch in loader:
            assert int(batch.hop.max()) == 2 and bool((batch.hop[batch.node_label_index] == 0).all())
            seeds = batch.orig_node[batch.node_label_index].cpu()
            pred, true = model(batch)
            assert torch.equal(true.cpu(), y[seeds])
            close(pred, (ref64[seeds], ref32[seeds]), what=f"{layer_type} at the seeds")
            seen += seeds.tolist()
    assert sorted(seen) == torch.nonzero(mask).view(-1).tolist()


def test_the_sampled_example_trains_on_neighbor_batches(dev, gcfg):
    """examples/train_sampled_ba.py --sampler neighbor_subgraph on BA(4000, 5): three epochs of 256 seeds a batch under the
    fanouts [20, 15, 10] of the example's three message-passing layers; the loss is finite and falls"""
    spec = importlib.util.spec_from_file_location("train_sampled_ba", os.path.join(ROOT, "examples", "train_sampled_ba.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    records = mod.main(["--nodes", "4000", "--epochs", "3", "--sampler", "neighbor_subgraph", "--batch-size", "256"])
    assert [r["epoch"] for r in records] == [0, 1, 2] and all(r["sampler"] == "neighbor_subgraph" for r in records)
    assert all(math.isfinite(r["train_loss"]) and math.isfinite(r["val_acc"]) for r in records)
    assert all(r["batches"] == 13 for r in records)                               # about 3200 training nodes, 256 a batch
    assert records[2]["train_loss"] < records[1]["train_loss"] < records[0]["train_loss"], records
