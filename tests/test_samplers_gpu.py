"""Mini-batch subgraph samplers on the device (csrc/sample.hip, graphgym_amd.samplers): every kind on every hand-made
base and on BA(2000, 3) against the NumPy restatement, bit for bit; the batch's CSR against CSRGraph.from_edge_index and
the torch formulation of the induced subgraph, independently of the restatement; a long row; a side stream; layers on the
seeded graph cache against the edge_index path; and the scaled-down example_node.yaml through harness.GNN."""
import pytest
import torch

import _sampler_graphs as SG
from _tol import close, close_all
from graphgym_amd import CSRGraph
from graphgym_amd import samplers as S
from graphgym_amd.link_pred import _on_cpu

pytestmark = pytest.mark.gpu

BASES = sorted(SG.CASES) + ["ba2000"]
_cache = {}


def _base(name, dev):
    """(device base, the same base on the CPU), built once per session"""
    if name not in _cache:
        if name == "ba2000":
            from graphgym_amd import graphgen
            g = CSRGraph.from_edge_index(graphgen.ba_edge_index(2000, 3, seed=7).to(dev), 2000)
        else:
            g = SG.build(name, dev)
        _cache[name] = (g, _on_cpu(g))
    return _cache[name]


def _plans(name, kind, dev):
    g, h = _base(name, dev)
    kw = dict(batch_size=48, walk_length=3, num_parts=3)
    return S.plan_sampler(g, kind, **kw), S.plan_sampler(h, kind, **kw)


def _same_batch(a, b):
    assert a.num_nodes == b.num_nodes and a.graph.nnz == b.graph.nnz
    assert torch.equal(a.orig_node.cpu(), b.orig_node.cpu())
    assert torch.equal(a.graph.rowptr.cpu(), b.graph.rowptr.cpu())
    assert torch.equal(a.graph.col.cpu(), b.graph.col.cpu())
    assert torch.equal(a.base_entry.cpu(), b.base_entry.cpu())
    assert torch.equal(a.edge_index.cpu(), b.edge_index.cpu())


@pytest.mark.parametrize("name", BASES)
@pytest.mark.parametrize("kind", S.KINDS)
def test_device_batch_equals_the_host_restatement(dev, name, kind):
    plan, host = _plans(name, kind, dev)
    for seed, step in ((1, 0), (1, 5), (2 ** 40 + 3, 2)):
        nodes = S.sample_nodes(plan, seed, step)
        want = S.sample_nodes_host(host, seed, step)
        assert nodes.dtype == torch.int32 and nodes.is_cuda
        assert torch.equal(nodes.cpu(), want)
        _same_batch(S.sample_batch(plan, seed, step), S.induced_subgraph_host(host.base, want))


def _torch_formulation(g, members):
    """the induced edge list of the base in (src, dst) base ids: mask both endpoints of the base's edge list, keep order"""
    rp = g.rowptr.long()
    row = torch.repeat_interleave(torch.arange(g.num_nodes, device=g.device), rp[1:] - rp[:-1])
    col = g.col.long()
    mask = torch.zeros(g.num_nodes, dtype=torch.bool, device=g.device)
    mask[members] = True
    keep = mask[row] & mask[col]
    return col[keep], row[keep]


@pytest.mark.parametrize("name", BASES)
@pytest.mark.parametrize("kind", S.KINDS)
def test_batch_graph_is_what_from_edge_index_builds(dev, name, kind):
    plan, _ = _plans(name, kind, dev)
    g = plan.base
    b = S.sample_batch(plan, 3, 1)
    n, N = b.num_nodes, g.num_nodes
    assert b.edge_index.dtype == torch.int64 and tuple(b.edge_index.shape) == (2, b.graph.nnz)
    assert b.orig_node.dtype == torch.int64 and b.orig_node.numel() == n
    if n:
        assert bool((b.orig_node[1:] > b.orig_node[:-1]).all())
    if n == 0:                                  # (an empty part of a tiny base: nothing for from_edge_index to build)
        assert b.graph.nnz == 0 and b.graph.rowptr.tolist() == [0]
        return
    ref = CSRGraph.from_edge_index(b.edge_index, n)
    assert torch.equal(ref.rowptr, b.graph.rowptr) and torch.equal(ref.col, b.graph.col)
    assert torch.equal(ref.eid, b.graph.eid)
    assert torch.equal(b.graph.eid, torch.arange(b.graph.nnz, dtype=torch.int32, device=dev))
    src, dst = _torch_formulation(g, b.orig_node)
    ours = b.orig_node[b.edge_index[1]] * N + b.orig_node[b.edge_index[0]]
    assert torch.equal(torch.sort(ours).values, torch.sort(dst * N + src).values)       # the same multiset in every row
    # base_entry names the base's entry of every kept edge
    assert torch.equal(g.col.long()[b.base_entry.long()], b.orig_node[b.edge_index[0]])
    assert torch.equal(g.row_ids().long()[b.base_entry.long()], b.orig_node[b.edge_index[1]])


def test_a_row_of_5000_entries_with_half_of_them_selected(dev):
    """node 0 is linked to 1 .. 5000, which also form a ring: row 0 is walked in 313 chunks of 16 with a running offset"""
    n = 5001
    leaves = torch.arange(1, n)
    ring = torch.stack([leaves, (leaves % (n - 1)) + 1])
    star = torch.stack([torch.zeros(n - 1, dtype=torch.int64), leaves])
    ei = torch.cat([star, star.flip(0), ring, ring.flip(0)], 1)
    g = CSRGraph.from_edge_index(ei.to(dev), n)
    gen = torch.Generator().manual_seed(5)
    half = leaves[torch.randperm(n - 1, generator=gen)[:(n - 1) // 2]]
    nodes = torch.cat([half, torch.zeros(1, dtype=torch.int64)])
    got = S.induced_subgraph(g, nodes.to(dev))
    _same_batch(got, S.induced_subgraph_host(_on_cpu(g), nodes))
    assert int(got.graph.rowptr[1]) == half.numel()                       # row 0 keeps exactly the selected leaves
    assert torch.equal(got.graph.col[:half.numel()].cpu().long(), torch.arange(1, half.numel() + 1))
    with pytest.raises(ValueError, match="outside"):
        S.induced_subgraph(g, torch.tensor([0, n], device=dev))


@pytest.mark.parametrize("kind", S.KINDS)
def test_a_side_stream_builds_the_same_batch(dev, kind):
    plan, _ = _plans("ba2000", kind, dev)
    a = S.sample_batch(plan, 9, 2)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        b = S.sample_batch(plan, 9, 2)
    side.synchronize()
    _same_batch(a, b)


def test_loader_gathers_integer_coded_features(dev):
    g, _ = _base("ba2000", dev)
    codes = (torch.arange(2000)[:, None] * torch.tensor([1, 3])).to(dev)            # int64 [N, 2], as OGB's codes
    plan = S.plan_sampler(g, "saint_node", batch_size=100)
    b = S.SubgraphLoader(g, codes, codes[:, 0], torch.arange(0, 2000, 2), plan, seed=1, iter_per_epoch=1).batch(0)
    assert b.node_feature.dtype == torch.int64 and torch.equal(b.node_feature, codes[b.orig_node])
    assert torch.equal(b.node_label, b.orig_node) and bool((b.orig_node[b.node_label_index] % 2 == 0).all())
    assert b.node_label_index.numel() == int((b.orig_node % 2 == 0).sum())


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


@pytest.mark.parametrize("layer_type", ["gcnconv", "sageconv"])
def test_layers_on_the_seeded_cache_equal_the_edge_index_path(dev, gcfg, layer_type):
    """the same layer, the same weights: once on the loader's batch (its CSR seeded into the graph cache), once on a
    Batch that carries edge_index alone (layers build the CSR through from_edge_index)"""
    from graphgym_amd import harness as H
    from graphgym_amd.registry import layer_dict
    gcfg.gnn.agg, gcfg.gnn.normalize_adj, gcfg.gnn.self_msg = "mean", False, "concat"
    g, _ = _base("ba2000", dev)
    gen = torch.Generator().manual_seed(3)
    x, y = torch.randn(2000, 24, generator=gen).to(dev), torch.randint(0, 4, (2000,), generator=gen).to(dev)
    plan = S.plan_sampler(g, "saint_rw", batch_size=64, walk_length=3)
    loader = S.SubgraphLoader(g, x, y, torch.ones(2000, dtype=torch.bool), plan, seed=4, iter_per_epoch=2)
    seeded = loader.batch(1)
    assert getattr(seeded, "_mp_graph_cache", None) is not None and seeded.num_nodes > 64
    torch.manual_seed(1)
    layer = layer_dict[layer_type](24, 16, bias=True).to(dev)
    up = torch.randn(seeded.num_nodes, 16, generator=gen).to(dev)
    out = []
    for batch in (seeded, H.Batch(node_feature=seeded.node_feature.detach().clone(),
                                  edge_index=seeded.edge_index.clone())):
        batch.node_feature = batch.node_feature.detach().requires_grad_(True)
        xin = batch.node_feature
        layer.zero_grad()
        h = layer(batch).node_feature
        h.backward(up)
        out.append([h.detach(), xin.grad] + [p.grad.clone() for p in layer.parameters()])
    close(out[0][0], out[1][0].double(), what=f"{layer_type} forward")
    close(out[0][1], out[1][1].double(), what=f"{layer_type} grad x")
    for a, b in zip(out[0][2:], out[1][2:]):
        close_all(a, b.double(), what=f"{layer_type} grad w")


def test_example_node_scaled_down_trains_on_sampled_batches(dev, gcfg):
    """run/configs/pyg/example_node.yaml (sageconv + skipsum, one graph) on BA(4000, 5) with dim_inner 32: three optimiser
    steps on saint_rw batches (batch_size 64, walk_length 4), three on random_node batches (4 parts)"""
    from graphgym_amd import graphgen, harness as H
    c = gcfg
    c.gnn.layers_pre_mp, c.gnn.layers_mp, c.gnn.layers_post_mp, c.gnn.dim_inner = 1, 3, 1, 32
    c.gnn.layer_type, c.gnn.stage_type, c.gnn.batchnorm, c.gnn.act, c.gnn.dropout = "sageconv", "skipsum", True, "prelu", 0.1
    c.gnn.agg, c.gnn.normalize_adj, c.gnn.skip_every, c.gnn.l2norm = "mean", False, 1, True
    c.dataset.task, c.dataset.transform = "node", "none"
    N, F_IN, CLASSES = 4000, 16, 5
    g = CSRGraph.from_edge_index(graphgen.ba_edge_index(N, 5, seed=3).to(dev), N)
    gen = torch.Generator().manual_seed(8)
    x, y = torch.randn(N, F_IN, generator=gen).to(dev), torch.randint(0, CLASSES, (N,), generator=gen).to(dev)
    train_mask = (torch.arange(N) % 5 != 0).to(dev)
    torch.manual_seed(2)
    model = H.GNN(F_IN, CLASSES).to(dev).train()
    opt = torch.optim.Adam(model.parameters(), lr=c.optim.base_lr)
    c.train.batch_size, c.train.walk_length, c.train.iter_per_epoch = 64, 4, 3
    for sampler in ("saint_rw", "random_node"):
        c.train.sampler, c.train.train_parts = sampler, 4
        loader = S.loader_from_cfg(c, g, x, y, train_mask, "train", seed=6)
        assert len(loader) == (3 if sampler == "saint_rw" else 4)
        steps = 0
        for batch in loader:
            if steps == 3:
                break
            assert bool(train_mask[batch.orig_node[batch.node_label_index]].all())
            assert batch.node_label_index.numel() == int(train_mask[batch.orig_node].sum())
            assert torch.equal(batch.node_feature, x[batch.orig_node])
            assert torch.equal(batch.node_label, y[batch.orig_node])
            assert getattr(batch, "_mp_graph_cache", None) is not None
            if sampler == "saint_rw":
                assert 64 < batch.num_nodes <= 64 * 5
            else:
                assert abs(batch.num_nodes - N // 4) < 6 * (N * 3 / 16) ** 0.5     # binomial(N, 1/4): six deviations

            def loss_fn(batch=batch):
                pred, true = model(batch)
                return torch.nn.functional.cross_entropy(pred, true)
            loss = H.train_step(model, opt, loss_fn)
            assert bool(torch.isfinite(loss))
            steps += 1
        assert steps == 3
    val = S.loader_from_cfg(c, g, x, y, ~train_mask, "val")
    assert len(val) == 1
    only = list(val)[0]
    assert only.node_feature is x and only.num_nodes == N
    assert torch.equal(only.node_label_index, torch.nonzero(~train_mask).view(-1))
    ref = CSRGraph.from_edge_index(only.edge_index, N)
    assert torch.equal(ref.rowptr, g.rowptr) and torch.equal(ref.col, g.col)
    model.eval()
    with torch.no_grad():
        pred, true = model(only)
    assert pred.shape == (int((~train_mask).sum()), CLASSES) and bool(torch.isfinite(pred).all())
    again = list(val)[0]                        # the forward replaced node_feature on `only`, not on the loader's batch
    assert again.node_feature is x and again._mp_graph_cache is only._mp_graph_cache
