"""Graph-task loaders on the device (csrc/collate.hip, graphgym_amd.graph_loader): collate against the NumPy restatement,
bit for bit, on the host tests' datasets, on directed / repeated-entry / valued datasets, on 40 graphs of 1-70 nodes
(several workgroups, a 70-node graph across a wave), on bf16 features and integer codes and with B on both sides of the
LDS staging cap; the seeding contract against CSRGraph.from_edge_index and samplers.induced_subgraph; layers and the
graph head on a loader batch against a plain batch; pooling through pool_operator against a per-graph float64 loop;
collate under torch's sync debug mode; the ego transform against ego.ego_batch; and the golden config end to end."""
import copy
import os

import numpy as np
import pytest
import torch

import _graph_sets as GS
from _tol import close, close_all
from graphgym_amd import CSRGraph, _lib
from graphgym_amd import graph_loader as GL

pytestmark = pytest.mark.gpu

GOLDEN_CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cfg_idgnn_graph.yaml")
_cache = {}


def _sizes40():
    """40 graphs of 1-70 nodes, the extremes included: ~1400 nodes (six workgroups of 256) and ~3500 entries"""
    s = np.random.RandomState(11).randint(1, 71, size=40)
    s[5], s[20] = 1, 70
    return s.tolist()


def _valued(dev):
    """the symmetric 12-graph set with a value per stored entry (equal on both directions of a link)"""
    graphs = GS.make_graphs(GS.SIZES12, "symmetric", seed=5)
    plain = GL.GraphDataset.from_graphs(graphs, dev)
    ei_parts, at = [], 0
    for ei, x, _, _ in graphs:
        ei_parts.append(ei + at)
        at += x.size(0)
    ei = torch.cat(ei_parts, 1)
    lo, hi = torch.minimum(ei[0], ei[1]), torch.maximum(ei[0], ei[1])
    w = ((lo * 131 + hi * 7) % 97).float() / 16 + 0.25
    base = CSRGraph.from_edge_index(ei.to(dev), at, edge_weight=w.to(dev))
    return GL.GraphDataset(base, plain.graph_ptr, plain.x, plain.graph_label, plain.edge_feature)


def _dataset(name, dev):
    if name not in _cache:
        if name == "valued":
            _cache[name] = _valued(dev)
        elif name == "forty":
            _cache[name] = GL.GraphDataset.from_graphs(GS.make_graphs(_sizes40(), seed=6), dev)
        elif name == "singles":              # 1-node graphs that store two self entries each: n stays small above the cap
            _cache[name] = GL.GraphDataset.from_graphs(GS.make_graphs([1] * 64, "multi", seed=7), dev)
        elif name in ("bf16", "codes"):
            dtype = torch.bfloat16 if name == "bf16" else torch.int64
            _cache[name] = GL.GraphDataset.from_graphs(GS.make_graphs(GS.SIZES12, seed=8, dtype=dtype), dev)
        else:
            _cache[name] = GL.GraphDataset.from_graphs(GS.make_graphs(GS.SIZES12, name, seed=1), dev)
    return _cache[name]


def _ids(name):
    if name == "forty":
        r = np.random.RandomState(3)
        return {"all_shuffled": r.permutation(40).tolist(), "some": [20, 5, 39, 0, 20]}
    if name == "singles":
        cap = _lib.lib().mp_collate_stage_cap()
        r = np.random.RandomState(4)                 # B + 1 offsets are staged up to the cap: B = cap is the first above
        return {f"B{B}": r.randint(0, 64, size=B).tolist() for B in (cap - 1, cap, cap + 1)}
    return GS.IDS12


PARITY = [(n, c) for n in ("symmetric", "directed", "multi", "valued", "bf16", "codes") for c in sorted(GS.IDS12)] + \
         [("forty", "all_shuffled"), ("forty", "some"), ("singles", "B1023"), ("singles", "B1024"), ("singles", "B1025")]


@pytest.mark.parametrize("name,case", PARITY)
def test_device_collate_equals_the_host_restatement(dev, name, case):
    ds = _dataset(name, dev)
    ids = _ids(name)[case]
    got, want = GL.collate(ds, ids), GL.collate_host(ds, ids)
    assert got.edge_index.is_cuda and got.graph.rowptr.is_cuda and not want.edge_index.is_cuda
    assert (got.graph.val is not None) == (name == "valued")
    assert ds.seedable == (name not in ("directed", "multi", "singles"))
    GS.assert_batches_equal(got, want, f"{name}/{case}")
    assert torch.equal(got.graph.row_ids().cpu(), want.graph.row_ids())
    assert torch.equal(got.pool_operator.transpose().col.cpu().long(), want.batch)
    if name == "codes":
        assert got.node_feature.dtype == torch.int64
    if name == "bf16":
        assert got.node_feature.dtype == torch.bfloat16


def test_device_dataset_rejects_crossing_entries(dev):
    ei = torch.tensor([[0, 1, 2, 3], [1, 0, 3, 2]], device=dev)
    base = CSRGraph.from_edge_index(ei, 5)
    x, y = torch.zeros(5, 2, device=dev), torch.zeros(2, dtype=torch.int64, device=dev)
    assert GL.GraphDataset(base, [0, 2, 5], x, y).seedable
    with pytest.raises(ValueError, match=r"stored entry 2 \(row 2, column 3\) joins graph 0 and graph 1"):
        GL.GraphDataset(base, [0, 3, 5], x, y)


# ---- the seeding contract -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["symmetric", "directed", "multi", "valued", "forty"])
def test_batch_graph_is_what_from_edge_index_builds(dev, name):
    ds = _dataset(name, dev)
    for case, ids in _ids(name).items():
        b = GL.collate(ds, ids)
        n, g = b.num_nodes, b.graph
        assert (getattr(b, "_mp_graph_cache", None) is not None) == ds.seedable
        ref = CSRGraph.from_edge_index(b.edge_index, n)
        assert torch.equal(ref.rowptr, g.rowptr) and torch.equal(ref.col, g.col), case
        assert torch.equal(ref.eid, g.eid) and torch.equal(g.eid, torch.arange(g.nnz, dtype=torch.int32, device=dev))
        if ds.seedable:
            from graphgym_amd.layers import get_graph
            seeded = get_graph(b, b.edge_index, n, dst_row=1, loops="none")
            assert g.symmetric and seeded is b._mp_graph_cache[(1, "none", None, 1.0)]
            assert seeded.rowptr is g.rowptr and seeded.col is g.col and seeded.val is None     # (the pattern alone)
            assert (seeded is g) == (g.val is None)


@pytest.mark.parametrize("name", ["symmetric", "multi", "forty"])
def test_ascending_ids_give_the_induced_subgraph(dev, name):
    from graphgym_amd import samplers as S
    ds = _dataset(name, dev)
    ids = sorted(set(_ids(name)["all_shuffled"][:7]))
    b = GL.collate(ds, ids)
    nodes = torch.cat([torch.arange(ds.graph_ptr[i], ds.graph_ptr[i + 1]) for i in ids]).to(dev)
    want = S.induced_subgraph(ds.base, nodes)
    assert torch.equal(b.graph.rowptr, want.graph.rowptr) and torch.equal(b.graph.col, want.graph.col)
    assert torch.equal(b.orig_node, want.orig_node) and torch.equal(b.base_entry, want.base_entry)
    assert torch.equal(b.edge_index, want.edge_index)


# ---- layers, head, pooling ------------------------------------------------------------------------------------------------

@pytest.fixture
def gcfg():
    from graphgym_amd.config import cfg
    import graphgym_amd.graphgym_plugin  # noqa: F401  (registers the layer keys)
    saved = copy.deepcopy(vars(cfg))
    yield cfg
    for k in list(vars(cfg)):
        if k not in saved:
            delattr(cfg, k)
    for k, v in saved.items():
        setattr(cfg, k, v)


def _plain(loaded, **more):
    """a harness.Batch with the loader batch's node_feature and edge_index (copies) and nothing seeded"""
    from graphgym_amd import harness as H
    return H.Batch(node_feature=loaded.node_feature.detach().clone(), edge_index=loaded.edge_index.clone(), **more)


@pytest.mark.parametrize("layer_type", ["generalconv", "gcnconv"])
def test_layers_on_a_loader_batch_equal_the_edge_index_path(dev, gcfg, layer_type):
    from graphgym_amd.registry import layer_dict
    gcfg.gnn.agg, gcfg.gnn.normalize_adj, gcfg.gnn.self_msg = "add", False, "concat"
    ds = _dataset("forty", dev)
    seeded = GL.collate(ds, _ids("forty")["all_shuffled"])
    assert getattr(seeded, "_mp_graph_cache", None) is not None and seeded.num_nodes > 1024
    torch.manual_seed(1)
    layer = layer_dict[layer_type](8, 16, bias=True).to(dev)
    up = torch.randn(seeded.num_nodes, 16, generator=torch.Generator().manual_seed(2)).to(dev)
    out = []
    for batch in (seeded, _plain(seeded)):
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


@pytest.mark.parametrize("pooling", ["add", "mean", "max"])
def test_graph_head_on_a_loader_batch_equals_the_plain_batch(dev, gcfg, pooling):
    from graphgym_amd import harness as H
    gcfg.model.graph_pooling, gcfg.gnn.layers_post_mp, gcfg.dataset.transform = pooling, 2, "none"
    ds = _dataset("forty", dev)
    loaded = GL.collate(ds, _ids("forty")["all_shuffled"])
    torch.manual_seed(3)
    head = H.GNNGraphHead(8, 4).to(dev)
    up = torch.randn(40, 4, generator=torch.Generator().manual_seed(4)).to(dev)
    out = []
    for batch in (loaded, _plain(loaded, batch=loaded.batch.clone(), graph_label=loaded.graph_label)):
        assert hasattr(batch, "pool_operator") == (batch is loaded)
        batch.node_feature = batch.node_feature.detach().requires_grad_(True)
        xin = batch.node_feature
        head.zero_grad()
        pred, true = head(batch)
        pred.backward(up)
        assert torch.equal(true, loaded.graph_label)
        out.append([pred.detach(), xin.grad] + [p.grad.clone() for p in head.parameters()])
    close(out[0][0], out[1][0].double(), what=f"head {pooling} forward")
    close(out[0][1], out[1][1].double(), what=f"head {pooling} grad x")
    for a, b in zip(out[0][2:], out[1][2:]):
        close_all(a, b.double(), what=f"head {pooling} grad w")


def _pool_loop(x64, owner, B, reduce, rows):
    """per-graph float64 loop over the pooled rows `rows` (positions into x64) whose graph is owner[row]"""
    out = []
    for j in range(B):
        mine = x64[rows[owner[rows] == j]]
        out.append(mine.sum(0) if reduce == "add" else (mine.mean(0) if reduce == "mean" else mine.max(0).values))
    return torch.stack(out)


def _ego_batch6(dev):
    ds = _dataset("symmetric", dev)
    ids = [6, 0, 4, 3, 10, 2]
    return ds, ids, GL.GraphLoader(ds, ids, 6, shuffle=False, transform="ego", radius=2).batch(0, 0)


@pytest.mark.parametrize("form", ["collate", "ego"])
@pytest.mark.parametrize("reduce", ["add", "mean", "max"])
def test_pooling_through_the_pool_operator(dev, gcfg, form, reduce):
    from graphgym_amd.pooling import pooling_dict
    if form == "ego":
        gcfg.dataset.transform = "ego"
        _, ids, b = _ego_batch6(dev)
        rows = b.node_id_index.cpu()                                            # the centres only
        assert rows.numel() < b.num_nodes
    else:
        b = GL.collate(_dataset("forty", dev), _ids("forty")["all_shuffled"])
        rows = torch.arange(b.num_nodes)
    B = b.num_graphs
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(b.num_nodes, 8, generator=gen).to(dev).requires_grad_(True)
    up = torch.randn(B, 8, generator=gen)
    y = pooling_dict[reduce](x, b.batch, getattr(b, "node_id_index", None), operator=b.pool_operator)
    y.backward(up.to(dev))
    x64 = x.detach().cpu().double().requires_grad_(True)
    ref = _pool_loop(x64, b.batch.cpu(), B, reduce, rows)
    ref.backward(up.double())
    close(y.detach(), ref.detach(), what=f"{form} pool {reduce}")
    close(x.grad, x64.grad, what=f"{form} pool {reduce} grad")


# ---- no host read ----------------------------------------------------------------------------------------------------------

def test_collate_makes_no_host_read(dev):
    ds = _dataset("forty", dev)
    ids = _ids("forty")
    GL.collate(ds, ids["all_shuffled"])                                        # warmed: buffers grown, code loaded
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            control = False
        except RuntimeError:
            control = True
        if control:
            b = GL.collate(ds, ids["all_shuffled"])
            short = GL.collate(ds, ids["some"])
    finally:
        torch.cuda.set_sync_debug_mode(old)
    if not control:
        pytest.skip("torch's sync debug mode does not raise on .item() in this build: nothing to check against")
    GS.assert_batches_equal(b, GL.collate_host(ds, ids["all_shuffled"]), "under sync debug")
    GS.assert_batches_equal(short, GL.collate_host(ds, ids["some"]), "under sync debug")
    assert getattr(b, "_mp_graph_cache", None) is not None and hasattr(b, "edge_feature")


# ---- the ego transform ------------------------------------------------------------------------------------------------------

def test_ego_loader_batches_follow_ego_batch(dev):
    from graphgym_amd.ego import ego_batch
    ds, ids, b = _ego_batch6(dev)
    host = GL.collate_host(ds, ids)
    centres = host.orig_node.to(dev)
    ei, orig, idx, ego_of = ego_batch(ds.base, centres, 2)
    assert torch.equal(b.edge_index, ei) and torch.equal(b.orig_node, orig) and torch.equal(b.node_id_index, idx)
    assert torch.equal(b.node_id_index, torch.arange(centres.numel(), device=dev))
    assert torch.equal(b.orig_node[:centres.numel()], centres)
    position = {g: j for j, g in enumerate(ids)}
    graph_of = np.searchsorted(ds.graph_ptr, b.orig_node.cpu().numpy(), side="right") - 1
    assert b.batch.cpu().tolist() == [position[int(g)] for g in graph_of]       # batch[k] is the graph of orig_node[k]
    assert torch.equal(b.node_feature, ds.x[b.orig_node]) and torch.equal(b.graph_label.cpu(), host.graph_label)
    assert b.num_graphs == 6 and b.num_nodes == orig.numel()
    assert getattr(b, "_mp_graph_cache", None) is not None                     # a symmetric, loop-free base: seeded
    ref = CSRGraph.from_edge_index(ei, b.num_nodes)
    assert torch.equal(ref.rowptr, b.graph.rowptr) and torch.equal(ref.col, b.graph.col)
    p = b.pool_operator
    assert (p.num_nodes, p.num_cols, p.nnz) == (6, b.num_nodes, centres.numel())
    assert torch.equal(p.rowptr.cpu(), host.pool_operator.rowptr) and torch.equal(p.col.cpu(), host.pool_operator.col)


# ---- end to end ---------------------------------------------------------------------------------------------------------------

def _ba_dataset(dev):
    """48 BA(n, 2) graphs of 12-40 nodes, features (1, log(1 + degree)) — a constant column alone is what BatchNorm
    maps to zero, and the model would not see the graph — label = the balanced class of graph_path_len"""
    from graphgym_amd import graphgen, structure
    sizes = np.random.RandomState(21).randint(12, 41, size=48).tolist()
    graphs = []
    for i, n in enumerate(sizes):
        ei = graphgen.connected_ba_edge_index(n, 2, seed=100 + i)
        deg = torch.bincount(ei[1], minlength=n).float()
        graphs.append((ei, torch.stack([torch.ones(n), deg.log1p()], 1), torch.tensor(0)))
    ds = GL.GraphDataset.from_graphs(graphs, dev)
    tensors, _, classes = structure.augment(ds.base, torch.from_numpy(ds.graph_ptr), [], [], label="graph_path_len",
                                            label_dim=10)
    ds.graph_label = tensors["graph_path_len_label"].to(dev).long()
    return ds, int(classes)


@pytest.mark.parametrize("transform", ["ego", "none"])
def test_golden_config_steps_equal_the_rebuilt_batches(dev, gcfg, transform):
    """cfg_idgnn_graph.yaml (run/configs/IDGNN/graph.yaml) with train.batch_size 16 — and, for transform 'none', the
    generalconv counterpart of its idconv: two identical models, one stepped on the loader's batches, one on batches
    rebuilt from collate_host / ego_batch with nothing seeded and no pool_operator.  Two paths through the same
    arithmetic: the per-step losses agree; that the loss falls is not asserted here."""
    from graphgym_amd import config, harness as H
    from graphgym_amd.ego import ego_batch
    cfg = config.load_cfg(GOLDEN_CFG, target=gcfg)
    assert cfg.dataset.transform == "ego" and cfg.gnn.layer_type == "idconv" and cfg.train.batch_size == 64
    cfg.train.batch_size = 16
    if transform == "none":
        cfg.dataset.transform, cfg.gnn.layer_type = "none", "generalconv"
    ds, classes = _ba_dataset(dev)
    assert ds.num_graphs == 48 and ds.seedable and classes > 1
    train, val = GL.graph_loaders_from_cfg(cfg, ds, seed=2)
    assert (train.ids.size, val.ids.size, len(train)) == (38, 10, 3) and train.shuffle and not val.shuffle
    models = []
    for _ in range(2):
        torch.manual_seed(0)
        models.append(H.GNN(dim_in=2, dim_out=classes).to(dev).train())
    opts = [torch.optim.Adam(m.parameters(), lr=cfg.optim.base_lr) for m in models]

    def rebuilt(ids):
        host = GL.collate_host(ds, ids)
        label = host.graph_label.to(dev)
        if transform == "none":
            return H.Batch(node_feature=host.node_feature.to(dev), edge_index=host.edge_index.to(dev),
                           batch=host.batch.to(dev), graph_label=label)
        ei, orig, idx, ego_of = ego_batch(ds.base, host.orig_node.to(dev), cfg.gnn.layers_mp)
        return H.Batch(node_feature=ds.x[orig], edge_index=ei, node_id_index=idx,
                       batch=host.batch.to(dev)[ego_of.long()], graph_label=label)

    losses = [[], []]
    for i, batch in enumerate(train):
        assert hasattr(batch, "pool_operator") and getattr(batch, "_mp_graph_cache", None) is not None
        other = rebuilt(train.batch_ids(0, i))
        assert not hasattr(other, "pool_operator") and getattr(other, "_mp_graph_cache", None) is None
        for k, (model, opt, b) in enumerate(zip(models, opts, (batch, other))):
            def fl(model=model, b=b):
                pred, true = model(b)
                assert float(pred.detach().std(0).max()) > 0           # (the prediction depends on the graph)
                return torch.nn.functional.cross_entropy(pred, true)
            losses[k].append(float(H.train_step(model, opt, fl)))
    print(f"{transform}: loader {losses[0]}, rebuilt {losses[1]}")
    assert len(losses[0]) == 3 and np.isfinite(losses[0]).all() and np.isfinite(losses[1]).all()
    close_all(torch.tensor(losses[0], dtype=torch.float64), torch.tensor(losses[1], dtype=torch.float64), tol=1e-5,
              what=f"{transform} losses")
