"""Edge-level ID-GNN tasks on the GPU (graphgym_amd.edge_nets, csrc/edge.hip) against the networkx restatement of
transform.py:41-90 in tests/_edge_ref.py: edge-net batches, the CSR the expansion writes, label-source copies, hop
distances and path-length labels, the edge head, and an edge.yaml-shaped model trained on a device-built batch."""
import collections
import contextlib

import numpy as np
import pytest
import torch

import _edge_ref as R

pytestmark = pytest.mark.gpu

BASES = ["simple", "disconnected", "digraph", "multigraph", "multidigraph"]


def _base(dev, graphs):
    import graphgym_amd as ga
    ei, w, gp = R.union(graphs)
    base = ga.CSRGraph.from_edge_index(torch.from_numpy(ei).to(dev), int(gp[-1]))
    return base, torch.from_numpy(w).to(dev), gp


def _labels(graphs, k, seed):
    """k random local (src, dst) pairs per graph, and the same pairs as global ids"""
    gen = torch.Generator().manual_seed(seed)
    local, glob, off = [], [], 0
    for G in graphs:
        p = torch.randint(G.number_of_nodes(), (2, k), generator=gen)
        local.append(p)
        glob.append(p + off)
        off += G.number_of_nodes()
    return local, torch.cat(glob, 1)


@contextlib.contextmanager
def _cfg(**kw):
    import graphgym_amd.graphgym_plugin  # noqa: F401  (registers the GraphGym layer keys, 'idconv' among them)
    from graphgym_amd.config import cfg
    old = {}
    for key, v in kw.items():
        sect, name = key.split("__")
        node = getattr(cfg, sect)
        old[key] = getattr(node, name, None)
        setattr(node, name, v)
    try:
        yield cfg
    finally:
        for key, v in old.items():
            sect, name = key.split("__")
            if v is None:
                delattr(getattr(cfg, sect), name)
            else:
                setattr(getattr(cfg, sect), name, v)


@pytest.mark.parametrize("kind", BASES)
@pytest.mark.parametrize("n_graphs", [1, 3])
def test_expansion_equals_the_restatement(dev, kind, n_graphs):
    """node ids, the edge multiset (direction, parallel copies, replicated edge features), node_id_index and
    node_label_index = src * n + dst (graphs offset by the n^2 ids before them) against transform.py:41-65"""
    from graphgym_amd.edge_nets import edge_batch
    graphs = [R.base_graph(kind, seed=s) for s in range(n_graphs)]
    base, w, gp = _base(dev, graphs)
    local, li = _labels(graphs, 25, seed=n_graphs)
    lab = torch.arange(li.size(1), device=dev)
    x = torch.rand(base.num_nodes, 3, device=dev)
    b = edge_batch(base, gp, li.to(dev), lab, x=x)
    edges, ids, nli, total = R.edge_nets_batch(graphs, local)
    assert b.orig_node.numel() == total and b.edge_index.size(1) == sum(edges.values())
    want_orig, want_copy, want_graph = [], [], []
    lo = 0
    for g, G in enumerate(graphs):
        n = G.number_of_nodes()
        want_orig.append(torch.arange(n).repeat(n) + lo)
        want_copy.append(torch.arange(n).repeat_interleave(n) + lo)
        want_graph.append(torch.full((n * n,), g))
        lo += n
    assert torch.equal(b.orig_node.cpu(), torch.cat(want_orig))
    assert torch.equal(b.copy_of_node.cpu().long(), torch.cat(want_copy))
    assert torch.equal(b.batch.cpu(), torch.cat(want_graph))
    assert torch.equal(b.node_id_index.cpu(), ids)
    assert torch.equal(b.node_label_index.cpu(), nli)
    assert torch.equal(b.node_label, lab)
    assert torch.equal(b.node_feature, x[b.orig_node])
    ei = b.edge_index.cpu()
    got = collections.Counter(zip(ei[0].tolist(), ei[1].tolist(), w[b.orig_edge].cpu().tolist()))
    assert got == edges
    key = ei[1] * total + ei[0]                                   # the engine's CSR order: (dst, src)
    assert bool((key[1:] >= key[:-1]).all())


@pytest.mark.parametrize("kind", BASES)
def test_csr_written_by_the_expansion_is_the_general_build_or_none(dev, kind):
    """csr='none' / 'add': entry for entry what CSRGraph.from_edge_index builds from the batch's own edge list (rowptr,
    col, eid), flagged symmetric; None on directed and multi-edge bases"""
    import graphgym_amd as ga
    from graphgym_amd.edge_nets import edge_batch
    graphs = [R.base_graph(kind, seed=s) for s in range(3)]
    base, _, gp = _base(dev, graphs)
    _, li = _labels(graphs, 10, seed=7)
    for loops in ("none", "add"):
        for sources in (None, "labels"):
            b, g = edge_batch(base, gp, li.to(dev), torch.zeros(li.size(1), device=dev), sources=sources, csr=loops)
            if kind in ("digraph", "multigraph", "multidigraph"):
                assert g is None
                continue
            assert g is not None and g.symmetric
            n2 = b.orig_node.numel()
            want = ga.CSRGraph.from_edge_index(b.edge_index, n2, add_self_loops=(loops == "add"))
            assert g.num_nodes == want.num_nodes and g.nnz == want.nnz
            assert torch.equal(g.rowptr, want.rowptr)
            assert torch.equal(g.col, want.col)
            assert torch.equal(g.eid, want.eid)
            assert want.is_symmetric(run=True)


def _gnn_cfg(**extra):
    """edge.yaml's model (idconv, add aggregation, no adjacency normalisation, L2-normalised embeddings) at
    layers_mp = 3, d = 64; transform: edge makes the task node classification (loader.py:181-187)"""
    kw = dict(gnn__layer_type="idconv", gnn__layers_mp=3, gnn__dim_inner=64, gnn__layers_pre_mp=1,
              gnn__layers_post_mp=1, gnn__batchnorm=False, gnn__l2norm=True, gnn__act="relu", gnn__dropout=0.0,
              gnn__agg="add", gnn__normalize_adj=False, gnn__stage_type="stack", dataset__task="node",
              dataset__transform="edge")
    kw.update(extra)
    return _cfg(**kw)


def test_label_source_copies_give_the_full_expansion_s_outputs(dev):
    """sources='labels' against the full expansion: a 3-layer idconv GNN gives the same outputs at the label nodes (the
    copies are independent components and every row's entries come in the same order).  Within fp32 rounding, row by
    row, not bit for bit: the engine picks its aggregation and transform kernels by the batch's size and degrees, and
    the two batches differ in both"""
    from _tol import assert_close_rows
    from graphgym_amd import harness as H
    from graphgym_amd.edge_nets import edge_batch
    graphs = [R.base_graph("simple", seed=s) for s in range(3)]
    base, _, gp = _base(dev, graphs)
    _, li = _labels(graphs, 12, seed=3)
    li = li.to(dev)
    lab = torch.randint(0, 5, (li.size(1),), device=dev)
    x = torch.rand(base.num_nodes, 10, device=dev, generator=torch.Generator(device=dev).manual_seed(0))
    full = edge_batch(base, gp, li, lab, x=x)
    part = edge_batch(base, gp, li, lab, x=x, sources="labels")
    assert part.node_id_index.numel() == torch.unique(li[0]).numel() < full.node_id_index.numel()
    assert torch.equal(part.orig_node[part.node_label_index], full.orig_node[full.node_label_index])
    with _gnn_cfg(gnn__layers_pre_mp=0):
        torch.manual_seed(0)
        model = H.GNN(10, 5).to(dev).eval()
        with torch.no_grad():
            emb = []
            for b in (full, part):
                b = model.mp(b)
                emb.append(b.node_feature[b.node_label_index].clone())
            p_full, y_full = model.post_mp(full)
            p_part, y_part = model.post_mp(part)
    assert_close_rows(emb[1], emb[0], what="label-source copies: embeddings at the label nodes")
    assert torch.equal(y_full, y_part)
    assert_close_rows(p_part, p_full, what="label-source copies: predictions")


@pytest.mark.parametrize("kind", BASES)
def test_hop_distances_equal_networkx(dev, kind):
    """every ordered pair of every graph of a 3-graph batch (and pairs across graphs: -1) against
    nx.shortest_path_length along the edge direction: 0 for (a, a), -1 when unreachable, paths longer than 4"""
    from graphgym_amd.edge_nets import hop_distances
    graphs = [R.base_graph(kind, seed=s) for s in range(3)]
    base, _, gp = _base(dev, graphs)
    src, dst, want = [], [], []
    for g, G in enumerate(graphs):
        n, lo = G.number_of_nodes(), int(gp[g])
        for s in range(n):
            for t in range(n):
                src.append(lo + s)
                dst.append(lo + t)
                want.append(R.hops(G, s, t))
    src += [0, int(gp[1]), int(gp[2]) - 1]                     # across graphs
    dst += [int(gp[1]), 0, int(gp[3]) - 1]
    want += [-1, -1, -1]
    d = hop_distances(base, torch.tensor(src, device=dev), torch.tensor(dst, device=dev), gp).cpu()
    assert d.dtype == torch.int32
    assert d.tolist() == want
    assert -1 in want and 0 in want
    if kind == "disconnected":
        assert max(want) > 4
    # the whole batch taken as one graph: the same distances inside each graph
    inside = [k for k in range(len(want) - 3)]
    d1 = hop_distances(base, torch.tensor(src, device=dev)[inside], torch.tensor(dst, device=dev)[inside]).cpu()
    assert d1.tolist() == want[:-3]


def test_hop_distances_long_path_and_the_lds_bound(dev):
    """a 3000-node path (depths far beyond 4, exact), and a graph above 65536 nodes: a clear error"""
    import graphgym_amd as ga
    from graphgym_amd._lib import EngineError
    from graphgym_amd.edge_nets import hop_distances
    n = 3000
    e = torch.stack([torch.arange(n - 1), torch.arange(1, n)])
    base = ga.CSRGraph.from_edge_index(torch.cat([e, e.flip(0)], 1).to(dev), n)
    src = torch.tensor([0, 0, 1500, n - 1, 17], device=dev)
    dst = torch.tensor([n - 1, 0, 10, 0, 18], device=dev)
    assert hop_distances(base, src, dst).cpu().tolist() == [n - 1, 0, 1490, n - 1, 1]
    big = (1 << 16) + 8
    e = torch.stack([torch.arange(big - 1), torch.arange(1, big)])
    base = ga.CSRGraph.from_edge_index(torch.cat([e, e.flip(0)], 1).to(dev), big)
    with pytest.raises(EngineError, match="65536"):
        hop_distances(base, torch.tensor([0], device=dev), torch.tensor([5], device=dev))
    # a source in a small graph of the same batch is fine: the bound is per graph that holds a source
    gp = torch.tensor([0, 100, big])
    assert hop_distances(base, torch.tensor([0], device=dev), torch.tensor([5], device=dev), gp).tolist() == [5]


@pytest.mark.parametrize("kind", ["simple", "disconnected", "digraph", "multidigraph"])
def test_path_len_labels_equal_the_restatement(dev, kind):
    """a seeded generator: the kept pairs and labels of transform.py:68-90, bit for bit, graph after graph"""
    from graphgym_amd.edge_nets import path_len_labels
    graphs = [R.base_graph(kind, seed=s) for s in range(3)]
    base, _, gp = _base(dev, graphs)
    eli, lab = path_len_labels(base, gp, num_label=400, generator=torch.Generator().manual_seed(5))
    want_i, want_l = R.path_len_batch(graphs, 400, torch.Generator().manual_seed(5))
    assert eli.device.type == "cuda" and lab.dtype == torch.int64
    assert torch.equal(eli.cpu(), want_i)
    assert torch.equal(lab.cpu(), want_l)
    assert want_l.numel() < 1200 or kind == "simple"


@pytest.mark.parametrize("decoding", ["concat", "dot", "cosine_similarity"])
def test_edge_head_against_torch(dev, decoding):
    """GNNEdgeHead (head.py:40-85) forward and gradients against the same decoder written in plain torch"""
    import torch.nn.functional as F
    from graphgym_amd import harness as H
    n, d, k = 50, 16, 30
    gen = torch.Generator(device=dev).manual_seed(1)
    h0 = torch.randn(n, d, device=dev, generator=gen)
    eli = torch.randint(0, n, (2, k), device=dev, generator=gen)
    dim_out = 3 if decoding == "concat" else 1
    with _cfg(model__edge_decoding=decoding, gnn__layers_post_mp=1):
        torch.manual_seed(2)
        head = H.GNNEdgeHead(d, dim_out).to(dev)
        h = h0.clone().requires_grad_(True)
        pred, label = head(H.Batch(node_feature=h, edge_label_index=eli, edge_label=torch.ones(k, device=dev)))
        assert torch.equal(label, torch.ones(k, device=dev))
        up = torch.randn(pred.shape, device=dev, generator=gen)
        (pred * up).sum().backward()
        lin = head.layer_post_mp.model[0].model
        W, b = lin.weight.detach().clone().requires_grad_(True), lin.bias.detach().clone().requires_grad_(True)
        hr = h0.clone().requires_grad_(True)
        if decoding == "concat":
            ref = F.linear(torch.cat([hr[eli[0]], hr[eli[1]]], -1), W, b)
        else:
            z = F.linear(hr, W, b)
            a, c = z[eli[0]], z[eli[1]]
            ref = (a * c).sum(-1) if decoding == "dot" else F.cosine_similarity(a, c, dim=-1)
        (ref * up).sum().backward()
    assert pred.shape == ref.shape
    torch.testing.assert_close(pred, ref, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(h.grad, hr.grad, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(lin.weight.grad, W.grad, rtol=1e-5, atol=1e-5)
    torch.testing.assert_close(lin.bias.grad, b.grad, rtol=1e-5, atol=1e-5)
    with _cfg(model__edge_decoding=decoding):
        if decoding != "concat":
            with pytest.raises(ValueError):
                H.GNNEdgeHead(d, 2)
    with _cfg(dataset__task="link_pred", gnn__layers_mp=1, gnn__layers_pre_mp=0, gnn__dim_inner=16,
              gnn__layer_type="idconv", model__edge_decoding=decoding):
        assert isinstance(H.GNN(d, dim_out).post_mp, H.GNNEdgeHead)


def test_edge_yaml_model_on_a_device_built_batch(dev):
    """run/configs/IDGNN/edge.yaml scaled down (idconv, layers_mp = 3, d = 64): 8 BA(64, 2) graphs with path-length
    labels; the model on the expansion's own CSR (seeded into the batch) and on the general build agree within
    tests/_tol.py, and ten Adam steps lower the loss"""
    from _tol import assert_close_all, assert_close_rows
    import graphgym_amd as ga
    from graphgym_amd import harness as H
    from graphgym_amd.edge_nets import edge_batch, path_len_labels, seed_graph
    graphs = [R.ba_graph(64, 2, seed=s) for s in range(8)]
    base, _, gp = _base(dev, graphs)
    eli, lab = path_len_labels(base, gp, num_label=200, generator=torch.Generator().manual_seed(0))
    x = torch.rand(base.num_nodes, 10, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    fast, g = edge_batch(base, gp, eli, lab, x=x, csr="none")
    assert g is not None
    seed_graph(fast, g, "none")
    plain = edge_batch(base, gp, eli, lab, x=x)
    assert torch.equal(fast.edge_index, plain.edge_index)
    with _gnn_cfg(gnn__batchnorm=True):
        torch.manual_seed(0)
        model = H.GNN(10, 5).to(dev)
        outs = []
        for b in (fast, plain):
            for p in model.parameters():
                p.grad = None
            b.node_feature = x[b.orig_node]
            pred, y = model(b)
            loss = torch.nn.functional.cross_entropy(pred, y)
            loss.backward()
            outs.append((pred.detach(), loss.detach(), [p.grad.clone() for p in model.parameters()]))
        assert isinstance(fast._mp_graph_cache[(1, "none", None, 1.0)], ga.CSRGraph)
        assert fast._mp_graph_cache[(1, "none", None, 1.0)] is g
        (pf, lf, gf), (pp, lp, gpp) = outs
        assert_close_rows(pf, pp, what="edge batch: logits, written vs general CSR")
        assert_close_all(lf, lp, what="edge batch: loss")
        for a, r in zip(gf, gpp):
            assert_close_all(a, r, what="edge batch: parameter gradient")
        opt = torch.optim.Adam(model.parameters(), lr=0.01)
        x0 = x[fast.orig_node]

        def fl():
            fast.node_feature = x0
            pred, y = model(fast)
            return torch.nn.functional.cross_entropy(pred, y)
        losses = [float(H.train_step(model, opt, fl)) for _ in range(10)]
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
