"""GPU ego-net batcher vs the oracle's restatement of transform.py:11-38 (networkx) — node
numbering bit-exact, edge multisets identical — on the committed golden graphs and fresh ones."""
import collections

import networkx as nx
import numpy as np
import pytest
import torch

from oracle import ref_layers as RL

pytestmark = pytest.mark.gpu


def directed(G):
    e = np.array(list(G.edges()), dtype=np.int64).reshape(-1, 2)
    return np.ascontiguousarray(np.concatenate([e, e[:, ::-1]], axis=0).T)


def expand_on_gpu(dev, base_ei, n, radius, centres=None):
    import graphgym_amd as ga
    from graphgym_amd.ego import ego_batch
    base = ga.CSRGraph.from_edge_index(torch.from_numpy(base_ei).to(dev), n)
    cen = torch.arange(n, device=dev) if centres is None else torch.as_tensor(centres, device=dev)
    return ego_batch(base, cen, radius)


def canon(ei, orig, ego_of):
    """expansion up to the relabelling inside each ego: the MULTISET {(centre, original u, original v): copies}
    (a set would not see a parallel edge dropped or doubled)"""
    ei, orig, ego_of = np.asarray(ei), np.asarray(orig), np.asarray(ego_of)
    assert (ego_of[ei[0]] == ego_of[ei[1]]).all()              # egos are disjoint components
    return collections.Counter(zip(ego_of[ei[0]].tolist(), orig[ei[0]].tolist(), orig[ei[1]].tolist()))


def test_matches_committed_golden(dev, golden):
    z = golden("ego.npz")
    for k in range(4):
        n, radius = int(z[f"g{k}/base_n"]), int(z[f"g{k}/radius"])
        ei, orig, ids, ego_of = expand_on_gpu(dev, z[f"g{k}/base_edge_index"], n, radius)
        assert orig.numel() == int(z[f"g{k}/ego_n"])
        assert ids.cpu().tolist() == z[f"g{k}/node_id_index"].tolist()
        ref = z[f"g{k}/ego_edge_index"]
        assert ei.size(1) == ref.shape[1]
        assert canon(ei.cpu().numpy(), orig.cpu().numpy(), ego_of.cpu().numpy()) == \
            canon(ref, z[f"g{k}/orig_node"], z[f"g{k}/ego_of_node"])
        assert orig[:n].cpu().tolist() == list(range(n))        # centres keep their ids
        # the sizes of the egos, hence the first fresh id of each, are bit-exact
        assert np.array_equal(np.bincount(ego_of.cpu().numpy()), np.bincount(z[f"g{k}/ego_of_node"]))


@pytest.mark.parametrize("radius", [1, 2, 3, 5])
def test_against_networkx_restatement(dev, radius):
    G = nx.powerlaw_cluster_graph(40, 2, 0.3, seed=radius)
    G.add_edge(3, 3)                                            # a self loop survives the induced subgraph
    H, ids, h_orig, h_ego = RL.ego_nets(G, radius, return_map=True)
    ei, orig, idx, ego_of = expand_on_gpu(dev, directed(G), 40, radius)
    assert orig.numel() == H.number_of_nodes()
    hd = directed(H)
    assert canon(ei.cpu().numpy(), orig.cpu().numpy(), ego_of.cpu().numpy()) == \
        canon(hd, h_orig.numpy(), h_ego.numpy())
    # orig maps fresh ids back: members of ego c are exactly nx.ego_graph(G, c, radius)
    orig_c, ego_c = orig.cpu().numpy(), ego_of.cpu().numpy()
    for c in range(40):
        members = set(orig_c[ego_c == c].tolist())
        want_m = set(G.nodes) if radius > 4 else set(nx.ego_graph(G, c, radius=radius).nodes)
        assert members == want_m
        fresh = orig_c[40:][ego_c[40:] == c]
        assert (np.diff(fresh) > 0).all()                       # our fresh ids ascend with the original id


def test_subset_of_centres_on_a_large_graph(dev):
    import graphgym_amd as ga
    from graphgym_amd import graphgen
    from graphgym_amd.ego import ego_batch
    n = 200_000
    ei = graphgen.ba_edge_index(n, 5, seed=3, device=dev)
    base = ga.CSRGraph.from_edge_index(ei, n)
    cen = torch.tensor([0, 17, 150_000, 199_999, 4242], device=dev)
    e2, orig, idx, ego_of = ego_batch(base, cen, 2)
    # independent check with torch ops: 2-hop sets by boolean frontier expansion
    src, dst = ei[0], ei[1]
    for k, c in enumerate(cen.tolist()):
        seen = torch.zeros(n, dtype=torch.bool, device=dev)
        seen[c] = True
        for _ in range(2):
            nxt = torch.zeros_like(seen)
            nxt[dst[seen[src]]] = True
            seen |= nxt
        members = torch.sort(orig[ego_of == k]).values
        assert torch.equal(members, torch.nonzero(seen).view(-1))
        m = ego_of[e2[1]] == k
        induced = int((seen[src] & seen[dst]).sum())
        assert int(m.sum()) == induced
    assert orig[:5].tolist() == cen.tolist()
    # fresh ids of each ego ascend with the original id
    for k in range(5):
        o = orig[(ego_of == k)].cpu()
        rest = o[o != cen[k].item()] if k < 5 else o
        fresh = orig[5:][(ego_of[5:] == k)].cpu()
        assert torch.equal(fresh, torch.sort(fresh).values)


@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("loops", ["none", "add"])
def test_csr_written_by_the_expansion_equals_the_csr_built_from_its_edge_list(dev, radius, loops):
    """ego_batch(csr=...) hands back the batch's CSRGraph written by the expansion itself; it must be, entry for entry,
    what CSRGraph.from_edge_index builds from the returned edge_index (rowptr, col, eid) — with and without the added
    self loops — and its GCN normalisation and aggregation must give the same numbers"""
    import graphgym_amd as ga
    from graphgym_amd import graphgen, ops
    from graphgym_amd.ego import ego_batch
    n = 20_000
    ei0 = graphgen.ba_edge_index(n, 4, seed=radius, device=dev)
    base = ga.CSRGraph.from_edge_index(ei0, n)
    gen = torch.Generator().manual_seed(5)
    cen = torch.randint(0, n, (300,), generator=gen).to(dev)
    cen[:3] = torch.tensor([0, 1, 2], device=dev)                     # hub-centred egos (larger than the LDS table)
    ei, orig, ids, ego_of, g = ego_batch(base, cen, radius, csr=loops)
    assert g is not None and g.symmetric
    n2 = orig.numel()
    for dst_row in (0, 1):
        want = ga.CSRGraph.from_edge_index(ei, n2, dst_row=dst_row, add_self_loops=(loops == "add"))
        assert g.nnz == want.nnz and g.num_nodes == want.num_nodes
        assert torch.equal(g.rowptr, want.rowptr)
        assert torch.equal(g.col, want.col)
        if dst_row == 1:
            assert torch.equal(g.eid, want.eid)                       # positions in edge_index; -1 - row for added loops
    gn, wn = g.gcn_norm("row"), want.gcn_norm("row")
    assert torch.equal(gn.val, wn.val) and gn.symmetric
    x = torch.rand(n2, 64, device=dev)
    assert torch.equal(ops.spmm(gn, x, "sum"), ops.spmm(wn, x, "sum"))
    # the identity-branch operators through the ego-batch shortcut equal the general build's, field for field
    fast, slow = gn.id_branch(ids), gn._id_branch_build(ids)
    for f in ("rows", "crp", "slot", "val", "defer"):
        assert torch.equal(getattr(fast, f), getattr(slow, f)), f
    assert fast.n_rows == slow.n_rows and fast.t.nnz == slow.t.nnz and fast.t.num_nodes == slow.t.num_nodes
    assert torch.equal(fast.t.rowptr, slow.t.rowptr) and torch.equal(fast.t.col, slow.t.col)
    assert torch.equal(fast.t.val, slow.t.val)
    # its transpose is itself: the same numbers as the sorted transpose of the reference build
    assert gn.transpose() is gn
    assert torch.allclose(ops.spmm(gn.transpose(), x, "sum"), ops.spmm(wn.transpose(), x, "sum"), rtol=1e-6, atol=1e-6)
    # the 4-tuple form is unchanged, and a base graph with an explicit self loop falls back (fifth value None)
    assert len(ego_batch(base, cen, radius)) == 4
    loopy = ga.CSRGraph.from_edge_index(torch.cat([ei0, torch.tensor([[7], [7]], device=dev)], 1), n)
    assert ego_batch(loopy, cen[:5], radius, csr=loops)[4] is None


def test_attention_backward_on_the_expansion_s_own_csr(dev):
    """The CSR an expansion writes is flagged symmetric (transpose() is the graph itself), but attention scores and
    coefficients are per-entry values that are NOT symmetric: their backward passes permute them through the sorted
    transpose's entry map.  Scores, softmax and the weighted aggregation (TfgIDLayer.py:333-355), forward and all three
    gradients, must equal those on the CSR built from the returned edge list."""
    import graphgym_amd as ga
    from graphgym_amd import graphgen, ops
    from graphgym_amd.ego import ego_batch
    n = 5000
    base = ga.CSRGraph.from_edge_index(graphgen.ba_edge_index(n, 3, seed=4, device=dev), n)
    cen = torch.randint(0, n, (64,), generator=torch.Generator().manual_seed(2)).to(dev)
    ei, orig, ids, ego_of, g = ego_batch(base, cen, 2, csr="add")
    assert g is not None and g.symmetric and g.transpose() is g
    n2 = orig.numel()
    want = ga.CSRGraph.from_edge_index(ei, n2, dst_row=1, add_self_loops=True)
    assert torch.equal(g.col, want.col) and not want.symmetric
    gen = torch.Generator().manual_seed(9)
    q0, k0, v0 = (torch.randn(n2, 32, generator=gen).to(dev) for _ in range(3))
    up = torch.randn(n2, 32, generator=gen).to(dev)
    outs = []
    for G in (g, want):
        q, k, v = (t.clone().requires_grad_(True) for t in (q0, k0, v0))
        for heads in (1, 4):
            sc = ops.sddmm_dot(G, q, k, heads=heads, scale=0.25)
            a = ops.edge_softmax(G, sc)
            y = ops.spmm_edge_values(G, a, v, heads=heads)
            y.backward(up)
        outs.append((y.detach(), q.grad, k.grad, v.grad))
    for a_, b_ in zip(*outs):
        assert torch.equal(a_, b_)


@pytest.mark.parametrize("radius", [1, 2])
def test_repeated_isolated_and_single_centres(dev, radius):
    """A sampled batch may name a centre twice (two separate components, transform.py:24-36 builds one ego per listed
    node), a centre without any edge (an ego of one node), or a single centre; each ego of a batch must be what the
    batch of that centre alone gives, whatever else is in the batch."""
    import graphgym_amd as ga
    from graphgym_amd import graphgen
    from graphgym_amd.ego import ego_batch
    n = 3000
    ei = graphgen.ba_edge_index(n - 2, 3, seed=6, device=dev)               # nodes n-2, n-1 have no edges
    base = ga.CSRGraph.from_edge_index(ei, n)
    cen = torch.tensor([5, 0, 5, n - 1, 77, 0, n - 2, 5], device=dev)       # 0: a hub; repeats; isolated nodes
    for csr in (None, "add"):
        out = ego_batch(base, cen, radius, csr=csr)
        e2, orig, ids, ego_of = out[:4]
        assert ids.tolist() == list(range(cen.numel())) and orig[:cen.numel()].tolist() == cen.tolist()
        sizes = torch.bincount(ego_of, minlength=cen.numel())
        for k, c in enumerate(cen.tolist()):
            one = ego_batch(base, torch.tensor([c], device=dev), radius, csr=csr)
            assert int(sizes[k]) == one[1].numel()
            mem = orig[ego_of == k]
            assert torch.equal(torch.sort(mem).values, torch.sort(one[1]).values)
            m = ego_of[e2[0]] == k
            got = collections.Counter(zip(orig[e2[0][m]].tolist(), orig[e2[1][m]].tolist()))
            want = collections.Counter(zip(one[1][one[0][0]].tolist(), one[1][one[0][1]].tolist()))
            assert got == want and int(m.sum()) == one[0].size(1)
        assert int(sizes[3]) == 1 and int(sizes[6]) == 1                    # the isolated centres
        assert torch.equal(sizes[0], sizes[2]) and torch.equal(sizes[0], sizes[7]) and torch.equal(sizes[1], sizes[5])
        if csr is not None:
            g = out[4]
            want = ga.CSRGraph.from_edge_index(e2, orig.numel(), dst_row=1, add_self_loops=True)
            assert torch.equal(g.rowptr, want.rowptr) and torch.equal(g.col, want.col)


# ---- base graphs of every networkx class: directed, parallel edges, a self loop ---------------------------------------
# transform.py:23 builds the batch as graph.G.__class__(): nx.ego_graph follows SUCCESSORS on a DiGraph and keeps parallel
# edges of a MultiGraph; CSRGraph.from_edge_index takes any edge list.  The ego batch, and the CSR the expansion writes
# for it (ego_batch(csr=...)), must be right on all of them, not only on simple undirected graphs.
BASES = ["simple", "digraph", "multigraph", "multidigraph", "selfloop"]


def edge_list(G):
    """[2, E] int64, source -> destination: both directions of every undirected edge (each parallel copy), a directed
    graph's edges as they are"""
    e = np.array(list(G.edges()), dtype=np.int64).reshape(-1, 2)
    if not G.is_directed():
        e = np.concatenate([e, e[:, ::-1]], axis=0)
    return np.ascontiguousarray(e.T)


def make_base(kind, n=90, seed=0):
    """A small base graph of the networkx class `kind` with nodes 0..N-1; the last node is isolated.  Returns (G, hub):
    hub is a node of many neighbours (the digraph's sink hub)."""
    rng = np.random.default_rng(seed)
    U = nx.powerlaw_cluster_graph(n, 2, 0.3, seed=seed)
    hub = max(U.degree, key=lambda t: t[1])[0]
    if kind in ("simple", "selfloop"):
        G = nx.Graph(U)
        if kind == "selfloop":
            G.add_edge(3, 3)                                   # the expansion's CSR needs a loop-free base: fallback
    elif kind == "digraph":
        G = nx.DiGraph()
        G.add_nodes_from(range(n))
        for u, v in U.edges():                                 # random orientation, some pairs both ways
            r = rng.random()
            if r < 0.15:
                G.add_edges_from([(u, v), (v, u)])
            else:
                G.add_edge(*((u, v) if r < 0.575 else (v, u)))
        hub, src = n, n + 1
        G.add_edges_from((u, hub) for u in range(0, n, 2))     # a sink hub: many in-edges, no out-edge
        G.add_edges_from((src, u) for u in range(1, n, 7))     # a source-only node
    elif kind == "multigraph":
        G = nx.MultiGraph(U)
        E = list(U.edges())
        for k in rng.choice(len(E), 12, replace=False):         # doubled edges
            G.add_edge(*E[k])
        G.add_edges_from([E[0], E[0]])                          # a tripled one
        G.add_edge(0, next(iter(U[0])))                         # a repeated edge at centre 0 (A_id gets a repeated entry)
    elif kind == "multidigraph":
        n = 30
        G = nx.MultiDiGraph()
        G.add_nodes_from(range(n))
        for _ in range(70):
            u, v = rng.choice(n, 2, replace=False).tolist()
            G.add_edge(u, v)
        G.add_edges_from([(0, 1), (0, 1), (1, 0), (2, 0), (2, 0)])   # parallel and reciprocal edges at centre 0
        hub = 0
    else:
        raise ValueError(kind)
    G.add_node(G.number_of_nodes())
    return G, hub


def base_on_gpu(dev, G):
    import graphgym_amd as ga
    return ga.CSRGraph.from_edge_index(torch.from_numpy(edge_list(G)).to(dev), G.number_of_nodes())


def ref_egos(G, centres, radius):
    """per listed centre k: the members of nx.ego_graph(G, c, radius) (transform.py:17-19) and the multiset of its edges
    {(k, u, v): copies}, both directions of an undirected edge"""
    members, edges = [], collections.Counter()
    for k, c in enumerate(centres):
        E = G if radius > 4 else nx.ego_graph(G, c, radius=radius)
        members.append(set(E.nodes))
        for u, v in E.edges():
            edges[(k, u, v)] += 1
            if not G.is_directed():
                edges[(k, v, u)] += 1
    return members, edges


def nx_batch_in_gpu_ids(G, radius, orig, ego_of):
    """the oracle's expansion of every node (RL.ego_nets) as an edge list in the GPU batch's node ids: a node of ego c
    with original id u is the GPU node with ego_of == c and orig == u (the numbering inside an ego is not defined by the
    reference; test_bases_of_every_class_against_networkx checks the two expansions have the same nodes)"""
    H, _, h_orig, h_ego = RL.ego_nets(G, radius, return_map=True)
    at = {(e, o): k for k, (e, o) in enumerate(zip(ego_of.tolist(), orig.tolist()))}
    m = np.array([at[(int(e), int(o))] for e, o in zip(h_ego.tolist(), h_orig.tolist())], dtype=np.int64)
    return torch.from_numpy(m[edge_list(H)])


@pytest.mark.parametrize("radius", [1, 2, 3, 5])
@pytest.mark.parametrize("kind", BASES)
def test_bases_of_every_class_against_networkx(dev, kind, radius):
    """every node a centre, as the reference does: members per ego, edge direction and parallel-edge counts equal
    RL.ego_nets on the networkx graph of the same class (successors on a directed graph)"""
    G, _ = make_base(kind)
    n = G.number_of_nodes()
    H, ids, h_orig, h_ego = RL.ego_nets(G, radius, return_map=True)
    ei, orig, idx, ego_of = expand_on_gpu(dev, edge_list(G), n, radius)
    assert orig.numel() == H.number_of_nodes() and ei.size(1) == edge_list(H).shape[1]
    assert idx.cpu().tolist() == ids.tolist() and orig[:n].cpu().tolist() == list(range(n))
    orig_c, ego_c = orig.cpu().numpy(), ego_of.cpu().numpy()
    assert canon(ei.cpu().numpy(), orig_c, ego_c) == canon(edge_list(H), h_orig.numpy(), h_ego.numpy())
    members, edges = ref_egos(G, range(n), radius)
    for c in range(n):
        assert set(orig_c[ego_c == c].tolist()) == members[c], f"members of ego {c}"
    assert canon(ei.cpu().numpy(), orig_c, ego_c) == edges


@pytest.mark.parametrize("radius", [1, 2])
@pytest.mark.parametrize("kind", BASES)
def test_bases_of_every_class_repeated_and_isolated_centres(dev, kind, radius):
    from graphgym_amd.ego import ego_batch
    G, hub = make_base(kind)
    iso = G.number_of_nodes() - 1
    cen = [5, 0, 5, iso, hub, 0, 1]
    base = base_on_gpu(dev, G)
    for csr in (None, "none", "add"):
        out = ego_batch(base, torch.tensor(cen, device=dev), radius, csr=csr)
        ei, orig, ids, ego_of = (t.cpu() for t in out[:4])
        assert ids.tolist() == list(range(len(cen))) and orig[:len(cen)].tolist() == cen
        members, edges = ref_egos(G, cen, radius)
        for k in range(len(cen)):
            assert set(orig[ego_of == k].tolist()) == members[k]
        assert canon(ei.numpy(), orig.numpy(), ego_of.numpy()) == edges


@pytest.mark.parametrize("radius", [1, 2])
def test_directed_hubs_beyond_the_lds_table(dev, radius):
    """a directed base whose hubs have more neighbours than the expansion's LDS membership table holds (4096): the
    source hub's ego is large, the sink hub's is the hub alone (nx.ego_graph follows out-edges)"""
    from graphgym_amd.ego import ego_batch
    n, sink, source = 6000, 0, 1
    rng = np.random.default_rng(11)
    G = nx.DiGraph()
    G.add_nodes_from(range(n))
    for u in range(2, n):
        G.add_edges_from((u, int(v)) for v in rng.integers(2, n, 3) if v != u)
    G.add_edges_from((u, sink) for u in range(2, 5002))
    G.add_edges_from((source, u) for u in range(500, 5500))
    base = base_on_gpu(dev, G)
    cen = [sink, source, 2, 4000, 5999, source]
    ei, orig, ids, ego_of = (t.cpu() for t in ego_batch(base, torch.tensor(cen, device=dev), radius))
    members, edges = ref_egos(G, cen, radius)
    assert members[0] == {sink} and len(members[1]) > 4096
    for k in range(len(cen)):
        assert set(orig[ego_of == k].tolist()) == members[k]
    assert canon(ei.numpy(), orig.numpy(), ego_of.numpy()) == edges


def _same_id_branch(fast, slow):
    for f in ("rows", "crp", "slot", "val", "defer"):
        a, b = getattr(fast, f), getattr(slow, f)
        assert (a is None and b is None) or torch.equal(a, b), f
    assert fast.n_rows == slow.n_rows
    for f in ("nnz", "num_nodes", "num_cols"):
        assert getattr(fast.t, f) == getattr(slow.t, f), f
    for f in ("rowptr", "col", "val"):
        a, b = getattr(fast.t, f), getattr(slow.t, f)
        assert (a is None and b is None) or torch.equal(a, b), f"t.{f}"


@pytest.mark.parametrize("radius", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", BASES)
def test_csr_written_by_the_expansion_is_none_or_the_general_build(dev, kind, radius):
    """the fifth value of ego_batch(csr=...) is None (the caller builds the CSR the general way) or EXACTLY what the
    general path builds from the returned edge list: entries, symmetry flag, identity-branch operators, transpose"""
    import graphgym_amd as ga
    from graphgym_amd import ops
    from graphgym_amd.ego import ego_batch
    G, _ = make_base(kind)
    base = base_on_gpu(dev, G)
    cen = torch.arange(G.number_of_nodes(), device=dev)
    for loops in ("none", "add"):
        ei, orig, ids, ego_of, g = ego_batch(base, cen, radius, csr=loops)
        if kind == "simple":
            assert g is not None                                  # the shortcut is taken where it holds
        if g is None:
            continue
        n2 = orig.numel()
        want = ga.CSRGraph.from_edge_index(ei, n2, dst_row=1, add_self_loops=(loops == "add"))
        assert g.nnz == want.nnz and g.num_nodes == want.num_nodes
        assert torch.equal(g.rowptr, want.rowptr) and torch.equal(g.col, want.col) and torch.equal(g.eid, want.eid)
        assert g.symmetric == want.is_symmetric(run=True)
        _same_id_branch(g.id_branch(ids), g._id_branch_build(ids))
        x = torch.rand(n2, 64, device=dev, generator=torch.Generator(device=dev).manual_seed(radius))
        assert torch.allclose(ops.spmm(g.transpose(), x, "sum"), ops.spmm(want.transpose(), x, "sum"),
                              rtol=1e-6, atol=1e-6)


def _shortcut_and_plain(dev, base, cen, radius, csr):
    """the batch as the pipeline builds it (the expansion's CSR seeded into the holder when there is one) and as the
    plain path does (4-tuple, no holder: the layers build their structures lazily)"""
    from graphgym_amd import harness as H
    from graphgym_amd.ego import ego_batch
    from graphgym_amd.layers import seed_graph_cache
    ei, orig, ids, ego_of, g = ego_batch(base, cen, radius, csr=csr)
    holder = H.Batch()
    if g is not None:
        seed_graph_cache(holder, ei, int(orig.numel()), g, csr)
    plain = ego_batch(base, cen, radius)
    return (ei, orig, ids, ego_of, holder), plain


@pytest.mark.parametrize("width", [64, 128])
@pytest.mark.parametrize("kind", BASES)
def test_gradients_through_the_layers_on_shortcut_batches(dev, kind, width):
    """ID-GCN (IDGCN, csr='add') and ID-GIN (IDGIN, csr='none') — the two kinds the batch pipeline trains — and plain
    ops.spmm / ops.agg_dense / ops.idgnn_aggregate, forward and backward, on the shortcut batch: bit for bit what the
    plain path gives, and within tests/_tol.py of the float64 oracle on the networkx expansion"""
    import torch.nn as nn
    from graphgym_amd import layers as L, ops
    from _tol import both, close, close_all
    from oracle import ref_ops as R
    G, _ = make_base(kind)
    n, radius = G.number_of_nodes(), 2
    base = base_on_gpu(dev, G)
    cen = torch.arange(n, device=dev)
    gen = torch.Generator().manual_seed(width)

    def rnd(*shape):
        return (torch.rand(*shape, generator=gen) * 2 - 1).to(dev)

    def run(layer, batch, x0, up, prepare):
        ei, ids, holder = batch
        x = x0.clone().requires_grad_(True)
        for p in layer.parameters():
            p.grad = None
        if prepare and holder is not None:
            layer.prepare([x, ei, ids], holder)
        y = layer([x, ei, ids], holder=holder)
        y.backward(up)
        return [y.detach(), x.grad] + [p.grad.clone() for p in layer.parameters()]

    for which, csr in (("idgcn", "add"), ("idgin", "none"), ("ops", "none")):
        (ei, orig, ids, ego_of, holder), plain = _shortcut_and_plain(dev, base, cen, radius, csr)
        assert torch.equal(ei, plain[0]) and torch.equal(orig, plain[1])
        n2 = orig.numel()
        x0, up = rnd(n2, width), rnd(n2, width)
        torch.manual_seed(width)
        if which == "idgcn":
            layer = L.IDGCN(width, activation=None, in_features=width).to(dev)
        elif which == "idgin":
            layer = L.IDGIN(nn.Sequential(nn.Linear(width, width), nn.Tanh()),
                            nn.Sequential(nn.Linear(width, width), nn.Tanh())).to(dev)
        else:
            W = nn.Parameter(rnd(width, width))

            class _Ops(nn.Module):
                def __init__(self):
                    super().__init__()
                    self.W = W

                def forward(self, inputs, holder=None):
                    x, e, i = inputs
                    g = L.get_graph(holder, e, x.size(0), loops="none")
                    P, Q = ops.idgnn_aggregate(g, i, x)
                    return ops.spmm(g, x, "sum") + ops.agg_dense(g, x, self.W) + 0.5 * P + 0.25 * Q
            layer = _Ops()
        got = run(layer, (ei, ids, holder), x0, up, prepare=which != "ops")
        want = run(layer, (plain[0], plain[2], None), x0, up, prepare=False)
        for k, (a, b) in enumerate(zip(got, want)):
            assert torch.equal(a, b), f"{which}: tensor {k} differs from the plain path"
        # the float64 oracle on the networkx expansion, in the batch's node ids
        ei_ref = nx_batch_in_gpu_ids(G, radius, orig.cpu(), ego_of.cpu())
        ids_c = ids.cpu()
        params = [p.detach().cpu() for p in layer.parameters()]

        def ref_fn(c):
            x = c(x0.cpu()).clone().requires_grad_(True)
            P = [c(p).clone().requires_grad_(True) for p in params]
            if which == "idgcn":
                y = RL.gcn_id(x, ei_ref, ids_c, None, P[0], P[1], P[2])
            elif which == "idgin":
                y = RL.idgin(x, ei_ref, ids_c, lambda h: torch.tanh(h @ P[0].t() + P[1]),
                             lambda h: torch.tanh(h @ P[2].t() + P[3]))
            else:
                A = R.SparseAdj(torch.stack([ei_ref[1], ei_ref[0]]), None, [n2, n2])      # row = destination
                xs = torch.zeros_like(x).index_copy(0, ids_c, x[ids_c])
                y = A @ x + (A @ x) @ P[0] + 0.5 * (A @ x) + 0.25 * (A @ xs)
            y.backward(c(up.cpu()))
            return [y.detach(), x.grad] + [p.grad for p in P]
        r64, r32 = both(ref_fn)
        close(got[0], (r64[0], r32[0]), what=f"{kind} {which} d={width} out")
        close(got[1], (r64[1], r32[1]), what=f"{kind} {which} d={width} grad x")
        for k in range(2, len(got)):
            close_all(got[k], (r64[k], r32[k]), what=f"{kind} {which} d={width} grad param {k - 2}")
