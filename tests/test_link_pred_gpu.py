"""Link-prediction batches on the GPU (graphgym_amd.link_pred, csrc/link.hip): the device sampler against its NumPy
restatement bit for bit, ranks beyond 2^32, the pair-space counts against torch, the no-synchronisation contract on a side
stream, and run/configs/IDGNN/edge.yaml scaled down — split -> disjoint -> link_batch -> harness.GNN — with and without
the edge transform."""
import contextlib

import pytest
import torch

import _link_graphs as LG

pytestmark = pytest.mark.gpu

MODES = [False, True]         # directed?


def _both(base, gp, counts, directed, seed, offset=0):
    """(device draw, host draw) of the same plan arguments"""
    from graphgym_amd.link_pred import plan_negatives, run_negatives, sample_non_edges_host
    plan = plan_negatives(base, gp, counts, directed)
    got = run_negatives(plan, seed, offset).cpu()
    want = sample_non_edges_host(base, gp, counts, seed, offset, directed=plan.directed)
    return got, want, plan


@pytest.mark.parametrize("directed", MODES)
@pytest.mark.parametrize("name", sorted(LG.CASES))
def test_device_draw_equals_the_host_restatement(dev, name, directed):
    """every hand-made graph of the host file, a partial draw and K_g = C_g (the whole complement), bit for bit"""
    base, gp, stored = LG.build(name, directed, dev)
    free = LG.complement(stored, gp, directed)
    for want_k in (3, 10 ** 6):
        counts = [min(len(f), want_k) for f in free]
        got, want, plan = _both(base, gp, counts, directed, seed=11, offset=want_k % 7)
        assert plan.C_host == [len(f) for f in free]
        assert got.dtype == torch.int64 and torch.equal(got, want)
        pairs = LG.check_sample(got, counts, gp, stored, directed)
        if want_k > 3:
            assert set(pairs) == set().union(*free)


@pytest.fixture(scope="module")
def ba_batch(dev):
    """8 BA(64, 2) graphs as one base on the device: (base, graph_ptr, links per graph)"""
    import graphgym_amd as ga
    from graphgym_amd import graphgen
    parts = [graphgen.ba_edge_index(64, 2, seed=100 + s) + 64 * s for s in range(8)]
    gp = torch.arange(9, dtype=torch.int64) * 64
    base = ga.CSRGraph.from_edge_index(torch.cat(parts, 1).to(dev), 8 * 64)
    return base, gp, [p.size(1) // 2 for p in parts]


def test_device_draw_equals_the_host_restatement_on_ba_graphs(dev, ba_batch):
    """ratio 1: as many negatives as links in each of 8 BA(64, 2) graphs; the mode is read off the base"""
    base, gp, links = ba_batch
    got, want, plan = _both(base, gp, links, None, seed=2, offset=9)
    assert plan.directed is False and torch.equal(got, want)
    assert bool((got[0] < got[1]).all()) and bool((got[0] // 64 == got[1] // 64).all())
    assert torch.equal(got[0] // 64, torch.repeat_interleave(torch.arange(8), torch.tensor(links)))
    key = got[1] * 512 + got[0]
    stored = base.row_ids().long().cpu() * 512 + base.col.long().cpu()
    assert torch.unique(key).numel() == key.numel() and not bool(torch.isin(key, stored).any())


def test_ranks_beyond_two_to_the_32(dev):
    """one sparse graph of 100 000 nodes and about 200 000 links: 5e9 unordered pairs, so the ranks, the prefix and the
    Feistel halves (b = 17) leave 32 bits.  Every pair inside the graph, not stored (a sorted key list and
    torch.searchsorted), distinct, and equal to the host restatement"""
    import graphgym_amd as ga
    n, K = 100_000, 4096
    gen = torch.Generator().manual_seed(0)
    u, v = torch.randint(n, (2, 200_000), generator=gen)
    keep = u != v
    lo, hi = torch.minimum(u, v)[keep], torch.maximum(u, v)[keep]
    und = torch.unique(lo * n + hi)
    lo, hi = und // n, und % n
    ei = torch.stack([torch.cat([lo, hi]), torch.cat([hi, lo])])
    base = ga.CSRGraph.from_edge_index(ei.to(dev), n)
    gp = torch.tensor([0, n])
    got, want, plan = _both(base, gp, [K], None, seed=7)
    assert plan.C_host == [n * (n - 1) // 2 - und.numel()] and plan.C_host[0] > 2 ** 32
    assert torch.equal(got, want)
    g = got.to(dev)
    assert bool((g[0] >= 0).all()) and bool((g[0] < g[1]).all()) and bool((g[1] < n).all())
    keys = torch.sort(und.to(dev)).values
    k = g[0] * n + g[1]
    at = torch.searchsorted(keys, k).clamp(max=keys.numel() - 1)
    assert not bool((keys[at] == k).any())
    assert torch.unique(k).numel() == K
    assert int(g[0].max()) > n // 2                      # (the draw reaches the far rows: ranks beyond 2^32)


def test_free_counts_against_torch(dev):
    """mp_pair_space_rows on a directed batch of several components with self loops, both modes' definitions in torch:
    directed free[r] = (n_g - 1) - (entries of row r off the diagonal)"""
    import graphgym_amd as ga
    from graphgym_amd.link_pred import plan_negatives
    gen = torch.Generator().manual_seed(4)
    sizes = [7, 1, 12, 30]
    gp = LG.graph_ptr(sizes)
    N = int(gp[-1])
    edges = []
    for g, n in enumerate(sizes):
        lo = int(gp[g])
        m = torch.randint(n, (2, 3 * n), generator=gen) + lo            # self loops among them
        edges.append(m)
    ei = torch.cat(edges, 1)
    ei = torch.unique(ei[1] * N + ei[0])
    ei = torch.stack([ei % N, ei // N])
    assert bool((ei[0] == ei[1]).any())
    base = ga.CSRGraph.from_edge_index(ei.to(dev), N)
    plan = plan_negatives(base, gp, [0] * len(sizes))
    assert plan.directed is True
    graph_of = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    off_diag = torch.bincount(ei[1][ei[0] != ei[1]], minlength=N)
    want = torch.tensor(sizes)[graph_of] - 1 - off_diag
    assert plan.free.dtype == torch.int64 and torch.equal(plan.free.cpu(), want)
    assert torch.equal(plan.prefix.cpu(), torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(want, 0)]))
    # undirected counts on the symmetrised graph: the partners above r that row r does not store
    sym = torch.unique(torch.cat([ei[1] * N + ei[0], ei[0] * N + ei[1]]))
    sym = torch.stack([sym % N, sym // N])
    base = ga.CSRGraph.from_edge_index(sym.to(dev), N)
    plan = plan_negatives(base, gp, [0] * len(sizes))
    assert plan.directed is False
    above = torch.bincount(sym[1][sym[0] > sym[1]], minlength=N)
    want = gp[1:][graph_of] - 1 - torch.arange(N) - above
    assert torch.equal(plan.free.cpu(), want)


def test_two_draws_on_a_side_stream_with_one_synchronisation(dev, ba_batch):
    """run_negatives enqueues and returns: two draws of one plan with different offsets on a side stream, copied out on
    that stream, one synchronisation at the end — both equal the host's"""
    from graphgym_amd.link_pred import plan_negatives, run_negatives, sample_non_edges_host
    base, gp, links = ba_batch
    plan = plan_negatives(base, gp, links)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        first = run_negatives(plan, 5, offset=1).clone()
        second = run_negatives(plan, 5, offset=2).clone()
    side.synchronize()
    assert torch.equal(first.cpu(), sample_non_edges_host(base, gp, links, 5, 1))
    assert torch.equal(second.cpu(), sample_non_edges_host(base, gp, links, 5, 2))
    assert not torch.equal(first, second)


def test_refusals_on_the_device(dev):
    import graphgym_amd as ga
    from graphgym_amd.link_pred import plan_negatives
    ei = torch.tensor([[0, 1, 1, 2, 1], [1, 0, 2, 1, 0]], device=dev)          # 1 -> 0 twice
    base = ga.CSRGraph.from_edge_index(ei, 4)
    with pytest.raises(ValueError, match="twice"):
        plan_negatives(base, torch.tensor([0, 4]), [1], directed=True)
    base, gp, _ = LG.build("path4", False, dev)
    with pytest.raises(ValueError, match="two graphs"):
        plan_negatives(base, torch.tensor([0, 2, 4]), [0, 0])
    with pytest.raises(ValueError, match="graph 0: 4 negatives.* 3 non-edges"):
        plan_negatives(base, gp, [4])
    one_way, _, _ = LG.build("path4", True, dev)
    with pytest.raises(ValueError, match="symmetric"):
        plan_negatives(one_way, gp, [1], directed=False)


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


def _model_cfg(**extra):
    kw = dict(gnn__layers_mp=2, gnn__dim_inner=32, gnn__layers_pre_mp=1, gnn__layers_post_mp=1, gnn__batchnorm=True,
              gnn__l2norm=True, gnn__act="relu", gnn__dropout=0.0, gnn__agg="add", gnn__normalize_adj=False,
              gnn__stage_type="stack")
    kw.update(extra)
    return _cfg(**kw)


def test_edge_yaml_scaled_down(dev, ba_batch):
    """run/configs/IDGNN/edge.yaml at 8 BA(64, 2) graphs, idconv, layers_mp = 2, d = 32: split [0.8, 0.2] -> disjoint 0.8
    -> link_batch(transform='edge') -> harness.GNN as node classification.  One forward and backward: a finite loss and
    a finite gradient on every parameter; node_label_index addresses, in the copy of src, the node dst of every label
    pair; no positive of any split among the negatives.  (No accuracy bar: nobody has measured one.)"""
    from graphgym_amd import harness as H
    from graphgym_amd.link_pred import disjoint, link_batch, link_split
    base, gp, links = ba_batch
    gen = torch.Generator().manual_seed(0)
    splits = link_split(base, gp, (0.8, 0.2), generator=gen)
    train = disjoint(splits["train"], 0.8, generator=gen)
    assert train.pos_index.size(1) + train.pairs.size(1) == splits["train"].pos_index.size(1)
    x = torch.rand(base.num_nodes, 10, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    batch = link_batch(train, x, ratio=1.0, seed=3, offset=0, transform="edge")
    eli, P = batch.edge_label_index, train.pos_index.size(1)
    assert eli.size(1) == 2 * P and torch.equal(eli[:, :P], train.pos_index)
    assert batch.node_label.dtype == torch.int64
    assert torch.equal(batch.node_label, torch.cat([torch.ones(P), torch.zeros(P)]).long().to(dev))
    nli = batch.node_label_index
    assert torch.equal(batch.orig_node[nli], eli[1])
    assert torch.equal(batch.copy_source[batch.copy_of_node[nli].long()], eli[0])
    stored = base.row_ids().long() * 512 + base.col.long()
    assert not bool(torch.isin(eli[1, P:] * 512 + eli[0, P:], stored).any())
    # the copies are copies of the message graph: every edge of the batch is a message edge, no supervision edge is
    msg = train.edge_index[1] * 512 + train.edge_index[0]
    orig = batch.orig_node[batch.edge_index]
    assert bool(torch.isin(orig[1] * 512 + orig[0], msg).all())
    sup = torch.cat([train.pos_index[1] * 512 + train.pos_index[0], train.pos_index[0] * 512 + train.pos_index[1]])
    assert not bool(torch.isin(sup, msg).any())
    with _model_cfg(gnn__layer_type="idconv", dataset__task="node", dataset__transform="edge"):
        torch.manual_seed(0)
        model = H.GNN(10, 2).to(dev)
        pred, y = model(batch)
        loss = torch.nn.functional.cross_entropy(pred, y)
        loss.backward()
    assert pred.shape == (2 * P, 2) and bool(torch.isfinite(loss))
    for name, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name


def test_edge_head_without_the_transform(dev, ba_batch):
    """task: link_pred without transform: edge — the message graph, GNNEdgeHead with edge_decoding: dot, one training
    step with a finite loss; the validation batch predicts its held-out links from the train edges"""
    from graphgym_amd import harness as H
    from graphgym_amd.link_pred import link_batch, link_split
    base, gp, links = ba_batch
    splits = link_split(base, gp, (0.8, 0.2), generator=torch.Generator().manual_seed(0))
    x = torch.rand(base.num_nodes, 10, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    with _model_cfg(gnn__layer_type="generalconv", dataset__task="link_pred", dataset__transform="none",
                    model__edge_decoding="dot"):
        torch.manual_seed(0)
        model = H.GNN(10, 1).to(dev)
        assert isinstance(model.post_mp, H.GNNEdgeHead)
        opt = torch.optim.Adam(model.parameters(), lr=0.01)

        def forward_loss():
            batch = link_batch(splits["train"], x, ratio=1.0, seed=1, offset=0)
            pred, y = model(batch)
            assert pred.shape == y.shape == (2 * splits["train"].pos_index.size(1),)
            return torch.nn.functional.binary_cross_entropy_with_logits(pred, y)
        loss = H.train_step(model, opt, forward_loss)
        assert bool(torch.isfinite(torch.as_tensor(loss)))
        with torch.no_grad():
            val = link_batch(splits["val"], x, ratio=1.0, seed=1, offset=1)
            pred, y = model(val)
        assert torch.equal(val.edge_index, splits["train"].edge_index)
        assert bool(torch.isfinite(pred).all()) and y.numel() == 2 * splits["val"].pos_index.size(1)
