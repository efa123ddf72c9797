"""PageRank, betweenness and one-hot ids on the GPU (graphgym_amd.structure, csrc/centrality.hip) against networkx and the
host oracles of tests/_centrality_ref.py.

Tolerances (float64 on both sides, rtol = 0 everywhere):
  PageRank      iters equal the restated loop's exactly (tests/test_centrality_host.py asserts the margin that makes this
                a fair demand); values within n 2^-53 / (1 - alpha): the two sides differ in the order of sums of at most
                n terms that add up to at most 1, n 2^-53 a step, damped by alpha each step.  That is 7.6e-13 at n = 1024,
                so atol = 1e-12 for every graph of n <= 1024.
  betweenness   a dependency carries a relative error of about n 2^-52, the sum over sources adds n 2^-53, the scaled
                value is at most 1: either side is within 3 n 2^-53 = 3.4e-13 of the true value at n = 1024, atol = 1e-12;
                6 n 2^-53 for the graphs at the storage bound.  A node whose reference value is 0.0 must be 0.0 exactly.
Both are reproducible bit for bit and do not depend on the batch: a graph's slice of a union equals the graph alone."""
import functools

import networkx as nx
import numpy as np
import pytest
import torch

import _centrality_ref as CR
import _structure_ref as R
from test_centrality_host import SIZES, betweenness_inputs, boundary_graph

pytestmark = pytest.mark.gpu
ATOL = 1e-12


def _bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.view(torch.int64), b.view(torch.int64))


def _slices(graphs):
    at = np.concatenate([[0], np.cumsum([G.number_of_nodes() for G in graphs])])
    return [slice(int(a), int(b)) for a, b in zip(at[:-1], at[1:])]


@functools.lru_cache(maxsize=None)
def _pagerank_small():
    """name -> (graph, restated values, restated iteration count), computed once"""
    return {name: (G,) + CR.pagerank_loop(G)[:2] for name, G in CR.small_inputs().items()}


@functools.lru_cache(maxsize=None)
def _betweenness_small():
    return {name: (G, CR.nx_betweenness(G)) for name, G in betweenness_inputs().items()}


@functools.lru_cache(maxsize=None)
def _nx_labels(which, kind):
    graphs = R.pc_graphs() if which == "pc" else R.ba_graphs()
    fn = CR.nx_pagerank if kind == "node_pagerank" else CR.nx_betweenness
    return graphs, np.concatenate([fn(G) for G in graphs])


# ---- PageRank --------------------------------------------------------------------------------------------------------

def test_pagerank_union_and_alone(dev):
    from graphgym_amd import structure as S
    refs = _pagerank_small()
    graphs = [r[0] for r in refs.values()]
    base, gp = R.base_of(graphs, dev)
    out, iters = S.node_pagerank(base, gp, return_iters=True)
    assert out.dtype == torch.float64 and iters.dtype == torch.int32
    assert iters.tolist() == [r[2] for r in refs.values()]
    want = np.concatenate([r[1] for r in refs.values()])
    err = np.abs(out.cpu().numpy() - want).max()
    print("pagerank, union: max |diff|", err, "iters", int(iters.min()), "..", int(iters.max()))
    assert err <= ATOL
    again, iters2 = S.node_pagerank(base, gp, return_iters=True)
    assert _bits(out, again) and torch.equal(iters, iters2)                   # reproducible
    for (name, (G, x, it)), sl in zip(refs.items(), _slices(graphs)):
        b1, _ = R.base_of([G], dev)
        alone, it1 = S.node_pagerank(b1, return_iters=True)
        assert it1.tolist() == [it], name
        assert np.abs(alone.cpu().numpy() - x).max() <= ATOL, name
        assert _bits(alone, out[sl]), f"{name}: the batch changed the bits"    # batch-invariant


def test_pagerank_dangling_and_tiny_graphs(dev):
    from graphgym_amd import structure as S
    base, gp = R.base_of([nx.empty_graph(4), nx.path_graph(1), CR.path_with_isolated()], dev)
    out, iters = S.node_pagerank(base, gp, return_iters=True)
    assert out[:5].tolist() == [0.25] * 4 + [1.0] and iters[:2].tolist() == [1, 1]
    assert abs(float(out[5:].sum()) - 1.0) <= ATOL


def test_pagerank_other_arguments(dev):
    from graphgym_amd import structure as S
    graphs = R.pc_graphs(3) + [CR.path_with_isolated()]
    base, gp = R.base_of(graphs, dev)
    out, iters = S.node_pagerank(base, gp, alpha=0.5, tol=1e-9, return_iters=True)
    want = np.concatenate([CR.nx_pagerank(G, alpha=0.5, tol=1e-9) for G in graphs])
    assert np.abs(out.cpu().numpy() - want).max() <= ATOL           # (a step more or less would show as ~1e-9)
    assert int(iters.min()) >= 1
    with pytest.raises(ValueError, match="graph 1 has not converged"):
        S.node_pagerank(*R.base_of([nx.path_graph(2), nx.path_graph(200)], dev), max_iter=5)


def test_pagerank_both_forms(dev):
    """a graph at the LDS form's bound and one just above it (the large form: three chunks), with dangling nodes"""
    from graphgym_amd import _lib_structure as LS
    from graphgym_amd import structure as S
    graphs = [boundary_graph(LS.PAGERANK_LDS_NODES), boundary_graph(LS.PAGERANK_LDS_NODES + 1)]
    assert [G.number_of_nodes() for G in graphs] == [LS.PAGERANK_LDS_NODES, LS.PAGERANK_LDS_NODES + 1]
    base, gp = R.base_of(graphs, dev)
    out, iters = S.node_pagerank(base, gp, return_iters=True)
    for G, sl, it in zip(graphs, _slices(graphs), iters.tolist()):
        n = G.number_of_nodes()
        x, want_it, _ = CR.pagerank_loop(G)
        err = np.abs(out[sl].cpu().numpy() - x).max()
        print("pagerank, n =", n, "max |diff|", err, "iters", it)
        assert it == want_it
        assert err <= n * 2.0 ** -53 / (1 - 0.85)
        alone, it1 = S.node_pagerank(R.base_of([G], dev)[0], return_iters=True)
        assert _bits(alone, out[sl]) and it1.tolist() == [it]
    # a large-form graph that does not converge reports it, and one that has stopped is left alone by later steps
    with pytest.raises(ValueError, match="graph 0 has not converged"):
        S.node_pagerank(R.base_of([graphs[1]], dev)[0], max_iter=3)


# ---- betweenness -------------------------------------------------------------------------------------------------------

def test_betweenness_known_answers(dev):
    from graphgym_amd import structure as S
    got = S.node_betweenness_centrality(R.base_of([nx.path_graph(5)], dev)[0]).cpu().numpy()
    assert got.dtype == np.float64 and got[0] == 0.0 and got[4] == 0.0
    assert np.abs(got - np.array([0, 1 / 2, 2 / 3, 1 / 2, 0])).max() <= ATOL
    got = S.node_betweenness_centrality(R.base_of([nx.star_graph(199)], dev)[0]).cpu().numpy()
    assert abs(got[0] - 1.0) <= ATOL and (got[1:] == 0.0).all()
    base, gp = R.base_of([nx.path_graph(1), nx.path_graph(2)], dev)
    assert S.node_betweenness_centrality(base, gp).tolist() == [0.0, 0.0, 0.0]


def test_betweenness_against_networkx(dev):
    from graphgym_amd import structure as S
    refs = _betweenness_small()
    batches = ([n for n in refs if n[:2] in ("pc", "ba") and n != "pc300"],
               [n for n in refs if not (n[:2] in ("pc", "ba") and n != "pc300")])
    for names in batches:
        graphs = [refs[n][0] for n in names]
        base, gp = R.base_of(graphs, dev)
        out = S.node_betweenness_centrality(base, gp)
        assert _bits(out, S.node_betweenness_centrality(base, gp))                # reproducible
        for name, sl in zip(names, _slices(graphs)):
            G, want = refs[name]
            got = out[sl].cpu().numpy()
            assert np.abs(got - want).max() <= ATOL, name
            assert (got[want == 0.0] == 0.0).all(), name
            if names is batches[1] or name in ("pc0", "pc7", "ba19"):
                alone = S.node_betweenness_centrality(R.base_of([G], dev)[0])
                assert _bits(alone, out[sl]), f"{name}: the batch changed the bits"


def test_betweenness_both_forms(dev):
    """a graph at the LDS form's bound and one just above it (level, sigma and delta in the workspace), as one batch"""
    from graphgym_amd import _lib_structure as LS
    from graphgym_amd import structure as S
    graphs = [boundary_graph(LS.BETWEENNESS_LDS_NODES), boundary_graph(LS.BETWEENNESS_LDS_NODES + 1)]
    assert [G.number_of_nodes() for G in graphs] == [LS.BETWEENNESS_LDS_NODES, LS.BETWEENNESS_LDS_NODES + 1]
    base, gp = R.base_of(graphs, dev)
    out = S.node_betweenness_centrality(base, gp)
    for G, sl in zip(graphs, _slices(graphs)):
        n = G.number_of_nodes()
        want, top = CR.brandes(G)
        assert top < 2.0 ** 53
        got = out[sl].cpu().numpy()
        print("betweenness, n =", n, "max |diff|", np.abs(got - want).max())
        assert np.abs(got - want).max() <= 6 * n * 2.0 ** -53
        assert (got[want == 0.0] == 0.0).all()
    alone = S.node_betweenness_centrality(R.base_of([graphs[1]], dev)[0])
    assert _bits(alone, out[_slices(graphs)[1]])


# ---- one-hot ids -------------------------------------------------------------------------------------------------------

def test_onehot_is_the_host_permutation(dev):
    from graphgym_amd import structure as S
    graphs = [nx.path_graph(n) for n in SIZES]
    base, gp = R.base_of(graphs, dev)
    got = S.node_onehot(base, gp, seed=0)
    assert got.dtype == torch.int64
    assert np.array_equal(got.cpu().numpy(), S.onehot_host(SIZES, seed=0))
    assert np.array_equal(got.cpu().numpy(), CR.onehot_host(SIZES, seed=0))
    for sl in _slices(graphs):
        assert torch.equal(torch.sort(got[sl]).values, torch.arange(sl.stop - sl.start, device=dev))
    other = S.node_onehot(base, gp, seed=5)
    assert not torch.equal(other, got) and np.array_equal(other.cpu().numpy(), S.onehot_host(SIZES, seed=5))
    assert torch.equal(S.raw("node_onehot", base, gp, seed=5), other)
    whole = S.node_onehot(base, seed=0)                                       # one graph of all the nodes
    assert torch.equal(torch.sort(whole).values, torch.arange(base.num_nodes, device=dev))


# ---- refusals and degenerate inputs ------------------------------------------------------------------------------------

def _calls(S):
    return (S.node_pagerank, S.node_betweenness_centrality, S.node_onehot)


def test_refusals(dev):
    import graphgym_amd as ga
    from graphgym_amd import structure as S
    directed = ga.CSRGraph.from_edge_index(torch.tensor([[0, 1, 2], [1, 2, 0]], device=dev), 3)
    repeated = ga.CSRGraph.from_edge_index(torch.tensor([[0, 1, 0, 1], [1, 0, 1, 0]], device=dev), 2)
    ok, _ = R.base_of([nx.path_graph(4)], dev)
    for fn in _calls(S):
        for base in (directed, repeated):
            with pytest.raises(ValueError, match="undirected"):
                fn(base)
        with pytest.raises(ValueError, match="empty"):
            fn(ok, torch.tensor([0, 2, 2, 4]))
    a = torch.arange(65536, device=dev)
    path = ga.CSRGraph.from_edge_index(torch.stack([torch.cat([a, a + 1]), torch.cat([a + 1, a])]), 65537)
    with pytest.raises(ga.EngineError, match="65536"):
        S.node_betweenness_centrality(path)


def test_degenerate_inputs(dev):
    import graphgym_amd as ga
    from graphgym_amd import structure as S
    none = ga.CSRGraph.from_edge_index(torch.zeros((2, 0), dtype=torch.int64, device=dev), 0)
    pr, iters = S.node_pagerank(none, return_iters=True)
    assert pr.shape == (0,) and pr.dtype == torch.float64 and iters.shape == (0,)
    assert S.node_betweenness_centrality(none).shape == (0,) and S.node_onehot(none).shape == (0,)
    edgeless = ga.CSRGraph.from_edge_index(torch.zeros((2, 0), dtype=torch.int64, device=dev), 7)
    for gp, sizes in ((None, [7]), (torch.tensor([0, 3, 4, 7]), [3, 1, 3])):
        pr, iters = S.node_pagerank(edgeless, gp, return_iters=True)
        assert pr.tolist() == [1.0 / n for n in sizes for _ in range(n)] and iters.tolist() == [1] * len(sizes)
        assert S.node_betweenness_centrality(edgeless, gp).tolist() == [0.0] * 7
        ids = S.node_onehot(edgeless, gp)
        assert np.array_equal(ids.cpu().numpy(), S.onehot_host(sizes))
    one, _ = R.base_of([nx.path_graph(1)], dev)
    assert S.node_pagerank(one).tolist() == [1.0] and S.node_betweenness_centrality(one).tolist() == [0.0]
    assert S.node_onehot(one, seed=9).tolist() == [0]


# ---- the keys ----------------------------------------------------------------------------------------------------------

def test_edge_path_len_is_node_path_len(dev):
    from graphgym_amd import structure as S
    base, gp = R.base_of(R.ba_graphs(4), dev)
    cache = {}
    a = S.raw("edge_path_len", base, gp, _cache=cache)
    hops = cache["hops"]
    b = S.raw("node_path_len", base, gp, _cache=cache)
    assert _bits(a, b) and cache["hops"] is hops and _bits(a, S.edge_path_len(base, gp))


@pytest.mark.parametrize("label", ["node_pagerank", "node_betweenness_centrality"])
@pytest.mark.parametrize("which", ["pc", "ba"])
def test_augment_end_to_end(dev, which, label):
    """the design-space grids' call.  The class ids are those of the reference's binning of networkx's values, except at
    nodes whose networkx value lies within 1e-12 of a bin edge (for betweenness: non-zero ones only), at most 1 %"""
    from graphgym_amd import structure as S
    graphs, values = _nx_labels(which, label)
    edges = R.np_bin_edges(values, 10, "balanced")
    want = R.np_digitize(values, edges)
    near = np.abs(values[:, None] - edges[None, :]).min(axis=1) <= 1e-12
    if label == "node_betweenness_centrality":
        near &= values != 0.0
    print(which, label, "nodes within 1e-12 of an edge:", int(near.sum()), "of", len(values))
    assert near.mean() <= 0.01
    base, gp = R.base_of(graphs, dev)
    tensors, feat_dims, label_dim = S.augment(base, gp, ["node_const", "node_onehot", "node_clustering_coefficient"],
                                              [1, 8, 8], label=label, label_dim=10)
    got = tensors[label + "_label"].cpu().numpy()
    assert label_dim == len(edges) and got.dtype == np.int64
    assert np.array_equal(got[~near], want[~near])
    assert tensors["node_onehot"].shape == (len(values), feat_dims[1]) and feat_dims[1] == 8
    assert tensors["node_const"].shape[0] == len(values) and tensors["node_clustering_coefficient"].shape[0] == len(values)
    ids = S.node_onehot(base, gp)
    assert torch.equal(tensors["node_onehot"], S.represent(ids, 8, "balanced"))
