"""Structural labels and features on the GPU (graphgym_amd.structure, csrc/structure.hip) against networkx, the way
feature_augment.py:51-107 calls it (tests/_structure_ref.py).  Integers are compared with torch.equal, and so are the
float64 quotients: both sides are one correctly rounded division of the same two exact integers."""
import functools

import networkx as nx
import numpy as np
import pytest
import torch

import _structure_ref as R

pytestmark = pytest.mark.gpu


def _t(a, dev):
    return torch.from_numpy(np.asarray(a)).to(dev)


@functools.lru_cache(maxsize=None)
def _pc20():
    graphs = R.pc_graphs(20)
    return graphs, dict(tri=R.triangles(graphs), cc=R.clustering(graphs), deg=R.degree(graphs),
                        avg=R.average_clustering(graphs))


@functools.lru_cache(maxsize=None)
def _ba20():
    graphs = R.ba_graphs(20)
    return graphs, dict(node=R.node_path_len(graphs), graph=R.graph_path_len(graphs))


def _check_against_networkx(graphs, dev):
    from graphgym_amd import structure as S
    base, _ = R.base_of(graphs, dev)
    tri2, deg = S.triangles(base)
    assert tri2.dtype == torch.int64 and deg.dtype == torch.int64
    assert torch.equal(tri2, 2 * _t(R.triangles(graphs), dev))
    assert torch.equal(S.node_clustering_coefficient(base), _t(R.clustering(graphs), dev))
    assert torch.equal(S.node_degree(base), _t(R.degree(graphs), dev))
    return tri2, deg


def test_known_answers(dev):
    from graphgym_amd import structure as S
    tri_pendant = nx.Graph([(0, 1), (1, 2), (0, 2), (2, 3)])
    base, _ = R.base_of([tri_pendant], dev)
    tri2, deg = S.triangles(base)
    assert tri2.tolist() == [2, 2, 2, 0] and deg.tolist() == [2, 2, 3, 1]
    assert torch.equal(S.node_clustering_coefficient(base),
                       torch.tensor([1.0, 1.0, 1.0 / 3.0, 0.0], dtype=torch.float64, device=dev))
    base, _ = R.base_of([nx.complete_graph(5)], dev)
    assert S.node_clustering_coefficient(base).tolist() == [1.0] * 5
    assert S.triangles(base)[0].tolist() == [12] * 5
    base, _ = R.base_of([nx.star_graph(6)], dev)
    assert S.node_clustering_coefficient(base).tolist() == [0.0] * 7
    assert S.node_degree(base).tolist() == [6] + [1] * 6


def test_isolated_node_and_self_loop(dev):
    from graphgym_amd import structure as S
    G = nx.Graph([(0, 1), (1, 2), (0, 2), (2, 3)])
    G.add_node(4)                                          # isolated
    plain, _ = R.base_of([G], dev)
    t0, d0 = S.triangles(plain)
    assert d0.tolist() == [2, 2, 3, 1, 0] and S.node_clustering_coefficient(plain)[4].item() == 0.0
    G.add_edge(2, 2)
    G.add_edge(4, 4)
    looped, _ = R.base_of([G], dev)
    assert looped.has_self_loops()
    t1, d1 = S.triangles(looped)
    assert torch.equal(t1, t0) and torch.equal(d1, d0)
    assert torch.equal(S.node_clustering_coefficient(looped), S.node_clustering_coefficient(plain))
    assert (S.node_degree(looped) - S.node_degree(plain)).tolist() == [0, 0, 2, 0, 2]
    assert torch.equal(S.node_degree(looped), _t(R.degree([G]), dev))


def test_empty_operators(dev):
    import graphgym_amd as ga
    from graphgym_amd import structure as S
    none = ga.CSRGraph.from_csr(torch.zeros(1, dtype=torch.int32, device=dev),
                                torch.zeros(0, dtype=torch.int32, device=dev), None, 0)
    tri2, deg = S.triangles(none)
    assert tri2.numel() == 0 and deg.numel() == 0 and S.node_clustering_coefficient(none).numel() == 0
    s, r = S.hop_sums(none)
    assert s.numel() == 0 and r.numel() == 0
    bare = ga.CSRGraph.from_csr(torch.zeros(4, dtype=torch.int32, device=dev),
                                torch.zeros(0, dtype=torch.int32, device=dev), None, 3)
    tri2, deg = S.triangles(bare)
    assert tri2.tolist() == [0, 0, 0] and deg.tolist() == [0, 0, 0]
    assert S.node_clustering_coefficient(bare).tolist() == [0.0] * 3 and S.node_degree(bare).tolist() == [0] * 3
    s, r = S.hop_sums(bare, torch.tensor([0, 1, 2, 3]))
    assert s.tolist() == [0, 0, 0] and r.tolist() == [1, 1, 1]
    assert S.graph_path_len(bare, torch.tensor([0, 1, 2, 3])).tolist() == [0.0] * 3


def test_batch_of_powerlaw_cluster_graphs(dev):
    from graphgym_amd import structure as S
    graphs, ref = _pc20()
    base, gp = R.base_of(graphs, dev)
    tri2, _ = S.triangles(base)
    assert torch.equal(tri2 // 2, _t(ref["tri"], dev)) and bool((tri2 % 2 == 0).all())
    assert torch.equal(S.node_clustering_coefficient(base), _t(ref["cc"], dev))
    assert torch.equal(S.node_degree(base), _t(ref["deg"], dev))
    again, _ = S.triangles(base)
    assert torch.equal(again, tri2)                        # integer atomics: the same bits every run


def test_graph_clustering_coefficient(dev):
    """two summation orders of n_g values in [0, 1], each within (n_g - 1) 2^-53 n_g of the exact sum before the
    division by n_g: the means differ by at most 2 n_g 2^-53"""
    from graphgym_amd import structure as S
    graphs, ref = _pc20()
    base, gp = R.base_of(graphs, dev)
    got = S.graph_clustering_coefficient(base, gp)
    assert got.dtype == torch.float64 and got.shape == (20,)
    err = (got.cpu() - torch.from_numpy(ref["avg"])).abs().max().item()
    print("graph_clustering_coefficient max |diff|", err)
    assert err <= 2 * 64 * 2.0 ** -53
    with pytest.raises(ValueError, match="empty"):
        S.graph_clustering_coefficient(base, torch.tensor([0, 64, 64, int(gp[-1])]))


def test_hub_row_shared_by_many_waves(dev):
    G = nx.wheel_graph(3001)                               # node 0 is the hub, 3 000 rim nodes
    tri2, deg = _check_against_networkx([G], dev)
    assert tri2[0].item() == 2 * 3000 and deg[0].item() == 3000
    assert tri2[1:].tolist() == [4] * 3000


def test_powerlaw_cluster_3000(dev):
    _check_against_networkx([nx.powerlaw_cluster_graph(3000, 4, 0.3, seed=1)], dev)


def test_graph_and_row_boundaries_inside_entry_chunks(dev):
    graphs = [nx.powerlaw_cluster_graph(n, min(3, n - 1), 0.5, seed=n) if n > 3 else nx.complete_graph(n)
              for n in (1, 2, 3, 63, 64, 65)]
    _check_against_networkx(graphs, dev)
    from graphgym_amd import structure as S
    base, gp = R.base_of(graphs, dev)
    err = (S.graph_clustering_coefficient(base, gp).cpu() - torch.from_numpy(R.average_clustering(graphs))).abs()
    assert bool((err <= 2 * 65 * 2.0 ** -53).all())


@pytest.mark.parametrize("n", [1, 2, 31, 32, 33, 64, 65, 1025])
def test_hop_sums_on_a_path(dev, n):
    from graphgym_amd import structure as S
    base, gp = R.base_of([R.path_graph(n)], dev)
    s, r = S.hop_sums(base)
    i = torch.arange(n, device=dev)
    assert s.dtype == torch.int64 and r.dtype == torch.int64
    assert torch.equal(s, i * (i + 1) // 2 + (n - 1 - i) * (n - i) // 2)
    assert torch.equal(r, torch.full((n,), n, device=dev))


def test_path_lengths_against_networkx(dev):
    from graphgym_amd import structure as S
    graphs, ref = _ba20()
    base, gp = R.base_of(graphs, dev)
    assert torch.equal(S.node_path_len(base, gp), _t(ref["node"], dev))
    assert torch.equal(S.graph_path_len(base, gp), _t(ref["graph"], dev))
    some = torch.tensor([3, 64, 700, 1279])
    assert torch.equal(S.node_path_len(base, gp, nodes=some), _t(ref["node"], dev)[some.to(dev)])
    with pytest.raises(ValueError, match="outside"):
        S.hop_sums(base, gp, nodes=torch.tensor([1280]))
    W = nx.connected_watts_strogatz_graph(200, 4, 0.1, seed=3)
    base, gp = R.base_of([W], dev)
    assert torch.equal(S.node_path_len(base), _t(R.node_path_len([W]), dev))
    assert torch.equal(S.graph_path_len(base), _t(R.graph_path_len([W]), dev))


def test_two_components_and_a_single_node(dev):
    from graphgym_amd import structure as S
    two = nx.Graph()
    two.add_nodes_from(range(7))
    two.add_edges_from([(0, 1), (1, 2), (2, 3), (4, 5), (5, 6), (4, 6)])
    one = nx.Graph()
    one.add_node(0)
    graphs = [nx.path_graph(5), two, one]
    base, gp = R.base_of(graphs, dev)
    s, r = S.hop_sums(base, gp)
    assert r.tolist() == [5] * 5 + [4] * 4 + [3] * 3 + [1]
    assert torch.equal(S.node_path_len(base, gp), _t(R.node_path_len(graphs), dev))     # over the reachable set only
    with pytest.raises(ValueError, match="graph 1 is not connected"):
        S.graph_path_len(base, gp)
    base, gp = R.base_of([nx.path_graph(5), one], dev)
    assert S.graph_path_len(base, gp).tolist() == [2.0, 0.0]
    with pytest.raises(ValueError, match="empty"):
        S.graph_path_len(base, torch.tensor([0, 5, 5, 6]))


def test_size_limit_and_the_int64_sum(dev):
    import graphgym_amd as ga
    from graphgym_amd import structure as S

    def path(n):
        a = torch.arange(n - 1, device=dev)
        return ga.CSRGraph.from_edge_index(torch.stack([torch.cat([a, a + 1]), torch.cat([a + 1, a])]), n)

    s, r = S.hop_sums(path(65536), nodes=torch.tensor([0, 32768]))
    assert s[0].item() == 2147450880                       # 65535 * 65536 / 2: the largest sum a search can return
    assert s[1].item() == 32768 * 32769 // 2 + 32767 * 32768 // 2
    assert r.tolist() == [65536, 65536]
    with pytest.raises(ga.EngineError, match="65536"):
        S.hop_sums(path(65537), nodes=torch.tensor([0]))


def _every_function(S, base):
    return [lambda: S.triangles(base), lambda: S.node_degree(base), lambda: S.node_clustering_coefficient(base),
            lambda: S.graph_clustering_coefficient(base), lambda: S.hop_sums(base), lambda: S.node_path_len(base),
            lambda: S.graph_path_len(base), lambda: S.node_const(base), lambda: S.node_identity(base, feature_dim=2),
            lambda: S.raw("node_degree", base),
            lambda: S.augment(base, None, ["node_degree"], [4])]


def test_directed_and_repeated_entries_are_refused(dev):
    import graphgym_amd as ga
    from graphgym_amd import structure as S
    directed = ga.CSRGraph.from_edge_index(torch.tensor([[0, 1, 2], [1, 2, 0]], device=dev), 3)
    repeated = ga.CSRGraph.from_edge_index(torch.tensor([[0, 1, 0, 1, 1, 2], [1, 0, 1, 0, 2, 1]], device=dev), 3)
    assert repeated.nnz == 6
    for base in (directed, repeated):
        for call in _every_function(S, base):
            with pytest.raises(ValueError, match="undirected"):
                call()


def test_augment_end_to_end(dev):
    from graphgym_amd import structure as S
    graphs, ref = _pc20()
    base, gp = R.base_of(graphs, dev)
    edges = R.np_bin_edges(ref["cc"], 10, "balanced")
    want = R.np_digitize(ref["cc"], edges)
    tensors, feat_dims, label_dim = S.augment(base, gp, [], [], label="node_clustering_coefficient", label_dim=10)
    lab = tensors["node_clustering_coefficient_label"]
    assert feat_dims == [] and label_dim == len(edges)
    assert lab.dtype == torch.int64 and lab.device.type == "cuda" and torch.equal(lab, _t(want, dev))
    tensors, feat_dims, label_dim = S.augment(base, gp, ["node_degree", "node_clustering_coefficient"], [8, 8],
                                              label="node_clustering_coefficient", label_dim=10,
                                              feature_repr="balanced")
    assert torch.equal(tensors["node_clustering_coefficient_label"], lab) and label_dim == len(edges)
    for key, values, dim in zip(("node_degree", "node_clustering_coefficient"), (ref["deg"], ref["cc"]), feat_dims):
        e = R.np_bin_edges(values, 8, "balanced")
        assert dim == len(e)
        got = tensors[key]
        assert got.dtype == torch.float32 and got.shape == (len(values), len(e))
        assert torch.equal(got, _t(R.np_one_hot(R.np_digitize(values, e), len(e)), dev))
    assert feat_dims[0] < 8                               # integer degrees tie: balanced bins collapse
    # a regression label stays as it is, [n, 1] float32
    tensors, _, label_dim = S.augment(base, gp, ["node_const"], [1], label="node_clustering_coefficient", label_dim=1,
                                      task_type="regression", feature_repr="original")
    assert label_dim == 1 and tensors["node_const"].shape == (len(want), 1)
    assert torch.equal(tensors["node_clustering_coefficient_label"], _t(ref["cc"], dev).float().unsqueeze(-1))
