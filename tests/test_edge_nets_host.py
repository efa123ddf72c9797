"""Argument validation of the edge-net expansion and the hop-distance search (csrc/edge.hip) and of their bindings,
without a device (CPU suite).  Every case returns before anything is launched or dereferenced on the device."""
import ctypes as C

import pytest
import torch

from graphgym_amd import _lib

INVALID, UNSUPPORTED = 1, 2
FAKE = C.c_void_p(256)        # a non-null pointer that is never dereferenced
BIG = 2 ** 31


def _expand(N=10, nnz=20, n_graphs=1, n_copies=10, n_out_nodes=100, n_out_edges=200, max_size=20, flags=0,
            rowptr=FAKE, col=FAKE, row=FAKE, graph_ptr=FAKE, copy_graph=FAKE, node_base=FAKE, edge_index=FAKE,
            orig_node=FAKE, csr_rowptr=FAKE):
    return _lib.lib().mp_edge_expand(rowptr, col, row, None, N, nnz, graph_ptr, n_graphs, copy_graph, FAKE, node_base,
                                     FAKE, n_copies, n_out_nodes, n_out_edges, max_size, flags, edge_index, orig_node,
                                     FAKE, FAKE, FAKE, csr_rowptr, FAKE, FAKE, None)


def _hops(N=10, nnz=20, n_graphs=1, max_nodes=10, n_sources=3, n_pairs=5, rowptr=FAKE, col=FAKE, graph_ptr=FAKE,
          sources=FAKE, pair_dst=FAKE, dist=FAKE):
    return _lib.lib().mp_hop_distances(rowptr, col, N, nnz, graph_ptr, n_graphs, max_nodes, sources, FAKE, n_sources,
                                       FAKE, pair_dst, FAKE, n_pairs, dist, None)


def test_prototypes_exist():
    for name in ("mp_edge_expand", "mp_hop_distances"):
        assert name in _lib.PROTOTYPES
        assert hasattr(_lib.lib(), name)


def test_expand_null_pointers_and_sizes():
    assert _expand(rowptr=None) == INVALID
    assert _expand(col=None) == INVALID
    assert _expand(row=None) == INVALID
    assert _expand(graph_ptr=None) == INVALID
    assert _expand(copy_graph=None) == INVALID
    assert _expand(node_base=None) == INVALID
    assert _expand(edge_index=None) == INVALID
    assert _expand(orig_node=None) == INVALID
    assert _expand(flags=1, csr_rowptr=None) == INVALID
    assert _expand(flags=2) == INVALID                    # self loops without the CSR
    assert _expand(flags=4) == INVALID
    assert _expand(N=-1) == INVALID
    assert _expand(n_copies=-1) == INVALID
    assert _expand(n_graphs=0) == INVALID                 # copies of no graph


def test_expand_int32_overflow_of_the_outputs():
    assert _expand(n_out_nodes=BIG) == UNSUPPORTED
    assert _expand(n_out_edges=BIG) == UNSUPPORTED
    assert _expand(n_out_edges=BIG - 10, n_out_nodes=100, flags=3) == UNSUPPORTED    # E' + N' self entries
    assert _expand(n_copies=BIG) == UNSUPPORTED
    assert _expand(N=BIG) == UNSUPPORTED


def test_hops_null_pointers_and_sizes():
    assert _hops(rowptr=None) == INVALID
    assert _hops(col=None) == INVALID
    assert _hops(graph_ptr=None) == INVALID
    assert _hops(sources=None) == INVALID
    assert _hops(pair_dst=None) == INVALID
    assert _hops(dist=None) == INVALID
    assert _hops(n_pairs=-1) == INVALID
    assert _hops(n_graphs=0) == INVALID
    assert _hops(N=BIG) == UNSUPPORTED
    assert _hops(n_sources=BIG) == UNSUPPORTED
    assert _hops(max_nodes=(1 << 16) + 1) == UNSUPPORTED  # the search's bitmaps live in LDS
    assert _hops(n_sources=0, n_pairs=0) == 0             # nothing to do: no launch


def _cpu_base(N=6):
    """a stand-in for a CSRGraph on the host: the bindings check their arguments before they touch the device"""
    from graphgym_amd.graph import CSRGraph
    rowptr = torch.arange(N + 1, dtype=torch.int32)
    col = torch.roll(torch.arange(N, dtype=torch.int32), 1)
    return CSRGraph(rowptr, col, None, None, N, N)


def _binding_checks(monkeypatch):
    # (no device on this machine: the HIP check of the bindings is lifted so that the argument checks behind it run;
    # each case must raise before anything reaches the engine)
    from graphgym_amd import edge_nets
    monkeypatch.setattr(edge_nets, "_require_hip", lambda t, name: None)
    monkeypatch.setattr(edge_nets, "lib", lambda: pytest.fail("the engine was reached"))
    return edge_nets


def test_bindings_reject_graph_ptr_that_does_not_cover_the_nodes(monkeypatch):
    E = _binding_checks(monkeypatch)
    base = _cpu_base(6)
    li, lab = torch.tensor([[0], [1]]), torch.tensor([1])
    for gp in ([0, 3, 5], [1, 6], [0, 4, 2, 6], [0], [0, 3, 7]):
        with pytest.raises(ValueError, match="graph_ptr"):
            E.edge_batch(base, torch.tensor(gp), li, lab)
        with pytest.raises(ValueError, match="graph_ptr"):
            E.hop_distances(base, torch.tensor([0]), torch.tensor([1]), torch.tensor(gp))


def test_bindings_reject_sources_outside_their_graph(monkeypatch):
    E = _binding_checks(monkeypatch)
    base = _cpu_base(6)
    gp = torch.tensor([0, 3, 6])
    with pytest.raises(ValueError, match="different graphs"):
        E.edge_batch(base, gp, torch.tensor([[1], [4]]), torch.tensor([0]))
    with pytest.raises(ValueError, match="outside"):
        E.edge_batch(base, gp, torch.tensor([[6], [4]]), torch.tensor([0]))
    with pytest.raises(ValueError, match="outside"):
        E.edge_batch(base, gp, torch.tensor([[1], [2]]), torch.tensor([0]), sources=torch.tensor([1, 9]))
    with pytest.raises(ValueError, match="no copy"):
        E.edge_batch(base, gp, torch.tensor([[1], [2]]), torch.tensor([0]), sources=torch.tensor([0, 4]))
    with pytest.raises(ValueError, match="outside"):
        E.hop_distances(base, torch.tensor([-1]), torch.tensor([1]), gp)
    with pytest.raises(ValueError, match="outside"):
        E.hop_distances(base, torch.tensor([1]), torch.tensor([6]), gp)


def test_edge_head_is_registered_and_rejects_multiclass_binary_decoding():
    from graphgym_amd import harness as H
    from graphgym_amd.config import cfg
    assert H.head_dict["edge"] is H.GNNEdgeHead and H.head_dict["link_pred"] is H.GNNEdgeHead
    assert H.head_dict["node"] is H.GNNNodeHead and H.head_dict["graph"] is H.GNNGraphHead
    old = getattr(cfg.model, "edge_decoding", None)
    try:
        for dec in ("dot", "cosine_similarity"):
            cfg.model.edge_decoding = dec
            with pytest.raises(ValueError, match="Binary"):
                H.GNNEdgeHead(8, 2)
        cfg.model.edge_decoding = "bilinear"
        with pytest.raises(ValueError, match="Unknown"):
            H.GNNEdgeHead(8, 1)
    finally:
        if old is None:
            del cfg.model.edge_decoding
        else:
            cfg.model.edge_decoding = old
