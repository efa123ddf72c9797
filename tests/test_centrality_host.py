"""Centralities, host side (no device): the oracles of tests/_centrality_ref.py against networkx — the PageRank loop bit
for bit, with the margin the GPU test's equal iteration counts rest on; the vectorised Brandes within rounding — the
one-hot permutation, the closure of include/mp_structure.h over the library's exports, the binding and the poisoning
cases, and the argument validation of every mp_struct_* entry and of the Python functions before a device is reached."""
import ctypes as C
import os
import re

import networkx as nx
import numpy as np
import pytest
import torch

import _centrality_ref as CR
import _structure_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mp_structure.h")
INVALID, UNSUPPORTED, WORKSPACE = 1, 2, 3
FAKE = C.c_void_p(256)        # a non-null pointer that is never dereferenced
BIG = 2 ** 31
SIZES = (1, 2, 3, 4, 64, 65, 1000, 4096)


# ---- PageRank: the restated loop is nx.pagerank -----------------------------------------------------------------------

def test_pagerank_loop_is_networkx_bit_for_bit_with_a_stopping_margin():
    """the GPU test demands the loop's iteration counts: no err of any step may lie within a relative 1e-6 of n tol
    (measured on these inputs: the closest is 2.7e-3; the counts range from 1 to 76)"""
    closest, counts = np.inf, []
    for name, G in CR.small_inputs().items():
        x, iters, errs = CR.pagerank_loop(G)
        assert np.array_equal(x, CR.nx_pagerank(G)), name
        assert iters == len(errs) >= 1, name
        bound = G.number_of_nodes() * 1e-6
        closest = min(closest, min(abs(e - bound) / bound for e in errs))
        counts.append(iters)
    print("closest err to n tol (relative):", closest, "iteration counts:", min(counts), "..", max(counts))
    assert closest > 1e-6
    assert min(counts) == 1 and max(counts) > 50          # the one-step and the slow inputs are both in the list


def test_pagerank_loop_with_other_arguments_and_without_convergence():
    G = R.pc_graphs(1)[0]
    x, iters, errs = CR.pagerank_loop(G, alpha=0.5, tol=1e-9)
    assert np.array_equal(x, CR.nx_pagerank(G, alpha=0.5, tol=1e-9))
    bound = G.number_of_nodes() * 1e-9
    assert min(abs(e - bound) / bound for e in errs) > 1e-6
    _, iters, errs = CR.pagerank_loop(nx.path_graph(200), max_iter=5)
    assert iters == -1 and len(errs) == 5
    with pytest.raises(nx.PowerIterationFailedConvergence):
        nx.pagerank(nx.path_graph(200), max_iter=5)


@pytest.mark.parametrize("n", [2048, 2049])
def test_pagerank_margin_at_the_form_boundary(n):
    G = CR.with_isolated(nx.powerlaw_cluster_graph(n - 3, 3, 0.5, seed=1))
    x, iters, errs = CR.pagerank_loop(G)
    assert np.array_equal(x, CR.nx_pagerank(G))
    assert min(abs(e - n * 1e-6) / (n * 1e-6) for e in errs) > 1e-6


# ---- betweenness: the vectorised oracle --------------------------------------------------------------------------------

def betweenness_inputs():
    """the betweenness inputs of the GPU test: name -> graph (nodes 0..n-1)"""
    tri = nx.Graph([(0, 1), (1, 2), (0, 2), (2, 3)])
    tri.add_node(4)
    parts = nx.disjoint_union(nx.disjoint_union(nx.cycle_graph(5), nx.path_graph(4)), nx.empty_graph(1))
    out = {f"pc{k}": G for k, G in enumerate(R.pc_graphs())}
    out.update({f"ba{k}": G for k, G in enumerate(R.ba_graphs())})
    out.update(ring65=nx.cycle_graph(65), grid6x6=nx.convert_node_labels_to_integers(nx.grid_2d_graph(6, 6)),
               bipartite3x4=nx.complete_bipartite_graph(3, 4), triangle_pendant_isolated=tri,
               two_components_and_a_node=parts, pc300=nx.powerlaw_cluster_graph(300, 3, 0.5, seed=3),
               path5=nx.path_graph(5), star200=nx.star_graph(199), path1=nx.path_graph(1), path2=nx.path_graph(2))
    return out


def boundary_graph(n):
    return CR.with_isolated(nx.powerlaw_cluster_graph(n - 3, 3, 0.5, seed=1))


def test_vectorised_brandes_is_networkx_within_rounding():
    """3 n 2^-53 bounds either side's distance from the true value (the GPU test's derivation): the two agree within
    1e-12 for n <= 1024, zeros are exact zeros, and sigma stays exact (below 2^53)"""
    for name, G in betweenness_inputs().items():
        got, top = CR.brandes(G)
        want = CR.nx_betweenness(G)
        assert np.abs(got - want).max() <= 1e-12, name
        assert (got[want == 0.0] == 0.0).all(), name
        assert top < 2.0 ** 53, name


def test_sigma_stays_exact_on_the_boundary_graphs_and_not_on_a_grid():
    from graphgym_amd import _lib_structure as LS
    for n in (LS.BETWEENNESS_LDS_NODES, LS.BETWEENNESS_LDS_NODES + 1):
        assert CR.brandes(boundary_graph(n))[1] < 2.0 ** 53
    assert CR.brandes(nx.convert_node_labels_to_integers(nx.grid_2d_graph(30, 30)))[1] > 2.0 ** 53   # not an input


# ---- the permutation --------------------------------------------------------------------------------------------------

def test_onehot_host_is_a_permutation_keyed_by_seed_and_graph():
    from graphgym_amd import structure as S
    perm = CR.onehot_host(SIZES, seed=0)
    assert np.array_equal(S.onehot_host(SIZES, seed=0), perm) and perm.dtype == np.int64
    at = 0
    for n in SIZES:
        assert np.array_equal(np.sort(perm[at:at + n]), np.arange(n)), n
        at += n
    other = S.onehot_host(SIZES, seed=1)
    assert not np.array_equal(other[-4096:], perm[-4096:]) and not np.array_equal(other[-5096:-4096], perm[-5096:-4096])
    twice = S.onehot_host([1000, 1000], seed=0)
    assert not np.array_equal(twice[:1000], twice[1000:])
    assert np.array_equal(np.sort(twice[1000:]), np.arange(1000))
    assert S.onehot_host([], seed=0).shape == (0,)


# ---- the header's closure -----------------------------------------------------------------------------------------------

def declared_symbols(path=HEADER):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mp_struct_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound_and_the_reverse():
    from graphgym_amd import _lib, _lib_structure
    from graphgym_amd import build as mpbuild
    lib = _lib_structure.lib()
    names = declared_symbols()
    assert len(names) >= 5
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mp_structure.h but not exported"
        assert n in _lib_structure.PROTOTYPES_STRUCTURE, f"{n} has no ctypes prototype"
    for n in _lib_structure.PROTOTYPES_STRUCTURE:
        assert n.startswith("mp_struct_") and n in names, f"ctypes binds {n} which mp_structure.h does not declare"
        assert getattr(lib, n).argtypes == _lib_structure.PROTOTYPES_STRUCTURE[n][1]
    engine = open(os.path.join(ROOT, "include", "mp_engine.h")).read()
    assert "mp_struct_" not in engine
    assert not [n for n in _lib.PROTOTYPES if n.startswith("mp_struct_")]
    assert HEADER in mpbuild.HEADERS and "centrality.hip" in mpbuild.SOURCES
    from graphgym_amd.edge_nets import BFS_MAX_NODES
    assert _lib_structure.BETWEENNESS_MAX_NODES == BFS_MAX_NODES
    assert _lib_structure.PAGERANK_CHUNK <= _lib_structure.PAGERANK_LDS_NODES
    assert _lib_structure.ONEHOT_STREAM == CR.ONEHOT_STREAM


def test_every_entry_has_a_poisoning_case_or_is_a_host_entry():
    """mirrors tests/test_poison_host.py::test_every_c_entry_has_a_case_or_a_reason for include/mp_structure.h"""
    import test_poison_structure_gpu as P
    from graphgym_amd import _lib_structure
    covered = set()
    for case in P.CASES:
        assert case.entries and case.exact and callable(case.run), case.name
        covered |= set(case.entries)
    every = set(declared_symbols())
    assert every == set(_lib_structure.PROTOTYPES_STRUCTURE)
    assert covered <= every, f"cases name entries that do not exist: {sorted(covered - every)}"
    host_only = {n for n in every if n.endswith("_bytes")}
    assert not (covered & host_only)
    assert not (every - covered - host_only), f"C entries without a case: {sorted(every - covered - host_only)}"


# ---- the C entries, before anything is launched -------------------------------------------------------------------------

def _lib():
    from graphgym_amd import _lib_structure
    return _lib_structure.lib()


def _pagerank(N=10, nnz=20, n_graphs=1, n_chunks=0, alpha=0.85, tol=1e-6, max_iter=100, ws_bytes=1 << 20, rowptr=FAKE,
              col=FAKE, graph_ptr=FAKE, chunk_ptr=FAKE, out=FAKE, iters=FAKE, ws=FAKE):
    return _lib().mp_struct_pagerank(rowptr, col, N, nnz, graph_ptr, n_graphs, chunk_ptr, n_chunks, alpha, tol, max_iter,
                                     out, iters, ws, ws_bytes, None)


def _betweenness(N=10, nnz=20, n_graphs=1, max_nodes=10, n_slices=1, ws_bytes=1 << 20, rowptr=FAKE, col=FAKE,
                 graph_ptr=FAKE, slice_ptr=FAKE, out=FAKE, ws=FAKE):
    return _lib().mp_struct_betweenness(rowptr, col, N, nnz, graph_ptr, n_graphs, max_nodes, slice_ptr, n_slices, out,
                                        ws, ws_bytes, None)


def _onehot(N=10, n_graphs=1, graph_ptr=FAKE, out=FAKE):
    return _lib().mp_struct_onehot(graph_ptr, n_graphs, N, 0, out, None)


def test_pagerank_entry_validates_its_arguments():
    for name in ("rowptr", "col", "graph_ptr", "out", "iters"):
        assert _pagerank(**{name: None}) == INVALID, name
    for name in ("chunk_ptr", "ws"):                                   # (needed only with chunks)
        assert _pagerank(N=5000, n_chunks=5, **{name: None}) == INVALID, name
    for bad in (dict(N=-1), dict(nnz=-1), dict(n_graphs=-1), dict(n_graphs=0), dict(n_chunks=-1), dict(alpha=-0.1),
                dict(alpha=1.5), dict(alpha=float("nan")), dict(tol=-1.0), dict(max_iter=0)):
        assert _pagerank(**bad) == INVALID, bad
    assert _pagerank(N=BIG) == UNSUPPORTED and _pagerank(nnz=BIG + 1) == UNSUPPORTED
    assert _pagerank(N=5000, n_chunks=5, ws_bytes=64) == WORKSPACE
    assert _pagerank(N=0, nnz=0, col=None, out=None, iters=None, chunk_ptr=None, ws=None) == 0      # nothing to do
    nb = C.c_size_t(0)
    assert _lib().mp_struct_pagerank_ws_bytes(-1, 1, 0, C.byref(nb)) == INVALID
    assert _lib().mp_struct_pagerank_ws_bytes(10, 1, 0, None) == INVALID
    assert _lib().mp_struct_pagerank_ws_bytes(10, 1, 0, C.byref(nb)) == 0 and nb.value == 16
    assert _lib().mp_struct_pagerank_ws_bytes(5000, 2, 5, C.byref(nb)) == 0 and nb.value == 8 * (15000 + 10 + 2)


def test_betweenness_entry_validates_its_arguments_and_its_size_limit():
    for name in ("rowptr", "col", "graph_ptr", "slice_ptr", "out", "ws"):
        assert _betweenness(**{name: None}) == INVALID, name
    for bad in (dict(N=-1), dict(nnz=-1), dict(n_graphs=-1), dict(n_graphs=0), dict(max_nodes=-1), dict(max_nodes=11),
                dict(n_slices=-1)):
        assert _betweenness(**bad) == INVALID, bad
    assert _betweenness(N=BIG) == UNSUPPORTED
    assert _betweenness(N=1 << 17, max_nodes=(1 << 16) + 1) == UNSUPPORTED          # the size limit of hop_sums
    assert _betweenness(ws_bytes=8) == WORKSPACE
    assert _betweenness(N=0, nnz=0, max_nodes=0, col=None, slice_ptr=None, out=None, ws=None) == 0
    nb = C.c_size_t(0)
    lib = _lib()
    assert lib.mp_struct_betweenness_ws_bytes(-1, 0, C.byref(nb)) == INVALID
    assert lib.mp_struct_betweenness_ws_bytes(10, 10, None) == INVALID
    assert lib.mp_struct_betweenness_ws_bytes(1 << 17, (1 << 16) + 1, C.byref(nb)) == UNSUPPORTED
    assert lib.mp_struct_betweenness_ws_bytes(1280, 64, C.byref(nb)) == 0 and nb.value == 2 * 1280 * 8 + 16
    assert lib.mp_struct_betweenness_ws_bytes(3000, 3000, C.byref(nb)) == 0 and nb.value == 94 * 3000 * 28 + 16


def test_onehot_entry_validates_its_arguments():
    for name in ("graph_ptr", "out"):
        assert _onehot(**{name: None}) == INVALID, name
    assert _onehot(N=-1) == INVALID and _onehot(n_graphs=-1) == INVALID and _onehot(n_graphs=0) == INVALID
    assert _onehot(N=BIG) == UNSUPPORTED
    assert _onehot(N=0, out=None) == 0


# ---- the Python functions, before the engine is reached ------------------------------------------------------------------

def _cpu_base(N=6):
    from graphgym_amd.graph import CSRGraph
    rowptr = torch.arange(N + 1, dtype=torch.int32)
    g = CSRGraph(rowptr, torch.roll(torch.arange(N, dtype=torch.int32), 1), None, None, N, N)
    g.symmetric = True
    return g


def test_functions_check_before_the_engine_is_reached(monkeypatch):
    from graphgym_amd import _lib as L
    from graphgym_amd import structure as S
    monkeypatch.setattr(S, "_require_hip", lambda t, name: None)
    monkeypatch.setattr(S.LS, "lib", lambda: pytest.fail("the engine was reached"))
    base = _cpu_base(6)
    calls = (S.node_pagerank, S.node_betweenness_centrality, S.node_onehot)
    for fn in calls:
        for gp in ([0, 3, 5], [1, 6], [0, 4, 2, 6], [0]):
            with pytest.raises(ValueError, match="graph_ptr"):
                fn(base, torch.tensor(gp))
        with pytest.raises(ValueError, match="empty"):
            fn(base, torch.tensor([0, 3, 3, 6]))
    big = _cpu_base(1)
    big.num_nodes = (1 << 16) + 1
    with pytest.raises(L.EngineError, match="65536"):
        S.node_betweenness_centrality(big)
    directed = _cpu_base(6)
    directed.symmetric = False
    directed.is_symmetric = lambda run=None: False
    for call in [lambda fn=fn: fn(directed) for fn in calls] + [
            lambda: S.raw("node_pagerank", directed), lambda: S.raw("edge_path_len", directed)]:
        with pytest.raises(ValueError, match="undirected"):
            call()


def test_the_keys():
    from graphgym_amd import structure as S
    assert S.UNBUILT_KEYS == ("graph_laplacian_spectrum",) and isinstance(S.UNBUILT_KEYS, tuple)
    for key in ("node_pagerank", "node_betweenness_centrality", "node_onehot", "edge_path_len"):
        assert key in S.NODE_KEYS and key in S.SUPPORTED_KEYS
    assert len(S.SUPPORTED_KEYS) == 11
