"""The dataset-wide representation of graphgym_amd.structure (feature_augment.py:134-245 restated in torch) on CPU
tensors against the numpy restatement in tests/_structure_ref.py, the key dispatcher, and the argument validation of
mp_csr_triangles / mp_hop_sums and of their bindings, without a device (CPU suite)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _structure_ref as R
from graphgym_amd import _lib
from graphgym_amd import structure as S

INVALID, UNSUPPORTED = 1, 2
FAKE = C.c_void_p(256)        # a non-null pointer that is never dereferenced
BIG = 2 ** 31

# ties at the edges, repeated values that collapse balanced bins, the maximum several times (a value on the last edge)
FLOATS = np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.1, 0.1, 0.25, 1 / 3, 1 / 3, 0.5, 0.5, 0.5, 2 / 3, 0.75, 1.0, 1.0,
                   1.0, 0.2, 0.05, 0.0, 0.9, 1 / 7], dtype=np.float64)
INTS = np.array([2, 2, 2, 2, 3, 3, 3, 2, 2, 5, 9, 2, 4, 4, 2, 2, 31, 2, 3, 6], dtype=np.int64)


def _same(t, a):
    a = np.asarray(a)
    assert tuple(t.shape) == a.shape, (t.shape, a.shape)
    assert np.array_equal(t.numpy(), a), (t, a)


@pytest.mark.parametrize("values", [FLOATS, INTS], ids=["floats", "ints"])
@pytest.mark.parametrize("dim", [1, 2, 3, 5, 8, 10, 16])
def test_balanced_edges_and_classes(values, dim):
    edges = S.bin_edges(torch.from_numpy(values), dim, "balanced")
    want = R.np_bin_edges(values, dim, "balanced")
    _same(edges, want)
    _same(S.digitize(torch.from_numpy(values), edges), R.np_digitize(values, want))


def test_balanced_bins_collapse():
    edges = S.bin_edges(torch.from_numpy(INTS), 10, "balanced")
    assert edges.numel() < 10 and edges.numel() == len(R.np_bin_edges(INTS, 10, "balanced"))
    one_hot = S.represent(torch.from_numpy(INTS), 10, "balanced")
    assert one_hot.dtype == torch.float32 and one_hot.shape == (len(INTS), edges.numel())
    _same(one_hot, R.np_one_hot(R.np_digitize(INTS, edges.numpy()), edges.numel()))
    label = S.represent(torch.from_numpy(INTS), 10, "balanced", as_label=True)
    assert label.dtype == torch.int64
    _same(label, R.np_digitize(INTS, edges.numpy()))


@pytest.mark.parametrize("values", [FLOATS, INTS], ids=["floats", "ints"])
@pytest.mark.parametrize("dim", [1, 2, 4, 7, 10])
def test_equal_width_edges_and_classes(values, dim):
    edges = S.bin_edges(torch.from_numpy(values), dim, "equal_width")
    want = R.np_bin_edges(values, dim, "equal_width")
    _same(edges, want)
    if dim > 1:
        assert edges[-1].item() == values.max()                  # the maximum sits on the last edge: class dim - 1
        cls = S.digitize(torch.from_numpy(values), edges)
        _same(cls, R.np_digitize(values, want))
        assert cls.max().item() == dim - 1
        _same(S.represent(torch.from_numpy(values), dim, "equal_width"), R.np_one_hot(R.np_digitize(values, want), dim))


def test_bounded():
    small = np.array([0, 1, 1, 3, 7, 2], dtype=np.int64)
    edges = S.bin_edges(torch.from_numpy(small), 8, "bounded")
    _same(edges, np.arange(8))
    _same(S.digitize(torch.from_numpy(small), edges), R.np_digitize(small, np.arange(8)))
    _same(S.represent(torch.from_numpy(small), 8, "bounded"), R.np_one_hot(small, 8))
    # bins of width 1 up to dim - 1: an integer above the bound, or below 0, is refused
    with pytest.raises(ValueError, match="outside"):
        S.represent(torch.tensor([0, 1, 9]), 8, "bounded")
    with pytest.raises(ValueError, match="outside"):
        S.represent(torch.from_numpy(INTS), 8, "bounded", as_label=True)         # (holds 9 and 31)
    with pytest.raises(ValueError, match="outside"):
        S.represent(torch.tensor([0.5, -0.5]), 4, "bounded")
    with pytest.raises(ValueError, match="outside"):
        S.digitize(torch.tensor([-1]), edges)                                    # where the reference asserts


def test_unknown_method():
    for call in (lambda: S.bin_edges(torch.from_numpy(FLOATS), 4, "quantile"),
                 lambda: S.represent(torch.from_numpy(FLOATS), 4, "quantile"),
                 lambda: S.augment(None, None, ["node_degree"], [4], feature_repr="quantile")):
        with pytest.raises(ValueError, match="not supported"):
            call()


def test_original():
    v = torch.from_numpy(FLOATS)
    out = S.represent(v, 4, "original")
    assert out.shape == (len(FLOATS), 1) and out.dtype == torch.float64 and torch.equal(out[:, 0], v)
    lab = S.represent(v, 4, "original", as_label=True)
    assert lab.shape == (len(FLOATS), 1) and lab.dtype == torch.float32 and torch.equal(lab[:, 0], v.float())
    per_graph = S.represent(v, 4, "original", as_label=True, node_level=False)
    assert per_graph.shape == (len(FLOATS),) and per_graph.dtype == torch.float32


@pytest.mark.parametrize("values", [FLOATS, INTS], ids=["floats", "ints"])
@pytest.mark.parametrize("dim", [2, 4, 16, 64])
def test_position(values, dim):
    """fp32 against the float64 formula: the argument is at most dim / 2 and carries a few fp32 roundings (the cast,
    the scale, the product, the power and the quotient), sin and cos add their own: within dim 2^-23"""
    got = S.represent(torch.from_numpy(values), dim, "position")
    want = R.np_position(values, dim)
    assert got.dtype == torch.float32 and tuple(got.shape) == want.shape == (len(values), 2 * (dim // 2))
    err = np.abs(got.numpy().astype(np.float64) - want).max()
    print("position", dim, "max |diff|", err)
    assert err <= dim * 2.0 ** -23


def test_raw_names_the_supported_keys():
    for key in S.UNBUILT_KEYS + ("node_nonsense",):
        with pytest.raises(KeyError) as info:
            S.raw(key, None)
        for name in S.SUPPORTED_KEYS:
            assert name in str(info.value)
    assert set(S.SUPPORTED_KEYS) | set(S.UNBUILT_KEYS) == {
        "node_degree", "node_betweenness_centrality", "node_path_len", "node_pagerank", "node_clustering_coefficient",
        "node_identity", "node_const", "node_onehot", "edge_path_len", "graph_laplacian_spectrum", "graph_path_len",
        "graph_clustering_coefficient"}                          # feature_augment.py:109-122


# ---- the C entries and the bindings, before anything is launched -----------------------------------------------------

def _tri(N=10, nnz=20, rowptr=FAKE, col=FAKE, row_of=FAKE, tri2=FAKE, deg=FAKE):
    return _lib.lib().mp_csr_triangles(rowptr, col, row_of, N, nnz, tri2, deg, None)


def _sums(N=10, nnz=20, n_graphs=1, max_nodes=10, n_sources=3, rowptr=FAKE, col=FAKE, graph_ptr=FAKE, sources=FAKE,
          source_graph=FAKE, dist_sum=FAKE, reached=FAKE):
    return _lib.lib().mp_hop_sums(rowptr, col, N, nnz, graph_ptr, n_graphs, max_nodes, sources, source_graph,
                                  n_sources, dist_sum, reached, None)


def test_triangles_entry_validates_its_arguments():
    assert "mp_csr_triangles" in _lib.PROTOTYPES and hasattr(_lib.lib(), "mp_csr_triangles")
    for name in ("rowptr", "col", "row_of", "tri2", "deg"):
        assert _tri(**{name: None}) == INVALID, name
    assert _tri(N=-1) == INVALID and _tri(nnz=-1) == INVALID
    assert _tri(nnz=BIG) == UNSUPPORTED and _tri(N=BIG) == UNSUPPORTED
    assert _tri(N=0, nnz=0, rowptr=None, col=None, row_of=None, tri2=None, deg=None) == 0       # nothing to do


def test_hop_sums_entry_validates_its_arguments():
    assert "mp_hop_sums" in _lib.PROTOTYPES and hasattr(_lib.lib(), "mp_hop_sums")
    for name in ("rowptr", "col", "graph_ptr", "sources", "source_graph", "dist_sum", "reached"):
        assert _sums(**{name: None}) == INVALID, name
    assert _sums(N=-1) == INVALID and _sums(n_sources=-1) == INVALID and _sums(n_graphs=0) == INVALID
    assert _sums(N=BIG) == UNSUPPORTED and _sums(n_sources=BIG) == UNSUPPORTED
    assert _sums(max_nodes=(1 << 16) + 1) == UNSUPPORTED          # the search's bitmaps live in LDS
    assert _sums(max_nodes=1 << 16, n_sources=0) == 0             # nothing to do: no launch


def _cpu_base(N=6):
    """a stand-in for a CSRGraph on the host (a ring, flagged symmetric): the bindings check their arguments before
    they touch the device"""
    from graphgym_amd.graph import CSRGraph
    rowptr = torch.arange(N + 1, dtype=torch.int32)
    g = CSRGraph(rowptr, torch.roll(torch.arange(N, dtype=torch.int32), 1), None, None, N, N)
    g.symmetric = True
    return g


def test_bindings_check_before_the_engine_is_reached(monkeypatch):
    monkeypatch.setattr(S, "_require_hip", lambda t, name: None)
    monkeypatch.setattr(S, "lib", lambda: pytest.fail("the engine was reached"))
    base = _cpu_base(6)
    for gp in ([0, 3, 5], [1, 6], [0, 4, 2, 6], [0]):
        with pytest.raises(ValueError, match="graph_ptr"):
            S.hop_sums(base, torch.tensor(gp))
        with pytest.raises(ValueError, match="graph_ptr"):
            S.graph_clustering_coefficient(base, torch.tensor(gp))
    for nodes in ([-1], [6], [0, 9]):
        with pytest.raises(ValueError, match="outside"):
            S.hop_sums(base, torch.tensor([0, 3, 6]), nodes=torch.tensor(nodes))
    with pytest.raises(ValueError, match="empty"):
        S.graph_path_len(base, torch.tensor([0, 3, 3, 6]))
    big = _cpu_base(1)
    big.num_nodes = (1 << 16) + 1                                 # (only the sizes are read before the refusal)
    with pytest.raises(_lib.EngineError, match="65536"):
        S.hop_sums(big, nodes=torch.tensor([0]))
    with pytest.raises(ValueError, match="feature_dim"):
        S.node_identity(base)
    directed = _cpu_base(6)
    directed.symmetric = False
    directed.is_symmetric = lambda run=None: False
    for call in (lambda: S.triangles(directed), lambda: S.hop_sums(directed), lambda: S.node_const(directed),
                 lambda: S.raw("graph_path_len", directed)):
        with pytest.raises(ValueError, match="undirected"):
            call()
