"""Graph-task loaders without a device (CPU suite): the host integers of graphgym_amd.graph_loader — the keyed shuffle,
the inductive split, collate_host (the oracle of tests/test_graph_loader_gpu.py) against a per-graph loop written here
(tests/_graph_sets.loop_collate), the loaders on a CPU dataset, the golden config, the errors, and the argument checks of
the new entry points (every case returns before anything is launched)."""
import ctypes as C
import os
import types

import numpy as np
import pytest
import torch

import _graph_sets as GS
from graphgym_amd import _lib, config
from graphgym_amd import graph_loader as GL
from graphgym_amd.link_pred import host_csr

INVALID, UNSUPPORTED = 1, 2
FAKE = C.c_void_p(256)        # a non-null pointer that is never dereferenced
BIG = 2 ** 31
GOLDEN_CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cfg_idgnn_graph.yaml")


# ---- shuffle and split -------------------------------------------------------------------------------------------------

def test_epoch_order_is_a_keyed_permutation():
    ids = np.arange(100, 150)
    a, b = GL.epoch_order(ids, 3, 0), GL.epoch_order(ids, 3, 0)
    assert a.dtype == np.int64 and sorted(a.tolist()) == ids.tolist()
    assert np.array_equal(a, b)
    assert not np.array_equal(a, GL.epoch_order(ids, 3, 1))
    assert not np.array_equal(a, GL.epoch_order(ids, 4, 0))
    assert not np.array_equal(a, ids)
    rep = GL.epoch_order([5, 5, 2], 0, 0)
    assert sorted(rep.tolist()) == [2, 5, 5]
    assert GL.epoch_order(torch.tensor([9]), 0, 0).tolist() == [9]


@pytest.mark.parametrize("G,ratios,sizes", [
    (10, [0.8, 0.2], [8, 2]), (11, [0.8, 0.2], [8, 3]), (37, [0.8, 0.2], [29, 8]),
    (10, [0.8, 0.1, 0.1], [8, 1, 1]), (11, [0.8, 0.1, 0.1], [8, 1, 2]), (37, [0.8, 0.1, 0.1], [29, 4, 4])])
def test_split_graphs_sizes_and_cover(G, ratios, sizes):
    """cuts at floor(cumulative ratio * G): 0.8 * 37 = 29.6 -> 29, 0.9 * 37 = 33.3 -> 33, 0.9 * 11 = 9.9 -> 9"""
    parts = GL.split_graphs(G, ratios, seed=5)
    assert [p.size for p in parts] == sizes
    assert sorted(np.concatenate(parts).tolist()) == list(range(G))            # disjoint and covering
    again = GL.split_graphs(G, ratios, seed=5)
    assert all(np.array_equal(p, q) for p, q in zip(parts, again))
    plain = GL.split_graphs(G, ratios, seed=5, shuffle=False)
    assert np.concatenate(plain).tolist() == list(range(G)) and [p.size for p in plain] == sizes
    if G == 37:
        assert np.concatenate(parts).tolist() != list(range(G))
        other = GL.split_graphs(G, ratios, seed=6)
        assert any(not np.array_equal(p, q) for p, q in zip(parts, other))


# ---- collate_host against the loop oracle ---------------------------------------------------------------------------------

def _check_against_loop(graphs, ds, ids, what):
    b, want = GL.collate_host(ds, ids), GS.loop_collate(graphs, ids)
    n = want["num_nodes"]
    assert b.num_nodes == n and b.num_graphs == len(ids), what
    for k in ("edge_index", "node_feature", "edge_feature", "batch", "orig_node", "graph_label"):
        got = getattr(b, k)
        assert got.dtype == want[k].dtype and torch.equal(got, want[k]), (what, k)
    ref = host_csr(want["edge_index"], n)             # (already in CSR order: the stable sort keeps it)
    assert torch.equal(ref.eid, torch.arange(ref.nnz, dtype=torch.int32)), what
    g = b.graph
    assert (g.num_nodes, g.nnz) == (n, ref.nnz) and g.rowptr.dtype == torch.int32 and g.col.dtype == torch.int32
    assert torch.equal(g.rowptr, ref.rowptr) and torch.equal(g.col, ref.col) and torch.equal(g.eid, ref.eid), what
    assert torch.equal(g.row_ids().long(), want["edge_index"][1]), what
    # base_entry: the base's entry of the same graph, row and column
    base, be = ds.base, b.base_entry.long()
    rows = torch.repeat_interleave(torch.arange(base.num_nodes), (base.rowptr[1:] - base.rowptr[:-1]).long())
    assert torch.equal(rows[be], b.orig_node[want["edge_index"][1]]), what
    assert torch.equal(base.col[be].long(), b.orig_node[want["edge_index"][0]]), what
    assert torch.equal(b.edge_feature, ds.edge_feature[base.eid[be].long()]), what
    p = b.pool_operator
    assert (p.num_nodes, p.num_cols, p.nnz) == (len(ids), n, n), what
    assert torch.equal(p.rowptr, want["node_off"]) and torch.equal(p.col, torch.arange(n, dtype=torch.int32)), what


@pytest.mark.parametrize("kind", ["symmetric", "directed", "multi"])
@pytest.mark.parametrize("case", sorted(GS.IDS12))
def test_collate_host_against_a_per_graph_loop(kind, case):
    graphs = GS.make_graphs(GS.SIZES12, kind, seed=1)
    ds = GL.GraphDataset.from_graphs(graphs)
    assert ds.num_graphs == 12 and not ds.on_device
    assert ds.seedable == (kind == "symmetric") and ds.symmetric == (kind == "symmetric")
    if kind != "multi":
        assert all(graphs[i][0].numel() == 0 for i in GS.EDGELESS)
    _check_against_loop(graphs, ds, GS.IDS12[case], f"{kind}/{case}")


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.int64])
def test_collate_host_other_feature_types(dtype):
    graphs = GS.make_graphs(GS.SIZES12, seed=2, dtype=dtype)
    ds = GL.GraphDataset.from_graphs(graphs)
    _check_against_loop(graphs, ds, GS.IDS12["all_shuffled"], str(dtype))
    assert GL.collate_host(ds, [4]).node_feature.dtype == dtype


def test_collate_rejects_bad_ids():
    ds = GL.GraphDataset.from_graphs(GS.make_graphs(GS.SIZES12))
    for bad in ([], [12], [-1, 2]):
        with pytest.raises(ValueError):
            GL.collate_host(ds, bad)


# ---- errors ----------------------------------------------------------------------------------------------------------------

def test_dataset_rejects_a_bad_graph_ptr_and_crossing_entries():
    ei = torch.tensor([[0, 1, 2, 3], [1, 0, 3, 2]])
    base = host_csr(ei, 5)
    x, y = torch.zeros(5, 2), torch.zeros(2, dtype=torch.int64)
    GL.GraphDataset(base, [0, 2, 5], x, y)
    with pytest.raises(ValueError, match="end at"):
        GL.GraphDataset(base, [0, 2, 4], x, y)
    with pytest.raises(ValueError, match="start at 0"):
        GL.GraphDataset(base, [1, 2, 5], x, y)
    with pytest.raises(ValueError, match="decrease"):
        GL.GraphDataset(base, [0, 3, 2, 5], x, torch.zeros(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="one row per node"):
        GL.GraphDataset(base, [0, 2, 5], x[:4], y)
    # entries 2 and 3 of the CSR are (row 2, col 3) and (row 3, col 2); with graphs {0, 1, 2} and {3, 4} both cross
    with pytest.raises(ValueError, match=r"stored entry 2 \(row 2, column 3\) joins graph 0 and graph 1"):
        GL.GraphDataset(base, [0, 3, 5], x, y)


# ---- the CPU dataset path and the loaders ---------------------------------------------------------------------------------

def test_a_cpu_dataset_takes_the_host_path():
    graphs = GS.make_graphs(GS.SIZES12, seed=3)
    ds = GL.GraphDataset.from_graphs(graphs)
    ids = GS.IDS12["repeated"]
    GS.assert_batches_equal(GL.collate(ds, ids), GL.collate_host(ds, ids), "cpu collate")
    loader = GL.GraphLoader(ds, np.arange(12), 5, shuffle=False)
    got = list(loader)
    assert [b.num_graphs for b in got] == [5, 5, 2]
    GS.assert_batches_equal(got[2], GL.collate_host(ds, [10, 11]), "cpu loader")


def test_graph_loader_covers_the_split_once_per_epoch():
    ds = GL.GraphDataset.from_graphs(GS.make_graphs(GS.SIZES12, seed=3))
    ids = np.array([0, 2, 3, 4, 5, 7, 8, 9, 10, 11, 1])
    loader = GL.GraphLoader(ds, ids, batch_size=4, shuffle=True, seed=9)
    assert len(loader) == 3
    starts = ds.graph_ptr
    epochs = []
    for epoch in range(2):
        got = list(loader)
        assert [b.num_graphs for b in got] == [4, 4, 3]                      # the last batch is short
        seen = []
        for i, b in enumerate(got):
            first = b.orig_node[b.pool_operator.rowptr[:-1].long()]          # the first node of every batch graph
            these = (np.searchsorted(starts, first.numpy(), side="right") - 1).tolist()
            assert these == loader.batch_ids(epoch, i).tolist()
            seen += these
        assert sorted(seen) == sorted(ids.tolist())                           # every id exactly once
        epochs.append(seen)
    assert epochs[0] != epochs[1]
    loader.set_epoch(0)
    assert [b.orig_node.tolist() for b in loader] == [b.orig_node.tolist() for b in
                                                      GL.GraphLoader(ds, ids, 4, True, seed=9)]
    plain = GL.GraphLoader(ds, ids, 4, shuffle=False)
    assert np.concatenate([plain.batch_ids(7, i) for i in range(3)]).tolist() == ids.tolist()
    assert len(GL.GraphLoader(ds, ids[:8], 4, False)) == 2 and len(GL.GraphLoader(ds, ids[:1], 4, False)) == 1
    with pytest.raises(ValueError, match="transform"):
        GL.GraphLoader(ds, ids, 4, False, transform="line_graph")
    with pytest.raises(ValueError, match="radius"):
        GL.GraphLoader(ds, ids, 4, False, transform="ego")
    with pytest.raises(ValueError, match="batch_size"):
        GL.GraphLoader(ds, ids, 0, False)


def test_graph_loaders_from_the_golden_config():
    cfg = config.load_cfg(GOLDEN_CFG, target=config._defaults())
    assert cfg.dataset.task == "graph" and cfg.dataset.split == [0.8, 0.2] and cfg.dataset.transform == "ego"
    assert cfg.train.batch_size == 64 and cfg.gnn.layers_mp == 3 and cfg.dataset.augment_label == "graph_path_len"
    ds = GL.GraphDataset.from_graphs(GS.make_graphs([4] * 37, seed=4))
    two = GL.graph_loaders_from_cfg(cfg, ds, seed=1)
    assert [ld.ids.size for ld in two] == [29, 8] and [ld.shuffle for ld in two] == [True, False]
    assert all(ld.transform == "ego" and ld.radius == 3 and ld.batch_size == 64 for ld in two)
    assert sorted(np.concatenate([ld.ids for ld in two]).tolist()) == list(range(37))
    cfg.dataset.split, cfg.dataset.transform, cfg.train.batch_size = [0.8, 0.1, 0.1], "none", 16
    three = GL.graph_loaders_from_cfg(cfg, ds, seed=1)
    assert [ld.ids.size for ld in three] == [29, 4, 4] and [ld.shuffle for ld in three] == [True, False, False]
    assert all(ld.transform is None and ld.radius is None for ld in three) and [len(ld) for ld in three] == [2, 1, 1]
    cfg.dataset.shuffle_split = False
    assert np.concatenate([ld.ids for ld in GL.graph_loaders_from_cfg(cfg, ds)]).tolist() == list(range(37))
    assert [b.num_graphs for b in three[0]] == [16, 13]                        # a CPU dataset: the host path


def test_graph_head_hands_the_pool_operator_to_the_pooling_function():
    """harness.GNNGraphHead passes batch.pool_operator on, and None for a batch without one"""
    from graphgym_amd import harness as H
    head = H.GNNGraphHead.__new__(H.GNNGraphHead)
    torch.nn.Module.__init__(head)
    calls = []
    head.pooling_fun = lambda x, batch, id=None, size=None, operator=None: calls.append((id, operator)) or x[:2]
    head.layer_post_mp = torch.nn.Identity()
    x, owner = torch.ones(4, 3), torch.tensor([0, 0, 1, 1])
    marker = object()
    head(types.SimpleNamespace(node_feature=x, batch=owner, graph_label=torch.zeros(2), pool_operator=marker))
    head(types.SimpleNamespace(node_feature=x, batch=owner, graph_label=torch.zeros(2)))
    assert calls == [(None, marker), (None, None)]


# ---- the entry points' argument checks (no launch) -----------------------------------------------------------------------

def test_prototypes_exist():
    for name in ("mp_collate_graphs", "mp_collate_check_entries", "mp_collate_stage_cap"):
        assert name in _lib.PROTOTYPES and hasattr(_lib.lib(), name)
    assert _lib.lib().mp_collate_stage_cap() == 1024


def test_collate_entry_points_reject_bad_arguments_before_any_launch():
    L = _lib.lib()
    ok = dict(rowptr=FAKE, col=FAKE, val=None, N=10, nnz_base=20, graph_ptr=FAKE, G=3, ids=FAKE, node_off=FAKE,
              entry_off=FAKE, B=2, n=6, nnz=8, rowptr_out=FAKE, owner=FAKE, owner32=FAKE, orig_node=FAKE, col_out=FAKE,
              row_out=FAKE, base_entry=FAKE, edge_index=FAKE, val_out=None)

    def run(**kw):
        a = dict(ok, **kw)
        return L.mp_collate_graphs(*[a[k] for k in ok], None)

    for k in ("rowptr", "col", "graph_ptr", "ids", "node_off", "entry_off", "rowptr_out", "owner", "owner32", "orig_node",
              "col_out", "row_out", "base_entry", "edge_index"):
        assert run(**{k: None}) == INVALID, k
    assert run(val_out=FAKE) == INVALID                                       # values asked of a base without any
    for k in ("N", "nnz_base", "G", "B", "n", "nnz"):
        assert run(**{k: -1}) == INVALID, k
        assert run(**{k: BIG}) == UNSUPPORTED, k
        assert run(**{k: BIG - 1}) == UNSUPPORTED, k
    assert run(G=0) == INVALID and run(N=0) == INVALID and run(nnz_base=0) == INVALID
    assert run(B=0, ids=None, node_off=None, entry_off=None) == 0
    assert run(n=0, nnz=0, rowptr_out=None, owner=None) == 0
    check = dict(col=FAKE, row_of=FAKE, nnz=5, graph_ptr=FAKE, G=2, first_bad=FAKE)

    def run_check(**kw):
        a = dict(check, **kw)
        return L.mp_collate_check_entries(*[a[k] for k in check], None)

    for k in ("col", "row_of", "graph_ptr", "first_bad"):
        assert run_check(**{k: None}) == INVALID, k
    assert run_check(nnz=-1) == INVALID and run_check(G=-1) == INVALID and run_check(G=0) == INVALID
    assert run_check(nnz=BIG) == UNSUPPORTED and run_check(G=BIG) == UNSUPPORTED
    assert run_check(nnz=0, col=None, row_of=None) == 0
