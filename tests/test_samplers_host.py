"""Mini-batch subgraph samplers without a device (CPU suite): the NumPy restatements of csrc/sample.hip
(graphgym_amd.samplers.sample_nodes_host / induced_subgraph_host — the oracle of tests/test_samplers_gpu.py) on hand-made
bases against a brute-force dense count matrix, the properties and the distributions of the draws, the argument checks
of the new entry points (every case returns before anything is launched) and the error paths of the Python layer."""
import ctypes as C
import math
import types

import numpy as np
import pytest
import torch

import _sampler_graphs as SG
from graphgym_amd import _lib
from graphgym_amd import samplers as S

INVALID, UNSUPPORTED = 1, 2
FAKE = C.c_void_p(256)        # a non-null pointer that is never dereferenced
BIG = 2 ** 31
NAMES = sorted(SG.CASES)


# ---- induced subgraph ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", NAMES)
def test_induced_subgraph_host_against_dense_counts(name):
    base = SG.build(name)
    A, N = SG.dense_counts(name), base.num_nodes
    rowptr, col = base.rowptr.numpy(), base.col.numpy()
    row = np.repeat(np.arange(N), np.diff(rowptr))
    for nodes in SG.node_sets(N):
        b = S.induced_subgraph_host(base, torch.tensor(nodes, dtype=torch.int64))
        keep = sorted(set(nodes))
        assert b.orig_node.dtype == torch.int64 and b.orig_node.tolist() == keep and b.num_nodes == len(keep)
        g = b.graph
        assert g.num_nodes == len(keep) and g.rowptr.dtype == torch.int32 and g.col.dtype == torch.int32
        rp, c = g.rowptr.numpy(), g.col.numpy()
        assert np.array_equal(SG.csr_to_dense(rp, c, len(keep)), A[np.ix_(keep, keep)])
        for r in range(len(keep)):                                         # ascending inside a row
            assert (np.diff(c[rp[r]:rp[r + 1]]) >= 0).all()
        # base_entry: the base's entry with the right (row, col), ascending (the base's order kept)
        be = b.base_entry.numpy()
        assert (np.diff(be) > 0).all()
        sub_row = np.repeat(np.arange(len(keep)), np.diff(rp))
        assert np.array_equal(row[be], np.asarray(keep, dtype=np.int64)[sub_row])
        assert np.array_equal(col[be], np.asarray(keep, dtype=np.int64)[c])
        # edge_index is the CSR read out in order, eid = arange
        assert b.edge_index.dtype == torch.int64
        assert np.array_equal(b.edge_index[0].numpy(), c) and np.array_equal(b.edge_index[1].numpy(), sub_row)
        assert torch.equal(g.eid, torch.arange(g.nnz, dtype=torch.int32))


@pytest.mark.parametrize("name", NAMES)
def test_the_full_node_set_reproduces_the_base(name):
    base = SG.build(name)
    b = S.induced_subgraph_host(base, torch.arange(base.num_nodes))
    assert torch.equal(b.graph.rowptr, base.rowptr) and torch.equal(b.graph.col, base.col)
    assert torch.equal(b.base_entry, torch.arange(base.nnz, dtype=torch.int32))


def test_induced_subgraph_skips_negative_entries_and_rejects_large_ones():
    base = SG.build("path5")
    b = S.induced_subgraph_host(base, torch.tensor([-1, 3, -1, 2]))
    assert b.orig_node.tolist() == [2, 3] and b.graph.col.tolist() == [1, 0]
    with pytest.raises(ValueError, match="outside"):
        S.induced_subgraph_host(base, torch.tensor([0, 5]))


# ---- the draws: properties ------------------------------------------------------------------------------------------------

def _walk_edges(plan):
    """the (from, to) moves of the plan's walk graph"""
    rowptr, col = plan.host_walk
    row = np.repeat(np.arange(plan.base.num_nodes), np.diff(rowptr))
    return set(zip(row.tolist(), col.tolist()))


@pytest.mark.parametrize("name", NAMES)
def test_every_walk_step_is_a_stored_entry(name):
    base = SG.build(name)
    L = 5
    plan = S.plan_sampler(base, "saint_rw", batch_size=64, walk_length=L)
    moves = _walk_edges(plan)
    rowptr, _ = plan.host_walk
    assert moves == SG.stored(name)                 # walked over out-edges: a move u -> v is the stored edge (src u, dst v)
    for step in range(3):
        w = S.sample_nodes_host(plan, 7, step)
        assert w.dtype == torch.int32 and w.numel() == 64 * (L + 1)
        w = w.view(64, L + 1).tolist()
        for walk in w:
            assert 0 <= walk[0] < base.num_nodes
            for a, b in zip(walk[:-1], walk[1:]):
                if rowptr[a + 1] == rowptr[a]:
                    assert b == a                                           # a node without a move stays
                else:
                    assert (a, b) in moves


def test_the_isolated_node_stays():
    name, v = SG.ISOLATED
    plan = S.plan_sampler(SG.build(name), "saint_rw", batch_size=200, walk_length=3)
    w = S.sample_nodes_host(plan, 1, 0).view(200, 4)
    at = w[:, 0] == v
    assert int(at.sum()) > 0 and bool((w[at] == v).all())
    assert not bool((w[~at] == v).any())


@pytest.mark.parametrize("name", NAMES)
def test_every_saint_edge_draw_is_a_stored_entry(name):
    base = SG.build(name)
    plan = S.plan_sampler(base, "saint_edge", batch_size=100)
    assert plan.walk_length == 1
    moves = _walk_edges(plan)
    for step in range(3):
        pairs = S.sample_nodes_host(plan, 3, step).view(100, 2).tolist()
        assert all((a, b) in moves for a, b in pairs)


@pytest.mark.parametrize("name", NAMES)
def test_saint_node_draws_rows_that_hold_an_entry(name):
    base = SG.build(name)
    deg = np.diff(base.rowptr.numpy())
    plan = S.plan_sampler(base, "saint_node", batch_size=100)
    v = S.sample_nodes_host(plan, 3, 0)
    assert v.dtype == torch.int32 and v.numel() == 100
    assert (deg[v.numpy()] > 0).all()


@pytest.mark.parametrize("name", ["ring33", "star200", "cycle6_chord"])
def test_random_node_batches_partition_the_nodes_and_differ_between_epochs(name):
    base = SG.build(name)
    N, P = base.num_nodes, 4
    plan = S.plan_sampler(base, "random_node", num_parts=P)
    epochs = []
    for e in range(5):
        parts = [S.sample_nodes_host(plan, 11, e * P + p).tolist() for p in range(P)]
        assert all(p == sorted(p) for p in parts)
        assert sorted(sum(parts, [])) == list(range(N))                     # a partition
        epochs.append(parts)
    assert all(epochs[a] != epochs[b] for a in range(5) for b in range(a))


@pytest.mark.parametrize("kind", S.KINDS)
def test_the_same_seed_and_step_give_the_same_batch(kind):
    base = SG.build("ring65")
    plan = S.plan_sampler(base, kind, batch_size=12, walk_length=2, num_parts=3)
    a, b = S.sample_batch(plan, 5, 4), S.sample_batch(plan, 5, 4)
    assert torch.equal(a.orig_node, b.orig_node) and torch.equal(a.graph.col, b.graph.col)
    assert torch.equal(a.graph.rowptr, b.graph.rowptr) and torch.equal(a.base_entry, b.base_entry)
    other_step, other_seed = S.sample_batch(plan, 5, 5), S.sample_batch(plan, 6, 4)
    assert not torch.equal(a.orig_node, other_step.orig_node)
    assert not torch.equal(a.orig_node, other_seed.orig_node)
    assert torch.equal(S.sample_nodes(plan, 5, 4), S.sample_nodes_host(plan, 5, 4))     # a CPU base: the restatement


# ---- the draws: distributions ------------------------------------------------------------------------------------------------

def _chi2(freq, expected):
    return sum((f - e) ** 2 / e for f, e in zip(freq, expected))


def _bound(df):
    """df + 6 sqrt(2 df): the chi-square statistic of a correct sampler has mean df and variance 2 df"""
    return df + 6 * math.sqrt(2 * df)


def test_saint_node_frequencies_follow_the_in_degree():
    """triangle + pendant + isolated node: in-degrees 2, 2, 3, 1, 0 of 8 entries.  4000 draws (40 steps of 100): the
    smallest expected count is 500 (node 3); node 4 is never drawn.  df = 3.  A failure means the key mixing is too
    weak, not that the bound is wrong."""
    base = SG.build("triangle_pendant_isolated")
    deg = np.diff(base.rowptr.numpy())
    plan = S.plan_sampler(base, "saint_node", batch_size=100)
    freq = np.zeros(5, dtype=np.int64)
    for step in range(40):
        freq += np.bincount(S.sample_nodes_host(plan, 2, step).numpy(), minlength=5)
    assert freq[4] == 0
    expected = 4000 * deg[:4] / deg.sum()
    assert expected.min() >= 20
    x = _chi2(freq[:4], expected)
    print(f"saint_node chi2 {x:.2f}, df 3, bound {_bound(3):.2f}, counts {freq.tolist()}")
    assert x <= _bound(3)


def test_saint_edge_frequencies_follow_the_inverse_degrees():
    """the same base: n' = 4 rows hold an entry, the unordered edges {0,1}, {0,2}, {1,2}, {2,3} have probability
    (1 / n') (1 / deg u + 1 / deg v) = 6/24, 5/24, 5/24, 8/24.  4800 draws: the smallest expected count is 1000.  df = 3."""
    base = SG.build("triangle_pendant_isolated")
    deg = np.diff(base.rowptr.numpy()).astype(float)
    plan = S.plan_sampler(base, "saint_edge", batch_size=120)
    cells = [(0, 1), (0, 2), (1, 2), (2, 3)]
    freq = dict.fromkeys(cells, 0)
    for step in range(40):
        for a, b in S.sample_nodes_host(plan, 9, step).view(120, 2).tolist():
            freq[(min(a, b), max(a, b))] += 1
    expected = [4800 * (1 / 4) * (1 / deg[u] + 1 / deg[v]) for u, v in cells]
    assert abs(sum(expected) - 4800) < 1e-6 and min(expected) >= 20
    x = _chi2([freq[c] for c in cells], expected)
    print(f"saint_edge chi2 {x:.2f}, df 3, bound {_bound(3):.2f}, counts {[freq[c] for c in cells]}")
    assert x <= _bound(3)


def test_a_walk_step_is_uniform_over_the_neighbours():
    """the star: a walk that stands on the hub (node 0) after step 1 moves to one of the 200 leaves at step 2, uniformly.
    8 steps of 1000 walks, of which the ~995 rooted in a leaf qualify: ~39.8 expected per leaf.  df = 199."""
    base = SG.build("star200")
    plan = S.plan_sampler(base, "saint_rw", batch_size=1000, walk_length=2)
    freq = np.zeros(201, dtype=np.int64)
    for step in range(8):
        w = S.sample_nodes_host(plan, 4, step).view(1000, 3).numpy()
        on_hub = w[:, 1] == 0
        freq += np.bincount(w[on_hub, 2], minlength=201)
    assert freq[0] == 0
    total = int(freq.sum())
    expected = [total / 200] * 200
    assert expected[0] >= 20
    x = _chi2(freq[1:], expected)
    print(f"walk step chi2 {x:.1f}, df 199, bound {_bound(199):.1f}, draws {total}")
    assert x <= _bound(199)


def test_the_part_of_a_node_is_uniform():
    """random_node with 4 parts: the part of node 7 of ring33 over 400 epochs, 100 expected per part.  df = 3."""
    base = SG.build("ring33")
    P = 4
    plan = S.plan_sampler(base, "random_node", num_parts=P)
    freq = [0] * P
    for e in range(400):
        for p in range(P):
            if 7 in S.sample_nodes_host(plan, 13, e * P + p).tolist():
                freq[p] += 1
    assert sum(freq) == 400
    x = _chi2(freq, [100.0] * P)
    print(f"random_node chi2 {x:.2f}, df 3, bound {_bound(3):.2f}, counts {freq}")
    assert x <= _bound(3)


# ---- errors -----------------------------------------------------------------------------------------------------------------

def test_plan_sampler_rejects_bad_arguments():
    base = SG.build("path5")
    with pytest.raises(ValueError, match="kind"):
        S.plan_sampler(base, "saint_walk", batch_size=4)
    for kind in ("saint_node", "saint_edge", "saint_rw"):
        with pytest.raises(ValueError, match="batch_size"):
            S.plan_sampler(base, kind, batch_size=0)
        with pytest.raises(ValueError, match="batch_size"):
            S.plan_sampler(base, kind)
    with pytest.raises(ValueError, match="train_parts"):
        S.plan_sampler(base, "random_node")
    with pytest.raises(ValueError, match="num_parts"):
        S.plan_sampler(base, "random_node", num_parts=0)
    from graphgym_amd.link_pred import host_csr
    empty = host_csr(torch.zeros(2, 0, dtype=torch.int64), 4)
    for kind in ("saint_node", "saint_edge", "saint_rw"):
        with pytest.raises(ValueError, match="stored entry"):
            S.plan_sampler(empty, kind, batch_size=4)
    parts = [S.sample_batch(S.plan_sampler(empty, "random_node", num_parts=2), 0, p) for p in range(2)]
    assert sum(b.num_nodes for b in parts) == 4 and all(b.graph.nnz == 0 for b in parts)


def _cfg(sampler, val="full_batch", **train):
    return types.SimpleNamespace(train=types.SimpleNamespace(sampler=sampler, batch_size=8, walk_length=2,
                                                             iter_per_epoch=5, **train),
                                 val=types.SimpleNamespace(sampler=val))


def test_loader_from_cfg_names_what_is_not_built():
    base = SG.build("ring33")
    x, y, mask = torch.ones(33, 2), torch.zeros(33, dtype=torch.int64), torch.arange(33) % 2 == 0
    with pytest.raises(NotImplementedError, match="bipartite"):
        S.loader_from_cfg(_cfg("neighbor"), base, x, y, mask, "train")
    with pytest.raises(NotImplementedError, match="METIS"):
        S.loader_from_cfg(_cfg("cluster"), base, x, y, mask, "train")
    with pytest.raises(NotImplementedError, match="bogus sampler is not implemented!"):
        S.loader_from_cfg(_cfg("bogus"), base, x, y, mask, "train")
    with pytest.raises(NotImplementedError, match="bogus sampler is not implemented!"):
        S.loader_from_cfg(_cfg("saint_rw", val="bogus"), base, x, y, mask, "val")
    with pytest.raises(ValueError, match="train_parts"):
        S.loader_from_cfg(_cfg("random_node"), base, x, y, mask, "train")
    assert len(S.loader_from_cfg(_cfg("random_node", train_parts=3), base, x, y, mask, "train")) == 3
    assert len(S.loader_from_cfg(_cfg("saint_edge"), base, x, y, mask, "train")) == 5
    full = S.loader_from_cfg(_cfg("saint_rw"), base, x, y, mask, "val")
    assert len(full) == 1
    only = list(full)[0]
    assert only.node_feature is x and only.node_label is y
    assert only.node_label_index.tolist() == list(range(0, 33, 2))


def test_loader_batches_on_a_cpu_base():
    """epoch e, batch i is step e * len + i; features, labels and the split follow orig_node"""
    base = SG.build("ring65")
    x = torch.arange(65, dtype=torch.float32)[:, None] * torch.ones(1, 3)
    y = torch.arange(65) % 7
    mask = torch.arange(65) % 3 == 0
    loader = S.loader_from_cfg(_cfg("saint_rw"), base, x, y, mask, "train", seed=21)
    for epoch in range(2):
        got = list(loader)
        assert len(got) == 5
        for i, b in enumerate(got):
            want = S.sample_batch(loader.plan, 21, epoch * 5 + i)
            assert torch.equal(b.orig_node, want.orig_node) and torch.equal(b.edge_index, want.edge_index)
            assert torch.equal(b.node_feature[:, 0].long(), b.orig_node) and torch.equal(b.node_label, b.orig_node % 7)
            assert torch.equal(b.orig_node[b.node_label_index], b.orig_node[b.orig_node % 3 == 0])
    by_index = S.SubgraphLoader(base, x, y, torch.nonzero(mask).view(-1), loader.plan, 21, 5)
    assert torch.equal(list(by_index)[2].node_label_index, S.SubgraphLoader(base, x, y, mask, loader.plan, 21, 5)
                       .batch(2).node_label_index)


def test_config_defaults():
    from graphgym_amd.config import _defaults
    cfg = _defaults()
    assert cfg.train.sampler == "full_batch" and cfg.val.sampler == "full_batch"
    assert cfg.train.iter_per_epoch == 32 and cfg.train.walk_length == 4
    assert cfg.train.neighbor_sizes == [20, 15, 10, 5] and cfg.train.batch_size == 16
    assert not hasattr(cfg.train, "train_parts")


# ---- the entry points' argument checks (no launch) -----------------------------------------------------------------------

def test_prototypes_exist():
    for name in ("mp_sample_parts", "mp_sample_entry_rows", "mp_sample_walks", "mp_bitmap_mark", "mp_bitmap_word_counts",
                 "mp_bitmap_nodes", "mp_induced_count", "mp_induced_fill"):
        assert name in _lib.PROTOTYPES and hasattr(_lib.lib(), name)


def test_draw_entry_points_reject_bad_arguments_before_any_launch():
    L = _lib.lib()
    assert L.mp_sample_parts(10, 0, 1, 0, FAKE, None) == INVALID
    assert L.mp_sample_parts(-1, 2, 1, 0, FAKE, None) == INVALID
    assert L.mp_sample_parts(10, 2, 1, 0, None, None) == INVALID
    assert L.mp_sample_parts(BIG, 2, 1, 0, FAKE, None) == UNSUPPORTED
    assert L.mp_sample_parts(0, 2, 1, 0, None, None) == 0
    assert L.mp_sample_entry_rows(None, 10, 20, 5, 1, 0, FAKE, None) == INVALID
    assert L.mp_sample_entry_rows(FAKE, 10, 20, 5, 1, 0, None, None) == INVALID
    assert L.mp_sample_entry_rows(FAKE, 10, 0, 5, 1, 0, FAKE, None) == INVALID          # nnz == 0
    assert L.mp_sample_entry_rows(FAKE, 10, 20, -1, 1, 0, FAKE, None) == INVALID
    assert L.mp_sample_entry_rows(FAKE, 10, BIG, 5, 1, 0, FAKE, None) == UNSUPPORTED
    assert L.mp_sample_entry_rows(FAKE, 10, 20, 0, 1, 0, None, None) == 0
    assert L.mp_sample_walks(None, FAKE, 10, 20, None, 0, 5, 2, 1, 0, FAKE, None) == INVALID
    assert L.mp_sample_walks(FAKE, None, 10, 20, None, 0, 5, 2, 1, 0, FAKE, None) == INVALID
    assert L.mp_sample_walks(FAKE, FAKE, 10, 20, None, 0, 5, 2, 1, 0, None, None) == INVALID
    assert L.mp_sample_walks(FAKE, FAKE, 10, 20, FAKE, 0, 5, 2, 1, 0, FAKE, None) == INVALID   # an empty pool
    assert L.mp_sample_walks(FAKE, FAKE, 10, 20, None, 0, 5, -1, 1, 0, FAKE, None) == INVALID
    assert L.mp_sample_walks(FAKE, FAKE, 0, 0, None, 0, 5, 2, 1, 0, FAKE, None) == INVALID
    assert L.mp_sample_walks(FAKE, FAKE, BIG, 20, None, 0, 5, 2, 1, 0, FAKE, None) == UNSUPPORTED
    assert L.mp_sample_walks(FAKE, FAKE, 10, 20, None, 0, 0, 2, 1, 0, None, None) == 0


def test_bitmap_and_induced_entry_points_reject_bad_arguments_before_any_launch():
    L = _lib.lib()
    assert L.mp_bitmap_mark(None, 5, 10, FAKE, FAKE, None) == INVALID
    assert L.mp_bitmap_mark(FAKE, 5, 10, None, FAKE, None) == INVALID
    assert L.mp_bitmap_mark(FAKE, 5, 10, FAKE, None, None) == INVALID
    assert L.mp_bitmap_mark(FAKE, -1, 10, FAKE, FAKE, None) == INVALID
    assert L.mp_bitmap_mark(FAKE, 5, BIG, FAKE, FAKE, None) == UNSUPPORTED
    assert L.mp_bitmap_mark(None, 0, 10, FAKE, FAKE, None) == 0
    assert L.mp_bitmap_word_counts(None, 4, FAKE, None) == INVALID
    assert L.mp_bitmap_word_counts(FAKE, 4, None, None) == INVALID
    assert L.mp_bitmap_word_counts(FAKE, -1, FAKE, None) == INVALID
    assert L.mp_bitmap_word_counts(None, 0, None, None) == 0
    assert L.mp_bitmap_nodes(None, FAKE, 4, FAKE, None) == INVALID
    assert L.mp_bitmap_nodes(FAKE, None, 4, FAKE, None) == INVALID
    assert L.mp_bitmap_nodes(FAKE, FAKE, 4, None, None) == INVALID
    assert L.mp_bitmap_nodes(None, None, 0, None, None) == 0
    ok = dict(rowptr=FAKE, col=FAKE, N=10, nnz=20, orig=FAKE, n_sub=4, bitmap=FAKE)

    def count(cnt=FAKE, **kw):
        a = dict(ok, **kw)
        return L.mp_induced_count(a["rowptr"], a["col"], a["N"], a["nnz"], a["orig"], a["n_sub"], a["bitmap"], cnt, None)

    def fill(rank=FAKE, rp=FAKE, cs=FAKE, be=FAKE, **kw):
        a = dict(ok, **kw)
        return L.mp_induced_fill(a["rowptr"], a["col"], a["N"], a["nnz"], a["orig"], a["n_sub"], a["bitmap"], rank, rp,
                                 cs, be, None)

    for f in (count, fill):
        assert f(rowptr=None) == INVALID and f(col=None) == INVALID and f(orig=None) == INVALID
        assert f(bitmap=None) == INVALID and f(n_sub=-1) == INVALID and f(n_sub=11) == INVALID
        assert f(N=BIG) == UNSUPPORTED and f(nnz=BIG) == UNSUPPORTED
        assert f(n_sub=0, orig=None, bitmap=None) == 0
    assert count(cnt=None) == INVALID
    assert fill(rank=None) == INVALID and fill(rp=None) == INVALID and fill(cs=None) == INVALID
    assert fill(be=None) == INVALID
