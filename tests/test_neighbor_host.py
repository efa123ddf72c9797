"""The neighbour sampler, host side (no device): the structure of a batch on the host restatement (row lengths, entries,
relabelling, hops), the whole-row case against a NumPy BFS, the seed permutation of an epoch, determinism and the
independence of a node's sample from the rest of the batch, the marginals of the keyed draw, the refusals, the closure
of include/mp_neighbor.h over the library's exports with the argument checks of its entries before anything is
launched (mirroring tests/test_spline_host.py), and samplers.loader_from_cfg's new name."""
import ctypes as C
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import _sampler_graphs as SG
from graphgym_amd import neighbor as NB

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mp_neighbor.h")
INVALID, UNSUPPORTED = 1, 2
FAKE = C.c_void_p(256)        # a non-null pointer that is never dereferenced
BIG = 2 ** 31 - 1
SIZES = ([1], [2, 2], [-1, 1], [3, -1, 2], [20, 15, 10, 5])
ENTRIES = ["mp_nbr_count", "mp_nbr_fill", "mp_nbr_mark", "mp_nbr_seeds"]


def host(name):
    base = SG.build(name)
    return base, base.rowptr.numpy().astype(np.int64), base.col.numpy().astype(np.int64)


def seed_sets(name):
    """one node, the isolated node (where the case has one), all nodes, a seed with one of its in-neighbours, and a list
    with a repeat"""
    _, rowptr, col = host(name)
    N = rowptr.size - 1
    v = int(np.argmax(np.diff(rowptr) > 0))
    sets = [[N // 2], list(range(N)), [v, int(col[rowptr[v]])], [N - 1, 0, N - 1]]
    if name == SG.ISOLATED[0]:
        sets.append([SG.ISOLATED[1]])
    return sets


def bfs_hops(rowptr, col, sources, n, limit=None):
    """distance of every node from `sources` following entries from row to column; -1 where there is no path (or none
    within `limit` steps)"""
    dist = np.full(n, -1, dtype=np.int64)
    dist[sources] = 0
    frontier, d = np.unique(sources), 0
    while frontier.size and (limit is None or d < limit):
        nxt = np.unique(np.concatenate([col[rowptr[v]:rowptr[v + 1]] for v in frontier]))
        frontier = nxt[dist[nxt] < 0]
        d += 1
        dist[frontier] = d
    return dist


def check_batch(b, rowptr, col, sizes, seeds):
    """every structural property of the issue's list, for one batch"""
    L, n = len(sizes), b.num_nodes
    orig, hop = b.orig_node.numpy(), b.hop.numpy().astype(np.int64)
    rp, cs = b.graph.rowptr.numpy().astype(np.int64), b.graph.col.numpy().astype(np.int64)
    entry = b.base_entry.numpy().astype(np.int64)
    assert n == orig.size == hop.size == rp.size - 1 and b.graph.num_nodes == n and b.graph.nnz == entry.size == rp[-1]
    assert (np.diff(orig) > 0).all() and b.graph.symmetric is False
    assert torch.equal(b.graph.eid, torch.arange(entry.size, dtype=torch.int32))
    assert np.array_equal(orig[b.seed_index.numpy()], np.unique(seeds)) and (hop[b.seed_index.numpy()] == 0).all()
    assert (hop == 0).sum() == np.unique(seeds).size and hop.min() >= 0 and hop.max() <= L
    new_id = {int(v): k for k, v in enumerate(orig)}
    for k in range(n):
        v, e = orig[k], entry[rp[k]:rp[k + 1]]
        if hop[k] == L:
            assert e.size == 0
            continue
        deg, s = rowptr[v + 1] - rowptr[v], sizes[hop[k]]
        assert e.size == (deg if s < 0 else min(deg, s))
        assert (np.diff(e) > 0).all() and (e >= rowptr[v]).all() and (e < rowptr[v + 1]).all()
        assert [new_id[int(c)] for c in col[e]] == cs[rp[k]:rp[k + 1]].tolist()
    assert np.array_equal(b.edge_index[0].numpy(), cs)
    assert np.array_equal(b.edge_index[1].numpy(), np.repeat(np.arange(n), np.diff(rp)))
    assert np.array_equal(hop, bfs_hops(rp, cs, b.seed_index.numpy(), n))
    named = np.full(n, L + 1)                          # the lowest hop of a row that names the node
    np.minimum.at(named, cs, np.repeat(hop, np.diff(rp)))
    assert (named[hop > 0] == hop[hop > 0] - 1).all()


@pytest.mark.parametrize("name", sorted(SG.CASES))
def test_the_structure_of_a_batch(name):
    base, rowptr, col = host(name)
    for sizes in SIZES:
        plan = NB.plan_neighbor(base, sizes, 3)
        for seeds in seed_sets(name):
            check_batch(NB.neighbor_batch_nodes(plan, torch.tensor(seeds), 11, 2), rowptr, col, sizes, seeds)
        for step in (0, plan.num_batches - 1):
            check_batch(NB.neighbor_batch(plan, 11, step), rowptr, col, sizes, NB.seeds_host(plan, 11, step).numpy())


@pytest.mark.parametrize("name", sorted(SG.CASES))
def test_whole_rows_give_the_in_ball_of_the_seeds(name):
    base, rowptr, col = host(name)
    N = base.num_nodes
    for L in (1, 2, 3):
        plan = NB.plan_neighbor(base, [-1] * L, 2)
        for seeds in seed_sets(name):
            b = NB.neighbor_batch_nodes(plan, torch.tensor(seeds), 3, 0)
            dist = bfs_hops(rowptr, col, np.array(seeds), N, limit=L)
            assert np.array_equal(b.orig_node.numpy(), np.nonzero(dist >= 0)[0])
            assert np.array_equal(b.hop.numpy(), dist[dist >= 0])
            rp, entry = b.graph.rowptr.numpy(), b.base_entry.numpy()
            for k, v in enumerate(b.orig_node.numpy()):
                want = np.arange(rowptr[v], rowptr[v + 1]) if dist[v] < L else np.zeros(0)
                assert np.array_equal(entry[rp[k]:rp[k + 1]], want)


@pytest.mark.parametrize("n_pool", [1, 31, 32, 33, 65])
def test_an_epoch_of_seeds_is_a_permutation_of_the_pool(n_pool):
    base = SG.build("ring65")
    pool = (np.arange(n_pool) * 7 + 3) % 65                  # distinct (7 and 65 are coprime), not ascending
    for B in (1, 7, n_pool, n_pool + 3):
        plan = NB.plan_neighbor(base, [2], B, torch.from_numpy(pool))
        n = plan.num_batches
        assert n == math.ceil(n_pool / B)
        epochs = []
        for e in range(2):
            got = [NB.seeds_host(plan, 9, e * n + i).numpy() for i in range(n)]
            assert [g.size for g in got[:-1]] == [B] * (n - 1) and got[-1].size == n_pool - B * (n - 1) <= B
            assert sorted(np.concatenate(got).tolist()) == sorted(pool.tolist())
            epochs.append(np.concatenate(got))
        if n_pool > 8:
            assert not np.array_equal(epochs[0], epochs[1])
    all_nodes = NB.plan_neighbor(base, [2], 65)
    assert sorted(NB.seeds_host(all_nodes, 9, 0).tolist()) == list(range(65))


def _same(a, b):
    return all(torch.equal(getattr(a, f), getattr(b, f)) for f in ("orig_node", "edge_index", "base_entry", "hop",
                                                                    "seed_index")) \
        and torch.equal(a.graph.rowptr, b.graph.rowptr) and torch.equal(a.graph.col, b.graph.col)


def test_batches_are_a_function_of_seed_and_step_and_rows_of_nothing_else():
    base, rowptr, col = host("ring65")
    plan = NB.plan_neighbor(base, [2, 2], 8)
    a = NB.neighbor_batch(plan, 5, 3)
    assert _same(a, NB.neighbor_batch(plan, 5, 3))
    assert not _same(a, NB.neighbor_batch(plan, 5, 4)) and not _same(a, NB.neighbor_batch(plan, 6, 3))
    # the same seeds under another step: other rows
    s = NB.seeds_host(plan, 5, 3)
    assert not _same(NB.neighbor_batch_nodes(plan, s, 5, 3), NB.neighbor_batch_nodes(plan, s, 5, 4))
    assert _same(a, NB.neighbor_batch_nodes(plan, s, 5, 3))
    # node v at hop h: the same entries in two batches of one step whose seed sets differ
    x, y = NB.neighbor_batch_nodes(plan, torch.tensor([10, 30]), 5, 7), NB.neighbor_batch_nodes(plan, torch.tensor([10, 50, 51]), 5, 7)
    shared = 0
    for v in set(x.orig_node.tolist()) & set(y.orig_node.tolist()):
        kx, ky = x.orig_node.tolist().index(v), y.orig_node.tolist().index(v)
        if x.hop[kx] == y.hop[ky]:
            ex = x.base_entry[x.graph.rowptr[kx]:x.graph.rowptr[kx + 1]]
            assert torch.equal(ex, y.base_entry[y.graph.rowptr[ky]:y.graph.rowptr[ky + 1]])
            shared += int(x.hop[kx] < 2)
    assert shared >= 3                                            # node 10 and what it drew


def test_the_marginals_of_a_row_are_uniform():
    """6000 steps; every entry of a row of degree 7 under s = 3 and of a row of degree 33 under s = 10 is drawn
    6000 s / deg times within 5 binomial standard deviations.  The draws are keyed: the test is deterministic."""
    from graphgym_amd.link_pred import host_csr
    edges = [(i, 0) for i in range(1, 8)] + [(i, 8) for i in range(9, 42)]
    base = host_csr(torch.tensor(edges).t(), 42)
    rowptr = base.rowptr.numpy().astype(np.int64)
    steps = 6000
    for v, deg, s in ((0, 7, 3), (8, 33, 10)):
        assert rowptr[v + 1] - rowptr[v] == deg
        count = np.zeros(deg, dtype=np.int64)
        for step in range(steps):
            pos = NB.sampled_positions_host(rowptr, v, 0, s, 17, step) - rowptr[v]
            assert pos.size == s and (np.diff(pos) > 0).all()
            count[pos] += 1
        p = s / deg
        sigma = math.sqrt(steps * p * (1 - p))
        worst = float(np.abs(count - steps * p).max() / sigma)
        print(f"deg {deg}, s {s}: worst entry at {worst:.2f} sigma")
        assert worst <= 5.0, (deg, s, count.tolist())


def test_plan_neighbor_rejects_bad_arguments():
    base = SG.build("path5")
    with pytest.raises(ValueError, match="at least one hop"):
        NB.plan_neighbor(base, [], 4)
    for bad in (0, -2, 257):
        with pytest.raises(ValueError, match="size must be"):
            NB.plan_neighbor(base, [3, bad], 4)
    NB.plan_neighbor(base, [256, -1, 1], 4)
    for bad in (0, -1, None):
        with pytest.raises(ValueError, match="batch_size"):
            NB.plan_neighbor(base, [3], bad)
    with pytest.raises(ValueError, match="empty"):
        NB.plan_neighbor(base, [3], 4, torch.zeros(0, dtype=torch.int64))
    with pytest.raises(ValueError, match="empty"):
        NB.plan_neighbor(base, [3], 4, torch.zeros(5, dtype=torch.bool))
    for bad in ([0, 5], [-1, 2]):
        with pytest.raises(ValueError, match="outside"):
            NB.plan_neighbor(base, [3], 4, torch.tensor(bad))
    with pytest.raises(ValueError, match="twice"):
        NB.plan_neighbor(base, [3], 4, torch.tensor([1, 2, 1]))
    for bad in ([5], [-1]):
        with pytest.raises(ValueError, match="outside"):
            NB.neighbor_batch_nodes(NB.plan_neighbor(base, [3], 4), torch.tensor(bad), 0, 0)


# ---- the header's closure -----------------------------------------------------------------------------------------------

def declared_symbols(path=HEADER):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mp_nbr_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound_and_the_reverse():
    from graphgym_amd import _lib, _lib_neighbor
    from graphgym_amd import build as mpbuild
    lib = _lib_neighbor.lib()
    names = declared_symbols()
    assert names == ENTRIES
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mp_neighbor.h but not exported"
        assert n in _lib_neighbor.PROTOTYPES_NEIGHBOR, f"{n} has no ctypes prototype"
    for n in _lib_neighbor.PROTOTYPES_NEIGHBOR:
        assert n.startswith("mp_nbr_") and n in names, f"ctypes binds {n} which mp_neighbor.h does not declare"
        assert getattr(lib, n).argtypes == _lib_neighbor.PROTOTYPES_NEIGHBOR[n][1]
    engine = open(os.path.join(ROOT, "include", "mp_engine.h")).read()
    assert "mp_nbr_" not in engine
    assert not [n for n in _lib.PROTOTYPES if n.startswith("mp_nbr_")]
    assert HEADER in mpbuild.HEADERS and "neighbor.hip" in mpbuild.SOURCES
    assert _lib_neighbor.MAX_FANOUT == 256 and 0 < _lib_neighbor.STREAM < 2 ** 64


def test_every_entry_has_a_poisoning_case():
    """mirrors tests/test_poison_host.py::test_every_c_entry_has_a_case_or_a_reason for include/mp_neighbor.h"""
    import test_poison_neighbor_gpu as P
    from graphgym_amd import _lib_neighbor
    covered = set()
    for case in P.CASES:
        assert case.entries and case.exact and callable(case.run), case.name
        covered |= set(case.entries)
    every = set(declared_symbols())
    assert every == set(_lib_neighbor.PROTOTYPES_NEIGHBOR)
    assert covered >= every and covered - every <= {"mp_bitmap_mark", "mp_bitmap_word_counts", "mp_bitmap_nodes"}


# ---- the C entries, before anything is launched -------------------------------------------------------------------------

def _hop_entry(name, rowptr=FAKE, col=FAKE, N=10, nnz=20, frontier=FAKE, n=5, hop=0, fanout=3, bitmap=FAKE, rank=FAKE,
               out=(FAKE, FAKE, FAKE)):
    from graphgym_amd import _lib_neighbor
    L = _lib_neighbor.lib()
    if name == "mp_nbr_mark":
        return L.mp_nbr_mark(rowptr, col, N, nnz, frontier, n, hop, fanout, 1, 0, bitmap, None)
    if name == "mp_nbr_count":
        return L.mp_nbr_count(rowptr, N, frontier, n, hop, fanout, bitmap, rank, out[0], out[1], None)
    return L.mp_nbr_fill(rowptr, col, N, nnz, frontier, n, hop, fanout, 1, 0, bitmap, rank, out[0], out[1], out[2], None)


@pytest.mark.parametrize("name", ["mp_nbr_mark", "mp_nbr_count", "mp_nbr_fill"])
def test_hop_entries_check_their_arguments_before_any_launch(name):
    for missing in ("rowptr", "frontier", "bitmap"):
        assert _hop_entry(name, **{missing: None}) == INVALID, missing
    if name != "mp_nbr_mark":
        assert _hop_entry(name, rank=None) == INVALID
        assert _hop_entry(name, out=(None, FAKE, FAKE)) == INVALID and _hop_entry(name, out=(FAKE, None, FAKE)) == INVALID
    if name != "mp_nbr_count":
        assert _hop_entry(name, col=None) == INVALID and _hop_entry(name, nnz=-1) == INVALID
        assert _hop_entry(name, nnz=BIG) == UNSUPPORTED and _hop_entry(name, nnz=BIG - 15) == UNSUPPORTED
    if name == "mp_nbr_fill":
        assert _hop_entry(name, out=(FAKE, FAKE, None)) == INVALID
    assert _hop_entry(name, N=-1) == INVALID and _hop_entry(name, n=-1) == INVALID and _hop_entry(name, hop=-1) == INVALID
    assert _hop_entry(name, N=0) == INVALID                                       # a frontier of a graph without nodes
    for fanout in (0, -2, -100):
        assert _hop_entry(name, fanout=fanout) == INVALID
    assert _hop_entry(name, fanout=257) == UNSUPPORTED and _hop_entry(name, fanout=BIG) == UNSUPPORTED
    assert _hop_entry(name, N=BIG) == UNSUPPORTED
    # nothing to do: an empty frontier, no launch (and no pointer but rowptr is looked at)
    assert _hop_entry(name, n=0, frontier=None, bitmap=None, rank=None, out=(None, None, None)) == 0
    assert _hop_entry(name, n=0, fanout=-1) == 0 and _hop_entry(name, n=0, fanout=256) == 0


def test_seeds_entry_checks_its_arguments_before_any_launch():
    from graphgym_amd import _lib_neighbor
    L = _lib_neighbor.lib()
    assert L.mp_nbr_seeds(FAKE, 10, 0, 4, 1, 0, None, None) == INVALID
    assert L.mp_nbr_seeds(FAKE, -1, 0, 0, 1, 0, FAKE, None) == INVALID
    assert L.mp_nbr_seeds(FAKE, 10, -1, 4, 1, 0, FAKE, None) == INVALID
    assert L.mp_nbr_seeds(FAKE, 10, 0, -1, 1, 0, FAKE, None) == INVALID
    assert L.mp_nbr_seeds(FAKE, 10, 8, 4, 1, 0, FAKE, None) == INVALID              # past the pool's end
    assert L.mp_nbr_seeds(FAKE, 0, 0, 1, 1, 0, FAKE, None) == INVALID               # an empty pool
    assert L.mp_nbr_seeds(FAKE, 2 ** 31, 0, 4, 1, 0, FAKE, None) == UNSUPPORTED
    assert L.mp_nbr_seeds(None, 10, 10, 0, 1, 0, None, None) == 0


# ---- the loaders --------------------------------------------------------------------------------------------------------

def _cfg(sampler, layers_mp=2, **train):
    return types.SimpleNamespace(train=types.SimpleNamespace(sampler=sampler, batch_size=8, walk_length=2, iter_per_epoch=5,
                                                             neighbor_sizes=[20, 15, 10, 5], **train),
                                 val=types.SimpleNamespace(sampler="full_batch"), gnn=types.SimpleNamespace(layers_mp=layers_mp))


def test_loader_from_cfg_builds_the_new_name_and_still_refuses_neighbor():
    from graphgym_amd import samplers as S
    base = SG.build("ring33")
    x, y, mask = torch.ones(33, 2), torch.zeros(33, dtype=torch.int64), torch.arange(33) % 2 == 0
    for layers_mp, sizes in ((2, [20, 15]), (3, [20, 15, 10]), (6, [20, 15, 10, 5])):
        loader = S.loader_from_cfg(_cfg("neighbor_subgraph", layers_mp), base, x, y, mask, "train", seed=4)
        assert isinstance(loader, NB.NeighborLoader) and loader.sizes == sizes and loader.plan.sizes == sizes
        assert len(loader) == 3 and loader.plan.batch_size == 8 and loader.seed == 4        # 17 nodes of the split
        assert loader.plan.pool.tolist() == list(range(0, 33, 2))
    with pytest.raises(NotImplementedError, match="bipartite"):
        S.loader_from_cfg(_cfg("neighbor"), base, x, y, mask, "train")
    assert S.KINDS == ("random_node", "saint_node", "saint_edge", "saint_rw")


def test_loader_batches_on_a_cpu_base():
    """epoch e, batch i is step e * len + i; features and labels follow orig_node; the labelled rows are the seeds, and
    an epoch labels every node of the split once"""
    base = SG.build("ring65")
    x = torch.arange(65, dtype=torch.float32)[:, None] * torch.ones(1, 3)
    y = torch.arange(65) % 7
    mask = torch.arange(65) % 3 == 0
    loader = NB.NeighborLoader(base, x, y, mask, NB.plan_neighbor(base, [2, 1], 5), seed=21)
    assert len(loader) == 5                                                       # 22 nodes of the split
    for epoch in range(2):
        got = list(loader)
        assert len(got) == 5
        labelled = []
        for i, b in enumerate(got):
            want = NB.neighbor_batch(loader.plan, 21, epoch * 5 + i)
            assert torch.equal(b.orig_node, want.orig_node) and torch.equal(b.edge_index, want.edge_index)
            assert torch.equal(b.hop, want.hop) and torch.equal(b.node_label_index, want.seed_index)
            assert torch.equal(b.node_feature[:, 0].long(), b.orig_node) and torch.equal(b.node_label, b.orig_node % 7)
            assert bool((b.hop[b.node_label_index] == 0).all()) and b.num_nodes == b.orig_node.numel()
            labelled += b.orig_node[b.node_label_index].tolist()
        assert sorted(labelled) == list(range(0, 65, 3))
    by_index = NB.NeighborLoader(base, x, y, torch.nonzero(mask).view(-1), loader.plan, 21)
    assert torch.equal(by_index.batch(2).orig_node, loader.batch(2).orig_node)
