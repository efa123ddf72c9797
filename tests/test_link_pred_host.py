"""Link-prediction batches without a device (CPU suite): the argument checks of mp_pair_space_rows and
mp_sample_non_edges (csrc/link.hip; every case returns before anything is launched), the NumPy restatement of the
sampler (graphgym_amd.link_pred.sample_non_edges_host — the oracle of tests/test_link_pred_gpu.py) on hand-made graphs,
its uniformity, and the edge split / disjoint cut / batch assembly on CPU tensors."""
import ctypes as C
import math

import pytest
import torch

import _link_graphs as LG
from graphgym_amd import _lib

INVALID, UNSUPPORTED = 1, 2
FAKE = C.c_void_p(256)        # a non-null pointer that is never dereferenced
BIG = 2 ** 31
MODES = [False, True]         # directed?


def _space(N=10, nnz=20, n_graphs=1, mode=0, rowptr=FAKE, col=FAKE, graph_ptr=FAKE, free=FAKE, flags=FAKE):
    return _lib.lib().mp_pair_space_rows(rowptr, col, N, nnz, graph_ptr, n_graphs, mode, free, flags, None)


def _sample(N=10, nnz=20, n_graphs=1, K=5, mode=0, rowptr=FAKE, col=FAKE, graph_ptr=FAKE, prefix=FAKE, slot_base=FAKE,
            out=FAKE):
    return _lib.lib().mp_sample_non_edges(rowptr, col, N, nnz, graph_ptr, n_graphs, prefix, slot_base, K, mode, 1, 0,
                                          out, None)


def test_prototypes_exist():
    for name in ("mp_pair_space_rows", "mp_sample_non_edges"):
        assert name in _lib.PROTOTYPES
        assert hasattr(_lib.lib(), name)


def test_pair_space_rows_rejects_bad_arguments_before_any_launch():
    assert _space(rowptr=None) == INVALID
    assert _space(col=None) == INVALID
    assert _space(graph_ptr=None) == INVALID
    assert _space(free=None) == INVALID
    assert _space(flags=None) == INVALID
    assert _space(N=-1) == INVALID
    assert _space(nnz=-1) == INVALID
    assert _space(n_graphs=-1) == INVALID
    assert _space(n_graphs=0) == INVALID                  # rows of no graph
    assert _space(mode=2) == INVALID
    assert _space(mode=-1) == INVALID
    assert _space(N=BIG) == UNSUPPORTED
    assert _space(nnz=BIG) == UNSUPPORTED


def test_sample_non_edges_rejects_bad_arguments_before_any_launch():
    assert _sample(rowptr=None) == INVALID
    assert _sample(col=None) == INVALID
    assert _sample(graph_ptr=None) == INVALID
    assert _sample(prefix=None) == INVALID
    assert _sample(slot_base=None) == INVALID
    assert _sample(out=None) == INVALID
    assert _sample(K=-1) == INVALID
    assert _sample(N=-1) == INVALID
    assert _sample(nnz=-1) == INVALID
    assert _sample(n_graphs=0) == INVALID                 # samples of no graph
    assert _sample(mode=2) == INVALID
    assert _sample(N=BIG) == UNSUPPORTED
    assert _sample(K=0, out=None) == 0                    # nothing to draw: no launch


def test_config_carries_the_link_prediction_defaults():
    from graphgym_amd.config import _defaults
    d = _defaults().dataset
    assert (d.edge_train_mode, d.edge_message_ratio, d.edge_negative_sampling_ratio, d.resample_disjoint,
            d.resample_negative) == ("all", 0.8, 1.0, False, False)


# ---- the restatement on hand-made graphs ---------------------------------------------------------------------------

def _counts(free, want):
    """per graph: `want` negatives where the graph has that many, else all it has"""
    return [min(len(f), want) for f in free]


@pytest.mark.parametrize("directed", MODES)
@pytest.mark.parametrize("name", sorted(LG.CASES))
def test_host_sampler_on_hand_made_graphs(name, directed):
    """every pair inside its graph, not stored (in either direction when undirected), src != dst, no pair twice, exactly
    K_g per graph — for a partial draw and for the whole complement"""
    from graphgym_amd.link_pred import plan_negatives, sample_non_edges_host
    base, gp, stored = LG.build(name, directed)
    free = LG.complement(stored, gp, directed)
    plan = plan_negatives(base, gp, [0] * len(free), directed)
    assert plan.C_host == [len(f) for f in free]
    assert plan.directed == directed
    for want in (3, 10 ** 6):
        counts = _counts(free, want)
        out = sample_non_edges_host(base, gp, counts, seed=11, directed=directed)
        pairs = LG.check_sample(out, counts, gp, stored, directed)
        if want > 3:
            assert set(pairs) == set().union(*free)
    if name == "k4":
        assert sum(len(f) for f in free) == 0 and tuple(out.shape) == (2, 0)
    if name == "empty2":
        assert len(free[0]) == (2 if directed else 1)


def test_mode_is_read_off_the_base():
    """directed=None: undirected exactly when the base equals its transpose; undirected on a directed base is refused"""
    from graphgym_amd.link_pred import plan_negatives
    sym, gp, _ = LG.build("path4", False)
    one_way, _, _ = LG.build("path4", True)
    assert plan_negatives(sym, gp, [1]).directed is False
    assert plan_negatives(one_way, gp, [1]).directed is True
    assert plan_negatives(sym, gp, [1], directed=True).C_host == [4 * 3 - 6]
    with pytest.raises(ValueError, match="symmetric"):
        plan_negatives(one_way, gp, [1], directed=False)


@pytest.mark.parametrize("directed", MODES)
def test_whole_complement_at_every_small_domain_size(directed):
    """K = C returns the complement as a set for every C from 1 to 40: the bijection and the cycle walk at every small
    domain (b = 1, 2, 3 and the sizes on either side of a power of four)"""
    from graphgym_amd.link_pred import sample_non_edges_host
    for C_ in range(1, 41):
        links, sizes = LG.with_complement_of(C_, directed)
        base, gp, stored = LG.build_links(links, sizes, directed)
        free = LG.complement(stored, gp, directed)
        assert len(free[0]) == C_
        for seed in (0, 1, 2):
            out = sample_non_edges_host(base, gp, [C_], seed=seed, directed=directed)
            assert set(zip(out[0].tolist(), out[1].tolist())) == free[0], (C_, seed)


@pytest.mark.parametrize("directed", MODES)
def test_prefix_property_offsets_and_seeds(directed):
    """sample i depends on (seed, offset, g, i) alone: K and K + 5 agree on the first K of every graph; another offset
    or another seed is another draw; the same arguments the same draw"""
    from graphgym_amd.link_pred import sample_non_edges_host
    base, gp, _ = LG.build("batch_2_5_9", directed)
    small, large = [0, 2, 10], [0, 5, 15]
    a = sample_non_edges_host(base, gp, small, seed=5, offset=3, directed=directed)
    b = sample_non_edges_host(base, gp, large, seed=5, offset=3, directed=directed)
    assert torch.equal(a[:, :2], b[:, :2]) and torch.equal(a[:, 2:], b[:, 5:15])
    assert torch.equal(a, sample_non_edges_host(base, gp, small, seed=5, offset=3, directed=directed))
    assert not torch.equal(a, sample_non_edges_host(base, gp, small, seed=5, offset=4, directed=directed))
    assert not torch.equal(a, sample_non_edges_host(base, gp, small, seed=6, offset=3, directed=directed))


def test_more_negatives_than_non_edges_is_refused():
    from graphgym_amd.link_pred import sample_non_edges_host
    base, gp, stored = LG.build("batch_2_5_9", False)
    free = LG.complement(stored, gp, False)
    counts = [len(f) for f in free]
    counts[1] += 1
    with pytest.raises(ValueError, match=rf"graph 1: {counts[1]} negatives.* {counts[1] - 1} non-edges"):
        sample_non_edges_host(base, gp, counts, seed=0)
    with pytest.raises(ValueError, match="one entry per graph"):
        sample_non_edges_host(base, gp, [1, 1], seed=0)


@pytest.mark.parametrize("directed", MODES)
def test_repeated_entry_is_refused(directed):
    from graphgym_amd.link_pred import host_csr, plan_negatives
    ei = torch.tensor([[0, 1, 1, 2, 1], [1, 0, 2, 1, 0]])              # 1 -> 0 twice
    if directed:
        ei = ei[:, [0, 1, 2, 4]]
    base = host_csr(ei, 4)
    with pytest.raises(ValueError, match="twice"):
        plan_negatives(base, torch.tensor([0, 4]), [1], directed=True)
    if not directed:
        with pytest.raises(ValueError, match="twice|symmetric"):
            plan_negatives(base, torch.tensor([0, 4]), [1])


def test_edge_across_two_graphs_is_refused():
    from graphgym_amd.link_pred import plan_negatives
    base, _, _ = LG.build("path4", False)
    with pytest.raises(ValueError, match="two graphs"):
        plan_negatives(base, torch.tensor([0, 2, 4]), [0, 0])


def _chi2(freq, total):
    cells = len(freq)
    e = total / cells
    return sum((f - e) ** 2 / e for f in freq)


def test_draws_are_uniform_over_the_non_edges():
    """12 nodes, 50 free unordered pairs, K = 10, S = 400 seeds.  Under a uniform sampler the chi-square statistic of
    the pair frequencies has df = C - 1 degrees of freedom, mean df and variance 2 df (a draw without replacement only
    lowers it); the bound df + 6 sqrt(2 df) comes from that null distribution, for all slots and for slot 0 alone.  A
    failure means the round function is too weak: add rounds."""
    from graphgym_amd.link_pred import plan_negatives, run_negatives
    links, sizes = LG.UNIFORMITY
    base, gp, stored = LG.build_links(links, sizes, False)
    free = sorted(LG.complement(stored, gp, False)[0])
    C_, K, S = len(free), 10, 400
    assert C_ == 50
    at = {p: k for k, p in enumerate(free)}
    every, first = [0] * C_, [0] * C_
    plan = plan_negatives(base, gp, [K])
    for seed in range(S):
        out = run_negatives(plan, seed)
        pairs = list(zip(out[0].tolist(), out[1].tolist()))
        for p in pairs:
            every[at[p]] += 1
        first[at[pairs[0]]] += 1
    df = C_ - 1
    bound = df + 6 * math.sqrt(2 * df)
    x_all, x_first = _chi2(every, K * S), _chi2(first, S)
    print(f"chi2 all slots {x_all:.1f}, slot 0 {x_first:.1f}, df {df}, bound {bound:.1f}")
    assert x_all <= bound
    assert x_first <= bound


# ---- splits and batches on CPU tensors -----------------------------------------------------------------------------

def _random_batch(directed, seed=0):
    """three graphs of 10, 15 and 20 nodes with 12, 31 and 47 distinct links"""
    gen = torch.Generator().manual_seed(seed)
    links, sizes, lo = [], [10, 15, 20], 0
    for n, m in zip(sizes, [12, 31, 47]):
        cand = [(a, b) for a in range(n) for b in range(n) if (a != b if directed else a < b)]
        for k in torch.randperm(len(cand), generator=gen)[:m].tolist():
            links.append((cand[k][0] + lo, cand[k][1] + lo))
        lo += n
    base, gp, stored = LG.build_links(links, sizes, directed)
    return base, gp, stored, links, [12, 31, 47]


def _pairs(t):
    return list(zip(t[0].tolist(), t[1].tolist()))


def _per_graph(pairs, gp):
    gp = gp.tolist()
    return [sum(1 for p in pairs if lo <= p[1] < hi) for lo, hi in zip(gp[:-1], gp[1:])]


def _entries(g):
    rp = g.rowptr.tolist()
    col = g.col.tolist()
    return {(col[e], r) for r in range(g.num_nodes) for e in range(rp[r], rp[r + 1])}


@pytest.mark.parametrize("directed", MODES)
@pytest.mark.parametrize("split", [(0.8, 0.2), (0.7, 0.2, 0.1)])
def test_link_split_partitions_the_links(directed, split):
    from graphgym_amd.link_pred import link_split
    base, gp, stored, links, per_graph = _random_batch(directed)
    want = {(min(p), max(p)) for p in links} if not directed else set(links)
    s = link_split(base, gp, split, generator=torch.Generator().manual_seed(3))
    assert list(s) == ["train", "val", "test"][:len(split)]
    got = [p for part in s.values() for p in _pairs(part.pos_index)]
    assert len(got) == len(want) and set(got) == want                      # a partition: every link once
    cum = [sum(split[:k + 1]) for k in range(len(split) - 1)]
    for g, n in enumerate(per_graph):
        cuts = [0] + [int(math.floor(c * n + 1e-9)) for c in cum] + [n]    # the last split takes the remainder
        for k, part in enumerate(s.values()):
            assert _per_graph(_pairs(part.pos_index), gp)[g] == cuts[k + 1] - cuts[k]
    # message edges: train <- train, val <- train, test <- train + val; both directions of an undirected link
    train, val = set(_pairs(s["train"].pos_index)), set(_pairs(s["val"].pos_index))
    both = (lambda ps: ps | {(b, a) for a, b in ps}) if not directed else (lambda ps: ps)
    assert _entries(s["train"].graph) == both(train) == set(_pairs(s["train"].edge_index))
    assert _entries(s["val"].graph) == both(train)
    assert not (_entries(s["val"].graph) & both(val))                      # no held-out pair in its message graph
    if len(split) == 3:
        test = set(_pairs(s["test"].pos_index))
        assert _entries(s["test"].graph) == both(train | val)
        assert not (_entries(s["test"].graph) & both(test))
    # the same generator state gives the same split, another one another
    again = link_split(base, gp, split, generator=torch.Generator().manual_seed(3))
    other = link_split(base, gp, split, generator=torch.Generator().manual_seed(4))
    assert all(torch.equal(s[k].pos_index, again[k].pos_index) for k in s)
    assert not all(torch.equal(s[k].pos_index, other[k].pos_index) for k in s)


@pytest.mark.parametrize("directed", MODES)
def test_disjoint_cuts_the_train_links_again(directed):
    from graphgym_amd.link_pred import disjoint, link_split
    base, gp, _, _, _ = _random_batch(directed, seed=1)
    train = link_split(base, gp, (0.8, 0.2), generator=torch.Generator().manual_seed(0))["train"]
    gen = torch.Generator().manual_seed(9)
    d = disjoint(train, 0.8, generator=gen)
    msg, sup = set(_pairs(d.pairs)), set(_pairs(d.pos_index))
    assert not (msg & sup) and (msg | sup) == set(_pairs(train.pos_index))
    both = (lambda ps: ps | {(b, a) for a, b in ps}) if not directed else (lambda ps: ps)
    assert _entries(d.graph) == both(msg) and not (_entries(d.graph) & both(sup))
    for g, n in enumerate(_per_graph(_pairs(train.pos_index), gp)):
        assert _per_graph(_pairs(d.pairs), gp)[g] == int(math.floor(0.8 * n + 1e-9))
        assert _per_graph(_pairs(d.pos_index), gp)[g] == n - int(math.floor(0.8 * n + 1e-9))
    # resample_disjoint: calling it again (on the train split or on its own result) cuts the same train links anew
    for src in (train, d):
        d2 = disjoint(src, 0.8, generator=gen)
        assert set(_pairs(d2.pairs)) | set(_pairs(d2.pos_index)) == set(_pairs(train.pos_index))
        assert set(_pairs(d2.pos_index)) != sup
    same = disjoint(train, 0.8, generator=torch.Generator().manual_seed(9))
    assert torch.equal(same.pos_index, d.pos_index) and torch.equal(same.edge_index, d.edge_index)


@pytest.mark.parametrize("directed", MODES)
@pytest.mark.parametrize("ratio", [1.0, 2.0])
def test_link_batch_labels(directed, ratio):
    """ones then zeros as float32, P positives and round(ratio P) negatives, drawn against the BASE graph: no link of
    any split is handed out as a negative"""
    from graphgym_amd.link_pred import link_batch, link_split, plan_negatives
    base, gp, stored, links, _ = _random_batch(directed, seed=2)
    s = link_split(base, gp, (0.8, 0.2), generator=torch.Generator().manual_seed(1))
    x = torch.rand(base.num_nodes, 4)
    for part in s.values():
        b = link_batch(part, x, ratio=ratio, seed=3)
        P = part.pos_index.size(1)
        K = sum(int(round(ratio * p)) for p in _per_graph(_pairs(part.pos_index), gp))
        assert K == round(ratio * P)
        assert b.edge_label.dtype == torch.float32
        assert torch.equal(b.edge_label, torch.cat([torch.ones(P), torch.zeros(K)]))
        assert torch.equal(b.edge_label_index[:, :P], part.pos_index)
        assert b.node_feature is x and torch.equal(b.edge_index, part.edge_index)
        neg = b.edge_label_index[:, P:]
        LG.check_sample(neg, [int(round(ratio * p)) for p in _per_graph(_pairs(part.pos_index), gp)], gp, stored,
                        directed)
    # one plan, several draws (resample_negative: offset = step)
    part = s["train"]
    counts = _per_graph(_pairs(part.pos_index), gp)
    plan = plan_negatives(base, gp, counts, directed)
    b0 = link_batch(part, x, seed=3, offset=0, plan=plan)
    b1 = link_batch(part, x, seed=3, offset=1, plan=plan)
    assert not torch.equal(b0.edge_label_index, b1.edge_label_index)
    assert torch.equal(b0.edge_label_index, link_batch(part, x, seed=3).edge_label_index)
    with pytest.raises(ValueError, match="transform"):
        link_batch(part, x, transform="ego")
