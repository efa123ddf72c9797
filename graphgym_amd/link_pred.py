"""Link-prediction batches on the device (csrc/link.hip): the transductive edge split, the disjoint message /
supervision cut and negative sampling of run/configs/IDGNN/edge.yaml (task: link_pred, edge_train_mode: disjoint,
split: [0.8, 0.2]; cfg.dataset.edge_train_mode, edge_message_ratio, edge_negative_sampling_ratio, resample_disjoint,
resample_negative of graphgym/config.py:147-163, handed to DeepSNAP by loader.py:204-233).

    splits = link_split(base, graph_ptr, split=(0.8, 0.2), generator=gen)      # train / val (/ test)
    train = disjoint(splits["train"], cfg.dataset.edge_message_ratio, gen)     # edge_train_mode: disjoint
    batch = link_batch(train, x, ratio=cfg.dataset.edge_negative_sampling_ratio, seed=s, offset=step,
                       transform="edge")                                       # -> harness.GNN, cfg.dataset.task = 'node'

The negatives come from a keyed bijection on the graph's non-edges, not from a rejection loop: plan_negatives counts
the free partners of every row (mp_pair_space_rows) and run_negatives maps sample i of graph g to non-edge number
perm_g(i) (mp_sample_non_edges) — K_g distinct pairs, exactly, in one launch without a host synchronisation, so the
batch pipeline can draw on its side stream.  sample_non_edges_host restates the kernel in NumPy integers: the test
oracle, and the path of a base that lives on the CPU."""
import math
import types

import numpy as np
import torch

from . import _lib
from ._lib import check, lib, ptr
from .graph import CSRGraph, _stream

UNDIRECTED, DIRECTED = _lib.K["MP_PAIRS_UNDIRECTED"], _lib.K["MP_PAIRS_DIRECTED"]
ROUNDS = 6                                    # link.hip: kFeistelRounds
_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15
_I32_MAX = 2 ** 31 - 1


# ---- the restatement of csrc/link.hip on the host ------------------------------------------------------------------

def _mix64(z):
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _round_keys(seed, offset, g):
    h = _mix64((seed & _M64) + _GOLDEN)
    h = _mix64((h ^ (offset & _M64)) + _GOLDEN)
    h = _mix64((h ^ g) + _GOLDEN)
    return [_mix64(h + (k + 1) * _GOLDEN) >> 32 for k in range(ROUNDS)]


def _permute(i, C, keys):
    """perm_g on the uint64 array i (< C): the balanced Feistel network on 2b bits, walked until below C"""
    bits = (C - 1).bit_length()
    b = max(1, (bits + 1) // 2)
    mask = np.uint32((1 << b) - 1)
    x = i.astype(np.uint64).copy()
    todo = np.arange(x.size)
    with np.errstate(over="ignore"):
        while todo.size:
            v = x[todo]
            L, R = (v >> np.uint64(b)).astype(np.uint32), v.astype(np.uint32) & mask
            for key in keys:
                f = R + np.uint32(key)
                f ^= f >> np.uint32(16)
                f *= np.uint32(0x85EBCA6B)
                f ^= f >> np.uint32(13)
                f *= np.uint32(0xC2B2AE35)
                f ^= f >> np.uint32(16)
                L, R = R, L ^ (f & mask)
            v = (L.astype(np.uint64) << np.uint64(b)) | R.astype(np.uint64)
            x[todo] = v
            todo = todo[v >= np.uint64(C)]
    return x.astype(np.int64)


def _host_arrays(base, graph_ptr):
    rowptr = base.rowptr.detach().cpu().numpy().astype(np.int64)
    col = base.col.detach().cpu().numpy().astype(np.int64)[:base.nnz]
    gp = torch.as_tensor(graph_ptr).detach().cpu().numpy().astype(np.int64).reshape(-1)
    N = base.num_nodes
    row = np.repeat(np.arange(N, dtype=np.int64), np.diff(rowptr))
    return rowptr, col, row, gp, N


def pair_space_rows_host(base, graph_ptr, directed):
    """mp_pair_space_rows on the host: (free [N] int64, a column twice in a row?, a column outside its row's graph?)"""
    rowptr, col, row, gp, N = _host_arrays(base, graph_ptr)
    key = row * max(N, 1) + col
    r = np.arange(N, dtype=np.int64)
    g = np.clip(np.searchsorted(gp, r, side="right") - 1, 0, max(gp.size - 2, 0))
    lo, hi = gp[g], gp[g + 1]
    twice = bool((key[1:] == key[:-1]).any())
    outside = bool(((col < lo[row]) | (col >= hi[row])).any())
    rs, re = rowptr[:-1], rowptr[1:]
    above = np.searchsorted(key, r * max(N, 1) + r, side="right")          # first entry of the row with col > r
    if directed:
        diag = above - np.searchsorted(key, r * max(N, 1) + r, side="left")
        free = (hi - lo - 1) - ((re - rs) - np.minimum(diag, 1))
    else:
        free = (hi - 1 - r) - (re - above)
    return np.maximum(free, 0), twice, outside


def _sample_host(rowptr, col, row, gp, N, prefix, counts, directed, seed, offset):
    """steps 1-4 of csrc/link.hip for counts[g] samples of every graph; [2, K] int64 numpy"""
    key = row * max(N, 1) + col
    colp = np.concatenate([col, np.zeros(1, dtype=np.int64)])               # (a readable slot behind the last entry)
    out = []
    for g, K in enumerate(counts):
        if K == 0:
            continue
        lo, hi = int(gp[g]), int(gp[g + 1])
        p0 = int(prefix[lo])
        C = int(prefix[hi]) - p0
        rank = _permute(np.arange(K, dtype=np.uint64), C, _round_keys(seed, offset, g))
        target = p0 + rank
        r = np.searchsorted(prefix, target, side="right") - 1               # the last row whose prefix is <= the rank
        t = target - prefix[r]
        rs, re = rowptr[r], rowptr[r + 1]
        if directed:
            first, s0 = lo, rs
            no_diag = np.searchsorted(key, r * N + r, side="left") == np.searchsorted(key, r * N + r, side="right")
        else:
            first, s0 = r + 1, np.searchsorted(key, r * N + r, side="right")
        a, z = s0.copy(), re.copy()
        while True:                                                         # the binary search of every sample at once
            act = a < z
            if not act.any():
                break
            mid = (a + z) >> 1
            cm = colp[np.where(act, mid, 0)]
            below = (cm - first) - (mid - s0)
            if directed:
                below = below - ((cm > r) & no_diag)
            go = act & (below <= t)
            a = np.where(go, mid + 1, a)
            z = np.where(act & ~go, mid, z)
        c = first + t + (a - s0)
        if directed:
            c = c + (no_diag & (c >= r))
            out.append(np.stack([c, r]))
        else:
            out.append(np.stack([r, c]))
    return np.concatenate(out, 1) if out else np.zeros((2, 0), dtype=np.int64)


def _is_symmetric_host(base):
    rowptr, col, row, _, N = _host_arrays(base, [0, base.num_nodes])
    return bool(np.array_equal(np.sort(row * max(N, 1) + col), np.sort(col * max(N, 1) + row)))


def _directed(base, directed):
    """the pair mode of `base`: directed=None means undirected exactly when the base equals its transpose"""
    if base.nnz == 0:
        sym = True
    elif base.rowptr.is_cuda:
        sym = base.is_symmetric(run=True)
    else:
        sym = _is_symmetric_host(base)
    if directed is None:
        return not sym
    if not directed and not sym:
        raise ValueError("undirected pairs need a symmetric base (every edge stored in both directions)")
    return bool(directed)


def sample_non_edges_host(base, graph_ptr, counts, seed, offset=0, directed=None):
    """counts[g] distinct non-edges of every graph of `base` (CSRGraph: row = destination, columns ascending, graphs
    delimited by graph_ptr [G+1]) as [2, K] int64 on the CPU (row 0 = src, row 1 = dst; undirected pairs as (lo, hi)):
    csrc/link.hip restated in Python / NumPy integers — the Feistel bijection with cycle walking, rank -> row through
    the prefix of the free counts, rank -> column inside the row.  Bit for bit what run_negatives writes on the device.
    This sampler is the project's own: PyG's and DeepSNAP's negative_sampling are rejection samplers of third parties
    that may return fewer pairs than asked, and nothing of theirs was consulted or matched [3P-unverified]."""
    plan = plan_negatives(_on_cpu(base), graph_ptr, counts, directed)
    return run_negatives(plan, seed, offset).clone()


def _on_cpu(base):
    if not base.rowptr.is_cuda:
        return base
    return CSRGraph(base.rowptr.cpu(), base.col.cpu(), None, None, base.num_nodes, base.nnz)


# ---- negatives -----------------------------------------------------------------------------------------------------

def _graph_ptr(graph_ptr, N, dev):
    from .edge_nets import _graph_ptr as checked
    return checked(graph_ptr, N, dev)


def plan_negatives(base, graph_ptr, counts, directed=None):
    """The inputs and the preallocated output of mp_sample_non_edges for counts[g] negatives of every graph: free [N]
    (non-stored partners per row, mp_pair_space_rows), prefix [N+1] (its exclusive prefix sum), C [G] (non-edges per
    graph), slot_base [G+1], out [2, K].  directed=None: undirected pairs exactly when base.is_symmetric(run=True);
    undirected on a base that is not symmetric, a column stored twice in a row, an edge across two graphs and
    counts[g] > C[g] are ValueErrors.  One synchronisation (flags, C and counts in one read; the symmetry check is the
    base's own and is cached on it).  A base on the CPU takes the host restatement."""
    dev, N = base.device, base.num_nodes
    gp = _graph_ptr(graph_ptr, N, dev)
    G = gp.numel() - 1
    cnt = torch.as_tensor(counts).to(dev, torch.int64).reshape(-1)
    if cnt.numel() != G:
        raise ValueError(f"counts must hold one entry per graph: {cnt.numel()} for {G} graphs")
    directed = _directed(base, directed)
    if N >= _I32_MAX:
        raise ValueError("plan_negatives: a graph must hold fewer than 2^31 nodes")
    prefix = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    if dev.type == "cuda":
        free = torch.empty(N, dtype=torch.int64, device=dev)
        flags = torch.empty(2, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            check(lib().mp_pair_space_rows(ptr(base.rowptr), ptr(base.col), N, base.nnz, ptr(gp), G,
                                           DIRECTED if directed else UNDIRECTED, ptr(free), ptr(flags), _stream()),
                  "mp_pair_space_rows")
    else:
        f, twice, outside = pair_space_rows_host(base, gp, directed)
        free = torch.from_numpy(f)
        flags = torch.tensor([int(twice), int(outside)], dtype=torch.int32)
    torch.cumsum(free, 0, out=prefix[1:])
    C = prefix[gp[1:]] - prefix[gp[:-1]]
    slot_base = torch.zeros(G + 1, dtype=torch.int64, device=dev)
    torch.cumsum(cnt, 0, out=slot_base[1:])
    host = torch.cat([flags.to(torch.int64), C, cnt]).tolist()                     # the one synchronisation
    if host[0]:
        raise ValueError("the base stores an entry twice: negative sampling needs distinct columns inside a row")
    if host[1]:
        raise ValueError("an edge of the base joins two graphs of graph_ptr")
    C_host, cnt_host = host[2:2 + G], host[2 + G:]
    for g in range(G):
        if cnt_host[g] < 0 or cnt_host[g] > C_host[g]:
            raise ValueError(f"graph {g}: {cnt_host[g]} negatives asked, the graph has {C_host[g]} non-edges")
    K = sum(cnt_host)
    return types.SimpleNamespace(base=base, gp=gp, n_graphs=G, directed=directed, free=free, prefix=prefix, C=C,
                                 C_host=C_host, counts=cnt_host, slot_base=slot_base, K=K,
                                 out=torch.empty(2, K, dtype=torch.int64, device=dev))


def run_negatives(plan, seed, offset=0):
    """plan.out [2, K] <- the plan's negatives under (seed, offset): one mp_sample_non_edges launch on the current
    stream, no synchronisation (resample_negative: the same plan with offset = step).  Sample i of graph g depends on
    (seed, offset, g, i) alone.  Returns plan.out, which the next run overwrites."""
    b = plan.base
    if b.device.type != "cuda":
        rowptr, col, row, gp, N = _host_arrays(b, plan.gp)
        got = _sample_host(rowptr, col, row, gp, N, plan.prefix.numpy(), plan.counts, plan.directed, int(seed),
                           int(offset))
        plan.out.copy_(torch.from_numpy(got))
        return plan.out
    with torch.cuda.device(b.device):
        check(lib().mp_sample_non_edges(ptr(b.rowptr), ptr(b.col), b.num_nodes, b.nnz, ptr(plan.gp), plan.n_graphs,
                                        ptr(plan.prefix), ptr(plan.slot_base), plan.K,
                                        DIRECTED if plan.directed else UNDIRECTED, int(seed) & _M64,
                                        int(offset) & _M64, ptr(plan.out), _stream()), "mp_sample_non_edges")
    # plan.out was refilled through its raw pointer: move its version, as copy_ does on the host path, so that a cache
    # keyed on it (graph.tensor_stamp) sees the new contents
    torch.autograd.graph.increment_version(plan.out)
    return plan.out


# ---- splits --------------------------------------------------------------------------------------------------------

def host_csr(edge_index, num_nodes):
    """the CSRGraph CSRGraph.from_edge_index builds (row = destination, columns ascending, entries kept as given), from
    CPU tensors and on the CPU: for graphs that never reach the device (tests, the host sampler)"""
    ei = torch.as_tensor(edge_index).to(torch.int64)
    N = int(num_nodes)
    order = torch.argsort(ei[1] * max(N, 1) + ei[0], stable=True)
    rowptr = torch.zeros(N + 1, dtype=torch.int64)
    torch.cumsum(torch.bincount(ei[1], minlength=N), 0, out=rowptr[1:])
    return CSRGraph(rowptr.to(torch.int32), ei[0][order].to(torch.int32), None, order.to(torch.int32), N, ei.size(1))


def _message_graph(pairs, num_nodes, directed):
    """(edge_index, CSRGraph) of the message edges `pairs` [2, P]: undirected pairs stored in both directions"""
    ei = pairs if directed else torch.cat([pairs, pairs.flip(0)], 1)
    if ei.is_cuda:
        return ei, CSRGraph.from_edge_index(ei, num_nodes, validate=False)
    return ei, host_csr(ei, num_nodes)


def _cut(n, ratios):
    """the sizes of len(ratios) + 1 parts of n items: cuts at floor(cumulative ratio * n), the last part the rest"""
    cuts, acc = [0], 0.0
    for r in ratios:
        acc += float(r)
        cuts.append(min(n, max(cuts[-1], int(math.floor(acc * n + 1e-9)))))     # (0.29 * 100 is 28.999...)
    cuts.append(n)
    return [b - a for a, b in zip(cuts[:-1], cuts[1:])]


def _cut_per_graph(pairs, gp, ratios, generator):
    """pairs [2, P] (grouped by graph, graphs ascending) cut into len(ratios) + 1 parts graph by graph: a permutation
    from torch.randperm(P_g, generator=generator) per graph, cut at the cumulative ratios.  Every part stays grouped by
    graph.  One synchronisation (the per-graph sizes)."""
    dev = pairs.device
    G = gp.numel() - 1
    per_graph = torch.bincount(torch.searchsorted(gp, pairs[1], right=True) - 1, minlength=G)[:G].tolist()
    gen_dev = generator.device if generator is not None else torch.device("cpu")
    parts = [[] for _ in range(len(ratios) + 1)]
    at = 0
    for n in per_graph:
        perm = torch.randperm(n, generator=generator, device=gen_dev).to(dev) + at
        lo = 0
        for k, size in enumerate(_cut(n, ratios)):
            parts[k].append(perm[lo:lo + size])
            lo += size
        at += n
    empty = torch.empty(0, dtype=torch.int64, device=dev)
    return [pairs[:, torch.cat(p) if p else empty] for p in parts]


def _split(name, pos, message, base, gp, gp_host, directed):
    ei, g = _message_graph(message, base.num_nodes, directed)
    return types.SimpleNamespace(name=name, pos_index=pos, pairs=message, edge_index=ei, graph=g, base=base, gp=gp,
                                 gp_host=gp_host, directed=directed, num_nodes=base.num_nodes)


def link_split(base, graph_ptr, split=(0.8, 0.2), generator=None, directed=None):
    """A transductive split of the stored edges of `base` into train / val (/ test) supervision sets, graph by graph.
    Undirected base (symmetric; directed=None asks the base): one draw per unordered pair — the entries with col < row,
    oriented (lo, hi); directed base: one draw per stored entry, (src, dst).  Per graph a permutation from
    torch.randperm(P_g, generator=generator) is cut at the cumulative ratios of `split` (two or three of them); the
    last split takes the remainder.  Stored self loops are no links: they join no supervision set and no message graph.

    Returns {"train": s, "val": s[, "test": s]}, each s with pos_index [2, P] (the supervision edges, grouped by graph),
    edge_index [2, E] and graph (the message-passing edges and their CSRGraph; undirected edges stored in both
    directions), pairs (the message edges once each), base, gp (graph_ptr on the device; gp_host on the CPU), directed.
    The message graph of train is the train edges, of val the train edges, of test train + val: no held-out supervision
    edge is an entry of the message graph that predicts it.  This is DeepSNAP's transductive link-prediction split as we understand it; DeepSNAP itself was
    not available to compare against [3P-unverified]."""
    if len(split) not in (2, 3):
        raise ValueError("split must hold two or three ratios")
    dev, N = base.device, base.num_nodes
    gp_host = torch.as_tensor(graph_ptr).to("cpu", torch.int64).reshape(-1)     # (checked on the host: no device reads)
    gp = _graph_ptr(gp_host, N, dev)
    directed = _directed(base, directed)
    rp = base.rowptr.long()
    row = torch.repeat_interleave(torch.arange(N, device=dev), rp[1:] - rp[:-1])
    col = base.col.long()[:base.nnz]
    keep = (col != row) if directed else (col < row)
    pairs = torch.stack([col[keep], row[keep]])
    if bool((torch.searchsorted(gp, pairs[0], right=True) != torch.searchsorted(gp, pairs[1], right=True)).any()):
        raise ValueError("an edge of the base joins two graphs of graph_ptr")
    parts = _cut_per_graph(pairs, gp, list(split)[:-1], generator)
    out = {"train": _split("train", parts[0], parts[0], base, gp, gp_host, directed),
           "val": _split("val", parts[1], parts[0], base, gp, gp_host, directed)}
    if len(split) == 3:
        out["test"] = _split("test", parts[2], torch.cat([parts[0], parts[1]], 1), base, gp, gp_host, directed)
    return out


def disjoint(train, message_ratio=0.8, generator=None):
    """edge_train_mode: disjoint — the train edges (train.pairs) are cut again, graph by graph, into message edges (the
    first message_ratio of a fresh permutation) and supervision edges (the rest), and the message graph is rebuilt from
    the former.  Calling it again on the same train split is resample_disjoint.  (Mode 'all' is the train split as it
    is: supervision = message edges.)  The result carries the full train edges along, so it can be cut again."""
    src = getattr(train, "train_pairs", train.pairs)
    msg, sup = _cut_per_graph(src, train.gp, [message_ratio], generator)
    s = _split(train.name, sup, msg, train.base, train.gp, train.gp_host, train.directed)
    s.train_pairs = src
    return s


def link_batch(split, x, ratio=1.0, seed=0, offset=0, transform=None, plan=None):
    """The batch of one split: edge_label_index = cat(pos, neg), edge_label = cat(ones, zeros) as float32
    (get_link_label, transform.py:93-98), K_g = round(ratio * P_g) negatives per graph drawn against the BASE graph, so
    no held-out positive is ever handed out as a negative.  plan: a plan_negatives of split.base to reuse (its counts
    decide K_g; resample_negative = the same plan, another offset); without one the call plans (one synchronisation).

    transform=None: a harness.Batch with node_feature = x, edge_index (the message edges) and edge_label_index /
    edge_label for harness.GNNEdgeHead.  transform="edge": the message graph and the labels go through
    edge_nets.edge_batch(..., sources="labels", csr="none") — link prediction as node classification on the edge-net
    batch (loader.py:181-187), node_label int64, the expansion's CSR seeded into the batch."""
    pos, gp = split.pos_index, split.gp
    G = gp.numel() - 1
    if plan is None:
        per_graph = torch.bincount(torch.searchsorted(gp, pos[1], right=True) - 1, minlength=G)[:G].tolist()
        counts = [int(round(ratio * p)) for p in per_graph]
        plan = plan_negatives(split.base, split.gp_host, counts, split.directed)
    neg = run_negatives(plan, seed, offset)
    eli = torch.cat([pos, neg], 1)
    label = torch.cat([torch.ones(pos.size(1), dtype=torch.float32, device=pos.device),
                       torch.zeros(neg.size(1), dtype=torch.float32, device=pos.device)])
    if transform is None:
        from .harness import Batch
        return Batch(node_feature=x, edge_index=split.edge_index, edge_label_index=eli, edge_label=label)
    if transform != "edge":
        raise ValueError("transform must be None or 'edge'")
    from .edge_nets import edge_batch, seed_graph
    batch, g = edge_batch(split.graph, gp, eli, label.to(torch.int64), x, sources="labels", csr="none")
    if g is not None:
        seed_graph(batch, g, "none")
    batch.edge_label_index, batch.edge_label = eli, label
    return batch
