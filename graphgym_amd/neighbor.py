"""The neighbour sampler (csrc/neighbor.hip, include/mp_neighbor.h): the sampled computation tree of a batch of seed
nodes as ONE subgraph — seeds plus sampled in-neighbours per hop, the loss on the seeds — which harness.GNN.forward
consumes like any other batch.  This is the form of PyG's NeighborLoader.  GraphGym's own train.sampler = neighbor
(graphgym/config.py:248, graphgym/loader_pyg.py:209-215) asks PyG's older NeighborSampler for per-layer bipartite
blocks, which GNN.forward does not consume: samplers.loader_from_cfg keeps refusing that name and builds this sampler
under `neighbor_subgraph`, from the same cfg.train.neighbor_sizes.

    plan = plan_neighbor(base, [20, 15, 10], batch_size=1024, pool=train_nodes)
    batch = neighbor_batch(plan, seed, step)             # SubgraphBatch + hop, seed_index
    batch = neighbor_batch_nodes(plan, my_seeds, seed, step)
    loader = NeighborLoader(base, x, y, train_mask, plan, seed)          # yields harness.Batch objects

The draw, in integers only (perm = the keyed bijection of csrc/draws.h; link_pred._round_keys / _permute restate it).
    seeds   len(loader) = ceil(n_pool / B); batch i of epoch e takes positions q = i B .. min((i + 1) B, n_pool) - 1 and
            its seeds are pool[perm(seed ^ STREAM, e, 2^63, q, n_pool)]: an epoch visits every pool node exactly once, the
            last batch may be short; step = e * len + i
    hops    seeds have hop 0; hop(v) is the first hop at which v enters the batch.  For h = 0 .. L - 1 every node v that
            entered at hop h is sampled once with fanout s = sizes[h]: k = deg v if s = -1 or deg v <= s, else k = s; the
            sampled base positions are rowptr[v] + perm(seed ^ STREAM, step, (h << 32) | v, j, deg v), j < k (k = deg v:
            the whole row, no permutation); their columns enter with hop h + 1 unless they are in already.  Nodes of hop
            L have empty rows.
A node's sample is a pure function of (seed, step, h, v) and the base.

The batch: orig_node ascending; graph an n_sub x n_sub CSRGraph (eid = arange, symmetric = False) whose row k holds the
sampled entries of orig_node[k] in ascending base position — columns ascend, repeated and self entries of the base stay
as stored; edge_index in CSR order; base_entry; hop [n_sub] int32; seed_index, the batch positions of the seeds,
ascending.

Host reads per batch: L + 1 for neighbor_batch (the frontier sizes of hops 1 .. L - 1, n_sub, nnz) and L + 2 for
neighbor_batch_nodes (the caller's seeds may repeat: their distinct count is read as well).  Work follows the batch: the
only passes that follow the base are over its bitmaps of N / 8 bytes.

seeds_host / neighbor_batch_host restate the kernels in NumPy integers: the test oracle, and the path of a base that lives
on the CPU."""
import types

import numpy as np
import torch

from . import _lib_neighbor
from ._lib import check, ptr
from ._lib_neighbor import MAX_FANOUT, STREAM
from .graph import CSRGraph, _stream
from .link_pred import _M64, _permute, _round_keys
from .samplers import SubgraphBatch, _csr_host, _mask_of, _node_list

_I32_MAX = 2 ** 31 - 1
_SEED_GROUP = 1 << 63


def _u64(v):
    return int(v) & _M64


# ---- plans ---------------------------------------------------------------------------------------------------------------

def plan_neighbor(base, sizes, batch_size, pool=None):
    """What the batches of one base need: sizes (one fanout per hop, each -1 or in [1, MAX_FANOUT]), batch_size, and the
    seed pool (an integer node list or a bool mask [N]; None = all nodes) as an int32 list on the base's device.
    ValueError: empty sizes, a size of 0, below -1 or above MAX_FANOUT, batch_size < 1, an empty pool, a pool entry
    outside [0, N) or named twice.  A base on the CPU gives a plan for the host restatements."""
    N, dev = base.num_nodes, base.rowptr.device
    if N >= _I32_MAX:
        raise ValueError("plan_neighbor: a graph must hold fewer than 2^31 nodes")
    sizes = [int(s) for s in sizes]
    if not sizes:
        raise ValueError("sizes must name at least one hop")
    for s in sizes:
        if s != -1 and not 1 <= s <= MAX_FANOUT:
            raise ValueError(f"a size must be -1 (the whole row) or lie in [1, {MAX_FANOUT}], got {s}")
    if batch_size is None or int(batch_size) < 1:
        raise ValueError("batch_size must be at least 1")
    if pool is None:
        n_pool = N
    else:
        pool = torch.as_tensor(pool)
        if pool.dtype == torch.bool:
            pool = torch.nonzero(_mask_of(pool, N, pool.device)).view(-1)
        pool = pool.reshape(-1).to(device=dev, dtype=torch.int64)
        n_pool = pool.numel()
        if n_pool and (int(pool.min()) < 0 or int(pool.max()) >= N):
            raise ValueError(f"pool has entries outside [0, {N})")
        if n_pool and torch.unique(pool).numel() != n_pool:
            raise ValueError("pool names a node twice")
        pool = pool.to(torch.int32).contiguous()
    if n_pool < 1:
        raise ValueError("the seed pool is empty")
    plan = types.SimpleNamespace(base=base, sizes=sizes, batch_size=int(batch_size), pool=pool, n_pool=n_pool,
                                 num_batches=-(-n_pool // int(batch_size)), host_base=None)
    if dev.type != "cuda":
        plan.host_base = _csr_host(base)
    return plan


def _positions(plan, step):
    """(epoch, first, count) of batch `step`"""
    e, i = divmod(int(step), plan.num_batches)
    first = i * plan.batch_size
    return e, first, min(plan.batch_size, plan.n_pool - first)


# ---- the host restatement --------------------------------------------------------------------------------------------------

def seeds_host(plan, seed, step):
    """seeds on the host, bit for bit: int32 tensor on the CPU"""
    e, first, count = _positions(plan, step)
    at = _permute(np.arange(first, first + count, dtype=np.uint64), plan.n_pool,
                  _round_keys(_u64(seed) ^ STREAM, e, _SEED_GROUP))
    if plan.pool is not None:
        at = plan.pool.cpu().numpy().astype(np.int64)[at]
    return torch.from_numpy(at.astype(np.int32))


def sampled_positions_host(rowptr, v, hop, fanout, seed, step):
    """the base positions node v draws at hop `hop` under `fanout`, ascending (int64 array)"""
    rs, deg = int(rowptr[v]), int(rowptr[v + 1] - rowptr[v])
    if fanout < 0 or deg <= fanout:
        return rs + np.arange(deg, dtype=np.int64)
    keys = _round_keys(_u64(seed) ^ STREAM, _u64(step), (int(hop) << 32) | int(v))
    return rs + np.sort(_permute(np.arange(fanout, dtype=np.uint64), deg, keys))


def neighbor_batch_host(plan, seed, step, seeds=None):
    """neighbor_batch (seeds=None) / neighbor_batch_nodes on the host for a CPU or device base: the batch of CPU tensors
    the kernels write on the device, bit for bit"""
    base = plan.base
    rowptr, col = plan.host_base if plan.host_base is not None else _csr_host(base)
    N = base.num_nodes
    s0 = seeds_host(plan, seed, step) if seeds is None else torch.as_tensor(seeds).detach().cpu()
    s0 = s0.numpy().astype(np.int64).reshape(-1)
    if s0.size and (s0.min() < 0 or s0.max() >= N):
        raise ValueError(f"seeds has entries outside [0, {N})")
    hop = np.full(N, -1, dtype=np.int64)
    frontier = np.unique(s0)
    hop[frontier] = 0
    rows = {}
    for h, s in enumerate(plan.sizes):
        for v in frontier:
            rows[int(v)] = sampled_positions_host(rowptr, v, h, s, seed, step)
        drawn = np.concatenate([col[rows[int(v)]] for v in frontier]) if frontier.size else np.zeros(0, dtype=np.int64)
        frontier = np.unique(drawn[hop[drawn] < 0])
        hop[frontier] = h + 1
    orig = np.nonzero(hop >= 0)[0]
    n_sub = orig.size
    new_id = np.cumsum(hop >= 0) - 1
    empty = np.zeros(0, dtype=np.int64)
    per_row = [rows.get(int(v), empty) for v in orig]
    entry = np.concatenate(per_row) if per_row else empty
    rp = np.zeros(n_sub + 1, dtype=np.int64)
    np.cumsum([r.size for r in per_row], out=rp[1:])
    col_sub = torch.from_numpy(new_id[col[entry]].astype(np.int32))
    g = CSRGraph(torch.from_numpy(rp.astype(np.int32)), col_sub, None, torch.arange(entry.size, dtype=torch.int32), n_sub,
                 entry.size)
    g.symmetric = False
    row = np.repeat(np.arange(n_sub, dtype=np.int64), np.diff(rp))
    return SubgraphBatch(graph=g, edge_index=torch.stack([col_sub.long(), torch.from_numpy(row)]),
                         orig_node=torch.from_numpy(orig), num_nodes=n_sub,
                         base_entry=torch.from_numpy(entry.astype(np.int32)),
                         hop=torch.from_numpy(hop[orig].astype(np.int32)),
                         seed_index=torch.from_numpy(new_id[np.unique(s0)]))


# ---- the device path -------------------------------------------------------------------------------------------------------

def seeds(plan, seed, step):
    """The seeds of batch `step`: int32 on the base's device, on the current stream, no host read.  A base on the CPU
    takes the host restatement."""
    b = plan.base
    if b.device.type != "cuda":
        return seeds_host(plan, seed, step)
    e, first, count = _positions(plan, step)
    out = torch.empty(count, dtype=torch.int32, device=b.device)
    with torch.cuda.device(b.device):
        check(_lib_neighbor.lib().mp_nbr_seeds(ptr(plan.pool), plan.n_pool, first, count, _u64(seed), e, ptr(out),
                                               _stream()), "mp_nbr_seeds")
    return out


def neighbor_batch(plan, seed, step):
    """The batch of step `step`: its seeds (seeds(plan, seed, step): distinct, as the pool's entries are) and their sampled
    tree, on the current stream with L + 1 host reads.  A base on the CPU takes the host restatement."""
    b = plan.base
    if b.device.type != "cuda":
        return neighbor_batch_host(plan, seed, step)
    with torch.cuda.device(b.device):
        s0 = seeds(plan, seed, step)
        bitmap, _ = _seed_bitmap(s0, b.num_nodes)
        return _expand(plan, s0, bitmap, seed, step)


def neighbor_batch_nodes(plan, seeds, seed, step):
    """The sampled tree of the caller's own seeds (an integer tensor; repeats allowed, an entry outside [0, N) raises
    ValueError), under the draws of (seed, step): L + 2 host reads.  A base on the CPU takes the host restatement."""
    b = plan.base
    if b.device.type != "cuda":
        return neighbor_batch_host(plan, seed, step, seeds)
    N = b.num_nodes
    v = torch.as_tensor(seeds).to(device=b.device, dtype=torch.int32).contiguous().view(-1)
    with torch.cuda.device(b.device):
        bitmap, above = _seed_bitmap(v, N)
        rank = _rank(bitmap)
        below = (v < 0).any().to(torch.int32).view(1)                   # (mp_bitmap_mark skips these: here they are errors)
        n0, above, below = torch.cat([rank[-1:], above, below]).tolist()   # host read: the distinct seeds, the range flags
        if above or below:
            raise ValueError(f"seeds has entries outside [0, {N})")
        return _expand(plan, _node_list(bitmap, rank, n0)[:n0], bitmap, seed, step)


def _seed_bitmap(v, N):
    """(bitmap [W] int32 words, flag [1]: an entry at or above N was met) of the seed list v: zero and mp_bitmap_mark"""
    W = (N + 31) // 32
    words = torch.zeros(W + 1, dtype=torch.int32, device=v.device)               # the bitmap and, behind it, the flag
    check(_lib_neighbor.lib().mp_bitmap_mark(ptr(v), v.numel(), N, ptr(words), ptr(words[W:]), _stream()),
          "mp_bitmap_mark")
    return words[:W], words[W:]


def _rank(bitmap):
    """word_rank [W + 1] int32 of a bitmap: mp_bitmap_word_counts and one cumsum"""
    W = bitmap.numel()
    rank = torch.zeros(W + 1, dtype=torch.int32, device=bitmap.device)
    counts = torch.empty(max(W, 1), dtype=torch.int32, device=bitmap.device)
    check(_lib_neighbor.lib().mp_bitmap_word_counts(ptr(bitmap), W, ptr(counts), _stream()), "mp_bitmap_word_counts")
    if W:
        torch.cumsum(counts[:W], 0, dtype=torch.int32, out=rank[1:])
    return rank


def _expand(plan, frontier, bitmap, seed, step):
    """the hops from a frontier of distinct seeds whose bitmap is `bitmap`"""
    b, sizes, lib, st = plan.base, plan.sizes, _lib_neighbor.lib(), _stream()
    dev, N, L = b.device, b.num_nodes, len(plan.sizes)
    sd, sp = _u64(seed), _u64(step)
    frontiers = [frontier]
    for h, s in enumerate(sizes):
        f = frontiers[h]
        before = bitmap.clone() if h + 1 < L else None
        check(lib.mp_nbr_mark(ptr(b.rowptr), ptr(b.col), N, b.nnz, ptr(f), f.numel(), h, s, sd, sp, ptr(bitmap), st),
              "mp_nbr_mark")
        if before is not None:                                          # the next frontier: what this hop added
            new = bitmap & ~before
            rank = _rank(new)
            n_new = int(rank[-1].item())                                # host read: one per inner hop
            frontiers.append(_node_list(new, rank, n_new)[:n_new])
    rank = _rank(bitmap)
    n_sub = int(rank[-1].item())                                        # host read: n_sub
    orig = _node_list(bitmap, rank, n_sub)
    cnt = torch.zeros(max(n_sub, 1), dtype=torch.int32, device=dev)
    hop = torch.full((max(n_sub, 1),), L, dtype=torch.int32, device=dev)
    for h, f in enumerate(frontiers):
        check(lib.mp_nbr_count(ptr(b.rowptr), N, ptr(f), f.numel(), h, sizes[h], ptr(bitmap), ptr(rank), ptr(cnt),
                               ptr(hop), st), "mp_nbr_count")
    rowptr = torch.zeros(n_sub + 1, dtype=torch.int32, device=dev)
    if n_sub:
        torch.cumsum(cnt[:n_sub], 0, dtype=torch.int32, out=rowptr[1:])
    nnz = int(rowptr[n_sub].item())                                     # host read: nnz
    col = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
    entry = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
    for h, f in enumerate(frontiers):
        check(lib.mp_nbr_fill(ptr(b.rowptr), ptr(b.col), N, b.nnz, ptr(f), f.numel(), h, sizes[h], sd, sp, ptr(bitmap),
                              ptr(rank), ptr(rowptr), ptr(col), ptr(entry), st), "mp_nbr_fill")
    g = CSRGraph(rowptr, col[:nnz], None, torch.arange(nnz, dtype=torch.int32, device=dev), n_sub, nnz)
    g.symmetric = False
    orig = orig[:n_sub].long()
    seed_index = torch.searchsorted(orig, frontier.long()).sort().values   # (orig ascends and holds every seed)
    return SubgraphBatch(graph=g, edge_index=torch.stack([g.col.long(), g.row_ids().long()]), orig_node=orig,
                         num_nodes=n_sub, base_entry=entry[:nnz], hop=hop[:n_sub], seed_index=seed_index)


# ---- the loader ------------------------------------------------------------------------------------------------------------

class NeighborLoader:
    """One epoch of neighbour-sampled batches of `base` as harness.Batch objects shaped like samplers.SubgraphLoader's:
    node_feature = x[orig_node], node_label = y[orig_node], node_label_index = seed_index (the loss is on the seeds),
    edge_index, orig_node, base_entry, hop, num_nodes.  `plan` is plan_neighbor's; its pool is replaced by the split's
    nodes (label_index_mask: a bool mask [N] or an index list).  len() = ceil(n_pool / batch_size); batch i of epoch e
    (the e-th iteration over the loader, or set_epoch(e)) is step e * len + i of `seed`.  The batch's graph is not its
    own transpose, so it is not seeded into the graph cache: the layers build their CSR from edge_index."""

    def __init__(self, base, x, y, label_index_mask, plan, seed=0):
        pool = torch.nonzero(_mask_of(label_index_mask, base.num_nodes, base.device)).view(-1)
        self.base, self.x, self.y, self.seed = base, x, y, int(seed)
        self.plan = plan_neighbor(base, plan.sizes, plan.batch_size, pool)
        self.sizes = self.plan.sizes
        self.epoch = 0

    def __len__(self):
        return self.plan.num_batches

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def batch(self, step):
        from .harness import Batch
        from .ops import gather_rows
        sb = neighbor_batch(self.plan, self.seed, step)
        orig = sb.orig_node
        on_engine = self.x.is_cuda and self.x.dim() == 2 and self.x.dtype in (torch.float32, torch.bfloat16)
        x = gather_rows(self.x, orig) if on_engine else self.x[orig]          # (integer codes: torch's gather)
        return Batch(node_feature=x, node_label=self.y[orig], node_label_index=sb.seed_index, edge_index=sb.edge_index,
                     orig_node=orig, base_entry=sb.base_entry, hop=sb.hop, num_nodes=sb.num_nodes)

    def __iter__(self):
        e = self.epoch
        self.epoch += 1
        for i in range(len(self)):
            yield self.batch(e * len(self) + i)
