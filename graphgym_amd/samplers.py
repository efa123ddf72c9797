"""Mini-batch subgraph samplers on the device (csrc/sample.hip): cfg.train.sampler / cfg.val.sampler of
graphgym/config.py:215,242-248,261 as graphgym/loader_pyg.py:204-255 hands them to PyG — random_node, saint_node,
saint_edge, saint_rw.  The four are one operation with different draws: pick a node set, then take the induced subgraph.

    plan = plan_sampler(base, "saint_rw", batch_size=cfg.train.batch_size, walk_length=cfg.train.walk_length)
    batch = sample_batch(plan, seed, step)               # SubgraphBatch: graph, edge_index, orig_node, base_entry
    loader = SubgraphLoader(base, x, y, train_mask, plan, seed)          # yields harness.Batch objects
    loader = loader_from_cfg(cfg, base, x, y, train_mask, "train")

The draws (one thread per draw; `key` and `mulhi` below restate sample.hip's integers):
    random_node  part[v] = mulhi(key(seed, epoch, v, 0), P); batch p of an epoch = the nodes with part == p, so the P
                 batches of an epoch partition the nodes (step = epoch * P + p)
    saint_node   batch_size draws i: entry e = mulhi(key(seed, step, i, 0), nnz), the node is the row that holds e:
                 P(node) proportional to its stored in-degree
    saint_rw     batch_size walks of walk_length steps from roots mulhi(key(.., i, 0), N); step t moves to entry
                 mulhi(key(.., i, t), deg) of the current node's row of the walk graph; a node without one stays
    saint_edge   batch_size walks of ONE step from the rows with at least one entry (n' of them): on a symmetric base
                 without repeated entries the unordered edge {u, v} is drawn with probability
                 (1 / n') (1 / deg u + 1 / deg v) — GraphSAINT's edge distribution, in integers
A base that is not its own transpose is walked over base.transpose() (follow out-edges), as ego.ego_batch does.

These are the project's own samplers.  PyG's RandomNodeSampler and GraphSAINT*Sampler were not available to compare
against and their draws (torch's generator, a C++ random walk) are not matched [3P-unverified]; in particular PyG's
edge sampler draws WITHOUT replacement by a float top-k, ours draws with replacement from the same marginal
distribution, and GraphSAINT's sample_coverage normalisation (which the reference passes as 0) is not built.

The node set is a bitmap of N bits; its ascending list and the new ids come from the per-word ranks (sample.hip), and
the induced subgraph is written in the engine's CSR order from the selected rows only (mp_induced_count /
mp_induced_fill): work follows the batch, not the base.  sample_nodes_host / induced_subgraph_host restate the kernels
in NumPy integers: the test oracle, and the path of a base that lives on the CPU."""
import types

import numpy as np
import torch

from ._lib import check, lib, ptr
from .graph import CSRGraph, _stream
from .link_pred import _GOLDEN, _M64, _is_symmetric_host, host_csr

KINDS = ("random_node", "saint_node", "saint_edge", "saint_rw")
_I32_MAX = 2 ** 31 - 1


# ---- the integers of csrc/sample.hip on the host ------------------------------------------------------------------------

def _mix64(z):
    """draws.h mix64 on a uint64 array (wrapping arithmetic)"""
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def key(seed, offset, i, t):
    """key(seed, offset, i, t) of sample.hip: uint64 array over the broadcast of i and t"""
    g = np.uint64(_GOLDEN)
    i, t = np.asarray(i).astype(np.uint64), np.asarray(t).astype(np.uint64)
    with np.errstate(over="ignore"):
        h = _mix64(np.asarray(int(seed) & _M64, dtype=np.uint64) + g)
        h = _mix64((h ^ np.uint64(int(offset) & _M64)) + g)
        h = _mix64((h ^ i) + g)
        return _mix64((h ^ t) + g)


def mulhi(k, n):
    """the high 64 bits of k * n for a uint64 array k and bounds n < 2^32 (a scalar or an array): the bounded draw"""
    n = np.asarray(n).astype(np.uint64)
    assert (n < np.uint64(1 << 32)).all()
    hi, lo = k >> np.uint64(32), k & np.uint64(0xFFFFFFFF)
    return ((hi * n + ((lo * n) >> np.uint64(32))) >> np.uint64(32)).astype(np.int64)


def _csr_host(g):
    return (g.rowptr.detach().cpu().numpy().astype(np.int64), g.col.detach().cpu().numpy().astype(np.int64)[:g.nnz])


def sample_nodes_host(plan, seed, step):
    """sample_nodes on the host, bit for bit: int32 tensor on the CPU (NumPy integers, no device)"""
    N, K = plan.base.num_nodes, plan.batch_size
    if plan.kind == "random_node":
        P = plan.num_parts
        part = mulhi(key(seed, step // P, np.arange(N), 0), P)
        return torch.from_numpy(np.nonzero(part == step % P)[0].astype(np.int32))
    i = np.arange(K)
    if plan.kind == "saint_node":
        rowptr, _ = plan.host_base
        e = mulhi(key(seed, step, i, 0), plan.base.nnz)
        return torch.from_numpy((np.searchsorted(rowptr, e, side="right") - 1).astype(np.int32))
    rowptr, col = plan.host_walk
    L = plan.walk_length
    out = np.empty((K, L + 1), dtype=np.int64)
    if plan.pool is None:
        cur = mulhi(key(seed, step, i, 0), N)
    else:
        pool = plan.pool.cpu().numpy().astype(np.int64)
        cur = pool[mulhi(key(seed, step, i, 0), pool.size)]
    out[:, 0] = cur
    colp = np.concatenate([col, np.zeros(1, dtype=np.int64)])               # (a readable slot behind the last entry)
    for t in range(1, L + 1):
        rs = rowptr[cur]
        deg = rowptr[cur + 1] - rs
        nxt = colp[rs + mulhi(key(seed, step, i, t), deg)]                  # (deg 0: mulhi gives 0, the value is unused)
        cur = np.where(deg > 0, nxt, cur)
        out[:, t] = cur
    return torch.from_numpy(out.reshape(-1).astype(np.int32))


def induced_subgraph_host(base, nodes, symmetric=None):
    """induced_subgraph on the host for a CPU (or device) base and any integer tensor of nodes (repeats allowed, entries
    below 0 skipped): the SubgraphBatch of CPU tensors that mp_bitmap_* / mp_induced_* write on the device, bit for bit"""
    rowptr, col = _csr_host(base)
    N = base.num_nodes
    v = torch.as_tensor(nodes).detach().cpu().numpy().astype(np.int64).reshape(-1)
    v = v[v >= 0]
    if v.size and v.max() >= N:
        raise ValueError(f"nodes has entries outside [0, {N})")
    member = np.zeros(N, dtype=bool)
    member[v] = True
    orig = np.nonzero(member)[0]
    new_id = np.cumsum(member) - 1
    row = np.repeat(np.arange(N, dtype=np.int64), np.diff(rowptr))
    e = np.nonzero(member[row] & member[col])[0]                            # ascending: the base's CSR order
    n_sub = orig.size
    rp = np.zeros(n_sub + 1, dtype=np.int64)
    np.cumsum(np.bincount(new_id[row[e]], minlength=n_sub)[:n_sub], out=rp[1:])
    col_sub = torch.from_numpy(new_id[col[e]].astype(np.int32))
    g = CSRGraph(torch.from_numpy(rp.astype(np.int32)), col_sub, None, torch.arange(e.size, dtype=torch.int32), n_sub,
                 e.size)
    if symmetric is None:
        symmetric = base.nnz == 0 or (base.is_symmetric() if base.rowptr.is_cuda else _is_symmetric_host(base))
    g.symmetric = bool(symmetric)
    ei = torch.stack([col_sub.long(), torch.from_numpy(new_id[row[e]])])
    return SubgraphBatch(graph=g, edge_index=ei, orig_node=torch.from_numpy(orig), num_nodes=n_sub,
                         base_entry=torch.from_numpy(e.astype(np.int32)))


# ---- plans ---------------------------------------------------------------------------------------------------------------

class SubgraphBatch(types.SimpleNamespace):
    """graph (CSRGraph of the induced subgraph, eid = arange(nnz)), edge_index [2, nnz] int64 (PyG convention, in CSR
    order), orig_node [n_sub] int64 ascending, base_entry [nnz] int32 (position in the base CSR), num_nodes"""


def plan_sampler(base, kind, batch_size=None, walk_length=None, num_parts=None):
    """What the draws of `kind` need, computed once per base: its symmetry (base.is_symmetric(run=True); cached on the
    base), the walk graph (the base, or base.transpose() when it is not its own transpose) and, for saint_edge, the pool
    of rows with at least one entry.  ValueError: an unknown kind, batch_size < 1 (saint_*), num_parts < 1
    (random_node: cfg.train.train_parts has no default), walk_length < 0, an empty base for saint_*.  A base on the CPU
    gives a plan for the host restatements."""
    if kind not in KINDS:
        raise ValueError(f"kind must be one of {KINDS}, got {kind!r}")
    N, dev = base.num_nodes, base.rowptr.device
    if N >= _I32_MAX:
        raise ValueError("plan_sampler: a graph must hold fewer than 2^31 nodes")
    plan = types.SimpleNamespace(base=base, kind=kind, batch_size=None, walk_length=None, num_parts=None, pool=None,
                                 walk=None, host_base=None, host_walk=None)
    on_dev = dev.type == "cuda"
    if kind == "random_node":
        if num_parts is None:
            raise ValueError("random_node needs num_parts (cfg.train.train_parts, which has no default)")
        if int(num_parts) < 1:
            raise ValueError("num_parts must be at least 1")
        plan.num_parts = int(num_parts)
    else:
        if batch_size is None or int(batch_size) < 1:
            raise ValueError("batch_size must be at least 1")
        if N == 0 or base.nnz == 0:
            raise ValueError(f"{kind} needs a base with at least one stored entry")
        plan.batch_size = int(batch_size)
    if base.nnz == 0:
        plan.symmetric = True
    else:
        plan.symmetric = base.is_symmetric(run=True) if on_dev else _is_symmetric_host(base)
    plan.loop_free = not (base.has_self_loops() if on_dev else _has_loops_host(base))
    if kind in ("saint_rw", "saint_edge"):
        plan.walk_length = 1 if kind == "saint_edge" else int(4 if walk_length is None else walk_length)
        if plan.walk_length < 0:
            raise ValueError("walk_length must not be negative")
        plan.walk = base if plan.symmetric else (base.transpose() if on_dev else _transpose_host(base))
        if kind == "saint_edge":
            rp = plan.walk.rowptr
            plan.pool = torch.nonzero(rp[1:] > rp[:-1]).view(-1).to(torch.int32).contiguous()
    if not on_dev:
        plan.host_base = _csr_host(base)
        plan.host_walk = None if plan.walk is None else _csr_host(plan.walk)
    return plan


def _has_loops_host(base):
    rowptr, col = _csr_host(base)
    return bool((np.repeat(np.arange(base.num_nodes), np.diff(rowptr)) == col).any())


def _transpose_host(base):
    rowptr, col = _csr_host(base)
    row = np.repeat(np.arange(base.num_nodes, dtype=np.int64), np.diff(rowptr))
    return host_csr(torch.from_numpy(np.stack([row, col])), base.num_nodes)     # (entry (r, c) becomes (c, r))


def _u64(v):
    return int(v) & _M64


def _parts(plan, seed, epoch):
    b = plan.base
    part = torch.empty(b.num_nodes, dtype=torch.int32, device=b.device)
    check(lib().mp_sample_parts(b.num_nodes, plan.num_parts, _u64(seed), _u64(epoch), ptr(part), _stream()),
          "mp_sample_parts")
    return part


def sample_nodes(plan, seed, step):
    """The nodes batch `step` draws, before deduplication: int32 on the base's device, on the current stream.  saint_node:
    [batch_size]; saint_rw / saint_edge: [batch_size * (walk_length + 1)], walk after walk; random_node: the ascending
    nodes of part step % num_parts of epoch step // num_parts (a torch.nonzero: one host read; sample_batch avoids it).
    A base on the CPU takes the host restatement."""
    b = plan.base
    if b.device.type != "cuda":
        return sample_nodes_host(plan, seed, step)
    with torch.cuda.device(b.device):
        if plan.kind == "random_node":
            part = _parts(plan, seed, step // plan.num_parts)
            return torch.nonzero(part == step % plan.num_parts).view(-1).to(torch.int32)
        return _draw(plan, seed, step)


def _draw(plan, seed, step):
    b, K = plan.base, plan.batch_size
    if plan.kind == "saint_node":
        out = torch.empty(K, dtype=torch.int32, device=b.device)
        check(lib().mp_sample_entry_rows(ptr(b.rowptr), b.num_nodes, b.nnz, K, _u64(seed), _u64(step), ptr(out),
                                         _stream()), "mp_sample_entry_rows")
        return out
    w, L = plan.walk, plan.walk_length
    out = torch.empty(K * (L + 1), dtype=torch.int32, device=b.device)
    n_pool = 0 if plan.pool is None else plan.pool.numel()
    check(lib().mp_sample_walks(ptr(w.rowptr), ptr(w.col), w.num_nodes, w.nnz, ptr(plan.pool), n_pool, K, L, _u64(seed),
                                _u64(step), ptr(out), _stream()), "mp_sample_walks")
    return out


# ---- node set -> induced subgraph ------------------------------------------------------------------------------------------

def induced_subgraph(base, nodes, symmetric=None):
    """The subgraph of `base` (CSRGraph, row r = in-edges of r, columns ascending) induced by the node set of `nodes`
    (integer tensor on the device; repeats allowed, entries below 0 are no draw and are skipped, entries >= N raise
    ValueError), as a SubgraphBatch: node k of the batch is base node orig_node[k] (ascending), graph is what
    CSRGraph.from_edge_index(edge_index, n_sub) builds, entry for entry (eid = arange), written directly in CSR order
    from the selected rows; self entries and repeated entries of the base are kept as stored.  graph.symmetric is set
    when the base is known to equal its transpose (symmetric=None asks base.is_symmetric(), which never runs a check).
    Two host reads (n_sub with the range flag, nnz_sub), everything on the current stream.  A base on the CPU takes the
    host restatement."""
    if base.device.type != "cuda":
        return induced_subgraph_host(base, nodes, symmetric)
    dev, N = base.device, base.num_nodes
    v = nodes.to(device=dev, dtype=torch.int32).contiguous().view(-1)
    with torch.cuda.device(dev):
        bitmap, rank = _node_bitmap(v, N)
        n_sub, bad = rank[-2:].tolist()                                           # host read 1
        if bad:
            raise ValueError(f"nodes has entries outside [0, {N})")
        orig = _node_list(bitmap, rank, n_sub)
        rowptr = _count_rows(base, orig, n_sub, bitmap)
        nnz = int(rowptr[n_sub].item())                                           # host read 2
        col, entry = _fill_rows(base, orig, n_sub, bitmap, rank, rowptr, nnz)
        g = CSRGraph(rowptr, col, None, torch.arange(nnz, dtype=torch.int32, device=dev), n_sub, nnz)
        g.symmetric = bool(base.nnz == 0 or base.is_symmetric()) if symmetric is None else bool(symmetric)
        ei = torch.stack([g.col.long(), g.row_ids().long()])
    return SubgraphBatch(graph=g, edge_index=ei, orig_node=orig[:n_sub].long(), base_entry=entry, num_nodes=n_sub)


def _node_bitmap(v, N):
    """(bitmap [W] int32 words, rank [W + 2] int32: word_rank [W + 1] and, behind it, the out-of-range flag) of the node
    list v (int32, device): zero, mp_bitmap_mark, mp_bitmap_word_counts, one cumsum.  No host read."""
    L, dev, W, st = lib(), v.device, (N + 31) // 32, _stream()
    words = torch.zeros(W + 1, dtype=torch.int32, device=dev)                     # the bitmap and, behind it, the flag
    bitmap, flag = words[:W], words[W:]
    check(L.mp_bitmap_mark(ptr(v), v.numel(), N, ptr(bitmap), ptr(flag), st), "mp_bitmap_mark")
    rank = torch.zeros(W + 2, dtype=torch.int32, device=dev)
    counts = torch.empty(max(W, 1), dtype=torch.int32, device=dev)
    check(L.mp_bitmap_word_counts(ptr(bitmap), W, ptr(counts), st), "mp_bitmap_word_counts")
    if W:
        torch.cumsum(counts[:W], 0, dtype=torch.int32, out=rank[1:W + 1])
    rank[W + 1:].copy_(flag)
    return bitmap, rank


def _node_list(bitmap, rank, n_sub):
    """orig [max(n_sub, 1)] int32: the set bits in ascending order (mp_bitmap_nodes)"""
    orig = torch.empty(max(n_sub, 1), dtype=torch.int32, device=bitmap.device)
    if n_sub:
        check(lib().mp_bitmap_nodes(ptr(bitmap), ptr(rank), bitmap.numel(), ptr(orig), _stream()), "mp_bitmap_nodes")
    return orig


def _count_rows(base, orig, n_sub, bitmap):
    """rowptr_sub [n_sub + 1] int32: mp_induced_count and one cumsum"""
    dev = base.device
    cnt = torch.empty(max(n_sub, 1), dtype=torch.int32, device=dev)
    check(lib().mp_induced_count(ptr(base.rowptr), ptr(base.col), base.num_nodes, base.nnz, ptr(orig), n_sub,
                                 ptr(bitmap), ptr(cnt), _stream()), "mp_induced_count")
    rowptr = torch.zeros(n_sub + 1, dtype=torch.int32, device=dev)
    if n_sub:
        torch.cumsum(cnt[:n_sub], 0, dtype=torch.int32, out=rowptr[1:])
    return rowptr


def _fill_rows(base, orig, n_sub, bitmap, rank, rowptr, nnz):
    """(col_sub [nnz], base_entry [nnz]) int32: mp_induced_fill"""
    dev = base.device
    col = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
    entry = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
    check(lib().mp_induced_fill(ptr(base.rowptr), ptr(base.col), base.num_nodes, base.nnz, ptr(orig), n_sub,
                                ptr(bitmap), ptr(rank), ptr(rowptr), ptr(col), ptr(entry), _stream()),
          "mp_induced_fill")
    return col[:nnz], entry[:nnz]


def sample_batch(plan, seed, step):
    """induced_subgraph(plan.base, the nodes batch `step` draws): the draw, the bitmap, the ascending node list and the
    two passes over the selected rows, all on the current stream with TWO host reads (n_sub, nnz_sub) — random_node hands
    its part to the bitmap as a masked list (the nodes of other parts as -1) instead of a torch.nonzero."""
    b = plan.base
    if b.device.type != "cuda":
        return induced_subgraph_host(b, sample_nodes_host(plan, seed, step), plan.symmetric)
    with torch.cuda.device(b.device):
        return induced_subgraph(b, _draw_for_bitmap(plan, seed, step), plan.symmetric)


def _draw_for_bitmap(plan, seed, step):
    """the batch's draw as mp_bitmap_mark takes it, without a host read: random_node as a masked list"""
    if plan.kind != "random_node":
        return _draw(plan, seed, step)
    b = plan.base
    part = _parts(plan, seed, step // plan.num_parts)
    ids = torch.arange(b.num_nodes, dtype=torch.int32, device=b.device)
    return torch.where(part == step % plan.num_parts, ids, torch.full_like(ids, -1))


# ---- loaders ---------------------------------------------------------------------------------------------------------------

def _mask_of(label_index_mask, N, dev):
    """bool [N] from a bool mask or an index list"""
    m = torch.as_tensor(label_index_mask).to(dev)
    if m.dtype == torch.bool:
        if m.numel() != N:
            raise ValueError(f"the split mask must hold one entry per node: {m.numel()} for {N} nodes")
        return m
    mask = torch.zeros(N, dtype=torch.bool, device=dev)
    mask[m.long()] = True
    return mask


class SubgraphLoader:
    """One epoch of sampled batches of `base` as harness.Batch objects: node_feature = x[orig_node], node_label =
    y[orig_node], node_label_index = the batch positions whose base node is in the split (label_index_mask: a bool mask
    [N] or an index list), edge_index, orig_node, and — when the base is symmetric and stores no self entry, which
    layers.seed_graph_cache's contract asks for — the batch's CSRGraph seeded into its graph cache, so no layer sorts
    the edge list again.  len() is iter_per_epoch for saint_* and num_parts for random_node; batch i of epoch e (the
    e-th iteration over the loader, or set_epoch(e)) is step e * len + i of `seed`.  One host read per batch on top of
    sample_batch's two (the size of node_label_index)."""

    def __init__(self, base, x, y, label_index_mask, plan, seed=0, iter_per_epoch=32):
        self.base, self.x, self.y, self.plan, self.seed = base, x, y, plan, int(seed)
        self.mask = _mask_of(label_index_mask, base.num_nodes, base.device)
        self.n = plan.num_parts if plan.kind == "random_node" else int(iter_per_epoch)
        if self.n < 1:
            raise ValueError("iter_per_epoch must be at least 1")
        self.epoch = 0

    def __len__(self):
        return self.n

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def batch(self, step):
        from .harness import Batch
        from .layers import seed_graph_cache
        from .ops import gather_rows
        sb = sample_batch(self.plan, self.seed, step)
        orig = sb.orig_node
        on_engine = self.x.is_cuda and self.x.dim() == 2 and self.x.dtype in (torch.float32, torch.bfloat16)
        x = gather_rows(self.x, orig) if on_engine else self.x[orig]          # (integer codes: torch's gather)
        out = Batch(node_feature=x, node_label=self.y[orig], node_label_index=torch.nonzero(self.mask[orig]).view(-1),
                    edge_index=sb.edge_index, orig_node=orig, base_entry=sb.base_entry, num_nodes=sb.num_nodes)
        if sb.graph.symmetric and self.plan.loop_free and sb.graph.device.type == "cuda":
            seed_graph_cache(out, sb.edge_index, sb.num_nodes, sb.graph, "none")
        return out

    def __iter__(self):
        e = self.epoch
        self.epoch += 1
        for i in range(self.n):
            yield self.batch(e * self.n + i)


class FullBatchLoader:
    """train.sampler / val.sampler = 'full_batch' on one graph: a single batch, the base itself (its CSRGraph seeded
    into the batch when it is symmetric and stores no self entry); every iteration yields a fresh Batch over the same
    tensors and the same graph cache"""

    def __init__(self, base, x, y, label_index_mask):
        from .harness import Batch
        from .layers import seed_graph_cache
        mask = _mask_of(label_index_mask, base.num_nodes, base.device)
        rp = base.rowptr.long()
        row = torch.repeat_interleave(torch.arange(base.num_nodes, device=base.device), rp[1:] - rp[:-1])
        ei = torch.stack([base.col.long()[:base.nnz], row])
        self.base = base
        self.only = Batch(node_feature=x, node_label=y, node_label_index=torch.nonzero(mask).view(-1), edge_index=ei,
                          num_nodes=base.num_nodes)
        if base.device.type == "cuda" and base.nnz and base.is_symmetric(run=True) and not base.has_self_loops():
            g = base
            if g.eid is None or not bool((g.eid == torch.arange(g.nnz, dtype=torch.int32, device=g.device)).all()):
                g = base.with_values(base.val)                # (edge_index above is in CSR order: eid = arange)
                g.symmetric = True
                g.eid = torch.arange(base.nnz, dtype=torch.int32, device=base.device)
            seed_graph_cache(self.only, ei, base.num_nodes, g, "none")

    def __len__(self):
        return 1

    def __iter__(self):
        from .harness import Batch
        yield Batch(**vars(self.only))      # (a model's forward replaces node_feature on the batch it is given)


def loader_from_cfg(cfg, base, x, y, label_index_mask, split="train", seed=0):
    """The loader of graphgym/loader_pyg.py:204-255 for one graph: cfg.train.sampler for split 'train', cfg.val.sampler
    for every other split.  full_batch: the whole graph; random_node (cfg.train.train_parts — no default: ValueError
    without it), saint_node / saint_edge / saint_rw (cfg.train.batch_size, walk_length, iter_per_epoch): a
    SubgraphLoader.  neighbor_subgraph (the project's own name, graphgym_amd/neighbor.py): a NeighborLoader over the
    split's nodes with the fanouts cfg.train.neighbor_sizes[:cfg.gnn.layers_mp] and cfg.train.batch_size seeds a batch.
    neighbor (PyG's per-layer bipartite blocks) and cluster raise NotImplementedError with the reason; any other name
    raises the reference's NotImplementedError."""
    tr = cfg.train
    sampler = tr.sampler if split == "train" else cfg.val.sampler
    if sampler == "full_batch":
        return FullBatchLoader(base, x, y, label_index_mask)
    if sampler == "neighbor":
        raise NotImplementedError("neighbor sampler is not implemented: PyG's NeighborSampler yields per-layer bipartite "
                                  "blocks (sizes cfg.train.neighbor_sizes), which the reference's GNN.forward does not "
                                  "consume either")
    if sampler == "cluster":
        raise NotImplementedError("cluster sampler is not implemented: ClusterLoader needs a METIS partition of the base")
    if sampler == "neighbor_subgraph":
        from .neighbor import NeighborLoader, plan_neighbor
        sizes = list(tr.neighbor_sizes)[:cfg.gnn.layers_mp]
        return NeighborLoader(base, x, y, label_index_mask, plan_neighbor(base, sizes, tr.batch_size), seed)
    if sampler not in KINDS:
        raise NotImplementedError("%s sampler is not implemented!" % sampler)
    if sampler == "random_node":
        parts = getattr(tr, "train_parts", None)
        if parts is None:
            raise ValueError("train.sampler = random_node needs cfg.train.train_parts, which has no default")
        plan = plan_sampler(base, sampler, num_parts=parts)
    else:
        plan = plan_sampler(base, sampler, batch_size=tr.batch_size, walk_length=getattr(tr, "walk_length", 4))
    return SubgraphLoader(base, x, y, label_index_mask, plan, seed, getattr(tr, "iter_per_epoch", 32))
