"""Graph-task loaders on the device (csrc/collate.hip): dataset.task = graph of graphgym/loader.py:225-260 — the inductive
split of the dataset's graphs, the per-epoch shuffle and the per-step collation that the reference does with
DataLoader(dataset, collate_fn=Batch.collate(), batch_size=cfg.train.batch_size, shuffle=True) on the host.

    ds = GraphDataset(base, graph_ptr, x, graph_label)            # one CSRGraph: the disjoint union of G graphs
    train_ids, val_ids = split_graphs(ds.num_graphs, [0.8, 0.2], seed)
    loader = GraphLoader(ds, train_ids, batch_size=64, shuffle=True, seed=seed)       # yields harness.Batch objects
    loaders = graph_loaders_from_cfg(cfg, ds, seed)               # one per entry of cfg.dataset.split

A dataset's graphs are contiguous node ranges (graph_ptr) whose sizes the host knows, so a batch's node and entry counts
are known before anything is launched and the collation is a segmented copy with rebasing: mp_collate_graphs, one launch,
one thread per output element, no host read.  The ids and the two offset arrays go up in one non-blocking copy from pinned
memory.  collate_host restates the same integers in NumPy: the test oracle, and the path of a dataset that lives on the
CPU.  The shuffle (epoch_order) and the split (split_graphs) are keyed permutations in NumPy integers with samplers.key's
mixing: nothing depends on torch's generator.

Not served: dataset.format: OGB's shipped splits and loading real datasets — a GraphDataset is built from tensors."""
import math

import numpy as np
import torch

from ._lib import check, lib, ptr
from .graph import CSRGraph, _stream
from .link_pred import _cut, _is_symmetric_host, host_csr
from .samplers import _has_loops_host, key

_I32_MAX = 2 ** 31 - 1
_SPLIT_OFFSET = -1          # the `epoch` of the split's permutation: no epoch of a loader


def _np64(v):
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    return np.asarray(v).astype(np.int64).reshape(-1)


# ---- host integers: shuffle and split -----------------------------------------------------------------------------------

def epoch_order(ids, seed, epoch):
    """`ids` in the order of epoch `epoch`: position i is sorted by key(seed, epoch, i, 0) (a stable sort, so the order
    is a pure function of (seed, epoch) and len(ids); repeated ids are positions of their own).  int64 NumPy array."""
    ids = _np64(ids)
    return ids[np.argsort(key(seed, epoch, np.arange(ids.size), 0), kind="stable")]


def split_graphs(G, ratios, seed, shuffle=True):
    """The inductive split of dataset.split(transductive=False, split_ratio=ratios, shuffle=shuffle): len(ratios) disjoint
    id arrays that cover range(G).  The ids (shuffled by epoch_order under a key of its own when `shuffle`) are cut at
    floor(cumulative ratio * G); the last part takes the rest.  Deterministic in `seed`."""
    ratios = [float(r) for r in ratios]
    if not ratios or min(ratios) < 0:
        raise ValueError("ratios must be a non-empty list of non-negative numbers")
    ids = np.arange(int(G), dtype=np.int64)
    if shuffle:
        ids = epoch_order(ids, seed, _SPLIT_OFFSET)
    parts, at = [], 0
    for size in _cut(int(G), ratios[:-1]):
        parts.append(ids[at:at + size])
        at += size
    return parts


# ---- dataset --------------------------------------------------------------------------------------------------------------

class GraphDataset:
    """G graphs as one CSRGraph `base` (row r = in-edges of r; the disjoint union), graph g = nodes graph_ptr[g] ..
    graph_ptr[g + 1].  x [N, d]: fp32 or bf16 features, or integer codes; graph_label [G]; edge_feature [E, k], indexed
    by input edge position (base.eid).  ValueError: a graph_ptr that decreases, does not start at 0 or does not end at
    base.num_nodes, or a stored entry that joins two graphs (one pass over the entries at construction: mp_collate_check_
    entries, or NumPy for a base on the CPU; the message names the first such entry).

    Kept on the host: graph_ptr and entry_ptr = rowptr[graph_ptr] as int64 arrays — all a batch needs to know its sizes.
    `seedable` is decided once (base.is_symmetric(run=True) and not base.has_self_loops()): the batches of a symmetric,
    loop-free dataset hand their CSRGraph to the layers' graph cache."""

    def __init__(self, base, graph_ptr, x, graph_label, edge_feature=None):
        gp = _np64(graph_ptr)
        N = base.num_nodes
        if gp.size < 1 or gp[0] != 0 or gp[-1] != N:
            raise ValueError(f"graph_ptr must start at 0 and end at the number of nodes ({N})")
        if (np.diff(gp) < 0).any():
            raise ValueError("graph_ptr must not decrease")
        if N >= _I32_MAX or base.nnz >= _I32_MAX:
            raise ValueError("a dataset must hold fewer than 2^31 - 1 nodes and entries")
        self.base, self.x, self.graph_label, self.edge_feature = base, x, graph_label, edge_feature
        self.graph_ptr, self.num_graphs = gp, gp.size - 1
        self.device = base.device
        self.on_device = self.device.type == "cuda"
        if x.size(0) != N or graph_label.size(0) != self.num_graphs:
            raise ValueError("x holds one row per node and graph_label one entry per graph")
        self._host = None
        if self.on_device:
            with torch.cuda.device(self.device):
                self.graph_ptr_dev = torch.from_numpy(gp).to(self.device)
                self.entry_ptr = base.rowptr.long()[self.graph_ptr_dev].cpu().numpy()
                self._check_entries_device()
                self.symmetric = base.nnz == 0 or base.is_symmetric(run=True)
                self.seedable = bool(self.symmetric and not base.has_self_loops())
                self._iota_buf = torch.arange(1024, dtype=torch.int32, device=self.device)
        else:
            rowptr, col, _ = self.host_base()
            self.entry_ptr = rowptr[gp]
            row = np.repeat(np.arange(N, dtype=np.int64), np.diff(rowptr))
            owner = np.searchsorted(gp, row, side="right") - 1
            bad = np.nonzero((col < gp[owner]) | (col >= gp[np.minimum(owner + 1, self.num_graphs)]))[0]
            if bad.size:
                self._raise_crossing(int(bad[0]), int(row[bad[0]]), int(col[bad[0]]))
            self.symmetric = base.nnz == 0 or _is_symmetric_host(base)
            self.seedable = bool(self.symmetric and not _has_loops_host(base))
        self.ef_entry = None                  # edge_feature in the base's entry order
        if edge_feature is not None:
            eid = base.eid
            self.ef_entry = edge_feature if eid is None else edge_feature.index_select(0, eid.to(edge_feature.device))

    def _raise_crossing(self, e, r, c):
        ga, gb = (int(np.searchsorted(self.graph_ptr, v, side="right")) - 1 for v in (r, c))
        raise ValueError(f"stored entry {e} (row {r}, column {c}) joins graph {ga} and graph {gb}: a dataset is a "
                         "disjoint union of graphs")

    def _check_entries_device(self):
        b = self.base
        if b.nnz == 0:
            return
        first = torch.full((1,), _I32_MAX, dtype=torch.int32, device=self.device)
        check(lib().mp_collate_check_entries(ptr(b.col), ptr(b.row_ids()), b.nnz, ptr(self.graph_ptr_dev),
                                             self.num_graphs, ptr(first), _stream()), "mp_collate_check_entries")
        e = int(first.item())
        if e != _I32_MAX:
            self._raise_crossing(e, int(b.row_ids()[e]), int(b.col[e]))

    def host_base(self):
        """(rowptr, col, val or None) of the base as NumPy arrays (fetched once): collate_host's operands"""
        if self._host is None:
            b = self.base
            val = None if b.val is None else b.val.detach().cpu().numpy()[:b.nnz]
            self._host = (b.rowptr.detach().cpu().numpy().astype(np.int64),
                          b.col.detach().cpu().numpy().astype(np.int64)[:b.nnz], val)
        return self._host

    def iota(self, k):
        """arange(k) int32 on the device, a view of one buffer that grows by doubling: no launch per batch"""
        if k > self._iota_buf.numel():
            self._iota_buf = torch.arange(max(k, 2 * self._iota_buf.numel()), dtype=torch.int32, device=self.device)
        return self._iota_buf[:k]

    @classmethod
    def from_graphs(cls, graphs, device=None):
        """The dataset of a Python list of (edge_index [2, E_g] with local node ids, x [n_g, d], label[, edge_feature
        [E_g, k]]) tuples, concatenated once (examples and tests).  device=None keeps everything on the CPU."""
        eis, xs, labels, efs, gp = [], [], [], [], [0]
        for g in graphs:
            ei, x, label = g[0], g[1], g[2]
            eis.append(torch.as_tensor(ei).to(torch.int64).reshape(2, -1) + gp[-1])
            xs.append(torch.as_tensor(x))
            labels.append(torch.as_tensor(label))
            if len(g) > 3:
                efs.append(torch.as_tensor(g[3]))
            gp.append(gp[-1] + xs[-1].size(0))
        if efs and len(efs) != len(graphs):
            raise ValueError("either every graph carries an edge_feature or none does")
        ei, x, label = torch.cat(eis, 1), torch.cat(xs, 0), torch.stack(labels)
        ef = torch.cat(efs, 0) if efs else None
        if device is None or torch.device(device).type == "cpu":
            return cls(host_csr(ei, gp[-1]), gp, x, label, ef)
        base = CSRGraph.from_edge_index(ei.to(device), gp[-1])
        return cls(base, gp, x.to(device), label.to(device), None if ef is None else ef.to(device))


# ---- collation ------------------------------------------------------------------------------------------------------------

def _offsets(dataset, ids):
    """(ids, node_off [B + 1], entry_off [B + 1]) as int64 arrays from the dataset's host mirrors"""
    ids = _np64(ids)
    if ids.size == 0:
        raise ValueError("a batch lists at least one graph")
    if ids.min() < 0 or ids.max() >= dataset.num_graphs:
        raise ValueError(f"ids has entries outside [0, {dataset.num_graphs})")
    gp, ep = dataset.graph_ptr, dataset.entry_ptr
    node_off = np.zeros(ids.size + 1, dtype=np.int64)
    entry_off = np.zeros(ids.size + 1, dtype=np.int64)
    np.cumsum(gp[ids + 1] - gp[ids], out=node_off[1:])
    np.cumsum(ep[ids + 1] - ep[ids], out=entry_off[1:])
    if node_off[-1] >= _I32_MAX or entry_off[-1] >= _I32_MAX:
        raise ValueError("a batch must hold fewer than 2^31 - 1 nodes and entries")
    return ids, node_off, entry_off


def _features(x, orig):
    from .ops import gather_rows
    on_engine = x.is_cuda and x.dim() == 2 and x.dtype in (torch.float32, torch.bfloat16)
    return gather_rows(x, orig) if on_engine else x[orig]                # (integer codes: torch's gather)


def _pool_rows(node_off, cols, B, num_cols):
    """the operator pooling.pool_operator builds for nodes listed graph by graph: row j = columns node_off[j] ..
    node_off[j + 1] of `num_cols`"""
    return CSRGraph(node_off, cols, None, None, B, cols.numel(), num_cols)


def collate_host(dataset, ids):
    """collate on the host, bit for bit, for a dataset on either side: the harness.Batch of CPU tensors that a per-graph
    concatenation with offsets gives (and mp_collate_graphs writes on the device).  Nothing is seeded."""
    from .harness import Batch
    ids, node_off, entry_off = _offsets(dataset, ids)
    gp, ep = dataset.graph_ptr, dataset.entry_ptr
    rowptr, col, val = dataset.host_base()
    B, n, nnz = ids.size, int(node_off[-1]), int(entry_off[-1])
    owner = np.repeat(np.arange(B, dtype=np.int64), np.diff(node_off))
    orig = gp[ids][owner] + np.arange(n, dtype=np.int64) - node_off[owner]
    rp = np.empty(n + 1, dtype=np.int64)
    rp[:n] = rowptr[orig] - ep[ids][owner] + entry_off[owner]
    rp[n] = nnz
    e_owner = np.repeat(np.arange(B, dtype=np.int64), np.diff(entry_off))
    s = ep[ids][e_owner] + np.arange(nnz, dtype=np.int64) - entry_off[e_owner]
    c = col[s] - gp[ids][e_owner] + node_off[e_owner]
    r = np.repeat(np.arange(n, dtype=np.int64), np.diff(rp))
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32))          # noqa: E731
    g = CSRGraph(t32(rp), t32(c), None if val is None else torch.from_numpy(val[s]), torch.arange(nnz, dtype=torch.int32),
                 n, nnz)
    g._row_ids = t32(r)
    g.symmetric = bool(dataset.symmetric)
    orig_t, s_t = torch.from_numpy(orig), torch.from_numpy(s)
    cpu = lambda t: t.detach().cpu()                                                      # noqa: E731
    batch = Batch(node_feature=cpu(dataset.x)[orig_t], edge_index=torch.from_numpy(np.stack([c, r])),
                  batch=torch.from_numpy(owner), graph_label=cpu(dataset.graph_label)[torch.from_numpy(ids)],
                  orig_node=orig_t, base_entry=t32(s), num_nodes=n, num_graphs=B, graph=g,
                  pool_operator=_pool_rows(t32(node_off), torch.arange(n, dtype=torch.int32), B, n))
    if dataset.ef_entry is not None:
        batch.edge_feature = cpu(dataset.ef_entry)[s_t]
    return batch


def _collate_device(dataset, ids, entries=True):
    """mp_collate_graphs for `ids`: one pinned upload, one launch, no host read.  entries=False writes the node arrays
    alone (the ego transform needs the centres and their owners, not the graphs' entries)."""
    ids, node_off, entry_off = _offsets(dataset, ids)
    base, dev = dataset.base, dataset.device
    B, n = ids.size, int(node_off[-1])
    nnz = int(entry_off[-1]) if entries else 0
    with torch.cuda.device(dev):
        host = torch.empty(3 * B + 2, dtype=torch.int32, pin_memory=True)
        h = host.numpy()
        h[:B], h[B:2 * B + 1], h[2 * B + 1:] = ids, node_off, entry_off
        up = torch.empty(3 * B + 2, dtype=torch.int32, device=dev)
        up.copy_(host, non_blocking=True)
        ids_d, node_off_d, entry_off_d = up[:B], up[B:2 * B + 1], up[2 * B + 1:]
        i32 = (torch.zeros if n == 0 else torch.empty)(2 * n + 1 + 3 * nnz, dtype=torch.int32, device=dev)
        i64 = torch.empty(2 * n + 2 * nnz, dtype=torch.int64, device=dev)
        rowptr, owner32 = i32[:n + 1], i32[n + 1:2 * n + 1]
        col, row, entry = (i32[2 * n + 1 + k * nnz:2 * n + 1 + (k + 1) * nnz] for k in range(3))
        owner, orig, ei = i64[:n], i64[n:2 * n], i64[2 * n:].view(2, nnz)
        val = torch.empty(nnz, dtype=torch.float32, device=dev) if base.val is not None and entries else None
        check(lib().mp_collate_graphs(ptr(base.rowptr), ptr(base.col), ptr(base.val), base.num_nodes, base.nnz,
                                      ptr(dataset.graph_ptr_dev), dataset.num_graphs, ptr(ids_d), ptr(node_off_d),
                                      ptr(entry_off_d), B, n, nnz, ptr(rowptr), ptr(owner), ptr(owner32), ptr(orig),
                                      ptr(col), ptr(row), ptr(entry), ptr(ei), ptr(val), _stream()), "mp_collate_graphs")
    return dict(ids=ids_d, node_off=node_off_d, rowptr=rowptr, owner=owner, owner32=owner32, orig=orig, col=col, row=row,
                entry=entry, edge_index=ei, val=val, B=B, n=n, nnz=nnz)


def collate(dataset, ids):
    """The batch of the graphs `ids` (graph ids in batch order; any order, repeats allowed) as a harness.Batch:
    node_feature = x[orig_node], edge_index [2, nnz] int64 in CSR order (row 0 source, row 1 destination), batch [n]
    int64 (the batch graph of every node), graph_label = graph_label[ids], edge_feature (when the dataset has one) =
    edge_feature[base.eid[base_entry]], orig_node [n] int64, base_entry [nnz] int32 (position in the base CSR),
    num_nodes, num_graphs, graph (the batch's CSRGraph, eid = arange(nnz), values gathered when the base stores them)
    and pool_operator: the CSRGraph [B, n] pooling.pool_operator would build, written directly (rowptr = the node
    offsets, col = arange(n)) together with its transpose, so GNNGraphHead pools without a host read or a sort.

    When the dataset is `seedable`, `graph` (its pattern: the layers read edge_index without weights) is seeded into the
    batch's graph cache (layers.seed_graph_cache, "none"): no layer sorts the edge list again.  Otherwise the layers
    build their CSR from edge_index as for any batch.

    The device path makes no device-to-host read and no synchronising copy.  A dataset on the CPU takes collate_host."""
    if not dataset.on_device:
        return collate_host(dataset, ids)
    from .harness import Batch
    from .layers import seed_graph_cache
    c = _collate_device(dataset, ids)
    B, n, nnz = c["B"], c["n"], c["nnz"]
    with torch.cuda.device(dataset.device):
        g = CSRGraph(c["rowptr"], c["col"], c["val"], dataset.iota(nnz), n, nnz)
        g._row_ids = c["row"]
        g.symmetric = bool(dataset.symmetric)
        pool = _pool_rows(c["node_off"], dataset.iota(n), B, n)
        pool._t = CSRGraph(dataset.iota(n + 1), c["owner32"], None, None, n, n, B)     # one entry per node: its graph
        pool._t.pos = dataset.iota(n)
        batch = Batch(node_feature=_features(dataset.x, c["orig"]), edge_index=c["edge_index"], batch=c["owner"],
                      graph_label=dataset.graph_label.index_select(0, c["ids"]), orig_node=c["orig"],
                      base_entry=c["entry"], num_nodes=n, num_graphs=B, graph=g, pool_operator=pool)
        if dataset.ef_entry is not None:
            batch.edge_feature = dataset.ef_entry.index_select(0, c["entry"])
        if dataset.seedable:
            # the layers build their CSR from edge_index alone (from_edge_index without weights: seed_graph_cache's
            # contract), so a dataset with values seeds the same pattern without them; batch.graph keeps the values
            seeded = g
            if g.val is not None:
                seeded = g.with_values(None)
                seeded.symmetric = True
            seed_graph_cache(batch, batch.edge_index, n, seeded, "none")
    return batch


def ego_collate(dataset, ids, radius):
    """The batch of `ids` under dataset.transform: ego (graphgym/models/transform.py:11-38): every graph replaced by the
    union of its nodes' radius-`radius` ego nets.  The centres are the nodes of the graphs in collate order, expanded by
    ego.ego_batch(base, centres, radius, csr="none"): node_id_index = arange(len(centres)), batch[k] = the batch graph of
    node k's centre, node_feature = x[orig_node], pool_operator selects the centres (the `id` form of
    pooling.pool_operator), and the CSR the expansion wrote is seeded when it returns one.  Synchronises the current
    stream, as ego_batch documents; device datasets only."""
    from .ego import ego_batch
    from .harness import Batch
    from .layers import seed_graph_cache
    c = _collate_device(dataset, ids, entries=False)
    B, C = c["B"], c["n"]
    ei, orig, idx, ego_of, g = ego_batch(dataset.base, c["orig"], int(radius), csr="none")
    n = int(orig.numel())
    with torch.cuda.device(dataset.device):
        batch = Batch(node_feature=_features(dataset.x, orig), edge_index=ei, node_id_index=idx,
                      batch=c["owner"].index_select(0, ego_of), graph_label=dataset.graph_label.index_select(0, c["ids"]),
                      orig_node=orig, ego_of_node=ego_of, num_nodes=n, num_graphs=B,
                      pool_operator=_pool_rows(c["node_off"], dataset.iota(C), B, n))
        if g is not None:
            batch.graph = g
            seed_graph_cache(batch, ei, n, g, "none")
    return batch


# ---- loaders --------------------------------------------------------------------------------------------------------------

class GraphLoader:
    """One epoch of batches of the graphs `ids` of `dataset`: len() = ceil(len(ids) / batch_size), the last batch may be
    short.  shuffle: the ids in epoch_order(ids, seed, epoch), else as given; batch i of epoch e (the e-th iteration over
    the loader, or set_epoch(e)) is a pure function of (seed, e, i).  transform=None | "none": collate — no host read on
    a device dataset.  transform="ego" (dataset.transform: ego) with `radius` (cfg.gnn.layers_mp): ego_collate, which
    synchronises the current stream."""

    def __init__(self, dataset, ids, batch_size, shuffle, seed=0, transform=None, radius=None):
        transform = None if transform in (None, "none") else transform
        if transform not in (None, "ego"):
            raise ValueError(f"transform must be None, 'none' or 'ego', got {transform!r}")
        if transform == "ego" and radius is None:
            raise ValueError("transform='ego' needs a radius (cfg.gnn.layers_mp)")
        if int(batch_size) < 1:
            raise ValueError("batch_size must be at least 1")
        self.dataset, self.ids, self.batch_size = dataset, _np64(ids), int(batch_size)
        self.shuffle, self.seed, self.transform, self.radius = bool(shuffle), int(seed), transform, radius
        self.epoch = 0

    def __len__(self):
        return math.ceil(self.ids.size / self.batch_size)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def order(self, epoch):
        return epoch_order(self.ids, self.seed, epoch) if self.shuffle else self.ids

    def batch_ids(self, epoch, i):
        return self.order(epoch)[i * self.batch_size:(i + 1) * self.batch_size]

    def _collate(self, ids):
        if self.transform == "ego":
            return ego_collate(self.dataset, ids, self.radius)
        return collate(self.dataset, ids)

    def batch(self, epoch, i):
        return self._collate(self.batch_ids(epoch, i))

    def __iter__(self):
        order = self.order(self.epoch)
        self.epoch += 1
        for i in range(len(self)):
            yield self._collate(order[i * self.batch_size:(i + 1) * self.batch_size])


def graph_loaders_from_cfg(cfg, dataset, seed=0):
    """The loaders of graphgym/loader.py:225-260 for a graph-task dataset: one per entry of cfg.dataset.split (the
    inductive split, shuffled when cfg.dataset.shuffle_split — default True), each with cfg.train.batch_size; the first
    shuffles per epoch, the others do not.  cfg.dataset.transform == 'ego' expands every batch with radius
    cfg.gnn.layers_mp."""
    ds = cfg.dataset
    parts = split_graphs(dataset.num_graphs, ds.split, seed, shuffle=bool(getattr(ds, "shuffle_split", True)))
    transform = getattr(ds, "transform", "none")
    radius = cfg.gnn.layers_mp if transform == "ego" else None
    return [GraphLoader(dataset, ids, cfg.train.batch_size, shuffle=(i == 0), seed=seed, transform=transform, radius=radius)
            for i, ids in enumerate(parts)]
