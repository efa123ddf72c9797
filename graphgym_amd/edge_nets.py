"""Edge-level ID-GNN tasks on the GPU: edge-net batches (graphgym/models/transform.py:41-65) through mp_edge_expand and
path-length labels (transform.py:68-90, applied by loader.py:162) through mp_hop_distances (csrc/edge.hip).

    batch = edge_batch(base, graph_ptr, label_index, label, x)        # transform: edge, on the device
    eli, lab = path_len_labels(base, graph_ptr, generator=gen)        # task: edge with an ID layer

`transform: edge` turns link prediction into node classification on the edge-net batch (loader.py:181-187): the batch
trains through harness.GNNNodeHead (cfg.dataset.task = 'node'), with node_label_index / node_label set here."""
import types

import torch

from ._lib import EngineError, K, check, lib, ptr
from .graph import CSRGraph, _require_hip, _stream

FLAG_CSR, FLAG_CSR_SELF_LOOPS = K["MP_EGO_CSR"], K["MP_EGO_CSR_SELF_LOOPS"]
BFS_MAX_NODES = 1 << 16                       # mp_hop_distances: the search's bitmaps live in LDS
_I32_MAX = 2 ** 31 - 1


def _graph_ptr(graph_ptr, N, dev):
    """graph_ptr [G+1] (int64, any device) checked to cover the N base nodes in order; returned on `dev`"""
    gp = torch.as_tensor(graph_ptr).to(torch.int64).reshape(-1)
    if gp.numel() < 2 or int(gp[0]) != 0 or int(gp[-1]) != N or bool((gp[1:] < gp[:-1]).any()):
        raise ValueError(f"graph_ptr must rise from 0 to the base graph's {N} nodes, got {gp.tolist()[:8]}...")
    return gp.to(dev)


def _check_ids(t, N, what):
    if t.numel() and (int(t.min()) < 0 or int(t.max()) >= N):
        raise ValueError(f"{what} holds node ids outside [0, {N})")


def _symmetric(base):
    return base.nnz == 0 or base.is_symmetric(run=True)


def edge_batch(base, graph_ptr, label_index, label, x=None, sources=None, csr=None):
    """The edge-net batch of `base` (CSRGraph in the engine's convention: row = destination, as
    CSRGraph.from_edge_index builds it; the disjoint union of the graphs graph_ptr [G+1] delimits, as in a DeepSNAP
    batch) for the label pairs label_index [2, K] (global base ids (src, dst), both ends in one graph) and labels [K].

    Copy c of graph g is a relabelled copy of the whole graph whose identity node is its source: node j of the copy gets
    the id node_base[c] + j.  sources=None makes a copy for every node (transform.py:41-65: with one graph of n nodes
    node j of copy i is i*n + j; graphs in batch order, each taking n_g^2 ids).  sources="labels" makes copies only for
    the distinct label sources, in the same order: the copies are independent components, so a model gives the same
    outputs at the label nodes of either batch.  Edges keep their direction and multiplicity and come out in the
    engine's CSR order; edge features replicate as edge_feature[orig_edge].

    Returns a harness.Batch with node_feature (= x[orig_node], when x is given), edge_index [2, E'], node_id_index [C]
    (the identity node of every copy), node_label_index [K] (= node_base[copy(src)] + local(dst)), node_label, orig_node
    [N'], copy_of_node [N'] int32, orig_edge [E'], batch [N'] (graph of every node) and copy_source [C] (global base id).
    The identity nodes are not rows 0..C-1, so the identity branch takes its general path (no ego-batch shortcut).

    csr = "none" | "add": also returns the batch's CSRGraph written by the expansion (what
    CSRGraph.from_edge_index(edge_index, N', add_self_loops=(csr == "add")) builds, entry for entry), flagged symmetric;
    or None where the base is not symmetric (directed, repeated entries) or holds self loops: the caller then builds it
    the general way.  seed_graph(batch, g, csr) hands it to the layers.  Synchronises the current stream."""
    _require_hip(base.rowptr, "base.rowptr")
    dev, N = base.device, base.num_nodes
    gp = _graph_ptr(graph_ptr, N, dev)
    li = torch.as_tensor(label_index).to(dev, torch.int64)
    if li.dim() != 2 or li.size(0) != 2:
        raise ValueError("label_index must be [2, K]")
    lab = torch.as_tensor(label).to(dev)
    if lab.size(0) != li.size(1):
        raise ValueError("label must hold one entry per label pair")
    _check_ids(li, N, "label_index")
    g_src = torch.searchsorted(gp, li[0], right=True) - 1
    g_dst = torch.searchsorted(gp, li[1], right=True) - 1
    if bool((g_src != g_dst).any()):
        raise ValueError("a label pair joins two different graphs of the batch")
    if sources is None:
        copies = torch.arange(N, device=dev)
    elif isinstance(sources, str) and sources == "labels":
        copies = torch.unique(li[0])
    else:
        copies = torch.unique(torch.as_tensor(sources).to(dev, torch.int64))
        _check_ids(copies, N, "sources")
    at = torch.searchsorted(copies, li[0]).clamp(max=max(copies.numel() - 1, 0))
    if li.size(1) and (copies.numel() == 0 or bool((copies[at] != li[0]).any())):
        raise ValueError("a label pair's source has no copy in `sources`")
    if base.nnz:
        rows = base.row_ids().long()
        if bool((torch.searchsorted(gp, rows, right=True) != torch.searchsorted(gp, base.col.long(), right=True)).any()):
            raise ValueError("an edge of the base joins two graphs of graph_ptr")
    flags = 0
    if csr is not None:
        if csr not in ("none", "add"):
            raise ValueError("csr must be None, 'none' or 'add'")
        if _symmetric(base) and not base.has_self_loops():
            flags = FLAG_CSR | (FLAG_CSR_SELF_LOOPS if csr == "add" else 0)
    plan = plan_expansion(base, gp, copies, flags)
    run_expansion(plan)
    ei, orig, copy_of, node_base = plan.edge_index, plan.orig_node, plan.copy_of_node, plan.node_base
    from .harness import Batch
    batch = Batch(edge_index=ei, node_id_index=plan.id_index, orig_node=orig, copy_of_node=copy_of,
                  orig_edge=plan.orig_edge, node_label_index=node_base[at] + (li[1] - gp[g_dst]),
                  node_label=lab, batch=plan.copy_graph.long()[copy_of.long()], copy_source=copies)
    if x is not None:
        batch.node_feature = x[orig]
    if csr is None:
        return batch
    g = None
    if flags:
        n_out, nnz_out = plan.n_out, plan.nnz_out
        g = CSRGraph(plan.rowptr, plan.col[:nnz_out], None, plan.eid[:nnz_out], n_out, nnz_out)
        g.symmetric = True                    # copies of a symmetric graph: A^T = A (no _ego_ids: see the docstring)
    return batch, g


def plan_expansion(base, gp, copies, flags=0):
    """the inputs and the preallocated outputs of one mp_edge_expand call: copies [C] are global base ids (ascending),
    gp the checked graph_ptr on the device.  One synchronisation (the output sizes)."""
    dev = base.device
    C_ = copies.numel()
    copy_graph = (torch.searchsorted(gp, copies, right=True) - 1).to(torch.int32)
    cg = copy_graph.long()
    lo = gp[cg]
    n_of = gp[cg + 1] - lo
    rp = base.rowptr.long()
    e_of = rp[gp[cg + 1]] - rp[lo]
    zero = torch.zeros(1, dtype=torch.int64, device=dev)
    biggest = torch.maximum(n_of, e_of).max() if C_ else zero[0]
    node_base = torch.cat([zero, torch.cumsum(n_of, 0)])
    entry_base = torch.cat([zero, torch.cumsum(e_of, 0)])
    n_out, e_out, max_size = (int(v) for v in torch.stack([node_base[-1], entry_base[-1], biggest]).tolist())
    nnz_out = e_out + (n_out if flags & FLAG_CSR_SELF_LOOPS else 0)
    if n_out >= _I32_MAX or nnz_out > _I32_MAX:
        raise EngineError(f"mp_edge_expand: {n_out} nodes / {nnz_out} entries exceed the int32 index range")
    plan = types.SimpleNamespace(
        base=base, row=base.row_ids() if base.nnz else None, gp=gp, copy_graph=copy_graph,
        copy_src=(copies - lo).to(torch.int32), node_base=node_base, entry_base=entry_base, n_copies=C_,
        n_out=n_out, e_out=e_out, nnz_out=nnz_out, max_size=max_size, flags=flags,
        edge_index=torch.empty(2, e_out, dtype=torch.int64, device=dev),
        orig_node=torch.empty(n_out, dtype=torch.int64, device=dev),
        copy_of_node=torch.empty(n_out, dtype=torch.int32, device=dev),
        orig_edge=torch.empty(e_out, dtype=torch.int64, device=dev),
        id_index=torch.empty(C_, dtype=torch.int64, device=dev), rowptr=None, col=None, eid=None)
    if flags:
        plan.rowptr = torch.empty(n_out + 1, dtype=torch.int32, device=dev)
        plan.col = torch.empty(max(nnz_out, 1), dtype=torch.int32, device=dev)
        plan.eid = torch.empty(max(nnz_out, 1), dtype=torch.int32, device=dev)
    return plan


def run_expansion(plan):
    """one mp_edge_expand launch on the current stream (every output of `plan` written; no synchronisation)"""
    b, L = plan.base, lib()
    with torch.cuda.device(b.device):
        check(L.mp_edge_expand(ptr(b.rowptr), ptr(b.col), ptr(plan.row), ptr(b.eid), b.num_nodes, b.nnz, ptr(plan.gp),
                               plan.gp.numel() - 1, ptr(plan.copy_graph), ptr(plan.copy_src), ptr(plan.node_base),
                               ptr(plan.entry_base), plan.n_copies, plan.n_out, plan.e_out, plan.max_size, plan.flags,
                               ptr(plan.edge_index), ptr(plan.orig_node), ptr(plan.copy_of_node), ptr(plan.orig_edge),
                               ptr(plan.id_index), ptr(plan.rowptr), ptr(plan.col), ptr(plan.eid), _stream()),
              "mp_edge_expand")


def seed_graph(batch, g, csr):
    """hand the CSR edge_batch(csr=...) wrote to the layers (layers.seed_graph_cache on the batch, the holder the
    GraphGym layers pass): the ID layers then reuse it instead of sorting the edge list again"""
    from .layers import seed_graph_cache
    return seed_graph_cache(batch, batch.edge_index, int(batch.orig_node.numel()), g, csr)


def hop_distances(base, src, dst, graph_ptr=None):
    """int32 [P]: hops of the shortest path from src[p] to dst[p] (global base ids) along the edge direction
    (nx.shortest_path_length on graph.G: successors on a directed graph), inside their graph of graph_ptr (default: the
    whole base is one graph); 0 for (a, a), -1 if unreachable or in another graph.  Exact at any depth.  A base that is
    not its own transpose is searched over its transposed CSR (rows = out-edges, cached on `base`).  Pairs that share a
    source share one search; a graph above 65536 nodes that holds a source is an EngineError (the search keeps its
    bitmaps in LDS)."""
    _require_hip(base.rowptr, "base.rowptr")
    dev, N = base.device, base.num_nodes
    gp = _graph_ptr([0, N] if graph_ptr is None else graph_ptr, N, dev)
    s = torch.as_tensor(src).to(dev, torch.int64).reshape(-1)
    d = torch.as_tensor(dst).to(dev, torch.int64).reshape(-1)
    if s.numel() != d.numel():
        raise ValueError("src and dst must hold the same number of pairs")
    _check_ids(s, N, "src")
    _check_ids(d, N, "dst")
    plan = plan_hops(base, s, d, gp)
    run_hops(plan)
    return plan.dist


def plan_hops(base, s, d, gp):
    """the inputs and the output of one mp_hop_distances call for checked pairs (s, d) and graph_ptr gp: pairs grouped
    by their distinct source (a stable sort), the source graphs' sizes checked against the LDS bound"""
    dev, P = base.device, s.numel()
    plan = types.SimpleNamespace(dist=torch.empty(P, dtype=torch.int32, device=dev), n_pairs=P, n_sources=0)
    if P == 0:
        return plan
    walk = base if _symmetric(base) else base.transpose()
    uniq, inv = torch.unique(s, return_inverse=True)
    sg = torch.searchsorted(gp, uniq, right=True) - 1
    biggest = int((gp[sg + 1] - gp[sg]).max())
    if biggest > BFS_MAX_NODES:
        raise EngineError(f"hop_distances: a graph of {biggest} nodes holds a source; the search keeps its bitmaps in "
                          f"LDS and takes graphs of up to {BFS_MAX_NODES} nodes")
    order = torch.argsort(inv, stable=True)
    pair_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev),
                          torch.cumsum(torch.bincount(inv, minlength=uniq.numel()), 0)])
    plan.__dict__.update(walk=walk, gp=gp, biggest=biggest, sources=uniq, source_graph=sg.to(torch.int32),
                         n_sources=uniq.numel(), pair_off=pair_off, pair_dst=d[order].contiguous(), pair_pos=order)
    return plan


def run_hops(plan):
    """one mp_hop_distances launch on the current stream (no synchronisation)"""
    if plan.n_pairs == 0:
        return
    w, L = plan.walk, lib()
    with torch.cuda.device(w.device):
        check(L.mp_hop_distances(ptr(w.rowptr), ptr(w.col), w.num_nodes, w.nnz, ptr(plan.gp), plan.gp.numel() - 1,
                                 plan.biggest, ptr(plan.sources), ptr(plan.source_graph), plan.n_sources,
                                 ptr(plan.pair_off), ptr(plan.pair_dst), ptr(plan.pair_pos), plan.n_pairs,
                                 ptr(plan.dist), _stream()), "mp_hop_distances")


def path_len_labels(base, graph_ptr, num_label=1000, generator=None):
    """transform.py:68-90 for every graph of the batch, in order: num_label pairs drawn as
    torch.randint(n_g, (2, num_label), generator=generator) (on the generator's device), unreachable pairs dropped,
    label = min(hops, 4).  Returns (edge_label_index [2, K] global base ids, edge_label [K] int64) on the base's device;
    given the same generator state the pairs are the reference's."""
    dev, N = base.device, base.num_nodes
    gp = [int(v) for v in _graph_ptr(graph_ptr, N, "cpu").tolist()]
    gen_dev = generator.device if generator is not None else torch.device("cpu")
    parts = []
    for g in range(len(gp) - 1):
        n = gp[g + 1] - gp[g]
        if n == 0:
            continue
        parts.append(torch.randint(n, (2, int(num_label)), generator=generator, device=gen_dev).to(dev) + gp[g])
    if not parts:
        return torch.empty(2, 0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int64, device=dev)
    pairs = torch.cat(parts, 1)
    dist = hop_distances(base, pairs[0], pairs[1], torch.tensor(gp, dtype=torch.int64))
    keep = dist >= 0
    return pairs[:, keep], dist[keep].clamp(max=4).to(torch.int64)
