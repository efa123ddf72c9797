"""GraphGym's structural labels and features on the GPU: the raw quantities of graphgym/models/feature_augment.py:51-107
(one networkx call per node or graph in the reference) through mp_csr_triangles and mp_hop_sums (csrc/structure.hip)
and mp_struct_pagerank, mp_struct_betweenness and mp_struct_onehot (csrc/centrality.hip), and the dataset-wide
representation of :134-310 (binning, one-hot, position) in plain torch.

    tensors, feat_dims, label_dim = augment(base, graph_ptr, ["node_degree"], [8],
                                            label="node_clustering_coefficient", label_dim=10)
    y = tensors["node_clustering_coefficient_label"]            # dataset.augment_label: node_clustering_coefficient

`base` is a CSRGraph on the HIP device holding the disjoint union of the dataset's graphs, graph_ptr [G+1] delimits
them (default: one graph).  The reference's datasets are undirected nx.Graphs: every raw quantity requires
base.is_symmetric(run=True) — the stored operator equals its transpose and stores no (r, c) twice — and raises
ValueError otherwise (networkx's directed clustering and path definitions are other formulas).  The kernels return exact
integers; the quotients are one float64 division each, on the device, so they equal networkx's bit for bit.  PageRank
and betweenness are float64 sums in an order of their own: they agree with networkx within rounding (the bounds are in
DESIGN.md 4.21), reproduce bit for bit, and do not depend on the batch a graph is computed in.

The representation functions take any tensors, CPU ones included."""
import numpy as np
import torch

from . import _lib_structure as LS
from ._lib import EngineError, check, lib, ptr
from .edge_nets import BFS_MAX_NODES, _check_ids, _graph_ptr
from .graph import _require_hip, _stream

# node_onehot and node_pagerank are features, and node_pagerank a label, of the reference's synthetic design-space grids
# (run/grids/design/round1.txt:52,72-73,92, round1att.txt, round2.txt:53); edge_path_len is a node quantity the reference
# files under an edge key (feature_augment.py:65-68 is path_len_fun word for word)
NODE_KEYS = ("node_degree", "node_path_len", "node_clustering_coefficient", "node_identity", "node_const",
             "node_pagerank", "node_betweenness_centrality", "node_onehot", "edge_path_len")
GRAPH_KEYS = ("graph_path_len", "graph_clustering_coefficient")
SUPPORTED_KEYS = NODE_KEYS + GRAPH_KEYS
# the reference's last key (feature_augment.py:109-122): a dense eigensolve, with no kernel of this library in it
UNBUILT_KEYS = ("graph_laplacian_spectrum",)
BIN_METHODS = ("balanced", "equal_width", "bounded")


# ---- raw quantities ------------------------------------------------------------------------------------------------

def _undirected(base, what):
    _require_hip(base.rowptr, "base.rowptr")
    if base.nnz and not base.is_symmetric(run=True):
        raise ValueError(f"{what} needs an undirected graph: the stored operator must equal its transpose and store no "
                         "entry twice (networkx defines the directed quantities by other formulas)")


def _gp(base, graph_ptr):
    N = base.num_nodes
    return _graph_ptr([0, N] if graph_ptr is None else graph_ptr, N, base.device)


def _sizes(gp, what):
    n = gp[1:] - gp[:-1]
    if bool((n == 0).any()):
        raise ValueError(f"{what}: graph {int(torch.nonzero(n == 0)[0])} of graph_ptr is empty")
    return n


def _segment_int_sums(v, gp):
    """exact per-graph sums of an int64 vector (differences of its running sum)"""
    run = torch.cat([torch.zeros(1, dtype=torch.int64, device=v.device), torch.cumsum(v, 0)])
    return run[gp[1:]] - run[gp[:-1]]


def triangles(base):
    """(tri2 int64 [N], deg int64 [N]): twice the triangles through every node and its number of neighbours (self
    loops skipped) — the t and d of nx.clustering's t / (d (d - 1)).  One mp_csr_triangles call, no synchronisation
    beyond the symmetry check's (cached on `base`)."""
    _undirected(base, "triangles")
    N, dev = base.num_nodes, base.device
    tri2 = torch.empty(N, dtype=torch.int64, device=dev)
    deg = torch.empty(N, dtype=torch.int32, device=dev)
    run_triangles(base, tri2, deg)
    return tri2, deg.long()


def run_triangles(base, tri2, deg):
    """one mp_csr_triangles call on the current stream into preallocated tri2 (int64 [N]) and deg (int32 [N])"""
    row_of = base.row_ids() if base.nnz else None
    with torch.cuda.device(base.device):
        check(lib().mp_csr_triangles(ptr(base.rowptr), ptr(base.col), ptr(row_of), base.num_nodes, base.nnz, ptr(tri2),
                                     ptr(deg), _stream()), "mp_csr_triangles")


def _self_loops(base):
    """int64 [N]: 1 where the row stores its own column"""
    if base.nnz == 0:
        return torch.zeros(base.num_nodes, dtype=torch.int64, device=base.device)
    rows = base.row_ids().long()
    return torch.bincount(rows[rows == base.col.long()], minlength=base.num_nodes)


def node_degree(base, _tri=None):
    """int64 [N]: G.degree() (feature_augment.py:51-53) — the neighbours, and 2 for a self loop"""
    deg = (triangles(base) if _tri is None else _tri)[1]
    return deg + 2 * _self_loops(base)


def node_clustering_coefficient(base, _tri=None):
    """float64 [N]: nx.clustering (feature_augment.py:81-82): tri2 / (deg (deg - 1)), 0 where deg < 2"""
    tri2, deg = triangles(base) if _tri is None else _tri
    d = deg.to(torch.float64)
    pairs = (d * (d - 1)).clamp(min=1.0)
    return torch.where(deg >= 2, tri2.to(torch.float64) / pairs, torch.zeros_like(d))


def graph_clustering_coefficient(base, graph_ptr=None, _tri=None):
    """float64 [G]: nx.average_clustering (feature_augment.py:105-107), the mean of the nodes' coefficients per graph
    (summed in node order by one thread per graph: reproducible)"""
    _undirected(base, "graph_clustering_coefficient")
    gp = _gp(base, graph_ptr)
    n = _sizes(gp, "graph_clustering_coefficient")
    cc = node_clustering_coefficient(base, _tri)
    return torch.segment_reduce(cc, "sum", lengths=n, unsafe=True) / n.to(torch.float64)


def hop_sums(base, graph_ptr=None, nodes=None):
    """(dist_sum int64 [S], reached int64 [S]) for the sources `nodes` (global ids; default: every node): the sum of the
    hop distances from the source to every node it reaches inside its graph, and their number, the source included.
    A graph above 65536 nodes that holds a source is an EngineError (the search keeps its bitmaps in LDS)."""
    _undirected(base, "hop_sums")
    plan = plan_hop_sums(base, _gp(base, graph_ptr), nodes)
    run_hop_sums(plan)
    return plan.dist_sum, plan.reached.long()


def plan_hop_sums(base, gp, nodes=None):
    """the inputs and preallocated outputs of one mp_hop_sums call; gp is the checked graph_ptr on the device"""
    import types
    dev, N = base.device, base.num_nodes
    if nodes is None:
        src = torch.arange(N, dtype=torch.int64, device=dev)
    else:
        src = torch.as_tensor(nodes).to(dev, torch.int64).reshape(-1).contiguous()
        _check_ids(src, N, "nodes")
    S = src.numel()
    sg = torch.searchsorted(gp, src, right=True) - 1
    biggest = int((gp[sg + 1] - gp[sg]).max()) if S else 0
    if biggest > BFS_MAX_NODES:
        raise EngineError(f"hop_sums: a graph of {biggest} nodes holds a source; the search keeps its bitmaps in LDS "
                          f"and takes graphs of up to {BFS_MAX_NODES} nodes")
    return types.SimpleNamespace(base=base, gp=gp, sources=src, source_graph=sg.to(torch.int32), n_sources=S,
                                 biggest=biggest, dist_sum=torch.empty(S, dtype=torch.int64, device=dev),
                                 reached=torch.empty(S, dtype=torch.int32, device=dev))


def run_hop_sums(plan):
    """one mp_hop_sums launch on the current stream (no synchronisation)"""
    b = plan.base
    with torch.cuda.device(b.device):
        check(lib().mp_hop_sums(ptr(b.rowptr), ptr(b.col), b.num_nodes, b.nnz, ptr(plan.gp), plan.gp.numel() - 1,
                                plan.biggest, ptr(plan.sources), ptr(plan.source_graph), plan.n_sources,
                                ptr(plan.dist_sum), ptr(plan.reached), _stream()), "mp_hop_sums")


def node_path_len(base, graph_ptr=None, nodes=None, _hops=None):
    """float64 [S]: path_len_fun (feature_augment.py:60-63) — np.mean of nx.shortest_path_length(G, source=x) over the
    nodes x reaches, x itself (distance 0) included"""
    dist_sum, reached = hop_sums(base, graph_ptr, nodes) if _hops is None else _hops
    return dist_sum.to(torch.float64) / reached.to(torch.float64)


def graph_path_len(base, graph_ptr=None, _hops=None):
    """float64 [G]: nx.average_shortest_path_length (feature_augment.py:101-103): the sum of all pair distances over
    n (n - 1); 0 for a one-node graph.  ValueError for a graph that is not connected (networkx raises there)."""
    _undirected(base, "graph_path_len")
    gp = _gp(base, graph_ptr)
    n = _sizes(gp, "graph_path_len")
    dist_sum, reached = hop_sums(base, gp) if _hops is None else _hops
    short = _segment_int_sums((reached != torch.repeat_interleave(n, n)).long(), gp)
    if bool((short > 0).any()):
        raise ValueError(f"graph_path_len: graph {int(torch.nonzero(short > 0)[0])} is not connected")
    total = _segment_int_sums(dist_sum, gp).to(torch.float64)
    pairs = (n * (n - 1)).to(torch.float64)
    return torch.where(n > 1, total / pairs.clamp(min=1.0), torch.zeros_like(total))


def node_const(base):
    """const_fun (feature_augment.py:84-86)"""
    _undirected(base, "node_const")
    return torch.ones(base.num_nodes, device=base.device)


def node_identity(base, graph_ptr=None, feature_dim=None):
    """identity_fun (feature_augment.py:75-79) through identity.compute_identity, the edge index rebuilt from the CSR
    (PyG's order: sources first; the engine's rows are destinations)"""
    from .identity import compute_identity
    if feature_dim is None:
        raise ValueError("Argument feature_dim not supplied")
    _undirected(base, "node_identity")
    gp = _gp(base, graph_ptr)
    N, dev = base.num_nodes, base.device
    rows = base.row_ids().long() if base.nnz else torch.zeros(0, dtype=torch.int64, device=dev)
    edge_index = torch.stack([base.col.long()[:base.nnz], rows])
    batch = torch.repeat_interleave(torch.arange(gp.numel() - 1, device=dev), gp[1:] - gp[:-1])
    return compute_identity(edge_index, N, int(feature_dim), batch=batch if N else None)


# ---- centralities and one-hot ids (csrc/centrality.hip, include/mp_structure.h) ----------------------------------------

def _sizes_host(gp, what):
    """the graphs' node counts as a NumPy array: the one read of graph_ptr's differences a call makes"""
    n = (gp[1:] - gp[:-1]).cpu().numpy()
    if (n == 0).any():
        raise ValueError(f"{what}: graph {int(np.flatnonzero(n == 0)[0])} of graph_ptr is empty")
    return n


def _prefix(counts, dev):
    """[0, counts[0], counts[0] + counts[1], ...] as an int64 tensor on `dev`"""
    return torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)).to(dev)


def _workspace(nbytes, dev):
    return torch.empty(int(nbytes), dtype=torch.uint8, device=dev)


def _ws_bytes(entry, *args):
    import ctypes
    nb = ctypes.c_size_t(0)
    check(getattr(LS.lib(), entry)(*args, ctypes.byref(nb)), entry)
    return nb.value


def node_pagerank(base, graph_ptr=None, alpha=0.85, tol=1e-6, max_iter=100, return_iters=False):
    """float64 [N]: pagerank_fun (feature_augment.py:70-73) — nx.pagerank(G) per graph, restated in float64: from
    x = 1 / n the step x' = alpha (x A / deg + dsum / n) + (1 - alpha) / n, the result being the x' of the first step
    with sum |x' - x| < n tol (include/mp_structure.h has the whole statement).  With return_iters also int32 [G], the
    number of that step.  Every graph stops on its own count, on the device; the call reads graph_ptr's sizes once
    before it enqueues anything and `iters` once after.  ValueError for a graph that has not stopped after max_iter
    steps (networkx raises PowerIterationFailedConvergence there)."""
    _undirected(base, "node_pagerank")
    gp = _gp(base, graph_ptr)
    dev, N = base.device, base.num_nodes
    if N == 0:
        out, iters = torch.empty(0, dtype=torch.float64, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
        return (out, iters) if return_iters else out
    plan = plan_pagerank(base, gp, _sizes_host(gp, "node_pagerank"), alpha, tol, max_iter)
    run_pagerank(plan)
    failed = torch.nonzero(plan.iters.cpu() < 0)
    if failed.numel():
        raise ValueError(f"node_pagerank: graph {int(failed[0])} has not converged within {int(max_iter)} iterations")
    return (plan.out, plan.iters) if return_iters else plan.out


def plan_pagerank(base, gp, n, alpha=0.85, tol=1e-6, max_iter=100):
    """the inputs and preallocated outputs of one mp_struct_pagerank call; gp is the checked graph_ptr on the device and
    n the graphs' sizes on the host"""
    import types
    dev, N, G = base.device, base.num_nodes, len(n)
    chunks = np.where(n > LS.PAGERANK_LDS_NODES, -(-n // LS.PAGERANK_CHUNK), 0)
    n_chunks = int(chunks.sum())
    ws = _workspace(_ws_bytes("mp_struct_pagerank_ws_bytes", N, G, n_chunks), dev)
    return types.SimpleNamespace(base=base, gp=gp, n_chunks=n_chunks, chunk_ptr=_prefix(chunks, dev) if n_chunks else None,
                                 alpha=float(alpha), tol=float(tol), max_iter=int(max_iter), ws=ws,
                                 out=torch.empty(N, dtype=torch.float64, device=dev),
                                 iters=torch.empty(G, dtype=torch.int32, device=dev))


def run_pagerank(plan):
    """one mp_struct_pagerank call on the current stream (no synchronisation)"""
    b = plan.base
    with torch.cuda.device(b.device):
        check(LS.lib().mp_struct_pagerank(ptr(b.rowptr), ptr(b.col), b.num_nodes, b.nnz, ptr(plan.gp),
                                          plan.gp.numel() - 1, ptr(plan.chunk_ptr), plan.n_chunks, plan.alpha, plan.tol,
                                          plan.max_iter, ptr(plan.out), ptr(plan.iters), ptr(plan.ws), plan.ws.numel(),
                                          _stream()), "mp_struct_pagerank")


def node_betweenness_centrality(base, graph_ptr=None):
    """float64 [N]: centrality_fun (feature_augment.py:55-58) — nx.betweenness_centrality(G) per graph: Brandes'
    algorithm from every node, unweighted, normalised by (n - 1) (n - 2), endpoints left out.  A node no shortest path
    passes through gets exactly 0.0.  A graph above 65536 nodes is an EngineError, as for hop_sums."""
    _undirected(base, "node_betweenness_centrality")
    gp = _gp(base, graph_ptr)
    if base.num_nodes == 0:
        return torch.empty(0, dtype=torch.float64, device=base.device)
    plan = plan_betweenness(base, gp, _sizes_host(gp, "node_betweenness_centrality"))
    run_betweenness(plan)
    return plan.out


def plan_betweenness(base, gp, n):
    """the inputs, workspace and preallocated output of one mp_struct_betweenness call"""
    import types
    dev, N = base.device, base.num_nodes
    biggest = int(n.max()) if len(n) else 0
    if biggest > BFS_MAX_NODES:
        raise EngineError(f"node_betweenness_centrality: a graph of {biggest} nodes; the search keeps one level, sigma "
                          f"and delta vector per slice of sources and takes graphs of up to {BFS_MAX_NODES} nodes")
    slices = -(-n // LS.BETWEENNESS_SLICE)
    ws = _workspace(_ws_bytes("mp_struct_betweenness_ws_bytes", N, biggest), dev)
    return types.SimpleNamespace(base=base, gp=gp, biggest=biggest, slice_ptr=_prefix(slices, dev),
                                 n_slices=int(slices.sum()), ws=ws, out=torch.empty(N, dtype=torch.float64, device=dev))


def run_betweenness(plan):
    """one mp_struct_betweenness call on the current stream (no synchronisation)"""
    b = plan.base
    with torch.cuda.device(b.device):
        check(LS.lib().mp_struct_betweenness(ptr(b.rowptr), ptr(b.col), b.num_nodes, b.nnz, ptr(plan.gp),
                                             plan.gp.numel() - 1, plan.biggest, ptr(plan.slice_ptr), plan.n_slices,
                                             ptr(plan.out), ptr(plan.ws), plan.ws.numel(), _stream()),
              "mp_struct_betweenness")


def node_onehot(base, graph_ptr=None, seed=0):
    """int64 [N]: onehot_fun (feature_augment.py:88-91) — a random permutation of 0 .. n - 1 per graph, where the
    reference calls torch.randperm: entry i of graph g is perm(i), the keyed bijection of csrc/draws.h with round keys
    from (seed, g).  It depends on (seed, g, i, n_g) and nothing else; onehot_host restates it."""
    _undirected(base, "node_onehot")
    gp = _gp(base, graph_ptr)
    dev, N = base.device, base.num_nodes
    if N:
        _sizes_host(gp, "node_onehot")
    out = torch.empty(N, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(LS.lib().mp_struct_onehot(ptr(gp), gp.numel() - 1, N, int(seed) & ((1 << 64) - 1), ptr(out), _stream()),
              "mp_struct_onehot")
    return out


def onehot_host(n_list, seed=0):
    """node_onehot for graphs of n_list nodes, restated in NumPy integers, bit for bit (int64 [sum of n_list])"""
    from .link_pred import _permute, _round_keys
    parts = [_permute(np.arange(int(n), dtype=np.uint64), int(n), _round_keys(int(seed), LS.ONEHOT_STREAM, g))
             for g, n in enumerate(n_list)]
    return np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64)


def edge_path_len(base, graph_ptr=None, _hops=None):
    """float64 [N]: edge_path_len_fun (feature_augment.py:65-68), which is path_len_fun under an edge key"""
    return node_path_len(base, graph_ptr, _hops=_hops)


def raw(key, base, graph_ptr=None, feature_dim=None, _cache=None, seed=0):
    """the raw quantity the reference files under `key` (feature_augment.py:109-122).  _cache (a dict) carries the
    kernels' integers from one key to the next: triangles and hop sums are computed once per dataset.  seed keys
    node_onehot's permutations."""
    if key not in SUPPORTED_KEYS:
        why = " (in the reference, but not built here)" if key in UNBUILT_KEYS else ""
        raise KeyError(f"{key!r}{why}: supported keys are {', '.join(SUPPORTED_KEYS)}")
    cache = {} if _cache is None else _cache

    def tri():
        if "tri" not in cache:
            cache["tri"] = triangles(base)
        return cache["tri"]

    def hops():
        if "hops" not in cache:
            cache["hops"] = hop_sums(base, graph_ptr)
        return cache["hops"]

    if key == "node_degree":
        return node_degree(base, tri())
    if key == "node_clustering_coefficient":
        return node_clustering_coefficient(base, tri())
    if key == "graph_clustering_coefficient":
        return graph_clustering_coefficient(base, graph_ptr, tri())
    if key in ("node_path_len", "edge_path_len"):
        return node_path_len(base, graph_ptr, _hops=hops())
    if key == "node_pagerank":
        return node_pagerank(base, graph_ptr)
    if key == "node_betweenness_centrality":
        return node_betweenness_centrality(base, graph_ptr)
    if key == "node_onehot":
        return node_onehot(base, graph_ptr, seed)
    if key == "graph_path_len":
        return graph_path_len(base, graph_ptr, hops())
    if key == "node_const":
        return node_const(base)
    return node_identity(base, graph_ptr, feature_dim)


# ---- representation (plain torch; feature_augment.py:134-245 restated) ----------------------------------------------

def bin_edges(values, dim, method):
    """the bin edges of _get_bin_edges (feature_augment.py:208-245) over ALL values handed in (dataset-wide):
    balanced    sorted[linspace(0, len, dim, endpoint=False).astype(int)], made unique — fewer than dim edges where ties
                collapse bins: the caller reads the dimension from the length
    equal_width linspace(min, max, dim)
    bounded     arange(dim) (integer features in [0, dim - 1], bins of width 1)"""
    v = torch.as_tensor(values).reshape(-1)
    dim = int(dim)
    if method == "balanced":
        # np.linspace(0, len, dim, endpoint=False) is arange(dim) * (len / dim); astype(int) truncates
        at = (torch.arange(dim, dtype=torch.float64) * (v.numel() / dim)).to(torch.int64).to(v.device)
        return torch.unique(torch.sort(v).values[at])
    if method == "equal_width":
        v = v.to(torch.float64)
        lo, hi = v.min(), v.max()
        if dim == 1:
            return lo.reshape(1)
        # np.linspace(lo, hi, dim): arange(dim) * step + lo with the last edge set to hi
        edges = torch.arange(dim, dtype=torch.float64, device=v.device) * ((hi - lo) / (dim - 1)) + lo
        edges[-1] = hi
        return edges
    if method == "bounded":
        return torch.arange(dim, device=v.device)
    raise ValueError(f"Bin method {method} not supported")


def digitize(values, edges):
    """np.digitize(values, edges) - 1 (feature_augment.py:141): the last edge at or below the value.  ValueError where
    the reference asserts: a class outside [0, len(edges) - 1]."""
    v, e = torch.as_tensor(values).reshape(-1), torch.as_tensor(edges)
    if v.dtype != e.dtype:
        both = torch.float64 if (v.is_floating_point() or e.is_floating_point()) else torch.int64
        v, e = v.to(both), e.to(both)
    cls = torch.bucketize(v, e.to(v.device), right=True) - 1
    if cls.numel() and (int(cls.min()) < 0 or int(cls.max()) > e.numel() - 1):
        raise ValueError(f"a value falls outside the {e.numel()} bins (classes {int(cls.min())}..{int(cls.max())})")
    return cls


def _position(values, dim, wavelength=10000):
    """_position_features (feature_augment.py:177-200) with scale = dim / 2 / max (:276)"""
    pos = torch.as_tensor(values).float()
    if pos.dim() == 1:
        pos = pos.unsqueeze(-1)
    rows = pos.size(0)
    pos = pos.reshape(-1) * (dim / 2 / float(torch.as_tensor(values).max()))
    half = int(dim) // 2
    cycle = torch.arange(0, half, device=pos.device).float() / half
    arg = pos.unsqueeze(-1) / wavelength ** cycle.unsqueeze(0)
    return torch.cat((torch.cos(arg), torch.sin(arg)), dim=-1).view(rows, -1)


def _represent(values, dim, method, as_label, node_level):
    v = torch.as_tensor(values)
    if method == "original":                       # _orig_features (:165-175): the config's dim is ignored
        if as_label:
            v = v.float()                          # (a label is left `original` only for regression, :253-254)
        if v.dim() == 1 and node_level:
            v = v.unsqueeze(-1)
        return v, (1 if v.dim() == 1 else v.size(-1))
    if method == "position":
        out = _position(v, dim)
        return out, out.size(-1)
    if method == "bounded" and v.numel() and float(v.max()) > int(dim) - 1:
        # np.digitize has no upper edge: the reference files such a value under class dim - 1 without a word; the
        # method's contract is values bounded by dim (:239-242), so it is refused here
        raise ValueError(f"bounded: a value ({float(v.max()):g}) falls outside the {int(dim)} bins of width 1")
    edges = bin_edges(v, dim, method)
    cls = digitize(v, edges)
    if as_label:
        return cls, edges.numel()
    one_hot = torch.zeros(cls.numel(), edges.numel(), device=cls.device)
    one_hot.scatter_(1, cls.unsqueeze(-1), 1.0)
    return one_hot, edges.numel()


def represent(values, dim, method, as_label=False, node_level=True):
    """one raw quantity of the whole dataset in the representation `method` (feature_augment.py:268-294):
    balanced / equal_width / bounded   one-hot float32 [n, len(edges)], or the int64 class ids as a label
    original                           the values themselves: [n, 1] for node attributes, float32 as a label
    position                           the transformer-style encoding of :177-200, [n, 2 (dim // 2)]"""
    if method not in BIN_METHODS + ("original", "position"):
        raise ValueError(f"Bin method {method} not supported")
    return _represent(values, dim, method, as_label, node_level)[0]


def augment(base, graph_ptr, features, feature_dims, label=None, label_dim=None, task_type="classification",
            feature_repr="balanced", seed=0):
    """FeatureAugment.augment (feature_augment.py:247-310) for the dataset whose graphs `base` / graph_ptr hold:
    dataset.augment_feature = features, augment_feature_dims = feature_dims, augment_feature_repr = feature_repr,
    augment_label = label, augment_label_dims = label_dim, dataset.task_type = task_type.

    Returns (tensors, actual_feat_dims, actual_label_dim): tensors[key] per feature and tensors[key + "_label"] for the
    label (balanced class ids when "classification" in task_type, else the original values), every tensor covering all
    nodes (node keys) or all graphs (graph keys) of the dataset in order.  The actual dimensions are those of the
    representation — the number of bin edges where balanced bins collapse — and None without a label.  Each raw
    quantity is computed once, also where it is both a feature and the label.  seed keys node_onehot's permutations."""
    features, feature_dims = list(features), list(feature_dims)
    if len(features) != len(feature_dims):
        raise ValueError("features and feature_dims must have the same length")
    if label and label_dim is None:
        raise ValueError("label_dim must be given with label")
    if feature_repr not in BIN_METHODS + ("original", "position"):
        raise ValueError(f"Bin method {feature_repr} not supported")
    cache, raws, tensors, feat_dims = {}, {}, {}, []

    def raw_of(key, dim):
        at = (key, int(dim)) if key == "node_identity" else key
        if at not in raws:
            raws[at] = raw(key, base, graph_ptr, feature_dim=dim, _cache=cache, seed=seed)
        return raws[at]

    for key, dim in zip(features, feature_dims):
        if key not in tensors:
            tensors[key], d = _represent(raw_of(key, dim), dim, feature_repr, False, key.startswith("node"))
            cache[("dim", key)] = d
        feat_dims.append(cache[("dim", key)])
    actual_label_dim = None
    if label:
        method = "balanced" if "classification" in task_type else "original"
        tensors[label + "_label"], actual_label_dim = _represent(raw_of(label, label_dim), label_dim, method, True,
                                                                 label.startswith("node"))
    return tensors, feat_dims, actual_label_dim
