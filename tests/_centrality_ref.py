"""Host oracles for the tests of graphgym_amd.structure's centralities (csrc/centrality.hip): the PageRank loop of
include/mp_structure.h restated in NumPy / SciPy the way nx.pagerank computes it, a level-synchronous Brandes in SciPy
sparse products for graphs networkx needs a minute for, and the one-hot permutation in Python integers.  Graphs are
nx.Graphs whose nodes are 0..n-1 in order (tests/_structure_ref.py builds them)."""
import networkx as nx
import numpy as np
import scipy.sparse as sp

import _structure_ref as R


# ---- inputs ---------------------------------------------------------------------------------------------------------

def path_with_isolated():
    return nx.disjoint_union(nx.path_graph(3), nx.empty_graph(2))


def small_inputs():
    """the PageRank inputs of the host and the GPU test, in one order: name -> graph"""
    out = {f"pc{k}": G for k, G in enumerate(R.pc_graphs())}
    out.update({f"ba{k}": G for k, G in enumerate(R.ba_graphs())})
    out.update({f"path{n}": nx.path_graph(n) for n in (1, 2, 3, 5, 64, 65, 200)})
    out.update(star200=nx.star_graph(199), ring65=nx.cycle_graph(65), empty4=nx.empty_graph(4),
               path3_isolated2=path_with_isolated())
    return out


def with_isolated(G, extra=3):
    """G with `extra` isolated nodes appended"""
    H = G.copy()
    H.add_nodes_from(range(G.number_of_nodes(), G.number_of_nodes() + extra))
    return H


def adjacency(G, loops=True):
    """the symmetric 0/1 CSR of G over nodes 0..n-1 (a self loop stored once), columns ascending"""
    n = G.number_of_nodes()
    ei, _, _ = R.union([G])
    r, c = ei.numpy()
    if not loops:
        keep = r != c
        r, c = r[keep], c[keep]
    A = sp.csr_array((np.ones(len(r)), (r, c)), shape=(n, n))
    A.sum_duplicates()
    A.sort_indices()
    return A


# ---- PageRank -------------------------------------------------------------------------------------------------------

def pagerank_loop(G, alpha=0.85, tol=1e-6, max_iter=100):
    """(x, iters, errs): the loop of include/mp_structure.h.  x is the x' of the first step with err < n tol, iters its
    number from 1 (-1 if max_iter steps did not get there), errs the err of every step taken.  The sums are SciPy's and
    NumPy's (a CSC product, builtin sum over the dangling nodes, a pairwise sum of |x' - x|), as in nx.pagerank."""
    n = G.number_of_nodes()
    A = adjacency(G)
    deg = np.asarray(A.sum(axis=1)).reshape(-1)
    inv = np.zeros(n)
    inv[deg != 0] = 1.0 / deg[deg != 0]
    A = sp.csr_array(sp.diags_array(inv)) @ A
    p = np.repeat(1.0 / n, n)
    x = p.copy()
    dangling = np.where(deg == 0)[0]
    errs = []
    for it in range(1, max_iter + 1):
        last = x
        x = alpha * (x @ A + sum(x[dangling]) * p) + (1 - alpha) * p
        errs.append(np.absolute(x - last).sum())
        if errs[-1] < n * tol:
            return x, it, errs
    return x, -1, errs


def nx_pagerank(G, **kw):
    pr = nx.pagerank(G, **kw)
    return np.array([pr[v] for v in range(G.number_of_nodes())], dtype=np.float64)


# ---- betweenness ----------------------------------------------------------------------------------------------------

def nx_betweenness(G):
    bc = nx.betweenness_centrality(G)
    return np.array([bc[v] for v in range(G.number_of_nodes())], dtype=np.float64)


def brandes(G, block=256):
    """(betweenness float64 [n], the largest sigma met): Brandes' algorithm, unweighted, normalized, endpoints left
    out, level-synchronous and for `block` sources at a time: column s of every [n, block] array belongs to source s.
    A dependency is sigma[v] (sum of coefficients) here and a sum of products in networkx: equal within rounding."""
    n = G.number_of_nodes()
    A = adjacency(G, loops=False)
    bc = np.zeros(n)
    top = 1.0 if n else 0.0
    for s0 in range(0, n, block):
        src = np.arange(s0, min(s0 + block, n))
        k = len(src)
        level = np.full((n, k), -1, dtype=np.int64)
        sigma = np.zeros((n, k))
        level[src, np.arange(k)] = 0
        sigma[src, np.arange(k)] = 1.0
        front = sigma.copy()
        depth = 0
        while True:
            paths = A @ front
            paths[level >= 0] = 0.0
            new = paths > 0
            if not new.any():
                break
            depth += 1
            level[new] = depth
            sigma[new] = paths[new]
            front = np.where(new, paths, 0.0)
        top = max(top, sigma.max())
        delta = np.zeros((n, k))
        for lv in range(depth - 1, -1, -1):
            coeff = np.zeros((n, k))
            below = level == lv + 1
            coeff[below] = (1.0 + delta[below]) / sigma[below]
            pulled = A @ coeff
            here = level == lv
            delta[here] = sigma[here] * pulled[here]
        delta[src, np.arange(k)] = 0.0
        bc += delta.sum(axis=1)
    scale = 1.0 / ((n - 1) * (n - 2)) if n > 2 else 0.0
    return bc * scale, top


# ---- the one-hot permutation ----------------------------------------------------------------------------------------

_M64 = (1 << 64) - 1
_M32 = (1 << 32) - 1
_GOLDEN = 0x9E3779B97F4A7C15
ONEHOT_STREAM = 0x6F6E65686F74       # include/mp_structure.h: MP_STRUCT_ONEHOT_STREAM
ROUNDS = 6


def _mix64(z):
    z &= _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def _round(half, key):
    x = (half + key) & _M32
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & _M32
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & _M32
    return x ^ (x >> 16)


def onehot_host(n_list, seed=0):
    """int64 [sum n_list]: entry i of graph g is perm(i) — csrc/draws.h keyed_perm, one Python integer at a time"""
    out = []
    for g, n in enumerate(n_list):
        h = _mix64((seed & _M64) + _GOLDEN)
        h = _mix64((h ^ ONEHOT_STREAM) + _GOLDEN)
        h = _mix64((h ^ g) + _GOLDEN)
        keys = [_mix64(h + (k + 1) * _GOLDEN) >> 32 for k in range(ROUNDS)]
        bits = (n - 1).bit_length()
        b = max(1, (bits + 1) // 2)
        mask = (1 << b) - 1
        for i in range(n):
            x = i
            while True:
                left, right = x >> b, x & mask
                for key in keys:
                    left, right = right, left ^ (_round(right, key) & mask)
                x = (left << b) | right
                if x < n:
                    break
            out.append(x)
    return np.array(out, dtype=np.int64)
