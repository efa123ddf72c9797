"""Hand-made graphs for the link-prediction tests (tests/test_link_pred_host.py, tests/test_link_pred_gpu.py) and the
brute-force complement they are checked against.  A case is (links, graph sizes): links are (u, v) in global ids.  The
undirected build stores every link in both directions (a self loop once); the directed build stores u -> v alone."""
import itertools

import torch

CASES = {
    "path4": ([(0, 1), (1, 2), (2, 3)], [4]),
    "star6": ([(0, i) for i in range(1, 6)], [6]),
    "components": ([(0, 1), (1, 2), (3, 4)], [6]),                  # two components and the isolated node 5
    "self_loop": ([(0, 1), (1, 1), (1, 2), (2, 3)], [4]),
    "k4": (list(itertools.combinations(range(4), 2)), [4]),         # C = 0 (the directed build stores both directions)
    "empty2": ([], [2]),                                            # C = 1 undirected, 2 directed
    "batch_2_5_9": ([(0, 1)] + [(2 + i, 2 + (i + 1) % 5) for i in range(5)]
                    + [(7, 8), (7, 9), (7, 15), (8, 9), (10, 11), (10, 10), (11, 12), (12, 13), (13, 14), (9, 14)],
                    [2, 5, 9]),
}


def graph_ptr(sizes):
    return torch.tensor([0] + list(itertools.accumulate(sizes)), dtype=torch.int64)


def edge_index(links, directed, both=False):
    """[2, E] int64 (src, dst): undirected links in both directions, directed ones as given (both: and reversed)"""
    e = set()
    for u, v in links:
        e.add((u, v))
        if (not directed or both) and u != v:
            e.add((v, u))
    e = sorted(e)
    return torch.tensor(e, dtype=torch.int64).reshape(-1, 2).t().contiguous()


def build(name, directed, device=None):
    """(base CSRGraph, graph_ptr, stored (src, dst) set) of a case: on the CPU, or on `device` through the engine"""
    links, sizes = CASES[name]
    return build_links(links, sizes, directed, device, both=(name == "k4"))


def build_links(links, sizes, directed, device=None, both=False):
    from graphgym_amd import CSRGraph
    from graphgym_amd.link_pred import host_csr
    ei, gp = edge_index(links, directed, both), graph_ptr(sizes)
    N = int(gp[-1])
    if device is None:
        base = host_csr(ei, N)
    else:
        base = CSRGraph.from_edge_index(ei.to(device), N)
    return base, gp, set(zip(ei[0].tolist(), ei[1].tolist()))


def complement(stored, gp, directed):
    """per graph, the set of candidate pairs that are not stored: (lo, hi) undirected, (src, dst) directed"""
    out = []
    gp = gp.tolist()
    for lo, hi in zip(gp[:-1], gp[1:]):
        if directed:
            out.append({(s, d) for s in range(lo, hi) for d in range(lo, hi) if s != d and (s, d) not in stored})
        else:
            out.append({(a, b) for a in range(lo, hi) for b in range(a + 1, hi) if (a, b) not in stored})
    return out


def with_complement_of(C, directed):
    """a one-graph case whose complement holds exactly C pairs (1 <= C <= 40): the first pairs in lexicographic order
    are links, the last C are not — 10 nodes (45 unordered pairs) or 7 nodes (42 ordered pairs)"""
    if directed:
        pairs = [(s, d) for s in range(7) for d in range(7) if s != d]
        return pairs[:len(pairs) - C], [7]
    pairs = list(itertools.combinations(range(10), 2))
    return pairs[:len(pairs) - C], [10]


# 12 nodes, 66 unordered pairs, 16 links: 50 free pairs
UNIFORMITY = ([(i, (i + 1) % 12) for i in range(12)] + [(0, 6), (1, 7), (2, 8), (3, 9)], [12])


def check_sample(out, counts, gp, stored, directed):
    """the properties every draw must have: counts[g] pairs per graph in slot order, inside the graph, src != dst, not
    stored (undirected: lo < hi, which with a symmetric `stored` covers both directions), no pair twice"""
    assert out.dtype == torch.int64 and tuple(out.shape) == (2, sum(counts))
    free = complement(stored, gp, directed)
    pairs = list(zip(out[0].tolist(), out[1].tolist()))
    at = 0
    for g, k in enumerate(counts):
        mine = pairs[at:at + k]
        at += k
        assert len(set(mine)) == k, f"graph {g}: a pair is repeated"
        for p in mine:
            assert p[0] != p[1]
            assert p in free[g], f"graph {g}: {p} is stored or outside the graph"
    return pairs
