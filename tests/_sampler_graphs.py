"""Hand-made bases for the sampler tests (tests/test_samplers_host.py, tests/test_samplers_gpu.py) and the brute-force
dense count matrix the induced subgraph is checked against.  A case is (edges, N): edges are (src, dst) pairs exactly as
stored (an undirected link appears in both directions), repeats and self loops included."""
import numpy as np
import torch


def _both(links):
    return [(u, v) for u, v in links] + [(v, u) for u, v in links if u != v]


def _ring_with_chords(n):
    """an undirected ring of n nodes with the chords i - (i + 5) of every third node: sizes at the bitmap's word edges"""
    return _both([(i, (i + 1) % n) for i in range(n)] + [(i, (i + 5) % n) for i in range(0, n, 3)])


CASES = {
    "path5": (_both([(0, 1), (1, 2), (2, 3), (3, 4)]), 5),
    "star200": (_both([(0, i) for i in range(1, 201)]), 201),            # row 0: more than three 64-entry chunks
    "triangle_pendant_isolated": (_both([(0, 1), (1, 2), (0, 2), (2, 3)]), 5),      # node 4 is isolated
    "multigraph": (_both([(0, 1), (1, 2)]) + [(1, 1), (0, 1), (1, 0), (2, 3), (3, 2), (2, 3), (3, 2)], 4),
    "cycle6_chord": ([(i, (i + 1) % 6) for i in range(6)] + [(0, 3)], 6),           # directed
    "ring31": (_ring_with_chords(31), 31),
    "ring32": (_ring_with_chords(32), 32),
    "ring33": (_ring_with_chords(33), 33),
    "ring64": (_ring_with_chords(64), 64),
    "ring65": (_ring_with_chords(65), 65),
}
ISOLATED = ("triangle_pendant_isolated", 4)


def edge_index(name):
    edges, N = CASES[name]
    return torch.tensor(edges, dtype=torch.int64).reshape(-1, 2).t().contiguous(), N


def build(name, device=None):
    """the base CSRGraph of a case: on the CPU (link_pred.host_csr), or on `device` through the engine"""
    from graphgym_amd import CSRGraph
    from graphgym_amd.link_pred import host_csr
    ei, N = edge_index(name)
    return host_csr(ei, N) if device is None else CSRGraph.from_edge_index(ei.to(device), N)


def dense_counts(name):
    """A[dst, src] = how often the case stores (src, dst)"""
    edges, N = CASES[name]
    A = np.zeros((N, N), dtype=np.int64)
    for s, d in edges:
        A[d, s] += 1
    return A


def node_sets(N, seed=0, n_random=20):
    """the node sets every base is cut by: empty, one node, all nodes, node N - 1 alone, n_random seeded random subsets
    (given with repeats and out of order, as draws come)"""
    rng = np.random.RandomState(seed)
    sets = [[], [N // 2], list(range(N)), [N - 1]]
    for _ in range(n_random):
        k = rng.randint(1, N + 1)
        sets.append(rng.randint(0, N, size=k).tolist())
    return sets


def csr_to_dense(rowptr, col, n):
    A = np.zeros((n, n), dtype=np.int64)
    rowptr, col = np.asarray(rowptr), np.asarray(col)
    for r in range(n):
        for c in col[rowptr[r]:rowptr[r + 1]]:
            A[r, c] += 1
    return A


def stored(name):
    """the set of (src, dst) pairs a case stores"""
    return set(CASES[name][0])
