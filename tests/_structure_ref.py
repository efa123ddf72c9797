"""networkx / numpy restatement of graphgym/models/feature_augment.py for the tests of graphgym_amd.structure: the raw
quantities the way the reference computes them (one networkx call per node or graph, :51-107) and the dataset-wide
representation (:134-245) in numpy.  Graphs are nx.Graphs whose nodes are 0..n-1 in order."""
import networkx as nx
import numpy as np
import torch


def path_graph(n):
    return nx.path_graph(n)


def pc_graphs(count=20, n=64, m=3, p=0.5, loops=True):
    """`count` powerlaw-cluster graphs; every other one gets an explicit self loop (networkx skips it in the
    clustering, G.degree() counts it twice)"""
    out = []
    for s in range(count):
        G = nx.powerlaw_cluster_graph(n, m, p, seed=s)
        if loops and s % 2 == 0:
            G.add_edge(5 + s, 5 + s)
        out.append(G)
    return out


def ba_graphs(count=20, n=64, m=2):
    return [nx.barabasi_albert_graph(n, m, seed=s) for s in range(count)]


def union(graphs):
    """(edge_index [2, E] int64 with both directions of every edge and a self loop once, graph_ptr [G+1], N)"""
    parts, ptr = [], [0]
    for G in graphs:
        assert list(G.nodes) == list(range(G.number_of_nodes()))
        e = np.array(list(G.edges()), dtype=np.int64).reshape(-1, 2)
        loop = e[:, 0] == e[:, 1]
        parts.append(np.concatenate([e[~loop], e[~loop][:, ::-1], e[loop]]) + ptr[-1])
        ptr.append(ptr[-1] + G.number_of_nodes())
    ei = np.concatenate(parts) if parts else np.zeros((0, 2), dtype=np.int64)
    return torch.from_numpy(ei.T.copy()), torch.tensor(ptr, dtype=torch.int64), ptr[-1]


def base_of(graphs, dev):
    import graphgym_amd as ga
    ei, gp, n = union(graphs)
    return ga.CSRGraph.from_edge_index(ei.to(dev), n), gp


# ---- raw quantities, as the reference computes them ----------------------------------------------------------------

def degree(graphs):
    return np.array([d for G in graphs for _, d in G.degree()], dtype=np.int64)                 # degree_fun


def triangles(graphs):
    return np.array([t for G in graphs for t in nx.triangles(G).values()], dtype=np.int64)


def clustering(graphs):
    return np.array([c for G in graphs for c in nx.clustering(G).values()], dtype=np.float64)   # clustering_coefficient_fun


def average_clustering(graphs):
    return np.array([nx.average_clustering(G) for G in graphs], dtype=np.float64)               # graph_clustering_fun


def node_path_len(graphs):
    return np.array([np.mean(list(nx.shortest_path_length(G, source=x).values()))                # path_len_fun
                     for G in graphs for x in G.nodes], dtype=np.float64)


def graph_path_len(graphs):
    return np.array([nx.average_shortest_path_length(G) for G in graphs], dtype=np.float64)     # graph_path_len_fun


# ---- representation (feature_augment.py:134-245) in numpy -----------------------------------------------------------

def np_bin_edges(values, dim, method):
    arr = np.asarray(values)
    if method == "balanced":
        at = np.linspace(0, len(arr), num=dim, endpoint=False).astype(int)
        bins = np.sort(arr)[at]
        unique = np.unique(bins)
        return unique if len(unique) < len(bins) else bins
    if method == "equal_width":
        return np.linspace(np.min(arr), np.max(arr), num=dim)
    if method == "bounded":
        return np.arange(dim)
    raise ValueError(method)


def np_digitize(values, edges):
    feat = np.digitize(np.asarray(values), edges) - 1
    assert np.min(feat) >= 0 and np.max(feat) <= len(edges) - 1
    return feat


def np_one_hot(classes, dim):
    out = np.zeros((len(classes), dim), dtype=np.float32)
    out[np.arange(len(classes)), classes] = 1.0
    return out


def np_position(values, dim, wavelength=10000):
    """_position_features with scale = dim / 2 / max, in float64"""
    pos = np.asarray(values, dtype=np.float64) * (dim / 2 / np.max(values))
    cycle = np.arange(dim // 2, dtype=np.float64) / (dim // 2)
    arg = pos[:, None] / wavelength ** cycle[None, :]
    return np.concatenate([np.cos(arg), np.sin(arg)], axis=-1)
