"""Hand-made graph-task datasets for tests/test_graph_loader_host.py and tests/test_graph_loader_gpu.py: Python lists of
(edge_index with local ids, x, label, edge_feature) tuples, as graphgym_amd.graph_loader.GraphDataset.from_graphs takes
them, and the per-graph loop oracle the collation is checked against."""
import numpy as np
import torch

# a 1-node graph, an edgeless 3-node graph in the middle (id 3) and another one (id 9), a graph of 70 nodes (id 4: more
# than a wave of nodes, more than 256 entries together with its neighbours in a batch)
SIZES12 = [5, 1, 9, 3, 70, 12, 33, 2, 17, 3, 8, 6]
EDGELESS = (1, 3, 9)
# batches of the 12-graph sets: all graphs shuffled (B = G), one graph (B = 1; the 70-node one and the 1-node one), an
# edgeless graph first and another last, a repeated id
IDS12 = {
    "all_shuffled": [7, 3, 11, 0, 4, 9, 2, 6, 1, 10, 5, 8],
    "one_large": [4],
    "one_single_node": [1],
    "edgeless_first_and_last": [3, 4, 0, 6, 9],
    "repeated": [4, 1, 4, 7, 7],
}


def _links(n, rng, kind):
    """stored (src, dst) pairs of one graph of n nodes.  symmetric: a ring with chords, both directions, no repeat, no
    loop; directed: the ring one way plus chords one way; multi: the symmetric links plus repeated entries and self loops"""
    if n == 1:
        return [(0, 0), (0, 0)] if kind == "multi" else []
    links = {(i, (i + 1) % n) for i in range(n)} if n > 2 else {(0, 1)}
    for _ in range(n // 3):
        a, b = (int(v) for v in rng.randint(0, n, size=2))
        if a != b:
            links.add((a, b))
    links = sorted({(min(a, b), max(a, b)) for a, b in links})
    if kind == "directed":
        return links
    both = links + [(b, a) for a, b in links]
    if kind == "multi":
        both += [both[0], both[-1], (0, 0), (n - 1, n - 1), (0, 0)]
    order = rng.permutation(len(both))
    return [both[i] for i in order]                        # (stored in no particular order: the CSR sorts them)


def make_graphs(sizes, kind="symmetric", seed=0, width=8, dtype=torch.float32, edge_width=3):
    """dtype float32 / bfloat16: random features; int64: integer codes in [0, 7)"""
    rng = np.random.RandomState(seed)
    graphs = []
    for gi, n in enumerate(sizes):
        links = [] if gi in EDGELESS and len(sizes) == len(SIZES12) and kind != "multi" else _links(n, rng, kind)
        ei = torch.tensor(links, dtype=torch.int64).reshape(-1, 2).t().contiguous()
        if dtype == torch.int64:
            x = torch.from_numpy(rng.randint(0, 7, size=(n, width)))
        else:
            x = torch.from_numpy(rng.randn(n, width).astype(np.float32)).to(dtype)
        ef = torch.from_numpy(rng.randn(ei.size(1), edge_width).astype(np.float32))
        graphs.append((ei, x, torch.tensor(int(rng.randint(0, 4))), ef))
    return graphs


def loop_collate(graphs, ids):
    """The batch of graphs[i] for i in ids as a PyG / DeepSNAP collate builds it — every graph's edge_index shifted by
    the nodes before it, everything concatenated — with each graph's edges in (destination, source) order, equal pairs
    in stored order: the order of a CSR whose rows are destinations.  A plain per-graph Python loop."""
    eis, xs, efs, owner, orig, labels, node_off, at = [], [], [], [], [], [], [0], 0
    starts = np.concatenate([[0], np.cumsum([g[1].size(0) for g in graphs])])
    for j, i in enumerate(ids):
        ei, x, label, ef = graphs[i]
        n = x.size(0)
        order = sorted(range(ei.size(1)), key=lambda e: (int(ei[1, e]), int(ei[0, e]), e))
        eis.append(ei[:, order] + at)
        efs.append(ef[order])
        xs.append(x)
        owner += [j] * n
        orig += list(range(int(starts[i]), int(starts[i]) + n))
        labels.append(label)
        at += n
        node_off.append(at)
    return dict(edge_index=torch.cat(eis, 1), node_feature=torch.cat(xs, 0), edge_feature=torch.cat(efs, 0),
                batch=torch.tensor(owner, dtype=torch.int64), orig_node=torch.tensor(orig, dtype=torch.int64),
                graph_label=torch.stack(labels), node_off=torch.tensor(node_off, dtype=torch.int32), num_nodes=at)


BATCH_TENSORS = ("edge_index", "node_feature", "edge_feature", "graph_label", "batch", "orig_node", "base_entry")


def assert_batches_equal(a, b, what=""):
    """bit for bit: the batch's CSR (rowptr, col, val), owner, orig_node, base_entry, edge_index, node_feature,
    edge_feature, graph_label and the pool operator's rowptr and col, of two harness.Batch objects on any devices"""
    cpu = lambda t: t.detach().cpu()                                                      # noqa: E731
    assert a.num_nodes == b.num_nodes and a.num_graphs == b.num_graphs, what
    for k in BATCH_TENSORS:
        assert hasattr(a, k) == hasattr(b, k), (what, k)
        if hasattr(a, k):
            ta, tb = cpu(getattr(a, k)), cpu(getattr(b, k))
            assert ta.dtype == tb.dtype and ta.shape == tb.shape and torch.equal(ta, tb), (what, k)
    for ga, gb, names in ((a.graph, b.graph, ("rowptr", "col", "val", "eid")),
                          (a.pool_operator, b.pool_operator, ("rowptr", "col"))):
        assert (ga.num_nodes, ga.num_cols, ga.nnz) == (gb.num_nodes, gb.num_cols, gb.nnz), what
        for k in names:
            ta, tb = getattr(ga, k), getattr(gb, k)
            assert (ta is None) == (tb is None), (what, k)
            if ta is not None:
                assert ta.dtype == tb.dtype and torch.equal(cpu(ta), cpu(tb)), (what, k)
