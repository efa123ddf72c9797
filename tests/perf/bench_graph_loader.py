"""Per-batch cost of the graph-task collation (graphgym_amd.graph_loader, csrc/collate.hip).  A script, not collected by
pytest.

Batches: 64 and 512 graphs of 20-30 nodes (molecule-like: a chain with ring closures, out of a dataset of 2048), and 64
graphs of 500 nodes (BA(500, 3), out of a dataset of 256).  Three paths build the same batch CSR:
  collate        graph_loader.collate: the whole harness.Batch (CSR, edge_index, owner, features, labels, pool operator,
                 seeded graph cache); collate_kernel is its upload + mp_collate_graphs alone
  induced        samplers.induced_subgraph on the node set of the same graphs (ids ascending: its only order), the node
                 list prepared outside the timed region
  torch          the torch formulation on the device: torch.cat of per-graph slices of the base's edge list with offsets
                 (the slices cut with host offsets, no read), then CSRGraph.from_edge_index
Per path and batch: wall_ms (host clock around the call and a final synchronise — a step waits for its batch this long),
device_ms (device events around the call), launches (kernels and copies torch's profiler lists for one call; null when
the profiler is unavailable) and host_reads (synchronising calls torch's sync debug mode reports for one call).
Medians of REPEATS calls after WARMUPS untimed ones, a different batch of the epoch per call.

    python tests/perf/bench_graph_loader.py profiles/graph_loader_bench.json"""
import json
import os
import statistics
import sys
import time
import warnings

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import graphgym_amd as ga  # noqa: E402
from graphgym_amd import graph_loader as GL, graphgen, samplers as S  # noqa: E402

dev = torch.device("cuda:0")
WARMUPS, REPEATS = int(os.environ.get("WARMUPS", "5")), int(os.environ.get("REPEATS", "30"))
out_path = sys.argv[1]


def molecules(G, seed):
    rng = np.random.RandomState(seed)
    graphs = []
    for _ in range(G):
        m = int(rng.randint(20, 31))
        links = {(i, i + 1) for i in range(m - 1)}
        for _ in range(3):
            a, b = sorted(int(v) for v in rng.randint(0, m, size=2))
            if b - a > 1:
                links.add((a, b))
        links = sorted(links)
        ei = torch.tensor(links + [(b, a) for a, b in links]).t().contiguous()
        graphs.append((ei, torch.from_numpy(rng.randn(m, 16).astype(np.float32)), torch.tensor(int(rng.randint(0, 2)))))
    return GL.GraphDataset.from_graphs(graphs, dev)


def ba500(G):
    graphs = [(graphgen.connected_ba_edge_index(500, 3, seed=50 + i), torch.randn(500, 16), torch.tensor(i % 2))
              for i in range(G)]
    return GL.GraphDataset.from_graphs(graphs, dev)


def measure(make_call, n_batches):
    """make_call(i) -> a zero-argument call that builds batch i"""
    calls = [make_call(i % n_batches) for i in range(WARMUPS + REPEATS)]
    for fn in calls[:WARMUPS]:
        fn()
    wall, device = [], []
    for fn in calls[WARMUPS:]:
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
        device.append(e0.elapsed_time(e1))
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            calls[0]()
        reads = sum("synchroniz" in str(w.message).lower() for w in caught)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    launches = None
    try:
        if os.environ.get("PROFILE", "1") != "1":
            raise RuntimeError("PROFILE=0")
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            calls[0]()
            torch.cuda.synchronize()
        launches = sum(1 for ev in prof.events() if "cuda" in str(ev.device_type).lower())
    except Exception as e:      # (the profiler is optional: the other three figures stand without it)
        print("profiler unavailable:", repr(e), flush=True)
    return {"wall_ms": round(statistics.median(wall), 4), "wall_min_ms": round(min(wall), 4),
            "device_ms": round(statistics.median(device), 4), "launches": launches, "host_reads": reads}


def bench(name, ds, B):
    base, gp, ep = ds.base, ds.graph_ptr, ds.entry_ptr
    src, dst = base.col.long(), base.row_ids().long()            # the base's edge list in CSR order (the torch path)
    order = GL.epoch_order(np.arange(ds.num_graphs), 1, 0)
    batches = [np.sort(order[i * B:(i + 1) * B]) for i in range(ds.num_graphs // B)]      # ascending: induced's order
    node_sets = [torch.cat([torch.arange(gp[g], gp[g + 1]) for g in ids]).to(dev) for ids in batches]

    def torch_path(ids):
        parts, at = [], 0
        for g in ids:
            e0, e1 = int(ep[g]), int(ep[g + 1])
            parts.append(torch.stack([src[e0:e1], dst[e0:e1]]) + (at - int(gp[g])))
            at += int(gp[g + 1] - gp[g])
        return ga.CSRGraph.from_edge_index(torch.cat(parts, 1), at, validate=False)

    ours, ind, ref = GL.collate(ds, batches[0]), S.induced_subgraph(base, node_sets[0]), torch_path(batches[0])
    same = all(torch.equal(ours.graph.rowptr, g.rowptr) and torch.equal(ours.graph.col, g.col) for g in (ind.graph, ref))
    r = {"graphs": B, "nodes": ours.num_nodes, "entries": ours.graph.nnz, "batches": len(batches), "same_csr": bool(same),
         "collate": measure(lambda i: (lambda: GL.collate(ds, batches[i])), len(batches)),
         "collate_kernel": measure(lambda i: (lambda: GL._collate_device(ds, batches[i])), len(batches)),
         "induced": measure(lambda i: (lambda: S.induced_subgraph(base, node_sets[i])), len(batches)),
         "torch": measure(lambda i: (lambda: torch_path(batches[i])), len(batches))}
    for other in ("induced", "torch"):
        r[other + "_over_collate_wall"] = round(r[other]["wall_ms"] / r["collate"]["wall_ms"], 2)
    print(name, json.dumps(r), flush=True)
    return r


small, large = molecules(2048, 1), ba500(256)
rec = {"device": torch.cuda.get_device_name(0), "warmups": WARMUPS, "repeats": REPEATS, "cases": {
    "64x20-30": bench("64x20-30", small, 64), "512x20-30": bench("512x20-30", small, 512),
    "64x500": bench("64x500", large, 64)}}
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(rec, f, indent=1)
print(json.dumps(rec))
