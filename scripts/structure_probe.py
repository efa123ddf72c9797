"""Structural labels on the GPU (csrc/structure.hip): mp_csr_triangles and mp_hop_sums at the shapes the project is
measured at, with the host loops they replace as context.

  triangles   100 x BA(64, 2) (the shape of the reference's ba.pkl), powerlaw_cluster(1e6, 5, 0.3), and the bench graph
              BA(1e7, 5); with the model's work  sum over entries of min(d_u, d_v) * ceil(log2 max(d_u, d_v))  probes
              and the probes per second achieved
  hop sums    every node a source, on 100 x BA(64, 2) and on BA(2708, 2) (Cora's size)
  host        nx.clustering per node and the reference's shortest_path_length loop on the 100-graph batch;
              scipy's (A @ A).multiply(A) row sums at 1e6 nodes

Kernel times are device events around the prepared launch (structure.run_triangles / run_hop_sums), median of 30 after 5
warm-ups; the binding (structure.triangles / hop_sums: symmetry check cached, allocation, launch) is timed with the host
clock to a synchronise.  Every case runs in a process of its own under a time limit; the first failure ends the run.

    python scripts/structure_probe.py [--out profiles/structure_probe.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WARM, REPS = 5, 30
CASES = {  # name -> time limit of its process, seconds
    "tri_ba64x100": 120, "tri_powerlaw_1e6": 240, "tri_ba_1e7": 420, "hops_ba64x100": 120, "hops_ba2708": 120,
    "host_ba64x100": 240, "host_scipy_1e6": 240}


def kernel_ms(fn):
    import torch
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return {"kernel_ms": statistics.median(ts), "kernel_ms_min": min(ts), "kernel_ms_max": max(ts)}


def wall_ms(fn):
    import torch
    for _ in range(WARM):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(REPS):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def union(n_graphs, n, m, dev):
    import torch
    import graphgym_amd as ga
    from graphgym_amd import graphgen
    eis, ptr = [], [0]
    for s in range(n_graphs):
        eis.append(graphgen.ba_edge_index(n, m, seed=s) + ptr[-1])
        ptr.append(ptr[-1] + n)
    return ga.CSRGraph.from_edge_index(torch.cat(eis, 1).to(dev), ptr[-1]), torch.tensor(ptr, dtype=torch.int64)


def model_probes(base):
    """the binary-search probes the triangle kernel's cost model counts"""
    import torch
    d = (base.rowptr[1:] - base.rowptr[:-1]).long()
    du, dv = d[base.row_ids().long()], d[base.col.long()]
    lo, hi = torch.minimum(du, dv), torch.maximum(du, dv)
    return int((lo * torch.ceil(torch.log2(hi.double())).long()).sum())


def triangles_case(name, base):
    import torch
    from graphgym_amd import structure as S
    tri2 = torch.empty(base.num_nodes, dtype=torch.int64, device=base.device)
    deg = torch.empty(base.num_nodes, dtype=torch.int32, device=base.device)
    base.row_ids()
    rec = {"case": name, "device": torch.cuda.get_device_name(0), "nodes": base.num_nodes, "entries": base.nnz,
           "longest_row": int((base.rowptr[1:] - base.rowptr[:-1]).max())}
    rec.update(kernel_ms(lambda: S.run_triangles(base, tri2, deg)))
    rec["binding_ms"] = wall_ms(lambda: S.triangles(base))
    rec["triangles"] = int(tri2.sum()) // 6
    rec["model_probes"] = model_probes(base)
    rec["probes_per_s"] = rec["model_probes"] / (rec["kernel_ms"] * 1e-3)
    rec["entries_per_s"] = base.nnz / (rec["kernel_ms"] * 1e-3)
    return rec


def hops_case(name, base, gp):
    import torch
    from graphgym_amd import structure as S
    plan = S.plan_hop_sums(base, gp.to(base.device))
    rec = {"case": name, "device": torch.cuda.get_device_name(0), "nodes": base.num_nodes, "entries": base.nnz,
           "sources": plan.n_sources,
           "largest_graph": plan.biggest}
    rec.update(kernel_ms(lambda: S.run_hop_sums(plan)))
    rec["binding_ms"] = wall_ms(lambda: S.hop_sums(base, gp))
    rec["deepest_sum"] = int(plan.dist_sum.max())
    return rec


def run_case(name):
    import numpy as np
    if name == "host_ba64x100":
        import networkx as nx
        graphs = [nx.barabasi_albert_graph(64, 2, seed=s) for s in range(100)]
        t0 = time.perf_counter()
        for G in graphs:
            [nx.clustering(G, v) for v in G.nodes]
        t1 = time.perf_counter()
        for G in graphs:
            [np.mean(list(nx.shortest_path_length(G, source=x).values())) for x in G.nodes]
        t2 = time.perf_counter()
        return {"case": "host: networkx on 100 x BA(64, 2)", "nx_clustering_ms": (t1 - t0) * 1e3,
                "shortest_path_length_loop_ms": (t2 - t1) * 1e3}
    if name == "host_scipy_1e6":
        import scipy.sparse as sp
        from graphgym_amd import graphgen
        ei = graphgen.ba_edge_index(10 ** 6, 5, triangle_p=0.3).numpy()
        A = sp.csr_matrix((np.ones(ei.shape[1], dtype=np.int64), (ei[1], ei[0])), shape=(10 ** 6, 10 ** 6))
        t0 = time.perf_counter()
        tri2 = np.asarray((A @ A).multiply(A).sum(1)).ravel()
        t1 = time.perf_counter()
        return {"case": "host: scipy (A @ A).multiply(A) row sums, powerlaw_cluster(1e6, 5, 0.3)", "entries": int(A.nnz),
                "ms": (t1 - t0) * 1e3, "triangles": int(tri2.sum()) // 6}
    import torch
    import graphgym_amd as ga
    from graphgym_amd import graphgen
    dev = torch.device("cuda:0")
    if name == "tri_ba64x100":
        return triangles_case("100 x BA(64, 2)", union(100, 64, 2, dev)[0])
    if name == "tri_powerlaw_1e6":
        ei = graphgen.ba_edge_index(10 ** 6, 5, device=dev, triangle_p=0.3)
        return triangles_case("powerlaw_cluster(1e6, 5, 0.3)", ga.CSRGraph.from_edge_index(ei, 10 ** 6))
    if name == "tri_ba_1e7":
        ei = graphgen.ba_edge_index(10 ** 7, 5, device=dev)
        return triangles_case("BA(1e7, 5)", ga.CSRGraph.from_edge_index(ei, 10 ** 7))
    if name == "hops_ba64x100":
        return hops_case("100 x BA(64, 2), every node a source", *union(100, 64, 2, dev))
    if name == "hops_ba2708":
        return hops_case("BA(2708, 2), every node a source", *union(1, 2708, 2, dev))
    raise SystemExit(f"unknown case {name}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "structure_probe.json"))
    ap.add_argument("--case", choices=sorted(CASES), help="run one case in this process and print its record")
    args = ap.parse_args()
    if args.case:
        print("RECORD " + json.dumps(run_case(args.case)), flush=True)
        return 0
    recs, device = [], None
    for name, limit in CASES.items():          # a fresh process per case, each under its own time limit
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", name], capture_output=True,
                               text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"{name}: no result within {limit} s; stopping", flush=True)
            return 1
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("RECORD ")]
        if p.returncode != 0 or not lines:
            print(f"{name}: exit status {p.returncode}; stopping\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}", flush=True)
            return 1
        recs.append(json.loads(lines[-1][len("RECORD "):]))
        device = recs[-1].pop("device", device)
        print(json.dumps(recs[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": device, "warmups": WARM, "repeats": REPS,
                   "note": "first measurement of these kernels: no earlier number exists to compare against",
                   "records": recs}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
