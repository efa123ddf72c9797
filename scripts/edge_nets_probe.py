"""Edge-net batches and hop distances (csrc/edge.hip) at two shapes, on the GPU:

  ba64   100 BA(64, 2) graphs (the shape of the reference's ba.pkl), every node a source; path-length labels
         (1 000 pairs per graph)
  cora   one BA(2708, 2) graph (Cora's size: 2 708 nodes, ~10.8k stored entries), 1 000 path-length pairs, copies for
         the label sources only (sources="labels")

Kernel times are device events around launches of the prepared call (edge_nets.plan_* / run_*), median over repeats
after warm-ups; end-to-end times (the binding: planning, one size read, the launch) are host clocks around a device
synchronise.  The expansion's bytes follow DESIGN.md's model: 24 B per emitted edge (two int64 ends + orig_edge), 8 B
per CSR entry (col, eid), 12 B per node (orig_node + copy_of_node) + 4 B with the CSR (its row start).  The networkx
restatement of tests/_edge_ref.py is timed on the host for ten graphs of the small shape.

    python scripts/edge_nets_probe.py [--out profiles/edge_nets_probe.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import graphgym_amd as ga                                  # noqa: E402
from graphgym_amd import edge_nets as E, graphgen            # noqa: E402

HBM_PEAK = 8.0e12          # MI355X HBM3E, spec (MI355X_MICROARCH: 6.29 TB/s measured with a float4 copy)
WARM, REPS = 5, 30


def kernel_ms(fn):
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
    return statistics.median(ts), min(ts), max(ts)


def wall_ms(fn):
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
    eis, ptr = [], [0]
    for s in range(n_graphs):
        eis.append(graphgen.ba_edge_index(n, m, seed=s) + ptr[-1])
        ptr.append(ptr[-1] + n)
    ei = torch.cat(eis, 1).to(dev)
    return ga.CSRGraph.from_edge_index(ei, ptr[-1]), torch.tensor(ptr, dtype=torch.int64)


def expansion_bytes(plan):
    csr = bool(plan.flags)
    return plan.e_out * 24 + (plan.nnz_out * 8 if csr else 0) + plan.n_out * (16 if csr else 12) + (4 if csr else 0)


def measure(name, base, gp, sources, num_label, dev):
    rec = {"case": name, "graphs": gp.numel() - 1, "base_nodes": base.num_nodes, "base_entries": base.nnz}
    gen = torch.Generator().manual_seed(0)
    eli, lab = E.path_len_labels(base, gp, num_label=num_label, generator=gen)
    rec["label_pairs_kept"] = int(lab.numel())
    rec["path_len_labels_ms"] = wall_ms(lambda: E.path_len_labels(base, gp, num_label=num_label,
                                                                  generator=torch.Generator().manual_seed(0)))
    # the hop distances of the drawn pairs alone
    pairs = torch.cat([torch.randint(int(gp[g + 1] - gp[g]), (2, num_label), generator=torch.Generator().manual_seed(g))
                       + int(gp[g]) for g in range(gp.numel() - 1)], 1).to(dev)
    hp = E.plan_hops(base, pairs[0].contiguous(), pairs[1].contiguous(), gp.to(dev))
    rec["hops"] = {"pairs": hp.n_pairs, "sources": hp.n_sources}
    med, lo, hi = kernel_ms(lambda: E.run_hops(hp))
    rec["hops"].update(kernel_ms=med, kernel_ms_min=lo, kernel_ms_max=hi)
    copies = torch.arange(base.num_nodes, device=dev) if sources is None else torch.unique(eli[0])
    for csr in (None, "add"):
        flags = 0 if csr is None else E.FLAG_CSR | E.FLAG_CSR_SELF_LOOPS
        plan = E.plan_expansion(base, gp.to(dev), copies, flags)
        med, lo, hi = kernel_ms(lambda: E.run_expansion(plan))
        nbytes = expansion_bytes(plan)
        e2e = wall_ms(lambda: E.edge_batch(base, gp, eli, lab, sources=sources, csr=csr))
        rec["expand_csr_" + str(csr).lower()] = {
            "copies": plan.n_copies, "nodes": plan.n_out, "edges": plan.e_out, "csr_entries": plan.nnz_out if flags else 0,
            "bytes_written": nbytes, "kernel_ms": med, "kernel_ms_min": lo, "kernel_ms_max": hi,
            "write_TBps": nbytes / (med * 1e-3) / 1e12, "frac_hbm_peak": nbytes / (med * 1e-3) / HBM_PEAK,
            "edge_batch_ms": e2e}
    return rec


def restatement(n_graphs=10):
    import _edge_ref as R
    graphs = [R.ba_graph(64, 2, seed=s) for s in range(n_graphs)]
    t0 = time.perf_counter()
    for G in graphs:
        R.edge_nets(G)
    t1 = time.perf_counter()
    gen = torch.Generator().manual_seed(0)
    for G in graphs:
        R.path_len(G, 1000, gen)
    t2 = time.perf_counter()
    return {"case": "networkx restatement, BA(64, 2)", "graphs": n_graphs,
            "edge_nets_ms_per_graph": (t1 - t0) * 1e3 / n_graphs, "path_len_ms_per_graph": (t2 - t1) * 1e3 / n_graphs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "edge_nets_probe.json"))
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    recs = []
    base, gp = union(100, 64, 2, dev)
    recs.append(measure("ba64 x100, every node a source", base, gp, None, 1000, dev))
    print(json.dumps(recs[-1]), flush=True)
    base, gp = union(1, 2708, 2, dev)
    recs.append(measure("cora-size BA(2708, 2), 1000 pairs, sources='labels'", base, gp, "labels", 1000, dev))
    print(json.dumps(recs[-1]), flush=True)
    recs.append(restatement())
    print(json.dumps(recs[-1]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump({"device": torch.cuda.get_device_name(0), "warmups": WARM, "repeats": REPS, "records": recs}, f,
                  indent=1)


if __name__ == "__main__":
    main()
