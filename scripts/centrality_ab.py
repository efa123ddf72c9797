"""A/B of the three raw quantities behind node_pagerank, node_betweenness_centrality and node_onehot by two routes:

  networkx  the reference's route (graphgym/models/feature_augment.py:55-58,70-73,88-91): per graph nx.pagerank(G),
            nx.betweenness_centrality(G) and torch.randperm(n), on this box's CPU;
  device    graphgym_amd.structure.node_pagerank / node_betweenness_centrality / node_onehot on the union of the
            dataset's graphs: wall-clock from a synchronised device to a synchronised device, the call's own host reads
            (graph sizes before, PageRank's iteration counts after) included, the cached symmetry check not.

Two inputs: a dataset of GRAPHS powerlaw-cluster graphs of NODES nodes (the shape of the reference's scalefree.pkl) and
one powerlaw-cluster graph of BIG nodes.  The device route is timed over ROUNDS calls after one untimed call (median,
p90, min in ms); networkx is timed once per input (it takes seconds to a minute).  The record also holds the largest
difference between the two routes' values.

    python scripts/centrality_ab.py [OUT.json]        # default profiles/centrality_bench.json"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import networkx as nx
import numpy as np
import torch
import graphgym_amd as ga
from graphgym_amd import structure as S

dev = torch.device("cuda:0")
GRAPHS = int(os.environ.get("GRAPHS", "256"))
NODES = int(os.environ.get("NODES", "64"))
BIG = int(os.environ.get("BIG", "3000"))
ROUNDS = int(os.environ.get("ROUNDS", "10"))
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "centrality_bench.json")


def p90(v):
    s = sorted(v)
    return s[min(len(s) - 1, int(round(0.9 * (len(s) - 1))))]


def union(graphs):
    parts, ptr = [], [0]
    for G in graphs:
        e = np.array(list(G.edges()), dtype=np.int64).reshape(-1, 2)
        parts.append(np.concatenate([e, e[:, ::-1]]) + ptr[-1])
        ptr.append(ptr[-1] + G.number_of_nodes())
    ei = torch.from_numpy(np.concatenate(parts).T.copy()).to(dev)
    return ga.CSRGraph.from_edge_index(ei, ptr[-1]), torch.tensor(ptr, dtype=torch.int64, device=dev)


def host_once(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def device_rounds(fn):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(ROUNDS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(statistics.median(t), 3), "p90_ms": round(p90(t), 3), "min_ms": round(min(t), 3)}, out


def values(per_graph, graphs):
    return np.concatenate([[d[v] for v in range(G.number_of_nodes())] for d, G in zip(per_graph, graphs)])


def run(name, graphs):
    base, gp = union(graphs)
    base.is_symmetric(run=True)
    rec = {"what": "centrality_ab", "input": name, "graphs": len(graphs), "nodes": base.num_nodes, "nnz": base.nnz,
           "rounds": ROUNDS}
    routes = (("node_pagerank", lambda: [nx.pagerank(G) for G in graphs], lambda: S.node_pagerank(base, gp)),
              ("node_betweenness_centrality", lambda: [nx.betweenness_centrality(G) for G in graphs],
               lambda: S.node_betweenness_centrality(base, gp)),
              ("node_onehot", lambda: [torch.randperm(G.number_of_nodes()) for G in graphs],
               lambda: S.node_onehot(base, gp)))
    for key, host, device in routes:
        host_ms, ref = host_once(host)
        stats, got = device_rounds(device)
        rec[key] = {"networkx_ms": round(host_ms, 3), "device": stats,
                    "networkx_over_device_median": round(host_ms / stats["median_ms"], 1)}
        if key != "node_onehot":
            rec[key]["max_abs_diff"] = float(np.abs(got.cpu().numpy() - values(ref, graphs)).max())
    print(json.dumps(rec), flush=True)
    return rec


records = [run(f"{GRAPHS} powerlaw-cluster graphs of {NODES} nodes",
               [nx.powerlaw_cluster_graph(NODES, 3, 0.5, seed=s) for s in range(GRAPHS)]),
           run(f"one powerlaw-cluster graph of {BIG} nodes", [nx.powerlaw_cluster_graph(BIG, 3, 0.5, seed=0)])]
with open(out_path, "w") as f:
    json.dump(records, f, indent=1)
    f.write("\n")
