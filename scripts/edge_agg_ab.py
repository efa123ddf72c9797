"""A/B of the two-gather aggregation (ops.spmm_edge, mp_spmm_csr_edge_f32) against the composition it replaces,
gather_rows + add + spmm(edge_operator), for max over messages X[col] + M[eid], on a BA graph (graphgen, 2e6 nodes, m = 5:
~2e7 entries), d = 256, so M [E, d] is ~20 GB and the composition's per-entry tensor as much again.

One process, the same buffers; the two forms alternate over ROUNDS rounds of ITERS back-to-back runs each (one untimed run
first); medians in ms.  The outputs are compared with torch.equal.  Algorithmic bytes of the kernel:
nnz * (2 * d * 4 + 12) + N * d * 4.

    NODES=2000000 D=256 python scripts/edge_agg_ab.py OUT.jsonl"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import graphgym_amd as ga
from graphgym_amd import _lib, graphgen, ops

dev = torch.device("cuda:0")
n = int(os.environ.get("NODES", "2000000"))
d = int(os.environ.get("D", "256"))
ROUNDS = int(os.environ.get("ROUNDS", "5"))
ITERS = int(os.environ.get("ITERS", "3"))
out_path = sys.argv[1]


def timed(fn):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


ei = graphgen.ba_edge_index(n, 5, seed=12345, device=dev)
g = ga.CSRGraph.from_edge_index(ei, n)
E = ei.size(1)
gen = torch.Generator(device=dev).manual_seed(7)
X = torch.empty((n, d), device=dev).uniform_(-1.0, 1.0, generator=gen)
M = torch.empty((E, d), device=dev).uniform_(-1.0, 1.0, generator=gen)
col, eid = g.col.long(), g.eid.long()
g.plan(), g.edge_operator().plan(), g.max_row_entries()


def new():
    return ops._raw_spmm_edge(g, X, M, None, None, _lib.MAX, False)[0]


def old():
    msg = ops.gather_rows(X, col) + M[eid]
    return ops.spmm(g.edge_operator(), msg, "max")


with torch.no_grad():
    same = torch.equal(new(), old())
    t_new, t_old = [], []
    for _ in range(ROUNDS):
        t_new.append(timed(new))
        t_old.append(timed(old))
bytes_alg = g.nnz * (2 * d * 4 + 12) + n * d * 4
med_new, med_old = statistics.median(t_new), statistics.median(t_old)
rec = {"what": "edge_agg_ab", "reduce": "max", "n": n, "nnz": g.nnz, "d": d, "rounds": ROUNDS, "iters": ITERS,
       "M_GB": round(E * d * 4 / 1e9, 2), "equal": bool(same),
       "two_gather_ms": {"median": round(med_new, 3), "min": round(min(t_new), 3), "all": [round(t, 3) for t in t_new]},
       "composition_ms": {"median": round(med_old, 3), "min": round(min(t_old), 3), "all": [round(t, 3) for t in t_old]},
       "speedup": round(med_old / med_new, 3), "algorithmic_GB": round(bytes_alg / 1e9, 3),
       "algorithmic_TBps": round(bytes_alg / (med_new * 1e-3) / 1e12, 3),
       "fraction_of_8TBps": round(bytes_alg / (med_new * 1e-3) / 8e12, 3)}
print(json.dumps(rec), flush=True)
with open(out_path, "a") as f:
    f.write(json.dumps(rec) + "\n")
