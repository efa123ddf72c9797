"""Timings of the negative sampler (graphgym_amd.link_pred, csrc/link.hip) on the BA(N, 5) graph graphgen builds: K = nnz / 2
negatives (ratio 1 of an undirected graph).  A script, not collected by pytest.

  plan_negatives   mp_pair_space_rows + the prefix sum + the one host read, device events around the call
  run_negatives    one mp_sample_non_edges launch, device events
  host             the NumPy restatement (link_pred._sample_host, vectorised) over the first SLICE samples of the same
                   draw, wall clock, scaled by K / SLICE; its arrays are prepared outside the timed region.  The slice
                   is compared with the device's first SLICE samples (sample i does not depend on K).
  aggregation      ops.spmm(g, x, "sum") at d = D over the same graph, for scale

Medians of REPEATS runs after WARMUPS untimed ones.

    N=1000000 python tests/perf/bench_link_pred.py profiles/link_pred.json"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402
import graphgym_amd as ga  # noqa: E402
from graphgym_amd import graphgen, link_pred as LP, ops  # noqa: E402

dev = torch.device("cuda:0")
N = int(os.environ.get("N", "1000000"))
D = int(os.environ.get("D", "128"))
SLICE = int(os.environ.get("SLICE", "100000"))
WARMUPS, REPEATS = int(os.environ.get("WARMUPS", "5")), int(os.environ.get("REPEATS", "20"))
out_path = sys.argv[1]


def timed(fn):
    for _ in range(WARMUPS):
        fn()
    ts = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


ei = graphgen.ba_edge_index(N, 5, seed=12345).to(dev)
base = ga.CSRGraph.from_edge_index(ei, N)
gp = torch.tensor([0, N])
K = base.nnz // 2
plan = LP.plan_negatives(base, gp, [K])
assert plan.directed is False
rec = {"device": torch.cuda.get_device_name(0), "cpus_of_the_process": len(os.sched_getaffinity(0)),
       "cpus_of_the_machine": os.cpu_count(), "torch_threads": torch.get_num_threads(),
       "graph": f"BA({N}, 5)", "nodes": N, "entries": base.nnz, "negatives": K, "non_edges": plan.C_host[0],
       "warmups": WARMUPS, "repeats": REPEATS}
rec["plan_negatives"] = timed(lambda: LP.plan_negatives(base, gp, [K], False))
step = [0]


def draw():
    step[0] += 1
    LP.run_negatives(plan, 1, step[0])


rec["run_negatives"] = timed(draw)
rec["run_negatives"]["Msamples_per_s"] = round(K / rec["run_negatives"]["median_ms"] / 1e3, 1)

got = LP.run_negatives(plan, 1, 0)[:, :SLICE].cpu()
host_base = LP._on_cpu(base)
t0 = time.perf_counter()
rowptr, col, row, gph, n = LP._host_arrays(host_base, gp)
prefix = plan.prefix.cpu().numpy()
prep = time.perf_counter() - t0
ts = []
for _ in range(3):
    t0 = time.perf_counter()
    want = LP._sample_host(rowptr, col, row, gph, n, prefix, [SLICE], False, 1, 0)
    ts.append((time.perf_counter() - t0) * 1e3)
rec["host"] = {"slice": SLICE, "slice_ms": round(statistics.median(ts), 2), "prepare_arrays_ms": round(prep * 1e3, 2),
               "scaled_to_K_ms": round(statistics.median(ts) * K / SLICE, 1),
               "equals_device_slice": bool(torch.equal(torch.from_numpy(want), got))}

x = torch.rand(N, D, device=dev)
rec["aggregation_d%d" % D] = timed(lambda: ops.spmm(base, x, "sum"))
rec["run_negatives_over_aggregation"] = round(rec["run_negatives"]["median_ms"] /
                                              rec["aggregation_d%d" % D]["median_ms"], 3)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(rec, f, indent=1)
print(json.dumps(rec))
