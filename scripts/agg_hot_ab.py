"""In-process A/B of the hot-column budget of the tile aggregation (MP_AGG_HOT_MB) on the bench graph: same graph,
same buffers, budgets alternated round by round (forward, then backward order); medians, min, max; every output
checked with torch.equal against budget 0.  "0.001" is the control: the hot kernel with one hot column, i.e. every
gather in the new instruction form and almost all of them non-temporal.
    NODES=10000000 CASES=ba:256,ba:128,ba:512,perm:256,hk:256 python scripts/agg_hot_ab.py OUT.jsonl"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import graphgym_amd as ga
from graphgym_amd import _lib, graphgen, ops

dev = torch.device("cuda:0")
n = int(os.environ.get("NODES", "10000000"))
ROUNDS = int(os.environ.get("ROUNDS", "5"))
BUDGETS = os.environ.get("BUDGETS", "0,0.001,64,128,192,256").split(",")
out_path = sys.argv[1]
cases = [c.split(":") for c in os.environ.get("CASES", "ba:256,ba:128,ba:512,perm:256,hk:256").split(",")]
ops.AGG_TILES_MIN_ROWS = min(ops.AGG_TILES_MIN_ROWS, n)
ops.AGG_HOT_MIN_BYTES = int(os.environ.get("HOT_MIN_BYTES", ops.AGG_HOT_MIN_BYTES))


def timeit(fn, iters=8):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


cur = None
for kind, ds in cases:
    d = int(ds)
    if cur != kind:
        g = None
        torch.cuda.empty_cache()
        ei = graphgen.ba_edge_index(n, 5, seed=12345, device=dev, triangle_p=0.3 if kind == "hk" else None,
                                    permute_seed=1 if kind == "perm" else None)
        g = ga.CSRGraph.from_edge_index(ei, n, add_self_loops=True).gcn_norm("row")
        del ei
        cur = kind
    x = torch.empty((n, d), dtype=torch.float32, device=dev)
    x.uniform_(-1.0, 1.0, generator=torch.Generator(device=dev).manual_seed(7))
    y = torch.empty((n, d), dtype=torch.float32, device=dev)
    y0 = torch.empty_like(y)
    os.environ["MP_AGG_HOT_MB"] = "0"
    ops._raw_spmm(g, x, _lib.SUM, out=y0)
    times = {b: [] for b in BUDGETS}
    same = {b: True for b in BUDGETS}
    hot0 = ops.AGG_HOT_CALLS
    with torch.no_grad():
        for b in BUDGETS:   # tags built outside the timed rounds
            os.environ["MP_AGG_HOT_MB"] = b
            ops._raw_spmm(g, x, _lib.SUM, out=y)
        torch.cuda.synchronize()
        for r in range(ROUNDS):
            for b in (BUDGETS if r % 2 == 0 else BUDGETS[::-1]):
                os.environ["MP_AGG_HOT_MB"] = b
                y.zero_()
                times[b].append(timeit(lambda: ops._raw_spmm(g, x, _lib.SUM, out=y)))
                same[b] = same[b] and torch.equal(y, y0)
    row = {"graph": kind, "d": d, "n": n, "x_bytes": n * d * 4, "nnz": g.nnz, "rounds": ROUNDS,
           "hot_launches": ops.AGG_HOT_CALLS - hot0}
    for b in BUDGETS:
        t = sorted(times[b])
        row[f"mb{b}"] = {"median_ms": round(statistics.median(t), 3), "min": round(t[0], 3), "max": round(t[-1], 3),
                         "bitwise_equal_to_0": same[b]}
    print(json.dumps(row), flush=True)
    with open(out_path, "a") as f:
        f.write(json.dumps(row) + "\n")
    del x, y, y0
    torch.cuda.empty_cache()
