"""In-process A/B of the bf16 aggregation (mp_spmm_csr_bf16) against the fp32 launch ops.spmm dispatches today (the
hot-row tile kernel on the bench graph): same graph, the same X in both precisions (X fp32 uniform in [-1, 1), its bf16
rounding), the two alternated round by round (forward, then backward order).  Per form: median and p90 ms per launch,
edges/s, the algorithmic bytes of DESIGN.md §4.6 and their fraction of 8 TB/s.  Once per case the bf16 output is checked
bit for bit against the fp32 plan-based kernel on the widened X, rounded.
    NODES=10000000 CASES=ba:256,ba:128,ba:512,perm:256 python scripts/agg_bf16_ab.py OUT.jsonl"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import graphgym_amd as ga
from graphgym_amd import _lib, graphgen, ops

dev = torch.device("cuda:0")
n = int(os.environ.get("NODES", "10000000"))
ROUNDS = int(os.environ.get("ROUNDS", "6"))
ITERS = int(os.environ.get("ITERS", "8"))
PEAK = 8.0e12
out_path = sys.argv[1]
cases = [c.split(":") for c in os.environ.get("CASES", "ba:256,ba:128,ba:512,perm:256").split(",")]


def model_bytes(n, nnz, d, elem):
    """gathered rows + col + val per entry, one output row per node, rowptr"""
    return nnz * (d * elem + 4 + 4) + n * d * elem + (n + 1) * 4


def times_of(fn):
    """ms per launch of ITERS back-to-back launches, after one untimed launch"""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(ITERS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / ITERS


def pct(t, p):
    t = sorted(t)
    return t[min(len(t) - 1, int(round(p / 100 * (len(t) - 1))))]


cur = None
for kind, ds in cases:
    d = int(ds)
    if cur != kind:
        g = None
        torch.cuda.empty_cache()
        ei = graphgen.ba_edge_index(n, 5, seed=12345, device=dev, permute_seed=1 if kind == "perm" else None)
        g = ga.CSRGraph.from_edge_index(ei, n, add_self_loops=True).gcn_norm("row")
        del ei
        cur = kind
    x32 = torch.empty((n, d), dtype=torch.float32, device=dev)
    x32.uniform_(-1.0, 1.0, generator=torch.Generator(device=dev).manual_seed(7))
    xb = x32.to(torch.bfloat16)
    y32 = torch.empty((n, d), dtype=torch.float32, device=dev)
    yb = torch.empty((n, d), dtype=torch.bfloat16, device=dev)
    with torch.no_grad():
        # the bit-for-bit contract at this size: bf16 == fp32 plan kernel on xb.float(), rounded
        os.environ["MP_AGG_TILES"] = "0"
        ref, _ = ops._raw_spmm(g, xb.float(), _lib.SUM)
        os.environ["MP_AGG_TILES"] = "1"
        ops._raw_spmm(g, xb, _lib.SUM, out=yb)
        same = bool(torch.equal(yb.view(torch.int16), ref.to(torch.bfloat16).view(torch.int16)))
        del ref
        torch.cuda.empty_cache()
        tiles0, hot0 = ops.AGG_TILES_CALLS, ops.AGG_HOT_CALLS
        forms = {"fp32": lambda: ops._raw_spmm(g, x32, _lib.SUM, out=y32),
                 "bf16": lambda: ops._raw_spmm(g, xb, _lib.SUM, out=yb)}
        for f in forms.values():     # hot-row tag built, code objects loaded, outside the timed rounds
            f()
        torch.cuda.synchronize()
        t = {k: [] for k in forms}
        for r in range(ROUNDS):
            for k in (list(forms) if r % 2 == 0 else list(forms)[::-1]):
                t[k].append(times_of(forms[k]))
    row = {"graph": kind, "d": d, "n": n, "nnz": g.nnz, "rounds": ROUNDS, "iters": ITERS,
           "fp32_tile_launches": ops.AGG_TILES_CALLS - tiles0, "fp32_hot_launches": ops.AGG_HOT_CALLS - hot0,
           "bf16_bits_equal_fp32_plan_rounded": same}
    for k, elem in (("fp32", 4), ("bf16", 2)):
        med = statistics.median(t[k])
        b = model_bytes(n, g.nnz, d, elem)
        row[k] = {"median_ms": round(med, 3), "p90_ms": round(pct(t[k], 90), 3), "min_ms": round(min(t[k]), 3),
                  "edges_per_s": g.nnz / (med * 1e-3), "model_GB": round(b / 1e9, 3),
                  "frac_of_8TBps": round(b / (med * 1e-3) / PEAK, 4)}
    row["bf16_speedup"] = round(row["fp32"]["median_ms"] / row["bf16"]["median_ms"], 3)
    print(json.dumps(row), flush=True)
    with open(out_path, "a") as f:
        f.write(json.dumps(row) + "\n")
    del x32, xb, y32, yb
    torch.cuda.empty_cache()
