"""Times the multi-head weighted aggregation of the attention layers with sum, mean and max, forward and backward, on the
bench graph (graphgen BA, 10^7 nodes, self loops: ~1.1e8 entries), d = 256, H in {1, 4, 8}, and one gaddconv layer step
(forward + backward) per aggregation.  Per launch: median and min ms over ROUNDS rounds of ITERS back-to-back launches.

  fwd_sum / fwd_mean / fwd_max     ops.spmm_edge_values' forward launch (max: + the int32 argmax)
  bwd_sum / bwd_mean               da (entry-balanced per-entry dot) + dV (aggregation over the transpose)
  max_da                           the masked per-entry dot (mp_spmm_heads_max_da_f32)
  max_dv                           the argmax scatter of dV (mp_spmm_heads_max_bwd_f32; dV zeroing not included)
  sddmm_grad / sddmm_stream        the unmasked per-entry dot: mp_sddmm_dot_f32 (scale 1) and the entry-balanced kernel

    NODES=10000000 HEADS=1,4,8 python scripts/att_agg_ab.py OUT.jsonl"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import graphgym_amd as ga
from graphgym_amd import _lib, graphgen, ops
from graphgym_amd._lib import check, lib, ptr
from graphgym_amd.graph import _stream

dev = torch.device("cuda:0")
n = int(os.environ.get("NODES", "10000000"))
d = int(os.environ.get("D", "256"))
ROUNDS = int(os.environ.get("ROUNDS", "3"))
ITERS = int(os.environ.get("ITERS", "5"))
HEADS = [int(h) for h in os.environ.get("HEADS", "1,4,8").split(",")]
out_path = sys.argv[1]


def times_of(fn):
    """ms per launch over ROUNDS rounds of ITERS launches, each round after one untimed launch: (median, min)"""
    t = []
    for _ in range(ROUNDS):
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(ITERS):
            fn()
        e1.record()
        torch.cuda.synchronize()
        t.append(e0.elapsed_time(e1) / ITERS)
    return {"median_ms": round(statistics.median(t), 3), "min_ms": round(min(t), 3)}


def emit(rec):
    print(json.dumps(rec), flush=True)
    with open(out_path, "a") as f:
        f.write(json.dumps(rec) + "\n")


ei = graphgen.ba_edge_index(n, 5, seed=12345, device=dev)
g = ga.CSRGraph.from_edge_index(ei, n, add_self_loops=True).gcn_norm("row")
gt = g._transpose_sorted()
g.row_ids()
L = lib()
gen = torch.Generator(device=dev).manual_seed(7)
V = torch.empty((n, d), device=dev).uniform_(-1.0, 1.0, generator=gen)
dy = torch.empty((n, d), device=dev).uniform_(-1.0, 1.0, generator=gen)

for H in HEADS:
    a = torch.empty((g.nnz, H), device=dev).uniform_(0.05, 1.0, generator=gen)
    rec = {"what": "att_agg", "n": n, "nnz": g.nnz, "d": d, "heads": H, "rounds": ROUNDS, "iters": ITERS}
    with torch.no_grad():
        rec["fwd_sum"] = times_of(lambda: ops._raw_spmm_heads(g, a, V, H))
        rec["fwd_mean"] = times_of(lambda: ops._raw_spmm_heads_reduce(g, a, V, H, _lib.MEAN))
        rec["fwd_max"] = times_of(lambda: ops._raw_spmm_heads_reduce(g, a, V, H, _lib.MAX))
        _, argmax = ops._raw_spmm_heads_reduce(g, a, V, H, _lib.MAX)
        at = a[gt.pos.long()].contiguous()
        rec["bwd_sum"] = times_of(lambda: (ops._raw_sddmm_dot(g, dy, V, H, 1.0), ops._raw_spmm_heads(gt, at, dy, H)))
        dym = (dy / g.entry_counts().clamp(min=1.0)[:, None]).contiguous()
        rec["bwd_mean"] = times_of(lambda: (ops._raw_sddmm_dot(g, dym, V, H, 1.0), ops._raw_spmm_heads(gt, at, dym, H)))
        del dym
        rec["max_da"] = times_of(lambda: ops._raw_heads_max_da(g, argmax, dy, V, H))
        s = torch.empty((g.nnz, H), device=dev)
        rec["sddmm_grad"] = times_of(lambda: check(L.mp_sddmm_dot_f32(
            ptr(g.rowptr), ptr(g.col), n, g.nnz, ptr(dy), d, ptr(V), d, d, H, 1.0, ptr(s), _stream())))
        rec["sddmm_stream"] = times_of(lambda: ops._raw_sddmm_dot(g, dy, V, H, 1.0))
        dV = torch.zeros_like(V)
        rec["max_dv"] = times_of(lambda: check(L.mp_spmm_heads_max_bwd_f32(
            ptr(g.col), ptr(a), H, ptr(argmax), n, d, ptr(dy), d, ptr(dV), d, _stream())))
        rec["max_dv_GB_added"] = round(n * d * 4 / 1e9, 3)
        rec["max_dv_TBps_added"] = round(n * d * 4 / (rec["max_dv"]["median_ms"] * 1e-3) / 1e12, 3)
        rec["fwd_max_over_sum"] = round(rec["fwd_max"]["median_ms"] / rec["fwd_sum"]["median_ms"], 3)
        rec["max_da_over_sddmm_grad"] = round(rec["max_da"]["median_ms"] / rec["sddmm_grad"]["median_ms"], 3)
        rec["max_da_over_sddmm_stream"] = round(rec["max_da"]["median_ms"] / rec["sddmm_stream"]["median_ms"], 3)
        del argmax, at, s, dV
    emit(rec)
    del a
    torch.cuda.empty_cache()

# one gaddconv layer step, forward + backward, per aggregation
from graphgym_amd.attconv import GeneralAddAttConvLayer   # noqa: E402
from graphgym_amd.config import cfg                        # noqa: E402
from graphgym_amd.harness import Batch                     # noqa: E402
LH = int(os.environ.get("LAYER_HEADS", "4"))
x = V.detach().requires_grad_(True)
holder = Batch()                                           # the batch the layer caches its CSR on
for agg in ("add", "mean", "max"):
    cfg.gnn.agg, cfg.gnn.att_heads, cfg.gnn.normalize_adj = agg, LH, False
    torch.manual_seed(0)
    layer = GeneralAddAttConvLayer(d, d).to(dev)

    def step():
        layer.zero_grad(set_to_none=True)
        x.grad = None
        layer(x, ei, holder=holder).backward(dy)
    emit({"what": "gaddconv_step", "agg": agg, "heads": LH, "n": n, "d": d, "step": times_of(step)})
    del layer
    torch.cuda.empty_cache()
