"""A/B of the max backward: the pull form that ops.deterministic() selects (mp_spmm_max_bwd_pull_f32 / _bf16 /
mp_spmm_heads_max_bwd_pull_f32: two row gathers per transposed entry on the plan kernel, no atomics) against the scatter
form (mp_spmm_max_bwd_f32 / _bf16 / mp_spmm_heads_max_bwd_f32: one float atomic per output element onto zeros).  Both
run from one build, in one process, on the same argmax and dy; the forms alternate call by call.

  graph   BA(NODES, 5), both directions stored, gcn-normalised values
  forms   plain fp32, plain bf16, HEADS-head fp32 (a [nnz, HEADS]); d in WIDTHS
  timed   what the backward dispatches — scatter: the zero fill, the kernel (bf16: and the cast of the fp32 buffer);
          pull: the kernel (heads: and the permutation of a into transposed order) — one device-event pair per call,
          CALLS calls per form: `warm` back to back, `flushed` after a FLUSH_MB write that evicts the last-level cache
  first   the first pull call on a freshly built graph (host clock to a device synchronise): the sorted transpose, its
          plan and the permuted values are built there; the second call builds nothing

Per record: median, p10 and p90 in ms per form and regime, the ratio scatter / pull of the medians, the modelled bytes of
each form (scatter: argmax + dy read, dx zeroed, N d atomics; pull: 8 E d gathered, dx written once) and the achieved
rate of the pull form over its modelled bytes, max |difference| / max |value| between the forms, and whether five pull
calls gave the same bits.

    NODES=1000000 WIDTHS=64,128,256 python scripts/max_bwd_det_ab.py profiles/max_bwd_det_ab.jsonl"""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import graphgym_amd as ga
from graphgym_amd import graphgen, ops

dev = torch.device("cuda:0")
n = int(os.environ.get("NODES", "1000000"))
WIDTHS = [int(v) for v in os.environ.get("WIDTHS", "64,128,256").split(",")]
CALLS = int(os.environ.get("CALLS", "30"))
HEADS = int(os.environ.get("HEADS", "4"))
FLUSH_MB = int(os.environ.get("FLUSH_MB", "1024"))
out_path = sys.argv[1]
MAX = ops._lib.MAX


def pct(ts, q):
    s = sorted(ts)
    return s[min(len(s) - 1, max(0, round(q * (len(s) - 1))))]


def stats(ts):
    return {"median": round(pct(ts, 0.5), 4), "p10": round(pct(ts, 0.1), 4), "p90": round(pct(ts, 0.9), 4)}


def time_forms(forms, flush):
    """{name: [ms per call]}: CALLS rounds, the forms alternating inside a round, one event pair per call"""
    ts = {k: [] for k in forms}
    for _ in range(CALLS):
        for k, fn in forms.items():
            if flush is not None:
                flush.add_(1)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts[k].append(e0.elapsed_time(e1))
    return ts


def emit(rec):
    print(json.dumps(rec), flush=True)
    with open(out_path, "a") as f:
        f.write(json.dumps(rec) + "\n")


def build():
    ei = graphgen.ba_edge_index(n, 5, seed=12345, device=dev)
    return ga.CSRGraph.from_edge_index(ei, n, add_self_loops=True).gcn_norm("row")


saved = ops._DETERMINISTIC
try:
    G = build()
    E = G.nnz
    flush = torch.zeros(FLUSH_MB << 18, dtype=torch.int32, device=dev)
    gen = torch.Generator(device=dev).manual_seed(7)
    # the cost of the first call: the sorted transpose, its plan and the permuted values
    x = torch.empty((n, 64), device=dev).uniform_(-1.0, 1.0, generator=gen)
    _, am = ops._raw_spmm(G, x, MAX, want_argmax=True)
    dy = torch.empty((n, 64), device=dev).uniform_(-1.0, 1.0, generator=gen)
    torch.ops.mp.spmm_max_bwd_pull_raw(dy, am, G.handle)          # code objects loaded, the allocator warm
    G1 = build()
    _, am1 = ops._raw_spmm(G1, x, MAX, want_argmax=True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    torch.ops.mp.spmm_max_bwd_pull_raw(dy, am1, G1.handle)
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    torch.ops.mp.spmm_max_bwd_pull_raw(dy, am1, G1.handle)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    emit({"what": "first_call", "n": n, "nnz": E, "d": 64, "first_ms": round((t1 - t0) * 1e3, 3),
          "second_ms": round((t2 - t1) * 1e3, 3)})
    del G1, am1, x, am, dy

    for d in WIDTHS:
        for form in ("f32", "bf16", f"heads{HEADS}"):
            x = torch.empty((n, d), device=dev).uniform_(-1.0, 1.0, generator=gen)
            dy = torch.empty((n, d), device=dev).uniform_(-1.0, 1.0, generator=gen)
            if form.startswith("heads"):
                a = torch.empty((E, HEADS), device=dev).uniform_(0.25, 1.25, generator=gen)
                _, am = ops._raw_spmm_heads_reduce(G, a, x, HEADS, MAX)

                def run(det):
                    ops.set_deterministic(det)
                    return ops._heads_grad_by_source(G, a, x, HEADS, True, dy, am)
                forms = {"scatter": lambda: run(False), "pull": lambda: run(True)}
            else:
                if form == "bf16":
                    x, dy = x.to(torch.bfloat16), dy.to(torch.bfloat16)
                _, am = ops._raw_spmm(G, x, MAX, want_argmax=True)
                forms = {"scatter": lambda: torch.ops.mp.spmm_max_bwd_raw(dy, am, G.handle),
                         "pull": lambda: torch.ops.mp.spmm_max_bwd_pull_raw(dy, am, G.handle)}
            outs = {k: fn() for k, fn in forms.items()}
            for fn in forms.values():
                fn(), fn()
            torch.cuda.synchronize()
            same = all(torch.equal(forms["pull"](), outs["pull"]) for _ in range(4))
            warm = time_forms(forms, None)
            cold = time_forms(forms, flush)
            eb = 2 if form == "bf16" else 4
            pull_bytes = E * d * (4 + eb) + n * d * eb + E * 8
            scatter_bytes = n * d * (4 + eb) + 2 * n * d * 4 + (n * d * (4 + eb) if form == "bf16" else 0)
            rec = {"what": "max_bwd", "form": form, "n": n, "nnz": E, "d": d, "calls": CALLS,
                   "warm": {k: stats(v) for k, v in warm.items()}, "flushed": {k: stats(v) for k, v in cold.items()},
                   "pull_model_bytes": pull_bytes, "scatter_model_bytes": scatter_bytes, "scatter_atomics": n * d,
                   "pull_same_bits_5_calls": bool(same),
                   "rel_diff": float((outs["pull"].float() - outs["scatter"].float()).abs().max()
                                     / outs["scatter"].float().abs().max().clamp(min=1e-30))}
            for regime in ("warm", "flushed"):
                r = rec[regime]
                r["scatter_over_pull"] = round(r["scatter"]["median"] / r["pull"]["median"], 3)
                r["pull_TBps_of_model"] = round(pull_bytes / (r["pull"]["median"] * 1e-3) / 1e12, 3)
            emit(rec)
            del x, dy, am, outs
            torch.cuda.empty_cache()
finally:
    ops._DETERMINISTIC = saved
