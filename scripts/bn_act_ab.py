"""A/B of the activation-fused BatchNorm passes (nn.bn_act_module / nn.bn_skip_act(act=...): mp::bn_actx, mp::bn_skip_actx)
against the path they replace: the engine's BatchNorm1d(relu=False) followed by the torch activation, and for the skip
block BatchNorm, add, activation as separate passes.

One process, the same buffers; forward + backward on [ROWS, d] fp32 for d in WIDTHS, the kinds PRELU, ELU and SILU, the
plain form and the SUM skip form.  The two routes alternate over ROUNDS rounds of CALLS calls each (one untimed call of
each first); every call is timed by a device-event pair; median and p90 over all calls of a route, in ms.  Peak memory:
torch.cuda.max_memory_allocated over one forward + backward, above what was allocated before it.  The two routes'
outputs and input gradients are compared once per case (max |difference| over max |value|).

    ROWS=2000000 WIDTHS=256,128 python scripts/bn_act_ab.py OUT.jsonl"""
import json, os, statistics, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn as nn
from graphgym_amd import nn as mpnn

dev = torch.device("cuda:0")
ROWS = int(os.environ.get("ROWS", "2000000"))
WIDTHS = [int(v) for v in os.environ.get("WIDTHS", "256,128").split(",")]
ROUNDS = int(os.environ.get("ROUNDS", "6"))
CALLS = int(os.environ.get("CALLS", "8"))
out_path = sys.argv[1]
KINDS = {"prelu": lambda: nn.PReLU(), "elu": lambda: nn.ELU(), "silu": lambda: nn.SiLU()}


def p90(v):
    s = sorted(v)
    return s[min(len(s) - 1, int(round(0.9 * (len(s) - 1))))]


def case(kind, form, d):
    gen = torch.Generator(device=dev).manual_seed(d)
    x = torch.empty((ROWS, d), device=dev).normal_(generator=gen).requires_grad_(True)
    skip = torch.empty((ROWS, d), device=dev).normal_(generator=gen).requires_grad_(True) if form == "sum" else None
    dy = torch.empty((ROWS, d), device=dev).normal_(generator=gen)
    bn = mpnn.BatchNorm1d(d).to(dev).train()
    act = KINDS[kind]().to(dev)
    leaves = [x] + ([skip] if skip is not None else []) + list(bn.parameters()) + list(act.parameters())

    def fused():
        return mpnn.bn_act_module(bn, x, act) if skip is None else mpnn.bn_skip_act(bn, x, skip, "skipsum", act=act)

    def composition():
        return act(bn(x)) if skip is None else act(skip + bn(x))

    def step(fn):
        for t in leaves:
            t.grad = None
        out = fn()
        out.backward(dy)
        return out

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step(fn)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    def peak(fn):
        for t in leaves:
            t.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        out = step(fn)
        torch.cuda.synchronize()
        del out
        return torch.cuda.max_memory_allocated() - base

    # one untimed call of each, and the two routes' results side by side
    a = step(fused).detach()
    ga = [t.grad.clone() for t in leaves]
    b = step(composition).detach()
    gb = [t.grad for t in leaves]
    rel = lambda u, v: float((u - v).abs().max() / v.abs().max().clamp(min=1e-30))      # noqa: E731
    diff = {"out": rel(a, b), "grads": max(rel(u, v) for u, v in zip(ga, gb))}
    del a, b, ga, gb
    t = {"fused": [], "composition": []}
    for _ in range(ROUNDS):
        for name, fn in (("fused", fused), ("composition", composition)):
            for _ in range(CALLS):
                t[name].append(timed(fn))
    mem = {"fused": peak(fused), "composition": peak(composition)}
    rec = {"what": "bn_act_ab", "kind": kind, "form": form, "rows": ROWS, "d": d, "rounds": ROUNDS, "calls": CALLS,
           "max_rel_diff": diff}
    for name in t:
        med = statistics.median(t[name])
        rec[name] = {"median_ms": round(med, 3), "p90_ms": round(p90(t[name]), 3), "min_ms": round(min(t[name]), 3),
                     "peak_bytes": int(mem[name])}
    spread = max(rec[n]["p90_ms"] - rec[n]["median_ms"] for n in t)
    rec["spread_ms"] = round(spread, 3)
    rec["fused_faster_beyond_spread"] = bool(rec["composition"]["median_ms"] - rec["fused"]["median_ms"] > spread)
    rec["fused_peak_not_above"] = bool(mem["fused"] <= mem["composition"])
    # elements moved by the counts of DESIGN.md (plain: 3 + 5 N d fused, 5 + 8 composed; sum: 4 + 7 fused, 8 + 8 composed)
    moved = {"plain": (8, 13), "sum": (11, 16)}[form]
    rec["fused_TBps_by_count"] = round(moved[0] * ROWS * d * 4 / (rec["fused"]["median_ms"] * 1e-3) / 1e12, 3)
    rec["composition_TBps_by_count"] = round(moved[1] * ROWS * d * 4 / (rec["composition"]["median_ms"] * 1e-3) / 1e12, 3)
    print(json.dumps(rec), flush=True)
    with open(out_path, "a") as f:
        f.write(json.dumps(rec) + "\n")


for d in WIDTHS:
    for form in ("plain", "sum"):
        for kind in KINDS:
            case(kind, form, d)
            torch.cuda.empty_cache()
