"""A/B of the dropout-fused BatchNorm passes (nn.bn_act_module / nn.bn_skip_act(drop=...): mp::bn_drop_actx,
mp::bn_drop_skip_actx) against what gnn.dropout > 0 runs without gnn.keyed_dropout: the engine's BatchNorm1d(relu=False),
torch.nn.Dropout, the torch activation — for the skip block BatchNorm, dropout, add, activation as separate passes.
A second pair prices the hash alone: the fused op at T = 0 (every element kept, the draw still made) against mp::bn_actx /
mp::bn_skip_actx.

One process, the same buffers; forward + backward on [ROWS, d] fp32 for d in WIDTHS, p = P, the kinds RELU, PRELU and ELU,
the plain form and the SUM skip form.  The four routes alternate over ROUNDS rounds of CALLS calls each (one untimed call
of each first); every call is timed by a device-event pair; median and p90 over all calls of a route, in ms.  Peak memory:
torch.cuda.max_memory_allocated over one forward + backward, above what was allocated before it.

    ROWS=2000000 WIDTHS=256,128 python scripts/bn_drop_ab.py OUT.jsonl"""
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
P = float(os.environ.get("P", "0.3"))
out_path = sys.argv[1]
KINDS = {"relu": lambda: nn.ReLU(), "prelu": lambda: nn.PReLU(), "elu": lambda: nn.ELU()}
ROUTES = ("fused", "baseline", "fused_T0", "no_dropout")


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
    keyed, torch_drop = mpnn.Dropout(P, seed=1).train(), nn.Dropout(P).train()
    spec = mpnn.act_spec(act)
    slope, param = mpnn._spec_args(spec)
    leaves = [x] + ([skip] if skip is not None else []) + list(bn.parameters()) + list(act.parameters())

    def fused():
        if skip is None:
            return mpnn.bn_act_module(bn, x, act, drop=keyed)
        return mpnn.bn_skip_act(bn, x, skip, "skipsum", act=act, drop=keyed)

    def baseline():
        y = torch_drop(bn(x))
        return act(y) if skip is None else act(skip + y)

    def fused_T0():
        if skip is None:
            return torch.ops.mp.bn_drop_actx(x, bn.weight, bn.bias, slope, bn.eps, spec[0], param, 0, 1, 0)[0]
        return torch.ops.mp.bn_drop_skip_actx(x, skip, bn.weight, bn.bias, slope, bn.eps, spec[0], param, mpnn.SKIP_SUM,
                                              0, 1, 0)[0]

    def no_dropout():
        if skip is None:
            return torch.ops.mp.bn_actx(x, bn.weight, bn.bias, slope, bn.eps, spec[0], param)[0]
        return torch.ops.mp.bn_skip_actx(x, skip, bn.weight, bn.bias, slope, bn.eps, spec[0], param, mpnn.SKIP_SUM)[0]

    fns = dict(zip(ROUTES, (fused, baseline, fused_T0, no_dropout)))

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

    # one untimed call of each; the T = 0 pair computes the same thing: its outputs side by side
    outs = {name: step(fn).detach() for name, fn in fns.items()}
    same_T0 = bool(torch.equal(outs["fused_T0"], outs["no_dropout"]))
    zero_rate = {n: round(float((outs[n] == (0 if skip is None else skip)).float().mean()), 4) for n in ("fused", "baseline")}
    del outs
    t = {name: [] for name in ROUTES}
    for _ in range(ROUNDS):
        for name in ROUTES:
            for _ in range(CALLS):
                t[name].append(timed(fns[name]))
    mem = {name: peak(fns[name]) for name in ROUTES}
    rec = {"what": "bn_drop_ab", "kind": kind, "form": form, "rows": ROWS, "d": d, "p": P, "rounds": ROUNDS,
           "calls": CALLS, "T0_out_equals_no_dropout": same_T0, "dropped_share": zero_rate}
    for name in ROUTES:
        med = statistics.median(t[name])
        rec[name] = {"median_ms": round(med, 3), "p90_ms": round(p90(t[name]), 3), "min_ms": round(min(t[name]), 3),
                     "peak_bytes": int(mem[name])}
    spread = max(rec[n]["p90_ms"] - rec[n]["median_ms"] for n in ("fused", "baseline"))
    rec["spread_ms"] = round(spread, 3)
    rec["fused_faster_beyond_spread"] = bool(rec["baseline"]["median_ms"] - rec["fused"]["median_ms"] > spread)
    rec["fused_peak_below"] = bool(mem["fused"] < mem["baseline"])
    rec["hash_cost_ms"] = round(rec["fused_T0"]["median_ms"] - rec["no_dropout"]["median_ms"], 3)
    # elements moved by the counts of DESIGN.md §4.17 (the mask adds none): plain 3 + 5 N d, sum 4 + 7
    moved = {"plain": 8, "sum": 11}[form]
    rec["fused_TBps_by_count"] = round(moved * ROWS * d * 4 / (rec["fused"]["median_ms"] * 1e-3) / 1e12, 3)
    print(json.dumps(rec), flush=True)
    with open(out_path, "a") as f:
        f.write(json.dumps(rec) + "\n")


for d in WIDTHS:
    for form in ("plain", "sum"):
        for kind in KINDS:
            case(kind, form, d)
            torch.cuda.empty_cache()
