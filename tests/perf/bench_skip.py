"""Timings of the skip block's tail — act(skip + BN(x)) (skipsum) and act(cat(skip, BN(x))) (skipconcat) in training
mode — as ONE engine op (graphgym_amd.nn.bn_skip_act: mp::bn_skip_act) against the composition the engine offered before
it: graphgym_amd.nn.BatchNorm1d(relu=False), then torch add / cat, then torch.relu.  A script, not collected by pytest.

Sizes [2e6, 256] and [1e7, 256] fp32 (ROWS=a,b,... D=...), d_skip = d; both modes; forward alone (under no_grad) and
forward + backward (gradients of x, skip, weight, bias from one incoming gradient).  One process, the same buffers; the
two forms alternate over ROUNDS rounds of ITERS back-to-back runs each (one untimed run first), timed with device
events; medians and minima in ms.  The outputs and gradients of a pair are compared at the timed size.

Algorithmic bytes, from shapes (4 bytes per element, per-column vectors left out):
  forward    fused        sum: statistics read x; apply reads x, skip, writes out                      4 N d
                          cat: the same with out of width d_skip + d                          3 N d + 2 N d_skip
             composed     statistics 1, apply 2, add 3, relu 2                                         8 N d
                          cat: statistics 1, apply 2, cat 2 (d + d_skip), relu 2 (d + d_skip) 7 N d + 4 N d_skip
  backward   fused        sum: statistics read dy, out, x, write g; apply reads g, x, writes dx        7 N d
                          cat: the left mask 3 N d_skip; statistics 3, apply 4 on column views 7 N d + 3 N d_skip
             composed     sum: relu 3, statistics 2, apply 3                                           8 N d
                          cat: relu 3 (d + d_skip), dy's right slab copied 2, statistics 2, apply 3
                                                                                            10 N d + 3 N d_skip
The bar: the fused form's median below the composed form's minimum in every case.

    ROWS=2000000,10000000 D=256 python tests/perf/bench_skip.py profiles/skip_stage.json"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402
from graphgym_amd import nn as mpnn  # noqa: E402

dev = torch.device("cuda:0")
SIZES = [int(v) for v in os.environ.get("ROWS", "2000000,10000000").split(",")]
d = int(os.environ.get("D", "256"))
ROUNDS = int(os.environ.get("ROUNDS", "5"))
ITERS = int(os.environ.get("ITERS", "3"))
out_path = sys.argv[1]


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def ab(iters, *fns):
    ts = [[] for _ in fns]
    for _ in range(ROUNDS):
        for t, fn in zip(ts, fns):
            t.append(timed(fn, iters))
    pack = lambda t: {"median": round(statistics.median(t), 3), "min": round(min(t), 3), "all": [round(v, 3) for v in t]}  # noqa: E731
    return [pack(t) for t in ts]


def report(t_f, t_c, b_f, b_c, extra):
    gbps = lambda b, t: round(b / (t["median"] * 1e-3) / 1e9, 1)     # noqa: E731
    return dict(extra, fused_ms=t_f, composed_ms=t_c, fused_GB=round(b_f / 1e9, 3), composed_GB=round(b_c / 1e9, 3),
                fused_GBps=gbps(b_f, t_f), composed_GBps=gbps(b_c, t_c),
                ratio=round(t_f["median"] / t_c["median"], 3), byte_ratio=round(b_f / b_c, 3),
                meets_bar=bool(t_f["median"] < t_c["min"]))


def measure(n):
    gen = torch.Generator(device=dev).manual_seed(7)
    ds = d
    x = torch.empty((n, d), device=dev).normal_(generator=gen).requires_grad_(True)
    skip = torch.empty((n, ds), device=dev).normal_(generator=gen).requires_grad_(True)
    bn = mpnn.BatchNorm1d(d, relu=False).to(dev).train()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.3, 0.3)
    leaves = [x, skip, bn.weight, bn.bias]
    iters = ITERS * max(1, min(20, 2000000 // n))
    result = {"n": n, "d": d, "d_skip": ds, "iters": iters}
    E = 4 * n       # bytes of one column of all rows
    for mode in ("skipsum", "skipconcat"):
        cat = mode == "skipconcat"

        def fused():
            return mpnn.bn_skip_act(bn, x, skip, mode, relu=True)

        def composed():
            y = bn(x)
            return torch.relu(torch.cat((skip, y), 1) if cat else skip + y)
        dy = torch.empty((n, ds + d if cat else d), device=dev).normal_(generator=gen)

        def fused_step():
            return torch.autograd.grad(fused(), leaves, dy)

        def composed_step():
            return torch.autograd.grad(composed(), leaves, dy)
        with torch.no_grad():
            same = bool(torch.equal(fused(), composed()))
            t_f, t_c = ab(iters, fused, composed)
        gf, gc = fused_step(), composed_step()
        rel = [float((a - b).abs().max() / b.abs().max().clamp(min=1e-30)) for a, b in zip(gf, gc)]
        del gf, gc
        s_f, s_c = ab(iters, fused_step, composed_step)
        if cat:
            bf_f, bf_c = E * (3 * d + 2 * ds), E * (7 * d + 4 * ds)
            bb_f, bb_c = E * (7 * d + 3 * ds), E * (10 * d + 3 * ds)
        else:
            bf_f, bf_c, bb_f, bb_c = E * 4 * d, E * 8 * d, E * 7 * d, E * 8 * d
        result[mode] = {
            "forward": report(t_f, t_c, bf_f, bf_c, {"equal": same}),
            "forward_backward": report(s_f, s_c, bf_f + bb_f, bf_c + bb_c,
                                       {"grad_max_rel_diff": dict(zip(("x", "skip", "weight", "bias"), rel))}),
        }
        del dy
    return result


out = {"what": "skip_stage", "rounds": ROUNDS, "sizes": [measure(n) for n in SIZES]}
print(json.dumps(out), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
