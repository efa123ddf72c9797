"""A/B of the BatchNorm entries between two trees — the commit before the kernel families were folded into
csrc/bn_kernels.h (PARENT) and this one — at [ROWS, 256] and [ROWS, 64] fp32, the shapes of scripts/bn_act_ab.py.

    python scripts/bn_unify_ab.py PARENT_DIR OUT.jsonl       # the series; opens no device itself
    python scripts/bn_unify_ab.py --child ROOT               # one fresh process on the tree at ROOT: JSON of times

Every round starts three fresh child processes in turn: parent, new, parent again.  The first two are the comparison, the
first and third the parent-against-parent series that gives the spread.  A child calls each C entry on buffers it
allocates once: WARM untimed calls, then CALLS calls each between a pair of device events.  Per entry the output holds
median and p90 over all rounds' calls for the three series, and `regression`: the new median exceeds the parent's by
more than the two parent series differ."""
import ctypes as C, json, os, statistics, subprocess, sys

ROWS = int(os.environ.get("ROWS", "2000000"))
WIDTHS = [int(v) for v in os.environ.get("WIDTHS", "256,64").split(",")]
ROUNDS = int(os.environ.get("ROUNDS", "5"))
CALLS = int(os.environ.get("CALLS", "15"))
WARM = int(os.environ.get("WARM", "3"))
RELU, PRELU, ELU, SILU = 1, 3, 4, 6
SUM, CONCAT = 0, 1
T, SEED, OFFSET, EPS = 19661, 1, 0, 1e-5


def child(root):
    sys.path.insert(0, os.path.abspath(root))
    import torch
    from graphgym_amd._lib import check, lib, ptr
    dev = torch.device("cuda:0")
    L = lib()
    times = {}

    def timed(name, fn):
        for _ in range(WARM):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(CALLS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        times[name] = ts

    for d in WIDTHS:
        N = ROWS
        gen = torch.Generator(device=dev).manual_seed(d)
        x, skip, dy = (torch.empty((N, d), device=dev).normal_(generator=gen) for _ in range(3))
        dy2 = torch.empty((N, 2 * d), device=dev).normal_(generator=gen)
        out, dx, dskip = (torch.empty((N, d), device=dev) for _ in range(3))
        out2 = torch.empty((N, 2 * d), device=dev)
        gamma, beta = torch.rand(d, device=dev) + 0.5, torch.randn(d, device=dev)
        mean, invstd, var, dgamma, dbeta = (torch.empty(d, device=dev) for _ in range(5))
        slope, dslope = torch.full((1,), 0.25, device=dev), torch.empty(1, device=dev)
        nb = C.c_size_t(0)
        check(L.mp_bn_drop_ws_bytes(N, d, C.byref(nb)))      # the largest of the three layouts
        ws, nb = torch.empty(nb.value, dtype=torch.uint8, device=dev), nb.value
        P = ptr
        stats = (P(mean), P(invstd), P(var))
        tail = (P(ws), nb, None)
        grads = (P(dgamma), P(dbeta))
        tag = f"d{d}/"
        # the plain ReLU layer: the mask from x, and from the forward's output
        timed(tag + "relu_fwd", lambda: check(L.mp_bn_train_fwd_f32(P(x), d, N, d, P(gamma), P(beta), EPS, 1, P(out), d, *stats, *tail)))
        timed(tag + "relu_bwd_mask_from_x", lambda: check(L.mp_bn_train_bwd_relu_f32(P(dy), d, P(x), d, N, d, P(gamma), P(beta), P(mean), P(invstd),
                                                                                      P(dx), d, *grads, *tail)))
        timed(tag + "relu_bwd_mask_from_y", lambda: check(L.mp_bn_train_bwd_f32(P(dy), d, P(out), d, P(x), d, N, d, P(gamma), P(mean), P(invstd),
                                                                                 P(dx), d, *grads, *tail)))
        # the ReLU skip blocks
        timed(tag + "relu_sum_fwd", lambda: check(L.mp_bn_train_fwd_skip_f32(P(x), d, P(skip), d, N, d, d, SUM, P(gamma), P(beta), EPS, 1, P(out), d,
                                                                              *stats, *tail)))
        timed(tag + "relu_sum_bwd", lambda: check(L.mp_bn_train_bwd_skip_f32(P(dy), d, P(out), d, P(x), d, N, d, P(gamma), P(mean), P(invstd), P(dx), d,
                                                                              P(dskip), d, *grads, *tail)))
        timed(tag + "relu_concat_fwd", lambda: check(L.mp_bn_train_fwd_skip_f32(P(x), d, P(skip), d, N, d, d, CONCAT, P(gamma), P(beta), EPS, 1,
                                                                                 P(out2), 2 * d, *stats, *tail)))
        timed(tag + "relu_concat_bwd", lambda: check(L.mp_bn_train_bwd_skip_act_f32(P(dy2), 2 * d, P(x), d, P(skip), d, N, d, d, CONCAT, P(gamma),
                                                                                     P(beta), P(mean), P(invstd), RELU, 0.0, None, P(dx), d,
                                                                                     P(dskip), d, *grads, None, *tail)))
        for name, act, prm, sl, dsl in (("elu", ELU, 1.0, None, None), ("prelu", PRELU, 0.0, slope, dslope)):
            timed(tag + name + "_fwd", lambda: check(L.mp_bn_train_fwd_act_f32(P(x), d, N, d, P(gamma), P(beta), EPS, act, prm, P(sl), P(out), d, *stats,
                                                                               *tail)))
            timed(tag + name + "_bwd", lambda: check(L.mp_bn_train_bwd_act_f32(P(dy), d, P(x), d, N, d, P(gamma), P(beta), P(mean), P(invstd), act, prm,
                                                                               P(sl), P(dx), d, *grads, P(dsl), *tail)))
            timed(tag + name + "_sum_fwd", lambda: check(L.mp_bn_train_fwd_skip_act_f32(P(x), d, P(skip), d, N, d, d, SUM, P(gamma), P(beta), EPS, act,
                                                                                        prm, P(sl), P(out), d, *stats, *tail)))
            timed(tag + name + "_sum_bwd", lambda: check(L.mp_bn_train_bwd_skip_act_f32(P(dy), d, P(x), d, P(skip), d, N, d, d, SUM, P(gamma), P(beta),
                                                                                        P(mean), P(invstd), act, prm, P(sl), P(dx), d, P(dskip), d,
                                                                                        *grads, P(dsl), *tail)))
        for name, act in (("drop_relu", RELU), ("drop_silu", SILU)):
            timed(tag + name + "_fwd", lambda: check(L.mp_bn_train_fwd_drop_act_f32(P(x), d, N, d, P(gamma), P(beta), EPS, act, 0.0, None, T, SEED,
                                                                                    OFFSET, P(out), d, *stats, *tail)))
            timed(tag + name + "_bwd", lambda: check(L.mp_bn_train_bwd_drop_act_f32(P(dy), d, P(x), d, N, d, P(gamma), P(beta), P(mean), P(invstd), act,
                                                                                    0.0, None, T, SEED, OFFSET, P(dx), d, *grads, None, *tail)))
        del x, skip, dy, dy2, out, dx, dskip, out2, ws
        torch.cuda.empty_cache()
    print("BN_UNIFY_AB " + json.dumps(times), flush=True)


def p90(v):
    s = sorted(v)
    return s[min(len(s) - 1, int(round(0.9 * (len(s) - 1))))]


def main():
    parent, out_path = sys.argv[1], sys.argv[2]
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    series = {"parent": {}, "new": {}, "parent_again": {}}
    for rnd in range(ROUNDS):
        for name, root in (("parent", parent), ("new", here), ("parent_again", parent)):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root], capture_output=True, text=True,
                               timeout=600)
            line = [l for l in r.stdout.splitlines() if l.startswith("BN_UNIFY_AB ")]
            if r.returncode != 0 or not line:
                sys.exit(f"child on {root} failed ({r.returncode}); no further process is started\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
            for k, v in json.loads(line[0][len("BN_UNIFY_AB "):]).items():
                series[name].setdefault(k, []).extend(v)
        print(f"round {rnd + 1} of {ROUNDS} done", flush=True)
    bad = 0
    with open(out_path, "w") as f:
        for k in series["parent"]:
            rec = {"what": "bn_unify_ab", "entry": k, "rows": ROWS, "rounds": ROUNDS, "calls_per_round": CALLS}
            for name, s in series.items():
                rec[name] = {"median_ms": round(statistics.median(s[k]), 4), "p90_ms": round(p90(s[k]), 4)}
            rec["spread_ms"] = round(abs(rec["parent"]["median_ms"] - rec["parent_again"]["median_ms"]), 4)
            rec["new_minus_parent_ms"] = round(rec["new"]["median_ms"] - rec["parent"]["median_ms"], 4)
            rec["regression"] = bool(rec["new_minus_parent_ms"] > rec["spread_ms"])
            bad += rec["regression"]
            f.write(json.dumps(rec) + "\n")
            print(json.dumps(rec), flush=True)
    print(f"{bad} entries beyond the parent-against-parent spread")


if __name__ == "__main__":
    child(sys.argv[2]) if sys.argv[1] == "--child" else main()
