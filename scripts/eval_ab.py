"""A/B of an epoch's evaluation statistics by three routes, on one device:

  host    the reference's route: per update `true.cpu()`, `pred_score.cpu()`, `loss.item()` (graphgym/train.py:74-76),
          at the end of the epoch scikit-learn on the concatenation (graphgym/logger.py:92-113);
  torch   the plain torch-on-device formulation: the batches stay on the device, at the end argmax / comparisons /
          torch.sort plus torch arithmetic, one `.item()` per metric;
  meter   graphgym_amd.metrics.Meter: `update` per batch, `compute()` at the end (one copy of the state).

All three are given what Logger.update_stats is given: `true`, the score `compute_loss` returned, and the loss as a 0-d
device tensor; the multi-class epochs also time `Meter.update_logits` on the raw logits (`meter_logits`: statistics AND
loss from one pass; it replaces compute_loss + update, so it is listed beside the three, not against them).

One process; a binary epoch of N_BINARY scores and multi-class epochs of [rows, C] logits in UPDATES updates each.  The
routes alternate over ROUNDS rounds (one untimed epoch of each first; the host route runs in the first HOST_ROUNDS rounds
only: scikit-learn on 10^7 examples takes seconds); every epoch is timed wall-clock from a synchronised device to the
Python dictionary; median and p90 per route, in ms.

    python scripts/eval_ab.py OUT.jsonl"""
import json, math, os, statistics, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import torch.nn.functional as F
from graphgym_amd import metrics

dev = torch.device("cuda:0")
N_BINARY = int(os.environ.get("N_BINARY", "10000000"))
MULTI = [tuple(int(v) for v in s.split("x")) for s in os.environ.get("MULTI", "10000000x7,2000000x47").split(",")]
UPDATES = int(os.environ.get("UPDATES", "16"))
ROUNDS = int(os.environ.get("ROUNDS", "20"))
HOST_ROUNDS = int(os.environ.get("HOST_ROUNDS", "2"))
THRESH = 0.5
out_path = sys.argv[1]


def p90(v):
    s = sorted(v)
    return s[min(len(s) - 1, int(round(0.9 * (len(s) - 1))))]


def cuts(n):
    edges = [n * i // UPDATES for i in range(UPDATES + 1)]
    return list(zip(edges[:-1], edges[1:]))


# ---- binary ---------------------------------------------------------------------------------------------------------------
def binary_host(batches):
    import sklearn.metrics as sk
    true, pred, loss, size = [], [], 0.0, 0
    for t, s, l in batches:
        true.append(t.cpu())
        pred.append(s.cpu())
        loss += l.item() * t.shape[0]
        size += t.shape[0]
    true, score = torch.cat(true), torch.cat(pred)
    pred_int = (score > THRESH).long()
    return {"loss": loss / size, "accuracy": sk.accuracy_score(true, pred_int), "precision": sk.precision_score(true, pred_int),
            "recall": sk.recall_score(true, pred_int), "f1": sk.f1_score(true, pred_int), "auc": sk.roc_auc_score(true, score)}


def binary_torch(batches):
    loss = torch.zeros((), dtype=torch.float64, device=dev)
    for t, s, l in batches:
        loss += l.double() * t.shape[0]
    true = torch.cat([b[0] for b in batches]).long()
    score = torch.cat([b[1] for b in batches])
    n = true.numel()
    pred = score > THRESH
    pos = true == 1
    tp, fp, fn = int((pred & pos).sum().item()), int((pred & ~pos).sum().item()), int((~pred & pos).sum().item())
    tn = n - tp - fp - fn
    s_sorted, order = torch.sort(score)
    y_sorted = true[order]
    _, inv, cnt = torch.unique_consecutive(s_sorted, return_inverse=True, return_counts=True)
    negs = torch.zeros(cnt.numel(), dtype=torch.int64, device=dev).index_add_(0, inv, (y_sorted == 0).long())
    poss = cnt - negs
    below = torch.cumsum(negs, 0) - negs
    two_u = int((poss * (2 * below + negs)).sum().item())
    p = tp + fn
    out = metrics.binary_stats(tp, fp, tn, fn, two_u, p, n - p)
    out["loss"] = loss.item() / n
    return out


def binary_meter(batches):
    m = metrics.Meter("classification_binary", thresh=THRESH)
    for t, s, l in batches:
        m.update(t, s, l)
    return m.raw()


# ---- multi-class ------------------------------------------------------------------------------------------------------------
def multi_host(batches):
    import sklearn.metrics as sk
    true, pred, loss, size = [], [], 0.0, 0
    for t, s, l, _ in batches:
        true.append(t.cpu())
        pred.append(s.cpu())
        loss += l.item() * t.shape[0]
        size += t.shape[0]
    true, score = torch.cat(true), torch.cat(pred)
    return {"loss": loss / size, "accuracy": sk.accuracy_score(true, score.max(dim=1)[1])}


def multi_torch(batches):
    loss = torch.zeros((), dtype=torch.float64, device=dev)
    hits = torch.zeros((), dtype=torch.int64, device=dev)
    n = 0
    for t, s, l, _ in batches:
        loss += l.double() * t.shape[0]
        hits += (s.argmax(dim=1) == t).sum()
        n += t.shape[0]
    return {"loss": loss.item() / n, "accuracy": hits.item() / n}


def multi_meter(batches):
    m = metrics.Meter("classification_multi")
    for t, s, l, _ in batches:
        m.update(t, s, l)
    return m.raw()


def multi_meter_logits(batches):
    m = metrics.Meter("classification_multi")
    for t, _, _, z in batches:
        m.update_logits(z, t)
    return m.raw()


def run(what, shape, routes, batches, extra=()):
    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn(batches)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, out
    results = {name: timed(fn)[1] for name, fn in routes + list(extra)}      # one untimed epoch of each
    t = {name: [] for name, _ in routes + list(extra)}
    for r in range(ROUNDS):
        for name, fn in routes + list(extra):
            if name == "host" and r >= HOST_ROUNDS:
                continue
            t[name].append(timed(fn)[0])
    rec = {"what": "eval_ab", "task": what, "shape": list(shape), "updates": UPDATES, "rounds": ROUNDS,
           "host_rounds": HOST_ROUNDS}
    for name in t:
        rec[name] = {"median_ms": round(statistics.median(t[name]), 3), "p90_ms": round(p90(t[name]), 3),
                     "min_ms": round(min(t[name]), 3)}
    spread = max(rec[n]["p90_ms"] - rec[n]["median_ms"] for n in ("torch", "meter"))
    rec["spread_ms"] = round(spread, 3)
    rec["meter_below_torch_beyond_spread"] = bool(rec["torch"]["median_ms"] - rec["meter"]["median_ms"] > spread)
    base = results["meter"]
    rec["max_abs_diff_to_meter"] = {name: max(abs(res[k] - base[k]) for k in base if not math.isnan(base[k]))
                                    for name, res in results.items() if name != "meter"}
    print(json.dumps(rec), flush=True)
    with open(out_path, "a") as f:
        f.write(json.dumps(rec) + "\n")


gen = torch.Generator(device=dev).manual_seed(0)
logit = torch.empty(N_BINARY, device=dev).normal_(generator=gen) * 3
true = (torch.empty(N_BINARY, device=dev).uniform_(generator=gen) < torch.sigmoid(logit)).float()
batches = []
for a, b in cuts(N_BINARY):
    loss, score = metrics.compute_loss(logit[a:b], true[a:b], "cross_entropy", "mean")
    batches.append((true[a:b], score, loss))
run("classification_binary", (N_BINARY,), [("host", binary_host), ("torch", binary_torch), ("meter", binary_meter)], batches)
del batches, logit, true
torch.cuda.empty_cache()

for rows, C in MULTI:
    z = torch.empty((rows, C), device=dev).normal_(generator=gen) * 2
    y = torch.multinomial(torch.softmax(z[:, :C], 1), 1).reshape(-1)
    batches = []
    for a, b in cuts(rows):
        score = F.log_softmax(z[a:b], dim=-1)
        batches.append((y[a:b], score, F.nll_loss(score, y[a:b]), z[a:b]))
    run("classification_multi", (rows, C), [("host", multi_host), ("torch", multi_torch), ("meter", multi_meter)], batches,
        extra=[("meter_logits", multi_meter_logits)])
    del batches, z, y
    torch.cuda.empty_cache()
