"""A/B of the link-prediction head's pair decoding: harness.GNNEdgeHead on the engine route (ops.pair_score /
ops.pair_sum: graphgym_amd/pair_ops.py) against the reference's composition (h[edge_label_index] -> (a * b).sum(-1) /
F.cosine_similarity / cat -> MLP), the same module, process and tensors; the route is switched by harness.PAIR_DECODE_MIN
(1: engine, None: composition).

  full    link_batch of BA(NODES, 5) at ratio 1 (K = 2 x the supervision edges), d in WIDTHS, the three decodings
          (layers_post_mp = 1), forward + backward: the engine with the PairIndex built inside every step (a new pair list
          per step, as resampled negatives give), the engine with batch.pair_index built ahead, and the composition
  sweep   the same at d = 64 and d = 256 on random K-subsets of the pairs, K d halving from SWEEP_TOP down to SWEEP_BOTTOM:
          the crossover that sets harness.PAIR_DECODE_MIN (index build included)

Per record: ms per forward + backward (median over ROUNDS rounds of ITERS back-to-back runs between device events, after
untimed warm-up runs of every shape on both routes; the routes alternate), the comparand's spread (max - min) / median,
the peak of torch.cuda.max_memory_allocated above the inputs over one step, the host reads of one step (warnings of
torch.cuda.set_sync_debug_mode("warn")), the forward's dispatched ops, and max |difference| / max |value| of the
predictions and of dh between the routes.  The last line of the run states the crossover.

    NODES=1000000 WIDTHS=64,128,256 python scripts/pair_decode_ab.py profiles/pair_decode_ab.jsonl
    FULL=0 SWEEP_TOP=268435456 SWEEP_BOTTOM=67108864 python scripts/pair_decode_ab.py profiles/pair_decode_ab.jsonl   # appends"""
import json, os, statistics, sys, warnings
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from torch.utils._python_dispatch import TorchDispatchMode
import graphgym_amd as ga
import graphgym_amd.graphgym_plugin  # noqa: F401
from graphgym_amd import graphgen, ops, pair_ops
from graphgym_amd import harness as H
from graphgym_amd.config import cfg
from graphgym_amd.link_pred import link_batch, link_split

dev = torch.device("cuda:0")
n = int(os.environ.get("NODES", "1000000"))
WIDTHS = [int(v) for v in os.environ.get("WIDTHS", "64,128,256").split(",")]
ROUNDS = int(os.environ.get("ROUNDS", "3"))
ITERS = int(os.environ.get("ITERS", "5"))
SWEEP_ITERS = int(os.environ.get("SWEEP_ITERS", "20"))
SWEEP_TOP = int(os.environ.get("SWEEP_TOP", str(1 << 25)))
SWEEP_BOTTOM = int(os.environ.get("SWEEP_BOTTOM", str(1 << 14)))
DECODINGS = tuple(os.environ.get("DECODINGS", "dot,cosine_similarity,concat").split(","))
FULL_RUN = os.environ.get("FULL", "1") != "0"          # FULL=0: the sweep alone (a second sweep over another range)
out_path = sys.argv[1]


class Count(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.n = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.n += 1
        return func(*args, **(kwargs or {}))


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


def stats(ts):
    med = statistics.median(ts)
    return {"median": round(med, 4), "min": round(min(ts), 4), "max": round(max(ts), 4),
            "spread": round((max(ts) - min(ts)) / med, 4)}


def rel(a, b):
    return float((a - b).abs().max() / b.abs().max().clamp(min=1e-30))


def make_step(head, h, idx, label, route, prebuilt):
    """one forward + backward of the head on the given route; route 'engine': a PairIndex built inside the step unless
    `prebuilt` (then batch.pair_index carries one built ahead)"""
    pi = ops.pair_index(idx, h.size(0)) if prebuilt else None
    if prebuilt and head.decoding == "concat":
        pi.role_operators()

    def step():
        H.PAIR_DECODE_MIN = 1 if route == "engine" else None
        if route == "engine" and not prebuilt:
            pair_ops._cache.clear()
        head.zero_grad(set_to_none=True)
        h.grad = None
        batch = H.Batch(node_feature=h, edge_label_index=idx, edge_label=label)
        if pi is not None:
            batch.pair_index = pi
        pred, _ = head(batch)
        pred.sum().backward()
        return pred.detach(), h.grad
    return step


def facts(step):
    """(peak bytes above what is allocated before the step, host reads, dispatched forward + loss ops) of one step"""
    step()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            step()
            torch.cuda.synchronize()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    reads = sum("synchroniz" in str(x.message) for x in w)
    with Count() as c:
        step()
    return int(peak), int(reads), c.n


def ab(what, decoding, d, K, head, h, idx, label, iters, variants):
    steps = {name: make_step(head, h, idx, label, route, pre) for name, (route, pre) in variants.items()}
    for s in steps.values():
        s(), s()
    ts = {name: [] for name in steps}
    for _ in range(ROUNDS):
        for name, s in steps.items():
            ts[name].append(timed(s, iters))
    outs = {name: s() for name, s in steps.items()}
    rec = {"what": what, "decoding": decoding, "n": n, "K": K, "d": d, "Kd": K * d, "rounds": ROUNDS, "iters": iters}
    for name, s in steps.items():
        peak, reads, nops = facts(s)
        rec[name] = {"ms": stats(ts[name]), "peak_bytes": peak, "host_reads": reads, "forward_ops": nops}
    for name in steps:
        if name != "composition":
            rec[name]["speedup"] = round(rec["composition"]["ms"]["median"] / rec[name]["ms"]["median"], 3)
            rec[name]["rel_diff_pred"] = rel(outs[name][0], outs["composition"][0])
            rec[name]["rel_diff_dh"] = rel(outs[name][1], outs["composition"][1])
    rec["one_gathered_operand_bytes"] = K * d * 4
    print(json.dumps(rec), flush=True)
    with open(out_path, "a") as f:
        f.write(json.dumps(rec) + "\n")
    return rec


def head_of(decoding, d):
    cfg.model.edge_decoding, cfg.gnn.layers_post_mp = decoding, 1
    torch.manual_seed(0)
    return H.GNNEdgeHead(d, 1).to(dev)


ei = graphgen.ba_edge_index(n, 5, seed=12345, device=dev)
base = ga.CSRGraph.from_edge_index(ei, n)
splits = link_split(base, torch.tensor([0, n]), (0.8, 0.2), generator=torch.Generator().manual_seed(0))
x0 = torch.zeros((n, 1), device=dev)
batch = link_batch(splits["train"], x0, ratio=1.0, seed=1, offset=0)
index, labels = batch.edge_label_index.contiguous(), batch.edge_label
K_full = index.size(1)
gen = torch.Generator(device=dev).manual_seed(7)
FULL = {"engine": ("engine", False), "engine_prebuilt": ("engine", True), "composition": ("composition", False)}
SWEEP = {"engine": ("engine", False), "composition": ("composition", False)}
old_min = H.PAIR_DECODE_MIN
try:
    for d in (WIDTHS if FULL_RUN else ()):
        h = torch.empty((n, d), device=dev).uniform_(-1.0, 1.0, generator=gen).requires_grad_(True)
        for decoding in DECODINGS:
            ab("full", decoding, d, K_full, head_of(decoding, d), h, index, labels, ITERS, FULL)
        del h
        torch.cuda.empty_cache()
    perm = torch.randperm(K_full, device=dev, generator=gen)
    lost = {}
    for d in (64, 256):
        h = torch.empty((n, d), device=dev).uniform_(-1.0, 1.0, generator=gen).requires_grad_(True)
        kd = SWEEP_TOP
        while kd >= SWEEP_BOTTOM:
            K = min(kd // d, K_full)
            sub = index[:, perm[:K]].contiguous()
            for decoding in DECODINGS:
                rec = ab("sweep", decoding, d, K, head_of(decoding, d), h, sub, labels[perm[:K]], SWEEP_ITERS, SWEEP)
                if rec["engine"]["ms"]["median"] > rec["composition"]["ms"]["median"]:
                    lost[(d, decoding)] = max(lost.get((d, decoding), 0), K * d)
            kd //= 2
        del h
        torch.cuda.empty_cache()
    worst = max(lost.values(), default=0)
    crossover = 1
    while crossover <= worst:
        crossover *= 2
    rec = {"what": "crossover", "largest_Kd_lost": {f"{d}/{dec}": v for (d, dec), v in lost.items()},
           "smallest_power_of_two_above": crossover, "sweep": [SWEEP_BOTTOM, SWEEP_TOP]}
    print(json.dumps(rec), flush=True)
    with open(out_path, "a") as f:
        f.write(json.dumps(rec) + "\n")
finally:
    H.PAIR_DECODE_MIN = old_min
