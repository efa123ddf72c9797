"""A/B of one neighbour-sampled batch by two routes on one device, on BA(NODES, 5) with the fanouts SIZES and BATCH seeds:

  device  graphgym_amd.neighbor.neighbor_batch: the seed draw, the per-hop marks into the bitmap, the frontier lists,
          the counts and the in-group sort of every row (csrc/neighbor.hip), its host reads included;
  torch   the same subgraph from torch operators: per hop index_select of the drawn entries' columns and a unique over
          the nodes so far, then the relabelling by searchsorted and a sort of the entries into CSR order.  torch has no
          keyed draw, so this route is HANDED the base positions the device route drew (per hop) and its time holds the
          subgraph's construction only — it is the cheaper half of what a torch sampler would do.

Both routes build the same batch (orig_node and edge_index are compared on every round).  Wall-clock from a synchronised
device to a synchronised device, the two routes alternating inside one process, ROUNDS different steps after WARMUP
untimed ones; median, p90 and min in ms.  The record also holds the batch's n_sub and nnz (of the last round; they move
little from step to step) and the device route's host reads, counted on Tensor.item / Tensor.tolist.

    python scripts/neighbor_ab.py [OUT.json]        # default profiles/neighbor_bench.json"""
import json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import graphgym_amd as ga
from graphgym_amd import graphgen, neighbor as NB

dev = torch.device("cuda:0")
NODES = int(os.environ.get("NODES", "10000000"))
SIZES = [int(s) for s in os.environ.get("SIZES", "20,15,10").split(",")]
BATCH = int(os.environ.get("BATCH", "1024"))
ROUNDS = int(os.environ.get("ROUNDS", "30"))
WARMUP = int(os.environ.get("WARMUP", "3"))
out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "neighbor_bench.json")


def p90(v):
    s = sorted(v)
    return s[min(len(s) - 1, int(round(0.9 * (len(s) - 1))))]


def stats(t):
    return {"median_ms": round(statistics.median(t), 3), "p90_ms": round(p90(t), 3), "min_ms": round(min(t), 3)}


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def entries_by_hop(b):
    """the base positions drawn at every hop, as the torch route takes them"""
    rows = b.edge_index[1]
    return [b.base_entry[b.hop[rows] == h].long() for h in range(len(SIZES))]


def torch_route(base, seeds, drawn):
    rowptr, col = base.rowptr.long(), base.col.long()
    nodes = torch.unique(seeds.long())
    for e in drawn:
        nodes = torch.unique(torch.cat([nodes, col.index_select(0, e)]))
    e = torch.sort(torch.cat(drawn)).values                     # CSR order: ascending base position
    row = torch.searchsorted(rowptr, e, right=True) - 1
    src, dst = torch.searchsorted(nodes, col.index_select(0, e)), torch.searchsorted(nodes, row)
    rp = torch.zeros(nodes.numel() + 1, dtype=torch.int64, device=nodes.device)
    torch.cumsum(torch.bincount(dst, minlength=nodes.numel()), 0, out=rp[1:])
    return nodes, torch.stack([src, dst]), rp


def count_reads(fn):
    n = [0]
    item, tolist = torch.Tensor.item, torch.Tensor.tolist

    def counted(real):
        def f(self, *a, **k):
            n[0] += int(self.is_cuda)
            return real(self, *a, **k)
        return f
    torch.Tensor.item, torch.Tensor.tolist = counted(item), counted(tolist)
    try:
        fn()
    finally:
        torch.Tensor.item, torch.Tensor.tolist = item, tolist
    return n[0]


base = ga.CSRGraph.from_edge_index(graphgen.ba_edge_index(NODES, 5, seed=1, device=dev), NODES)
plan = NB.plan_neighbor(base, SIZES, BATCH)
ours, theirs = [], []
for step in range(WARMUP + ROUNDS):
    t_dev, b = timed(lambda: NB.neighbor_batch(plan, 0, step))
    seeds, drawn = NB.seeds(plan, 0, step), entries_by_hop(b)
    t_torch, (nodes, ei, rp) = timed(lambda: torch_route(base, seeds, drawn))
    assert torch.equal(nodes, b.orig_node) and torch.equal(ei, b.edge_index) and torch.equal(rp.int(), b.graph.rowptr)
    if step >= WARMUP:
        ours.append(t_dev)
        theirs.append(t_torch)
reads = count_reads(lambda: NB.neighbor_batch(plan, 0, 0))
rec = {"what": "neighbor_ab", "graph": f"BA({NODES}, 5)", "nodes": base.num_nodes, "nnz": base.nnz, "sizes": SIZES,
       "batch_size": BATCH, "rounds": ROUNDS, "warmup": WARMUP, "n_sub": b.num_nodes, "nnz_sub": b.graph.nnz,
       "nodes_per_hop": torch.bincount(b.hop.long(), minlength=len(SIZES) + 1).tolist(),
       "device": stats(ours), "torch_given_the_draw": stats(theirs), "host_reads_per_batch": reads,
       "torch_over_device_median": round(statistics.median(theirs) / statistics.median(ours), 2),
       "same_batch_every_round": True}
print(json.dumps(rec), flush=True)
with open(out_path, "w") as f:
    json.dump(rec, f, indent=1)
    f.write("\n")
