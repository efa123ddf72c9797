"""Timings of the mini-batch subgraph samplers (graphgym_amd.samplers, csrc/sample.hip) on the BA(N, 5) graph graphgen
builds.  A script, not collected by pytest.

  saint_rw     ROOTS walks of 4 steps          saint_node / saint_edge   DRAWS draws          random_node   PARTS parts
  sample_batch the whole call (draw, bitmap, node list, count, fill, edge_index; two host reads), device events
  draw         the draw alone (random_node: mp_sample_parts and the masked list)
  bitmap       zero + mp_bitmap_mark + mp_bitmap_word_counts + cumsum, and mp_bitmap_nodes
  count        mp_induced_count + cumsum
  fill         mp_induced_fill
  torch        the comparand: the torch formulation of the SAME batch from the same draw — mask both endpoints of the
               base's edge list (held on the device as int64 [2, nnz], prepared outside the timed region), relabel through
               an int64 [N] table, CSRGraph.from_edge_index — checked to give the same CSR

Medians of REPEATS runs after WARMUPS untimed ones.

    N=10000000 python tests/perf/bench_samplers.py profiles/sampler_bench.json"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402
import graphgym_amd as ga  # noqa: E402
from graphgym_amd import graphgen, samplers as S  # noqa: E402

dev = torch.device("cuda:0")
N = int(os.environ.get("N", "10000000"))
ROOTS, DRAWS, PARTS = int(os.environ.get("ROOTS", "100000")), int(os.environ.get("DRAWS", "200000")), \
    int(os.environ.get("PARTS", "32"))
WARMUPS, REPEATS = int(os.environ.get("WARMUPS", "5")), int(os.environ.get("REPEATS", "20"))
out_path = sys.argv[1]


def timed(fn):
    for _ in range(WARMUPS):
        fn()
    ts = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {"median_ms": round(statistics.median(ts), 4), "min_ms": round(min(ts), 4), "max_ms": round(max(ts), 4)}


ei = graphgen.ba_edge_index(N, 5, seed=12345, device=dev)
base = ga.CSRGraph.from_edge_index(ei, N)
src, dst = base.col.long(), base.row_ids().long()           # the base's edge list in CSR order, for the comparand
del ei
rec = {"device": torch.cuda.get_device_name(0), "graph": f"BA({N}, 5)", "nodes": N, "entries": base.nnz,
       "warmups": WARMUPS, "repeats": REPEATS, "samplers": {}}


def torch_formulation(nodes):
    v = nodes[nodes >= 0].long()
    mask = torch.zeros(N, dtype=torch.bool, device=dev)
    mask[v] = True
    keep = mask[src] & mask[dst]
    relabel = torch.cumsum(mask, 0) - 1
    n_sub = int(mask.sum())
    sub = torch.stack([relabel[src[keep]], relabel[dst[keep]]])
    return ga.CSRGraph.from_edge_index(sub, n_sub, validate=False), n_sub


PLANS = {"saint_rw": dict(batch_size=ROOTS, walk_length=4), "saint_node": dict(batch_size=DRAWS),
         "saint_edge": dict(batch_size=DRAWS), "random_node": dict(num_parts=PARTS)}
for kind, kw in PLANS.items():
    plan = S.plan_sampler(base, kind, **kw)
    step = [0]

    def whole():
        step[0] += 1
        return S.sample_batch(plan, 1, step[0])

    r = {"sample_batch": timed(whole)}
    # the pieces, on the draw of one fixed step
    nodes = S._draw_for_bitmap(plan, 1, 3)
    bitmap, rank = S._node_bitmap(nodes, N)
    n_sub = int(rank[-2])
    orig = S._node_list(bitmap, rank, n_sub)
    rowptr = S._count_rows(base, orig, n_sub, bitmap)
    nnz = int(rowptr[n_sub])
    r["n_sub"], r["nnz_sub"], r["drawn"] = n_sub, nnz, int((nodes >= 0).sum())
    r["draw"] = timed(lambda: S._draw_for_bitmap(plan, 1, 3))
    r["bitmap"] = timed(lambda: S._node_list(*S._node_bitmap(nodes, N), n_sub))
    r["count"] = timed(lambda: S._count_rows(base, orig, n_sub, bitmap))
    r["fill"] = timed(lambda: S._fill_rows(base, orig, n_sub, bitmap, rank, rowptr, nnz))
    r["torch"] = timed(lambda: torch_formulation(nodes))
    ours, (ref, n_ref) = S.induced_subgraph(base, nodes, plan.symmetric), torch_formulation(nodes)
    r["equals_torch"] = bool(n_ref == ours.num_nodes and torch.equal(ref.rowptr, ours.graph.rowptr)
                             and torch.equal(ref.col, ours.graph.col))
    r["torch_over_sample_batch"] = round(r["torch"]["median_ms"] / r["sample_batch"]["median_ms"], 2)
    rec["samplers"][kind] = r
    print(kind, json.dumps(r), flush=True)

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(rec, f, indent=1)
print(json.dumps(rec))
