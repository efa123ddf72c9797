"""Timings of the two kernels under generaledgeattconvv1 / v2 on BA graphs (graphgen, m = 5), d = 256, H = 4 — a script,
not collected by pytest.  Sizes: 2e6 nodes (~2e7 entries, the size tests/perf/bench_next.py uses for the other edge
kernels) and 2e4 nodes (~2e5 entries, a training batch), NODES=a,b,...

  (a) mp_spmm_csr_edge_heads_f32, all heads in one launch, against H launches of mp_spmm_csr_edge_f32 on column slices
      (the form every head count outside 1, 2, 4, 8 takes), reduce sum and max.  The H launches are timed twice: on
      per-head graphs and weight columns prepared once ("per_head_ms", the kernels alone) and as the operator runs them,
      slicing w and wrapping the graph per call ("per_head_op_ms");
  (b) mp_edge_att_alpha_f32 against the torch composition of the same coefficients: three gathers, two adds, leaky_relu
      and ops.edge_softmax (mp_csr_row_softmax_f32).

One process, the same buffers; the forms of a pair alternate over ROUNDS rounds of back-to-back runs each (one untimed
run first; ITERS runs at 2e6 nodes, more at smaller sizes so that a round lasts milliseconds), timed with device events;
medians in ms.  The outputs of a pair are compared (bit equality for (a): the same terms in the same order; a relative
bound for (b): other summation order).  Algorithmic bytes, from shapes:
  one launch   nnz * (2 d 4 + 8 + 4 H) + N d 4          H launches   nnz * (2 d 4 + H (8 + 4)) + N d 4
  alpha        nnz * (8 + 3 * 4 H) + 2 N * 4 H          composition  nnz * 4 H * 13 + nnz * 24 (index reads as int64)

    NODES=2000000,20000 D=256 HEADS=4 python tests/perf/bench_edgeatt.py profiles/edgeatt_kernels.json"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402
import graphgym_amd as ga  # noqa: E402
from graphgym_amd import _lib, graphgen, ops  # noqa: E402

dev = torch.device("cuda:0")
SIZES = [int(v) for v in os.environ.get("NODES", "2000000,20000").split(",")]
d = int(os.environ.get("D", "256"))
H = int(os.environ.get("HEADS", "4"))
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


def measure(n):
    ei = graphgen.ba_edge_index(n, 5, seed=12345, device=dev)
    g = ga.CSRGraph.from_edge_index(ei, n)
    E, nnz = ei.size(1), g.nnz
    gen = torch.Generator(device=dev).manual_seed(7)
    X = torch.empty((n, d), device=dev).uniform_(-1.0, 1.0, generator=gen)
    M = torch.empty((E, d), device=dev).uniform_(-1.0, 1.0, generator=gen)
    w = torch.empty((nnz, H), device=dev).uniform_(0.0, 1.0, generator=gen)
    g.plan(), g.max_row_entries(), g.row_ids()
    dh = d // H
    wh = [w[:, h].contiguous() for h in range(H)]
    gh = [g.with_values(v) for v in wh]
    for q in gh:
        ops._eid_checked(q, E)
    y_slices = torch.empty((n, d), device=dev)
    iters = ITERS * max(1, min(100, 2000000 // n))
    result = {"n": n, "nnz": nnz, "iters": iters, "M_GB": round(E * d * 4 / 1e9, 3)}

    with torch.no_grad():
        for name, red in (("sum", _lib.SUM), ("max", _lib.MAX)):
            def one(red=red):
                return ops._raw_spmm_edge_heads(g, w, X, M, None, None, H, red, False, one_launch=True)[0]

            def per_head(red=red):
                for h in range(H):
                    cs = slice(h * dh, (h + 1) * dh)
                    ops._raw_spmm_edge(gh[h], X[:, cs], M[:, cs], None, None, red, False, out=y_slices[:, cs])
                return y_slices

            def per_head_op(red=red):
                return ops._raw_spmm_edge_heads(g, w, X, M, None, None, H, red, False, one_launch=False)[0]
            same = torch.equal(one(), per_head()) and torch.equal(one(), per_head_op())
            t_one, t_per, t_op = ab(iters, one, per_head, per_head_op)
            b_one = nnz * (2 * d * 4 + 8 + 4 * H) + n * d * 4
            b_per = nnz * (2 * d * 4 + H * 12) + n * d * 4
            result["agg_" + name] = {"equal": bool(same), "one_launch_ms": t_one, "per_head_ms": t_per,
                                     "per_head_op_ms": t_op,
                                     "speedup": round(t_per["median"] / t_one["median"], 3),
                                     "one_launch_GB": round(b_one / 1e9, 3), "per_head_GB": round(b_per / 1e9, 3),
                                     "one_launch_TBps": round(b_one / (t_one["median"] * 1e-3) / 1e12, 3)}

        a_dst = torch.empty((n, H), device=dev).normal_(generator=gen)
        a_src = torch.empty((n, H), device=dev).normal_(generator=gen)
        a_edge = torch.empty((E, H), device=dev).normal_(generator=gen)
        rows, cols, eids = g.row_ids().long(), g.col.long(), g.eid.long()

        def kernel():
            return ops.edge_att_alpha(g, a_dst, a_src, a_edge, 0.2)

        def composition():
            s = torch.nn.functional.leaky_relu(a_dst[rows] + a_src[cols] + a_edge[eids], 0.2)
            return ops.edge_softmax(g, s)
        ak, ac = kernel(), composition()
        rel = float(((ak - ac).abs() / ac.abs().clamp(min=1e-30)).max())
        t_k, t_c = ab(iters, kernel, composition)
        b_k = nnz * (8 + 3 * 4 * H) + 2 * n * 4 * H
        b_c = nnz * 4 * H * 13 + nnz * 24
        result["alpha"] = {"max_rel_diff": rel, "kernel_ms": t_k, "composition_ms": t_c,
                           "speedup": round(t_c["median"] / t_k["median"], 3), "kernel_GB": round(b_k / 1e9, 3),
                           "composition_GB": round(b_c / 1e9, 3)}

    return result


out = {"what": "edgeatt_kernels", "d": d, "heads": H, "rounds": ROUNDS, "sizes": [measure(n) for n in SIZES]}
print(json.dumps(out), flush=True)
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(json.dumps(out, indent=1) + "\n")
