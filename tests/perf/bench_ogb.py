"""Timings of the molecule path — integer-coded features, generalogbconv — against the torch formulation of the
reference.  A script, not collected by pytest.

A molecule-like batch at ogbg-molhiv's ratios: N nodes, 2.2 N directed edges (every bond in both directions, degree <= 4
by construction: a node's bonds go to its next neighbours in node order), integer features drawn uniformly within the
dims; d in D.  One process, the same buffers; the forms of a pair alternate over ROUNDS rounds of ITERS back-to-back
runs each (one untimed run first), timed with device events; medians and minima in ms.

  (a) generalogbconv forward + backward (gradients of x, weight and the three bond tables), agg add and max:
      engine     GeneralOGBConvLayer: x W, the two-gather aggregation over a [60, d] table; the table gradient on the
                 default dispatch (ops.code_reduce_path: add on the one-hot operator, max on mp_code_reduce_f32)
      torch      sum of F.embedding -> [E, d], index_select -> [E, d], index_add_ / scatter_reduce(amax) by destination
      bytes      engine: x W writes N d; the aggregation reads ~2.2 N d gathered rows and writes N d; the backward
                 reads dY twice (dx on the transposed operator, the table reduce) and writes N d: ~ (1 + 3.2 + 1 + 2.2 + 1
                 + 1) N d * 4 B without the weight gradient.  torch: every [E, d] tensor written and read adds 2 * 2.2 N d.
  (b) the table reduce alone, mp_code_reduce_f32 against the aggregation on the transposed one-hot operator:
      Bond   C = 60, items = the 2.2 N entries by destination row (rowptr form), dY [N, d]: reads N d floats
      Atom   C = 173, R = N rows of K = 9 codes: reads N d floats
  (c) embed_sum forward (Atom, K = 9) against sum(F.embedding), and a plain [N, d] store stream (fill_) for the rate a
      store stream reaches: bytes = N d * 4 written (the 173-row table stays in cache).

    N=1000000 D=256,300 python tests/perf/bench_ogb.py profiles/ogb_bench.json"""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
import graphgym_amd as ga  # noqa: E402
from graphgym_amd import encoders, ops  # noqa: E402
from graphgym_amd.config import cfg  # noqa: E402
from graphgym_amd.harness import Batch  # noqa: E402
from graphgym_amd.ogbconv import GeneralOGBConvLayer, pack_bond_codes  # noqa: E402

dev = torch.device("cuda:0")
N = int(os.environ.get("N", "1000000"))
WIDTHS = [int(v) for v in os.environ.get("D", "256,300").split(",")]
ROUNDS = int(os.environ.get("ROUNDS", "3"))
ITERS = int(os.environ.get("ITERS", "5"))
out_path = sys.argv[1]
ATOM, BOND = encoders.full_atom_feature_dims, encoders.full_bond_feature_dims


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


def ab(*fns):
    ts = [[] for _ in fns]
    for _ in range(ROUNDS):
        for t, fn in zip(ts, fns):
            t.append(timed(fn, ITERS))
    return [{"median": round(statistics.median(t), 3), "min": round(min(t), 3), "all": [round(v, 3) for v in t]}
            for t in ts]


def molecule_edges(n, gen):
    """1.1 n bonds: node i -- i + 1 (a chain), and every tenth node i -- i + 3; both directions"""
    a = torch.arange(n - 1)
    b = torch.arange(0, n - 3, 10)
    src = torch.cat([a, b])
    dst = torch.cat([a + 1, b + 3])
    ei = torch.stack([torch.cat([src, dst]), torch.cat([dst, src])])
    bonds = torch.stack([torch.randint(0, k, (src.numel(),), generator=gen) for k in BOND], dim=1).repeat(2, 1)
    return ei, bonds


gen = torch.Generator().manual_seed(0)
ei_c, bonds_c = molecule_edges(N, gen)
E = ei_c.size(1)
ei, bonds = ei_c.to(dev), bonds_c.to(dev)
atoms = torch.stack([torch.randint(0, k, (N,), generator=gen) for k in ATOM], dim=1).to(dev)
result = {"what": "ogb", "N": N, "E": E, "rounds": ROUNDS, "iters": ITERS, "widths": {}}

for d in WIDTHS:
    res = {}
    x = (torch.rand(N, d, generator=gen) * 2 - 1).to(dev).requires_grad_(True)
    dy = (torch.rand(N, d, generator=gen) * 2 - 1).to(dev)
    row_bytes = N * d * 4

    # (a) the layer
    for agg in ("add", "max"):
        cfg.gnn.agg, cfg.gnn.normalize_adj = agg, False
        torch.manual_seed(0)
        layer = GeneralOGBConvLayer(d, d, bias=False).to(dev)
        tables = [e.weight for e in layer.bond_encoder.bond_embedding_list]
        leaves = [x, layer.weight] + tables
        batch = Batch(node_feature=x, edge_index=ei, edge_feature=bonds)
        src, dst = ei[0], ei[1]

        def engine():
            return torch.autograd.grad(layer(x, ei, bonds, holder=batch), leaves, dy)

        def reference():
            h = x @ layer.weight
            ef = 0
            for k in range(3):
                ef = ef + F.embedding(bonds[:, k], tables[k])
            msg = h.index_select(0, src) + ef
            if agg == "add":
                out = torch.zeros(N, d, device=dev).index_add_(0, dst, msg)
            else:
                out = torch.zeros(N, d, device=dev).scatter_reduce(0, dst[:, None].expand(-1, d), msg, "amax",
                                                                   include_self=False)
            return torch.autograd.grad(out, leaves, dy)
        ge, gr = engine(), reference()
        rel = [float((a - b).abs().max() / b.abs().max().clamp(min=1e-30)) for a, b in zip(ge, gr)]
        del ge, gr
        t_e, t_r = ab(engine, reference)
        res["layer_" + agg] = {"engine_ms": t_e, "torch_ms": t_r, "ratio": round(t_e["median"] / t_r["median"], 3),
                               "grad_max_rel_diff": dict(zip(("x", "weight", "T0", "T1", "T2"), rel)),
                               "rows_N_d_MB": round(row_bytes / 1e6, 1), "entry_rows_E_d_MB": round(E * d * 4 / 1e6, 1)}
        g = batch._mp_graph_cache[(1, "none", None, 1.0)]
        qe = ops.entry_codes(g, encoders.cached_codes(batch, "edge_feature", bonds, BOND, make=pack_bond_codes))[0]
        del layer, batch

    # (b) the table reduce alone
    def bond_kernel():
        return ops._raw_code_reduce(dy, qe, 60, rowptr=g.rowptr, rows=g.row_ids(), w=g.val)[0]
    onehot = ga.CSRGraph.from_edge_index(torch.stack([g.row_ids().long(), qe.long()]), 60, num_cols=N)
    onehot.plan()

    def bond_fallback():
        return ops._raw_spmm(onehot, dy, ops._lib.SUM)[0]
    rel_b = float((bond_kernel() - bond_fallback()).abs().max() / bond_fallback().abs().max())
    t_k, t_f = ab(bond_kernel, bond_fallback)
    res["reduce_bond_C60"] = {"kernel_ms": t_k, "fallback_ms": t_f, "max_rel_diff": rel_b,
                              "kernel_GBps": round(row_bytes / (t_k["median"] * 1e-3) / 1e9, 1),
                              "fallback_GBps": round(row_bytes / (t_f["median"] * 1e-3) / 1e9, 1)}
    codes = ops.check_codes(atoms, ATOM)
    off = ops._offsets_dev(encoders.table_offsets(ATOM), dev)

    def atom_kernel():
        return ops._raw_code_reduce(dy, codes, 173, K=9, off=off, disjoint=True)[0]
    off_host = encoders.table_offsets(ATOM)
    ops._code_reduce_fallback(dy, codes, off_host, 173)                 # builds and caches the operator

    def atom_fallback():
        return ops._code_reduce_fallback(dy, codes, off_host, 173)
    rel_a = float((atom_kernel() - atom_fallback()).abs().max() / atom_fallback().abs().max())
    t_k, t_f = ab(atom_kernel, atom_fallback)
    res["reduce_atom_C173"] = {"kernel_ms": t_k, "fallback_ms": t_f, "max_rel_diff": rel_a,
                               "kernel_GBps": round(row_bytes / (t_k["median"] * 1e-3) / 1e9, 1),
                               "fallback_GBps": round(row_bytes / (t_f["median"] * 1e-3) / 1e9, 1),
                               "slabs": ops._raw_code_reduce(dy, codes, 173, K=9, off=off, disjoint=True)[1]}

    # (c) embed_sum forward
    table = (torch.rand(173, d, generator=gen) * 2 - 1).to(dev)
    parts = list(torch.split(table, ATOM))
    out = torch.empty(N, d, device=dev)
    with torch.no_grad():
        def embed_engine():
            return ops._raw_embed_sum(codes, table, off, out=out)

        def embed_torch():
            acc = 0
            for k in range(9):
                acc = acc + F.embedding(atoms[:, k], parts[k])
            return acc

        def store_stream():
            return out.fill_(1.0)
        same = bool(torch.equal(embed_engine(), embed_torch()))
        t_e, t_t, t_s = ab(embed_engine, embed_torch, store_stream)
    res["embed_sum_atom"] = {"engine_ms": t_e, "torch_ms": t_t, "store_stream_ms": t_s, "equal": same,
                             "engine_GBps": round(row_bytes / (t_e["median"] * 1e-3) / 1e9, 1),
                             "store_stream_GBps": round(row_bytes / (t_s["median"] * 1e-3) / 1e9, 1)}
    result["widths"][str(d)] = res
    print(json.dumps({str(d): res}), flush=True)
    del x, dy, out, onehot

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, "w") as f:
    f.write(json.dumps(result, indent=1) + "\n")
