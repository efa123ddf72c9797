"""No op may depend on the contents of its fresh allocations.

Every buffer the engine writes into comes from Python as `torch.empty`.  In a fresh process those pages are mostly zero;
in a training loop the caching allocator hands back the previous step's activations.  Each case below runs one operator
family three times under tests/_poison.py — every `torch.empty` filled with 0, then with the integer 1 (a float
denormal), then with the sentinel NaN — building EVERYTHING inside the poisoned context (graphs, plans, transposes,
hot-column tags, modules), and asserts

  1. the guards around every allocation still hold the fill (nothing was written outside the bytes asked for);
  2. no returned element carries the fill's bit pattern where the baseline does not, and every float of the baseline is
     finite (every element the caller may read was written by the launch);
  3. every returned tensor equals the zero-filled run bit for bit (no workspace, plan blob or flag is read before the
     entry that uses it has initialised it);
  4. the recorder saw every C entry the case claims (tests/test_poison_host.py closes the table over _lib.PROTOTYPES);
  5. where tests/_*_ref.py or oracle.ref_ops holds an operator-level reference (aggregation, gcn_norm, the two-gather
     and multi-head aggregations, the attention coefficients and row softmax, the coded features, networkx for the
     structure counters and hop distances), the baseline run against it at the tolerances of _tol.py.  The cases
     without one (the BatchNorm family, the transforms, the loss, bf16, the samplers, splits and collation) have
     their references inside their own parity tests, not as shared helpers: here they are held by 1-4 alone.

The outputs that use float atomics (the `max` backward, mp_spmm_heads_max_bwd_f32, weighted
mp_csr_degree(AXIS_COL), mp_rows_scatter_add_f32 and mp_softmax_ce_bwd_f32 with repeated rows) get operands whose sums
are exact in fp32 in any order — integers in [-8, 8], weights that are powers of two in [1/4, 4], at most two terms where
the terms are not exact — so that they, too, are held bit for bit (tests/test_poison_host.py checks the exactness).

The order of the fills is a safety rule: an index or counter read uninitialised is 1 under the second fill, in range for
every case (all have at least 4 rows and columns), so the result comes out wrong instead of as a wild address; the NaN
fill runs only after the integer-1 run matched the baseline."""
import collections

import pytest
import torch

import _link_graphs as LG
import _sampler_graphs as SG
from _poison import FILLS, Recorder, fill_hits, poisoned, raw_bits, same_bits
from _tol import both, close

pytestmark = pytest.mark.gpu

# run(dev) -> tuple of tensors; entries: the C entries the run must reach; setup(monkeypatch): switches of the case;
# oracle(outs): holds the baseline outputs to an existing reference; unspecified: (header line quoted, fn(dev) -> one bool
# mask or None per output, computed from the inputs alone) for a region include/mp_engine.h leaves undefined
Case = collections.namedtuple("Case", "name entries run exact unspecified setup oracle",
                              defaults=(True, None, None, None))

N_NODES = 320
PLAN_CONFIG = (64, 1, 64, 64)


def gen(seed):
    return torch.Generator().manual_seed(seed)


def ints(*shape, seed, lo=-8, hi=8):
    """integers in [lo, hi] as fp32: sums of a few thousand of them (times a power of two) are exact in any order"""
    return torch.randint(lo, hi + 1, shape, generator=gen(seed)).float()


def pow2(n, seed):
    """powers of two in [1/4, 4]"""
    return 2.0 ** torch.randint(-2, 3, (n,), generator=gen(seed)).float()


def rnd(*shape, seed):
    return torch.randn(*shape, generator=gen(seed))


def hub_edges(n=N_NODES, E=4000, hub=1300, seed=1):
    """(src, dst, w): `hub` entries forced into destination 3 (a hub row under PLAN_CONFIG and under the defaults), one
    row in twenty empty — the recipe of _gradsub.hub_graph (keep the two alike), on the host so that oracles and the
    host test can rebuild it, and with weights that are powers of two (exact sums under float atomics)"""
    g = gen(seed)
    dst = torch.randint(0, n, (E,), generator=g)
    src = torch.randint(0, n, (E,), generator=g)
    dst[:hub] = 3
    keep = dst % 20 != 7
    src, dst = src[keep], dst[keep]
    return src, dst, pow2(dst.numel(), seed + 1)


def hub_graph(dev, weighted=True, **build):
    import graphgym_amd as ga
    src, dst, w = hub_edges()
    G = ga.CSRGraph.from_edge_index(torch.stack([src, dst]).to(dev), N_NODES, w.to(dev) if weighted else None, **build)
    assert G.plan()[1][1] > 0, "the hub pieces and the finalize kernel must be live"
    return G


def leaf(t, dev):
    return t.to(dev).requires_grad_(True)


def entries_of(g):
    """[rows, cols, eids, val or an empty tensor] of g's stored entries in CSR order: what the per-entry oracles index by"""
    return [g.row_ids(), g.col, g.eid, g.val if g.val is not None else torch.zeros(0, device=g.device)]


def host_entries(outs):
    rows, cols, eids, val = (t.cpu() for t in outs[-4:])
    return rows.long(), cols.long(), eids.long(), (val if val.numel() else None)


def counts_tensor(counts):
    return torch.tensor(list(counts), dtype=torch.int32)


# ---------------------------------------------------------------------------------------------- graph structures
def run_graph_build(dev):
    import graphgym_amd as ga
    src, dst, w = hub_edges()
    ei = torch.stack([src, dst]).to(dev)
    g = ga.CSRGraph.from_edge_index(ei, N_NODES, w.to(dev), add_self_loops=True, fill=2.0)
    gu = ga.CSRGraph.from_edge_index(ei, N_NODES, remove_self_loops=True)
    und = torch.cat([ei, ei.flip(0)], 1)
    gs = ga.CSRGraph.from_edge_index(torch.unique(und, dim=1), N_NODES)          # symmetric, no repeated entry
    t, tu = g._transpose_sorted(), gu._transpose_sorted()
    sym = torch.tensor([int(g.is_symmetric(run=True)), int(gs.is_symmetric(run=True))])
    assert sym.tolist() == [0, 1]
    gn, gc = g.gcn_norm("row"), g.gcn_norm("col")
    sc = g.scaled(row_scale=pow2(N_NODES, 5).to(dev), col_scale=pow2(N_NODES, 6).to(dev))
    ids = torch.randperm(N_NODES, generator=gen(7))[:30].to(dev)
    marked = g.mark_ids(ids)
    plan, counts = g.plan()
    assert counts[1] > 0
    return (g.rowptr, g.col, g.val, g.eid, g.row_ids(), gu.rowptr, gu.col, gu.eid, t.rowptr, t.col, t.val, t.pos,
            tu.rowptr, tu.col, tu.pos, g.degree("row"), g.degree("col"), gu.degree("row"), gn.val, gn.dinv, gc.val,
            sc.val, marked, sym, counts_tensor(counts), gs.rowptr, gs.col)


def oracle_graph_build(outs):
    """gn = D^-1/2 (A + 2 I) D^-1/2 with row degrees against gcn_norm_adj (improved: loops of weight 2), as dense matrices
    (tests/test_parity_gpu.py: test_gcn_norm_matches_golden_both_flavours)"""
    from oracle import ref_ops as R
    src, dst, w = hub_edges()
    n = N_NODES
    rows, cols, val, dinv = outs[4].cpu().long(), outs[1].cpu().long(), outs[18].cpu(), outs[19].cpu()
    A = torch.zeros(n, n).index_put_((rows, cols), val, accumulate=True)
    refs = both(lambda c: R.gcn_norm_adj(R.SparseAdj(torch.stack([dst, src]), c(w), [n, n]), improved=True))
    dense = [torch.zeros(n, n, dtype=r.edge_weight.dtype).index_put_((r.row, r.col), r.edge_weight, accumulate=True)
             for r in refs]
    close(A, (dense[0], dense[1]), what="gcn_norm row")
    deg = both(lambda c: torch.zeros(n, dtype=c(w).dtype).index_add_(0, dst, c(w)) + 2.0)
    close(dinv[:, None], tuple(d.pow(-0.5)[:, None] for d in deg), what="dinv")
    assert torch.equal(outs[15].cpu().double(), deg[0])                       # degree('row'): powers of two, exact


def run_degree_col(dev):
    """weighted mp_csr_degree(AXIS_COL) on the C ABI (float atomics; CSRGraph.degree('col') takes the transposed CSR)"""
    from graphgym_amd import _lib
    from graphgym_amd._lib import check, ptr
    from graphgym_amd.graph import _stream
    g = hub_graph(dev)
    out = []
    for val in (g.val, None):
        deg = torch.empty(N_NODES, dtype=torch.float32, device=dev)
        check(_lib.lib().mp_csr_degree(ptr(g.rowptr), ptr(g.col), ptr(val), N_NODES, g.nnz, _lib.AXIS_COL, ptr(deg),
                                       _stream()), "mp_csr_degree")
        out.append(deg)
    return tuple(out)


def oracle_degree_col(outs):
    src, dst, w = hub_edges()
    ref = torch.zeros(N_NODES, dtype=torch.float64).index_add_(0, src, w.double())
    assert torch.equal(outs[0].cpu().double(), ref)
    assert torch.equal(outs[1].cpu().long(), torch.bincount(src, minlength=N_NODES))


# ---------------------------------------------------------------------------------------- plan-based aggregation
AGG = [("sum", 1.5, True, True), ("mean", 0.0, False, False), ("max", 1.25, True, True)]


def _agg_inputs(d):
    return ints(N_NODES, d, seed=d), ints(d, seed=d + 1), ints(N_NODES, d, seed=d + 2)


def run_spmm(dev, d):
    from graphgym_amd import ops
    g = hub_graph(dev)
    x0, b0, dy = _agg_inputs(d)
    out = []
    for red, ss, has_b, relu in AGG:
        x, b = leaf(x0, dev), (leaf(b0, dev) if has_b else None)
        y = ops.spmm(g, x, red, self_scale=ss, bias=b, relu=relu)
        y.backward(dy.to(dev))
        out += [y.detach(), x.grad] + ([b.grad] if has_b else [])
    return tuple(out)


def oracle_spmm(d):
    def check(outs):
        from oracle import ref_ops as R
        src, dst, w = hub_edges()
        x0, b0, _ = _agg_inputs(d)
        at = 0
        for red, ss, has_b, relu in AGG:
            def ref(c):
                r = R.coo_aggregate(dst, src, c(w), c(x0), N_NODES, red) + ss * c(x0)
                r = r + c(b0) if has_b else r
                return torch.relu(r) if relu else r
            close(outs[at].cpu(), both(ref), what=f"spmm {red} d={d}")
            at += 3 if has_b else 2
    return check


def run_spmm_eval(dev, d):
    from graphgym_amd import ops
    g = hub_graph(dev)
    x = rnd(N_NODES, d, seed=d).to(dev)
    cs, ct = (torch.rand(d, generator=gen(d)) + 0.5).to(dev), rnd(d, seed=d + 3).to(dev)
    return tuple(ops.spmm_fused_eval(g, x, "sum", self_scale=0.5, col_scale=cs, col_shift=ct, relu=True, l2norm=l2)
                 for l2 in (False, True))


def run_idgnn(dev, d, dtype=torch.float32):
    from graphgym_amd import ops
    g = hub_graph(dev)
    x = leaf(ints(N_NODES, d, seed=d).to(dtype), dev)
    ids = torch.randperm(N_NODES, generator=gen(d))[:N_NODES // 9].to(dev)
    P, Q = ops.idgnn_aggregate(g, ids, x)
    torch.autograd.backward([P, Q], [ints(N_NODES, d, seed=d + 1).to(dtype).to(dev),
                                     ints(N_NODES, d, seed=d + 2).to(dtype).to(dev)])
    return P.detach(), Q.detach(), x.grad


def oracle_idgnn(d):
    def check(outs):
        from oracle import ref_ops as R
        src, dst, w = hub_edges()
        x = ints(N_NODES, d, seed=d)
        sel = torch.zeros(N_NODES, 1)
        sel[torch.randperm(N_NODES, generator=gen(d))[:N_NODES // 9]] = 1
        close(outs[0].cpu(), both(lambda c: R.coo_aggregate(dst, src, c(w), c(x), N_NODES, "sum")), what=f"P d={d}")
        close(outs[1].cpu(), both(lambda c: R.coo_aggregate(dst, src, c(w), c(x * sel), N_NODES, "sum")),
              what=f"Q d={d}")
    return check


def run_bf16(dev, d):
    from graphgym_amd import ops
    g = hub_graph(dev)
    out = []
    for red in ("sum", "max"):
        x = leaf(ints(N_NODES, d, seed=d).to(torch.bfloat16), dev)
        y = ops.spmm(g, x, red, self_scale=0.5)
        y.backward(ints(N_NODES, d, seed=d + 1, lo=-2, hi=2).to(torch.bfloat16).to(dev))
        out += [y.detach(), x.grad]
    return tuple(out) + run_idgnn(dev, d, torch.bfloat16)


# ------------------------------------------------------------------------------------------------ tile kernels
def setup_tiles(mp):
    from graphgym_amd import ops
    mp.setenv("MP_AGG_TILES", "1")
    mp.setattr(ops, "AGG_TILES_MIN_ROWS", 1)


def setup_hot(mp):
    from graphgym_amd import ops
    setup_tiles(mp)
    mp.setattr(ops, "AGG_HOT_MIN_BYTES", 1)
    mp.setenv("MP_AGG_HOT_MB", "0.1")           # about a hundred (d = 256) or two hundred (d = 128) of the 320 rows


TILE_AGG = [("sum", 1.5), ("mean", 0.0), ("max", 0.0)]


def run_tiles(dev, d, hot=False):
    from graphgym_amd import ops
    g = hub_graph(dev)
    x = rnd(N_NODES, d, seed=d).to(dev)
    out = []
    for red, ss in TILE_AGG:
        tiles, hots = ops.AGG_TILES_CALLS, ops.AGG_HOT_CALLS
        with torch.no_grad():
            out.append(ops.spmm(g, x, red, self_scale=ss))
        assert ops.AGG_TILES_CALLS == tiles + 1 and ops.AGG_HOT_CALLS == hots + (1 if hot else 0)
    return tuple(out)


def oracle_tiles(d):
    def check(outs):
        from oracle import ref_ops as R
        src, dst, w = hub_edges()
        x = rnd(N_NODES, d, seed=d)
        for (red, ss), y in zip(TILE_AGG, outs):
            close(y.cpu(), both(lambda c: R.coo_aggregate(dst, src, c(w), c(x), N_NODES, red) + ss * c(x)),
                  what=f"tiles {red} d={d}")
    return check


def run_idgnn_tiles(dev, d):
    from graphgym_amd import _lib, ops
    from graphgym_amd._lib import check, ptr
    from graphgym_amd.graph import _stream
    before = ops.AGG_TILES_CALLS
    out = run_idgnn(dev, d)
    assert ops.AGG_TILES_CALLS > before          # (the forward; the backward's aggregations take the tile kernel too)
    # the small kernel alone, on the C ABI: it writes the rows that own an identity entry and no other
    g = hub_graph(dev)
    ids = torch.randperm(N_NODES, generator=gen(d))[:N_NODES // 9].to(dev)
    br = g.id_branch(ids)
    Z = rnd(ids.numel(), d, seed=d + 5).to(dev)
    rows_out = torch.empty((N_NODES, d), dtype=torch.float32, device=dev)
    check(_lib.lib().mp_id_rows_f32(ptr(br.rows), ptr(br.crp), ptr(br.slot), ptr(br.val), br.n_rows, ptr(Z), Z.stride(0),
                                    ptr(rows_out), rows_out.stride(0), d, _stream()), "mp_id_rows_f32")
    return out + (rows_out,)


ID_ROWS_HEADER = ("include/mp_engine.h, mp_id_rows_f32: \"it writes out[rows[k], :] for the n_rows listed rows; every other "
                  "row of out is left untouched and is undefined in a fresh buffer\"")


def unspecified_id_rows(d):
    """the rows of mp_id_rows_f32's output that own no entry from an identity node, from the inputs alone"""
    def masks(dev):
        src, dst, _ = hub_edges()
        ids = torch.randperm(N_NODES, generator=gen(d))[:N_NODES // 9]
        listed = torch.zeros(N_NODES, dtype=torch.bool)
        listed[dst[torch.isin(src, ids)]] = True
        assert 0 < int(listed.sum()) < N_NODES
        return (None, None, None, (~listed)[:, None].expand(N_NODES, d).contiguous())
    return (ID_ROWS_HEADER, masks)


# ------------------------------------------------------------------------------- one-kernel layer and transforms
def run_fused(dev, F):
    from graphgym_amd import ops
    g = hub_graph(dev)
    dout = 64
    x0, W0, b0 = rnd(N_NODES, F, seed=F), rnd(F, dout, seed=F + 1) / F ** 0.5, rnd(dout, seed=F + 2)
    Wi0 = rnd(F, dout, seed=F + 3) / F ** 0.5
    dy = rnd(N_NODES, dout, seed=F + 4).to(dev)
    ids = torch.randperm(N_NODES, generator=gen(F))[:N_NODES // 9].to(dev)
    out = []
    for ss in (0.0, 0.5):
        x, W, b = leaf(x0, dev), leaf(W0, dev), leaf(b0, dev)
        assert ops.agg_dense_supported(g, x, W)
        y = ops.agg_dense(g, x, W, bias=b, relu=True, self_scale=ss)
        y.backward(dy)
        out += [y.detach(), x.grad, W.grad, b.grad]
        x, W, Wi, b = leaf(x0, dev), leaf(W0, dev), leaf(Wi0, dev), leaf(b0, dev)
        y = ops.agg_dense_id(g, x, W, Wi, ids, bias=b, relu=True, self_scale=ss)
        assert y is not None and ids.numel() > 0
        y.backward(dy)
        out += [y.detach(), x.grad, W.grad, Wi.grad, b.grad]
    # the bf16 x 3 product (on by default only from 2^14 rows)
    with torch.no_grad():
        y, P = ops._raw_agg_dense(g, x0.to(dev), W0.to(dev), b0.to(dev), True, S=x0.to(dev), self_scale=0.5, want_P=True,
                                  bf16x3=True)
    return tuple(out) + (y, P)


def oracle_fused(F):
    def check(outs):
        from oracle import ref_ops as R
        src, dst, w = hub_edges()
        x, W, b = rnd(N_NODES, F, seed=F), rnd(F, 64, seed=F + 1) / F ** 0.5, rnd(64, seed=F + 2)
        for at, ss in ((0, 0.0), (9, 0.5)):
            close(outs[at].cpu(), both(lambda c: torch.relu(
                (R.coo_aggregate(dst, src, c(w), c(x), N_NODES, "sum") + ss * c(x)) @ c(W) + c(b))),
                what=f"one-kernel layer F={F} self={ss}")
    return check


def run_sage(dev):
    from graphgym_amd import ops
    g = hub_graph(dev, weighted=False)
    F, k = 64, 64
    x, Ws, Wn = leaf(rnd(N_NODES, F, seed=1), dev), leaf(rnd(F, k, seed=2) / 8, dev), leaf(rnd(F, k, seed=3) / 8, dev)
    b = leaf(rnd(2 * k, seed=4), dev)
    assert ops.agg_dense_supported(g, x, Wn)
    y = ops.sage_concat(g, x, Ws, Wn, bias=b, relu=True)
    y.backward(rnd(N_NODES, 2 * k, seed=5).to(dev))
    return y.detach(), x.grad, Ws.grad, Wn.grad, b.grad


def setup_x3(mp):
    from graphgym_amd import ops
    mp.setattr(ops, "X3_MIN_ROWS", 1)


WGRAD_SHAPES = [(1, 64), (8, 64), (64, 7), (64, 16), (256, 256), (264, 132)]      # one per form of the weight gradient


def run_dense(dev, x3):
    from graphgym_amd import ops
    out = []
    shapes = [(300, 64, 128)] if x3 else [(300, 64, 128), (129, 72, 100), (200, 13, 33)]
    for M, F, d in shapes:
        for dual in ((False,) if x3 else (False, True)):
            P, W = leaf(rnd(M, F, seed=F), dev), leaf(rnd(F, d, seed=F + 1) / F ** 0.5, dev)
            b = leaf(rnd(d, seed=F + 2), dev)
            Q = leaf(rnd(M, F, seed=F + 3), dev) if dual else None
            Wi = leaf(rnd(F, d, seed=F + 4) / F ** 0.5, dev) if dual else None
            assert ops.dense_x3_supported(P, F, d) == (x3 and not dual)
            y = ops.dense_fused(P, W, Q, Wi, bias=b, relu=True)
            y.backward(rnd(M, d, seed=F + 5).to(dev))
            out += [y.detach(), P.grad, W.grad, b.grad] + ([Q.grad, Wi.grad] if dual else [])
    if not x3:
        for F, d in WGRAD_SHAPES:
            M = 2100 if F <= 8 else 700
            P, G, Y = rnd(M, F, seed=F).to(dev), rnd(M, d, seed=F + d).to(dev), rnd(M, d, seed=F + d + 1).to(dev)
            out += list(ops._raw_dense_wgrad(P, G, want_bias=True))
            out += list(ops._raw_dense_wgrad_relu(P, G, Y, want_bias=True))
        for ku, kn in ((64, 64), (7, 9)):
            x, m = leaf(rnd(500, 64, seed=ku), dev), leaf(rnd(500, 24, seed=ku + 1), dev)
            Ws, Wn = leaf(rnd(64, ku, seed=ku + 2) / 8, dev), leaf(rnd(24, kn, seed=ku + 3) / 5, dev)
            b = leaf(rnd(ku + kn, seed=ku + 4), dev)
            y = ops.concat_dense(x, m, Ws, Wn, b, relu=True)
            y.backward(rnd(500, ku + kn, seed=ku + 5).to(dev))
            out += [y.detach(), x.grad, m.grad, Ws.grad, Wn.grad, b.grad]
    return tuple(out)


# -------------------------------------------------------------------- BatchNorm, activation, skip and dropout
BN_SHAPES = [(2, 4), (333, 7), (4097, 100)]


def _bn(d, dev, relu=False):
    from graphgym_amd import nn as mpnn
    bn = mpnn.BatchNorm1d(d, relu=relu)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(d, generator=gen(d)) + 0.5)
        bn.bias.copy_(rnd(d, seed=d + 1) * 0.1)
    return bn.to(dev).train()


def _bn_x(N, d, dev, seed=0):
    return leaf(rnd(N, d, seed=N + seed) * 2 + rnd(d, seed=d + seed), dev)


def _module_outs(y, bn, *leaves):
    return [y.detach()] + [t.grad for t in leaves] + [bn.weight.grad, bn.bias.grad, bn.running_mean, bn.running_var]


def run_bn(dev, N, d):
    out = []
    for relu in (False, True):
        bn, x = _bn(d, dev, relu), _bn_x(N, d, dev)
        y = bn(x)
        y.backward(rnd(N, d, seed=3).to(dev))
        out += _module_outs(y, bn, x)
    return tuple(out)


def _acts(dev):
    return [torch.nn.PReLU().to(dev), torch.nn.ELU()]


def run_bn_act(dev, N, d):
    from graphgym_amd import nn as mpnn
    out = []
    for act in _acts(dev):
        bn, x = _bn(d, dev), _bn_x(N, d, dev)
        y = mpnn.bn_act_module(bn, x, act)
        y.backward(rnd(N, d, seed=3).to(dev))
        out += _module_outs(y, bn, x) + [p.grad for p in act.parameters()]
    return tuple(out)


def _skip(N, d, mode, dev):
    return leaf(rnd(N, d if mode == "skipsum" else d + 3, seed=N + d), dev)


def run_bn_skip(dev, N, d):
    from graphgym_amd import nn as mpnn
    out = []
    for mode in ("skipsum", "skipconcat"):
        for act in [None] + _acts(dev):
            bn, x, skip = _bn(d, dev), _bn_x(N, d, dev), _skip(N, d, mode, dev)
            y = mpnn.bn_skip_act(bn, x, skip, mode, relu=True, act=act)
            y.backward(rnd(*y.shape, seed=3).to(dev))
            out += _module_outs(y, bn, x, skip) + ([] if act is None else [p.grad for p in act.parameters()])
    return tuple(out)


def run_bn_drop(dev, N, d):
    from graphgym_amd import nn as mpnn
    out = []
    x = _bn_x(N, d, dev)
    drop = mpnn.Dropout(0.3, seed=11).train()
    y = drop(x)
    y.backward(rnd(N, d, seed=3).to(dev))
    out += [y.detach(), x.grad]
    for act in _acts(dev):
        bn, x, drop = _bn(d, dev), _bn_x(N, d, dev), mpnn.Dropout(0.3, seed=12).train()
        y = mpnn.bn_act_module(bn, x, act, drop=drop)
        y.backward(rnd(N, d, seed=3).to(dev))
        out += _module_outs(y, bn, x) + [p.grad for p in act.parameters()]
        for mode in ("skipsum", "skipconcat"):
            bn, x, skip = _bn(d, dev), _bn_x(N, d, dev), _skip(N, d, mode, dev)
            drop = mpnn.Dropout(0.3, seed=13).train()
            y = mpnn.bn_skip_act(bn, x, skip, mode, act=act, drop=drop)
            y.backward(rnd(*y.shape, seed=3).to(dev))
            out += _module_outs(y, bn, x, skip) + [p.grad for p in act.parameters()]
    return tuple(out)


# --------------------------------------------------------------------------------- loss, rows, coded features
def run_softmax_ce(dev):
    out = []
    n = 400
    for Cn in (3, 41):
        g = gen(Cn)
        z0 = torch.randn(n, Cn, generator=g) * 3
        # no row more than twice: two terms added onto zero give the same bits in either order
        idx = torch.cat([torch.randperm(n, generator=g)[:150], torch.randperm(n, generator=g)[:100]])
        assert int(torch.bincount(idx).max()) <= 2
        for index, n_lab in ((idx, idx.numel()), (None, n), (None, 250)):
            z = leaf(z0, dev)
            lab = torch.randint(0, Cn, (n_lab,), generator=gen(Cn + n_lab)).to(dev)
            loss = torch.ops.mp.softmax_ce(z, lab, None if index is None else index.to(dev))
            (loss * 0.75).backward()
            out += [loss.detach().reshape(1), z.grad]
    return tuple(out)


def run_rows(dev):
    from graphgym_amd import ops
    out = []
    n, k = 120, 90
    for d in (7, 64):
        x, h, u = leaf(ints(n, d, seed=d), dev), leaf(ints(n, d, seed=d + 1), dev), leaf(ints(k, d, seed=d + 2), dev)
        ids = torch.randint(0, n, (k,), generator=gen(d)).to(dev)                  # repeated rows: they accumulate
        y = ops.gather_rows(x, ids)
        y.backward(ints(k, d, seed=d + 3).to(dev))
        s = ops.index_add_rows(h, ids, u)
        s.backward(ints(n, d, seed=d + 4).to(dev))
        out += [y.detach(), x.grad, s.detach(), h.grad, u.grad]
    return tuple(out)


def oracle_rows(outs):
    at = 0
    for d in (7, 64):
        x, h, u = ints(120, d, seed=d), ints(120, d, seed=d + 1), ints(90, d, seed=d + 2)
        ids = torch.randint(0, 120, (90,), generator=gen(d))
        assert torch.equal(outs[at].cpu(), x[ids])
        assert torch.equal(outs[at + 1].cpu(), torch.zeros(120, d).index_add_(0, ids, ints(90, d, seed=d + 3)))
        assert torch.equal(outs[at + 2].cpu(), h.index_add(0, ids, u))
        at += 5


def setup_code_kernel(mp):
    mp.setenv("MP_CODE_REDUCE", "kernel")


def run_codes(dev, path):
    """embed_sum forward and backward with a table below (173 rows) and above (300 rows) the code-reduce kernel's cap;
    spmm_code with sum / mean / max; path: 'kernel' (MP_CODE_REDUCE=kernel, see setup) or 'operator'"""
    from graphgym_amd import ops
    cap = ops.code_reduce_cap()
    out = []
    R = 333
    for dims, d in CODE_TABLES:
        n_codes = sum(dims)
        assert (n_codes > cap) == (n_codes == 300) and ops.code_reduce_path(n_codes) == (
            "operator" if n_codes > cap else path)
        offsets = [sum(dims[:k]) for k in range(len(dims))]
        codes = torch.stack([torch.randint(0, m, (R,), generator=gen(m + k)) for k, m in enumerate(dims)], 1).to(dev)
        table = leaf(rnd(n_codes, d, seed=d), dev)
        y = ops.embed_sum(codes, table, offsets)
        y.backward(rnd(R, d, seed=d + 1).to(dev))
        out += [y.detach(), table.grad]
    g = hub_graph(dev)
    src, _, _ = hub_edges()
    E, n_codes = src.numel(), 60
    codes = torch.randint(0, n_codes, (E,), generator=gen(9)).to(torch.int32).to(dev)
    for d in (64, 100):
        for red in ("sum", "mean", "max"):
            x, table = leaf(ints(N_NODES, d, seed=d), dev), leaf(ints(n_codes, d, seed=d + 1), dev)
            b = leaf(ints(d, seed=d + 2), dev)
            y = ops.spmm_code(g, x, table, codes, reduce=red, bias=b)
            y.backward(ints(N_NODES, d, seed=d + 3).to(dev))
            out += [y.detach(), x.grad, table.grad, b.grad]
    return tuple(out + entries_of(g))


CODE_TABLES = (((119, 5, 12, 12, 10, 6, 6, 2, 1), 64), ((60, 40, 73), 100), ((150, 100, 50), 100))


def oracle_codes(outs):
    import _ogb_ref as OG
    rows, cols, eids, val = host_entries(outs)
    at = 0
    for dims, d in CODE_TABLES:
        codes = torch.stack([torch.randint(0, m, (333,), generator=gen(m + k)) for k, m in enumerate(dims)], 1)
        table, off = rnd(sum(dims), d, seed=d), [sum(dims[:k]) for k in range(len(dims))]
        close(outs[at].cpu(), both(lambda c: OG.encode(codes, [c(table)[o:o + m] for o, m in zip(off, dims)])),
              what=f"embed_sum {len(dims)} tables d={d}")
        at += 2
    q = torch.randint(0, 60, (hub_edges()[0].numel(),), generator=gen(9))[eids]
    for d in (64, 100):
        x, table, b = ints(N_NODES, d, seed=d), ints(60, d, seed=d + 1), ints(d, seed=d + 2)
        for red in ("sum", "mean", "max"):
            close(outs[at].cpu(), both(lambda c: OG.spmm_code(rows, cols, q, c(val), c(x), c(table), c(b), N_NODES, red)),
                  what=f"spmm_code {red} d={d}")
            at += 4


# --------------------------------------------------------------------------------------------------- attention
TIER_COUNTS = [0, 1, 5, 15, 16, 17, 63, 64, 65, 100, 300, 2047, 2048, 2049, 3000] + [(5 * i) % 17 for i in range(49)]


def tier_edges(seed=0):
    """64 rows with a short (one lane), a medium (a 16-lane group) and a long (the workgroup) row of the row softmax, and
    the boundaries between the tiers"""
    g = gen(seed)
    n = len(TIER_COUNTS)
    counts = torch.tensor(TIER_COUNTS)[torch.randperm(n, generator=g)]
    dst = torch.repeat_interleave(torch.arange(n), counts)
    src = torch.randint(0, n - 1, (dst.numel(),), generator=g)
    src = src + (src >= dst).long()
    ei = torch.stack([src, dst])
    return ei[:, torch.randperm(ei.size(1), generator=g)], n


def run_softmax_tiers(dev):
    import graphgym_amd as ga
    from graphgym_amd import ops
    ei, n = tier_edges()
    E = ei.size(1)
    out = []
    for loops in (False, True):
        g = ga.CSRGraph.from_edge_index(ei.to(dev), n, add_self_loops=loops)
        for H in (1, 4):
            s = leaf(rnd(g.nnz, H, seed=H), dev)
            p = ops.edge_softmax(g, s)
            p.backward(rnd(g.nnz, H, seed=H + 1).to(dev))
            a_dst, a_src = rnd(n, H, seed=H + 2).to(dev), rnd(n, H, seed=H + 3).to(dev)
            a_edge = rnd(E, H, seed=H + 4).to(dev)
            with torch.no_grad():
                al = ops.gat_alpha(g, a_dst, a_src)
                ae = ops.edge_att_alpha(g, a_dst, a_src, a_edge)
                ae0 = ops.edge_att_alpha(g, None, a_src, a_edge)
                ds = ops._raw_row_softmax_bwd(g, al, rnd(g.nnz, H, seed=H + 5).to(dev))
            out += [p.detach(), s.grad, al, ae, ae0, ds]
        out += entries_of(g)[:3]
    # the coefficients' own backward: d_dst and d_src are index_add_ sums (float atomics) of terms that are not exact, so
    # a ring in both directions — two entries per row and per column: two terms onto zero add alike in either order
    n, H = 64, 4
    fwd = torch.stack([torch.arange(n), (torch.arange(n) + 1) % n])
    g = ga.CSRGraph.from_edge_index(torch.cat([fwd, fwd.flip(0)], 1).to(dev), n)
    assert int(torch.bincount(g.col.cpu()).max()) == 2 and g.max_row_entries() == 2
    a_dst, a_src, a_edge = leaf(rnd(n, H, seed=21), dev), leaf(rnd(n, H, seed=22), dev), leaf(rnd(2 * n, H, seed=23), dev)
    ops.gat_alpha(g, a_dst, a_src).backward(rnd(g.nnz, H, seed=24).to(dev))
    out += [a_dst.grad, a_src.grad]
    a_dst, a_src = leaf(rnd(n, H, seed=21), dev), leaf(rnd(n, H, seed=22), dev)
    ops.edge_att_alpha(g, a_dst, a_src, a_edge).backward(rnd(g.nnz, H, seed=25).to(dev))
    return tuple(out + [a_dst.grad, a_src.grad, a_edge.grad])


def oracle_softmax_tiers(outs):
    import _att_ref as AT
    import _edgeatt_ref as EA
    ei, n = tier_edges()
    E = ei.size(1)
    for k in range(2):
        at = 15 * k
        rows, cols, eids = (t.cpu().long() for t in outs[at + 12:at + 15])
        for j, H in enumerate((1, 4)):
            s = rnd(rows.numel(), H, seed=H)
            a_dst, a_src, a_edge = rnd(n, H, seed=H + 2), rnd(n, H, seed=H + 3), rnd(E, H, seed=H + 4)
            o = outs[at + 6 * j:at + 6 * j + 6]
            what = f"softmax tiers loops={bool(k)} H={H}"
            close(o[0].cpu(), both(lambda c: AT.segment_softmax(c(s), rows, n)), what=what + " edge_softmax")
            close(o[2].cpu(), both(lambda c: EA.edge_att_alpha(rows, cols, eids, c(a_dst), c(a_src), c(a_edge)[:0], n)),
                  what=what + " gat_alpha")
            close(o[3].cpu(), both(lambda c: EA.edge_att_alpha(rows, cols, eids, c(a_dst), c(a_src), c(a_edge), n)),
                  what=what + " edge_att_alpha")
            close(o[4].cpu(), both(lambda c: EA.edge_att_alpha(rows, cols, eids, None, c(a_src), c(a_edge), n)),
                  what=what + " edge_att_alpha without a_dst")


def run_sddmm(dev):
    from graphgym_amd import ops
    g = hub_graph(dev, weighted=False)
    out = []
    for heads, d in SDDMM_SHAPES:
        Q, K = leaf(rnd(N_NODES, d, seed=d), dev), leaf(rnd(N_NODES, d, seed=d + 1), dev)
        s = ops.sddmm_dot(g, Q, K, heads=heads, scale=0.5)
        s.backward(rnd(g.nnz, heads, seed=d + 2).to(dev))
        out += [s.detach(), Q.grad, K.grad]
    # s = leaky_relu(ai[row] + aj[col]): the gradients are index_add_ sums (float atomics): integers, slope 1/4
    ai, aj = leaf(ints(N_NODES, seed=1), dev), leaf(ints(N_NODES, seed=2), dev)
    s = ops.sddmm_add(g, ai, aj, slope=0.25)
    s.backward(ints(g.nnz, 1, seed=3, lo=-2, hi=2).to(dev))
    return tuple(out) + (s.detach(), ai.grad, aj.grad) + tuple(entries_of(g))


SDDMM_SHAPES = ((1, 100), (4, 64), (8, 128), (4, 24), (2, 512))      # the last two: the row kernel's head layouts


def oracle_sddmm(outs):
    """the per-entry dot products and the additive scores, evaluated as tests/test_layouts_gpu.py does"""
    rows, cols, _, _ = host_entries(outs)
    for k, (heads, d) in enumerate(SDDMM_SHAPES):
        Q, K = rnd(N_NODES, d, seed=d), rnd(N_NODES, d, seed=d + 1)

        def ref(c, absolute=False):
            a = (lambda t: c(t).abs()) if absolute else c
            return (a(Q)[rows].view(-1, heads, d // heads) * a(K)[cols].view(-1, heads, d // heads)).sum(-1) * 0.5
        close(outs[3 * k].cpu(), both(ref), what=f"sddmm_dot heads={heads} d={d}", mag=both(lambda c: ref(c, True))[0])
    ai, aj = ints(N_NODES, seed=1), ints(N_NODES, seed=2)
    want = torch.nn.functional.leaky_relu(ai[rows] + aj[cols], 0.25)
    assert torch.equal(outs[3 * len(SDDMM_SHAPES)].cpu().view(-1), want)             # integers and quarters: exact


def run_edge_values(dev):
    from graphgym_amd import ops
    g = hub_graph(dev, weighted=False)
    out = []
    for heads, d in EDGE_VALUE_SHAPES:
        for red in ("sum", "mean", "max"):
            a = leaf(pow2(g.nnz * heads, seed=heads).view(g.nnz, heads), dev)
            V = leaf(ints(N_NODES, d, seed=d), dev)
            y = ops.spmm_edge_values(g, a, V, heads=heads, reduce=red)
            y.backward(ints(N_NODES, d, seed=d + 1, lo=-2, hi=2).to(dev))
            out += [y.detach(), a.grad, V.grad]
    return tuple(out + entries_of(g))


EDGE_VALUE_SHAPES = ((1, 100), (4, 64), (2, 6), (3, 12), (4, 24))


def oracle_edge_values(outs):
    import _att_ref as AT
    rows, cols, _, _ = host_entries(outs)
    at = 0
    for heads, d in EDGE_VALUE_SHAPES:
        a, V = pow2(rows.numel() * heads, seed=heads).view(-1, heads), ints(N_NODES, d, seed=d)
        for red in ("sum", "mean", "max"):
            close(outs[at].cpu(), both(lambda c: AT.edge_values_agg(rows, cols, c(a), c(V), N_NODES, heads, red)),
                  what=f"spmm_edge_values heads={heads} d={d} {red}")
            at += 3


def run_spmm_edge(dev):
    from graphgym_amd import ops
    g = hub_graph(dev, add_self_loops=True)            # inserted loops: entries without an edge term
    E = hub_edges()[0].numel()
    out = []
    for d in (64, 100):
        for red in ("sum", "mean", "max"):
            x, m = leaf(ints(N_NODES, d, seed=d), dev), leaf(ints(E, d, seed=d + 1), dev)
            t = leaf(ints(N_NODES, d, seed=d + 2), dev)
            b = leaf(ints(d, seed=d + 3), dev)
            y = ops.spmm_edge(g, x, m, reduce=red, t=t, bias=b)
            y.backward(ints(N_NODES, d, seed=d + 4, lo=-2, hi=2).to(dev))
            out += [y.detach(), x.grad, m.grad, t.grad, b.grad]
    return tuple(out + entries_of(g))


def _edge_operands(d):
    E = hub_edges()[0].numel()
    return ints(N_NODES, d, seed=d), ints(E, d, seed=d + 1), ints(N_NODES, d, seed=d + 2), ints(d, seed=d + 3)


def oracle_spmm_edge(outs):
    import _edgeconv_ref as EC
    rows, cols, eids, val = host_entries(outs)
    at = 0
    for d in (64, 100):
        x, m, t, b = _edge_operands(d)
        for red in ("sum", "mean", "max"):
            close(outs[at].cpu(),
                  both(lambda c: EC.edge_agg(rows, cols, eids, c(val), c(x), c(m), c(t), c(b), N_NODES, red)),
                  what=f"spmm_edge {red} d={d}")
            at += 5


def run_spmm_edge_heads(dev):
    from graphgym_amd import ops
    g = hub_graph(dev, weighted=False, add_self_loops=True)
    E = hub_edges()[0].numel()
    out = []
    for heads, d in EDGE_HEAD_SHAPES:
        for red in ("sum", "mean", "max"):
            w = leaf(pow2(g.nnz * heads, seed=heads).view(g.nnz, heads), dev)
            x, m = leaf(ints(N_NODES, d, seed=d), dev), leaf(ints(E, d, seed=d + 1), dev)
            t = leaf(ints(N_NODES, d, seed=d + 2), dev)
            b = leaf(ints(d, seed=d + 3), dev)
            y = ops.spmm_edge_heads(g, w, x, m, t=t, heads=heads, reduce=red, bias=b)
            y.backward(ints(N_NODES, d, seed=d + 4, lo=-2, hi=2).to(dev))
            out += [y.detach(), w.grad, x.grad, m.grad, t.grad, b.grad]
    return tuple(out + entries_of(g))


EDGE_HEAD_SHAPES = ((4, 64), (2, 100), (3, 12))


def oracle_spmm_edge_heads(outs):
    import _edgeatt_ref as EA
    rows, cols, eids, _ = host_entries(outs)
    at = 0
    for heads, d in EDGE_HEAD_SHAPES:
        w = pow2(rows.numel() * heads, seed=heads).view(-1, heads)
        x, m, t, b = _edge_operands(d)
        for red in ("sum", "mean", "max"):
            close(outs[at].cpu(), both(lambda c: EA.edge_heads_agg(rows, cols, eids, c(w), c(x), c(m), c(t), c(b), N_NODES,
                                                                   heads, red)),
                  what=f"spmm_edge_heads heads={heads} d={d} {red}")
            at += 6


# ------------------------------------------------------------------------------------------------ batch builders
def _csr_outs(g):
    return [] if g is None else [g.rowptr, g.col, g.eid]


def run_ego(dev):
    from graphgym_amd.ego import ego_batch
    out = []
    for name, centres in (("ring65", [0, 7, 33, 64]), ("ring33", [5, 6]), ("star200", [0, 17]), ("cycle6_chord", [0, 4])):
        base = SG.build(name, dev)
        cen = torch.tensor(centres, device=dev)
        for csr in (None, "none", "add"):
            r = ego_batch(base, cen, 2, csr=csr)
            out += list(r[:4]) + (_csr_outs(r[4]) if csr is not None else [])
            if csr is not None and r[4] is not None:
                br = r[4].id_branch(r[2])
                out += [br.rows, br.crp, br.slot, br.defer]
    return tuple(out)


EDGE_NET_CASES = [(name, directed) for name in ("batch_2_5_9", "components", "path4") for directed in (False, True)]


def _label_pairs(gp, N):
    """[2, 12] (src, dst) pairs, both ends in one graph of gp"""
    g = gen(N)
    graph_of = torch.searchsorted(gp, torch.arange(N), right=True) - 1
    s = torch.randint(0, N, (12,), generator=g)
    lo, hi = gp[graph_of[s]], gp[graph_of[s] + 1]
    t = lo + (torch.rand(12, generator=g) * (hi - lo)).long()
    return torch.stack([s, torch.minimum(t, hi - 1)])


def run_edge_nets(dev):
    from graphgym_amd import edge_nets
    out, hops = [], []
    for name, directed in EDGE_NET_CASES:
        base, gp, _ = LG.build(name, directed, dev)
        N = base.num_nodes
        li = _label_pairs(gp, N)
        x = rnd(N, 5, seed=N).to(dev)
        for sources in (None, "labels"):
            batch, gb = edge_nets.edge_batch(base, gp, li, torch.arange(12), x, sources=sources, csr="none")
            out += [batch.edge_index, batch.node_id_index, batch.orig_node, batch.copy_of_node, batch.orig_edge,
                    batch.node_label_index, batch.batch, batch.node_feature] + _csr_outs(gb)
        hops.append(edge_nets.hop_distances(base, li[0], li[1], gp))
    return tuple(out + hops)


def _nx_graph(edges, n, directed=False):
    import networkx as nx
    G = nx.DiGraph() if directed else nx.Graph()
    G.add_nodes_from(range(n))
    G.add_edges_from(edges)
    return G


def oracle_edge_nets(outs):
    import _edge_ref as ER
    for (name, directed), got in zip(EDGE_NET_CASES, outs[-len(EDGE_NET_CASES):]):
        links, sizes = LG.CASES[name]
        gp = LG.graph_ptr(sizes)
        G = _nx_graph(links, int(gp[-1]), directed)
        li = _label_pairs(gp, int(gp[-1]))
        want = [ER.hops(G, int(s), int(t)) for s, t in zip(li[0], li[1])]
        assert got.cpu().tolist() == want, f"hop_distances {name} directed={directed}"


def run_link(dev):
    from graphgym_amd import link_pred
    out = []
    # negatives per graph: within every graph's non-edges (graph 0 of the batch is one link on two nodes: none)
    for (links, sizes), counts in ((LG.UNIFORMITY, [6]), (LG.CASES["batch_2_5_9"], [0, 3, 5])):
        for directed in (False, True):
            base, gp, _ = LG.build_links(links, sizes, directed, dev)
            x = rnd(base.num_nodes, 4, seed=3).to(dev)
            split = link_pred.link_split(base, gp, split=(0.8, 0.2), generator=gen(0))
            plan = link_pred.plan_negatives(base, gp, counts, split["train"].directed)
            for name in ("train", "val"):
                s = split[name]
                b = link_pred.link_batch(s, x, seed=5, offset=2, plan=plan)
                out += [s.pos_index, s.edge_index, s.graph.rowptr, s.graph.col, b.edge_label_index, b.edge_label]
            be = link_pred.link_batch(split["train"], x, seed=5, offset=3, transform="edge", plan=plan)
            out += [be.edge_index, be.node_label_index, be.node_label, be.node_feature]
    return tuple(out)


def run_samplers(dev):
    from graphgym_amd import samplers
    out = []
    for name in ("ring65", "star200", "cycle6_chord", "multigraph", "triangle_pendant_isolated"):
        base = SG.build(name, dev)
        for kind in samplers.KINDS:
            plan = samplers.plan_sampler(base, kind, batch_size=9, walk_length=2, num_parts=3)
            for step in (0, 4):
                out.append(samplers.sample_nodes(plan, 7, step))
                b = samplers.sample_batch(plan, 7, step)
                out += [b.graph.rowptr, b.graph.col, b.edge_index, b.orig_node, b.base_entry]
    return tuple(out)


def run_structure(dev):
    from graphgym_amd import structure
    out = []
    for name in ("triangle_pendant_isolated", "ring65", "star200", "path5"):
        base = SG.build(name, dev)
        out += list(structure.triangles(base)) + list(structure.hop_sums(base))
    base, gp, _ = LG.build("batch_2_5_9", False, dev)
    out += list(structure.triangles(base)) + list(structure.hop_sums(base, gp))
    out += list(structure.hop_sums(base, gp, nodes=torch.tensor([15, 3, 3, 0])))
    return tuple(out)


def oracle_structure(outs):
    """triangles and path lengths against networkx (tests/_structure_ref.py), exact: integers, and one float64 division"""
    import _structure_ref as SR
    graphs = [_nx_graph(*SG.CASES[name]) for name in ("triangle_pendant_isolated", "ring65", "star200", "path5")]
    graphs.append(_nx_graph(LG.CASES["batch_2_5_9"][0], 16))
    for k, G in enumerate(graphs):
        tri2, deg, dist_sum, reached = (t.cpu() for t in outs[4 * k:4 * k + 4])
        assert torch.equal(tri2, 2 * torch.from_numpy(SR.triangles([G]))), f"triangles, graph {k}"
        assert deg.tolist() == [len(set(G[v]) - {v}) for v in G.nodes], f"neighbours, graph {k}"
        mean_len = dist_sum.double() / reached.double()
        assert torch.equal(mean_len, torch.from_numpy(SR.node_path_len([G]))), f"paths, graph {k}"
    dist_sum, reached = outs[-2].cpu(), outs[-1].cpu()
    want = torch.from_numpy(SR.node_path_len([graphs[-1]]))[[15, 3, 3, 0]]
    assert torch.equal(dist_sum.double() / reached.double(), want)


def _small_graphs():
    """twelve small undirected graphs with features, labels and edge features"""
    graphs = []
    for k in range(12):
        n = 3 + k % 6
        links = [(i, (i + 1) % n) for i in range(n)] + ([(0, n // 2)] if n > 4 else [])
        links = sorted({(min(a, b), max(a, b)) for a, b in links if a != b})
        ei = torch.tensor(links + [(b, a) for a, b in links], dtype=torch.int64).t().contiguous()
        graphs.append((ei, rnd(n, 6, seed=k), torch.tensor(k % 3), rnd(ei.size(1), 2, seed=100 + k)))
    return graphs


def run_collate(dev):
    from graphgym_amd import _lib, graph_loader
    ds = graph_loader.GraphDataset.from_graphs(_small_graphs(), device=dev)
    cap = int(_lib.lib().mp_collate_stage_cap())
    out = []
    for B in (5, cap, 2 * cap + 77):            # below, at and above what a workgroup stages, not a multiple of it
        ids = torch.randint(0, 12, (B,), generator=gen(B)).numpy()
        b = graph_loader.collate(ds, ids)
        out += [b.node_feature, b.edge_index, b.batch, b.graph_label, b.orig_node, b.base_entry, b.edge_feature,
                b.graph.rowptr, b.graph.col, b.graph.row_ids(), b.pool_operator.rowptr, b.pool_operator._t.col]
    e = graph_loader.ego_collate(ds, [3, 11, 3, 0, 7], 2)
    out += [e.node_feature, e.edge_index, e.node_id_index, e.batch, e.graph_label, e.orig_node, e.ego_of_node,
            e.pool_operator.rowptr] + _csr_outs(getattr(e, "graph", None))
    return tuple(out)


def run_identity(dev):
    """node_identity features: k aggregations at the width of the largest graph, on the normalised operator with
    remaining self loops (COO_KEEP_LOOP_WEIGHT)"""
    from graphgym_amd import identity
    graphs = _small_graphs()
    sizes = [g[1].size(0) for g in graphs]
    off = [sum(sizes[:k]) for k in range(len(sizes))]
    ei = torch.cat([g[0] + o for g, o in zip(graphs, off)], 1)
    ei = torch.cat([ei, torch.tensor([[0, 5], [0, 5]])], 1)                      # two explicit self loops
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    n = sum(sizes)
    return (identity.compute_identity(ei.to(dev), n, 3, batch=batch.to(dev), block=4),
            identity.compute_identity(ei.to(dev), n, 2))


def run_layer(dev):
    """one ID-GCN layer as the models call it, forward and backward, at unequal and at equal widths"""
    from graphgym_amd import layers
    torch.manual_seed(0)                            # (the layer draws its weights on the host)
    src, dst, _ = hub_edges()
    ei = torch.stack([src, dst]).to(dev)
    ids = torch.arange(0, N_NODES, 9).to(dev)
    out = []
    for d_in, units in ((100, 64), (64, 64)):
        layer = layers.IDGCN(units, activation="relu", in_features=d_in).to(dev)
        x = leaf(rnd(N_NODES, d_in, seed=d_in), dev)
        y = layer([x, ei, ids])
        y.backward(rnd(N_NODES, units, seed=units).to(dev))
        out += [y.detach(), x.grad] + [p.grad for p in layer.parameters()]
    return tuple(out)


# ------------------------------------------------------------------------------------------------------- table
def bind(fn, *a, **k):
    return lambda dev: fn(dev, *a, **k)


BUILD = ("mp_check_edge_index", "mp_csr_from_coo", "mp_spmm_plan_build")
CASES = [
    Case("graph_build", BUILD + ("mp_csr_row_ids", "mp_csr_transpose", "mp_csr_is_symmetric", "mp_csr_degree",
                                 "mp_gcn_norm_edges", "mp_csr_scale_f32", "mp_mark_id_sources"), run_graph_build,
         oracle=oracle_graph_build),
    Case("degree_col_atomics", ("mp_csr_degree",), run_degree_col, oracle=oracle_degree_col),
]
for _d in (3, 64, 100, 256, 260):
    CASES.append(Case(f"spmm_plan-d{_d}", BUILD + ("mp_spmm_csr_f32", "mp_spmm_max_bwd_f32", "mp_csr_transpose"),
                      bind(run_spmm, _d), oracle=oracle_spmm(_d)))
for _d in (64, 100):
    CASES += [
        Case(f"spmm_eval-d{_d}", ("mp_spmm_csr_epilogue_f32",), bind(run_spmm_eval, _d)),
        Case(f"idgnn_plan-d{_d}", ("mp_idgnn_agg_f32", "mp_mark_id_sources", "mp_spmm_csr_f32"), bind(run_idgnn, _d),
             oracle=oracle_idgnn(_d)),
        Case(f"bf16-d{_d}", ("mp_spmm_csr_bf16", "mp_spmm_max_bwd_bf16", "mp_idgnn_agg_bf16"), bind(run_bf16, _d)),
    ]
for _d in (128, 256):
    CASES += [
        Case(f"tiles-d{_d}", ("mp_agg_rows_tiles_f32",), bind(run_tiles, _d), setup=setup_tiles, oracle=oracle_tiles(_d)),
        Case(f"tiles_hot-d{_d}", ("mp_agg_rows_tiles_hot_f32",), bind(run_tiles, _d, hot=True), setup=setup_hot,
             oracle=oracle_tiles(_d)),
        Case(f"idgnn_tiles-d{_d}", ("mp_idgnn_agg_tiles_f32", "mp_id_rows_f32"), bind(run_idgnn_tiles, _d),
             setup=setup_tiles,
             oracle=oracle_idgnn(_d), unspecified=unspecified_id_rows(_d)),
    ]
for _F in (64, 256):
    CASES.append(Case(f"one_kernel_layer-F{_F}", ("mp_agg_dense_f32", "mp_id_fixup_f32", "mp_split_w_bf16x3",
                                                   "mp_dense_wgrad_relu_f32"), bind(run_fused, _F), oracle=oracle_fused(_F)))
CASES += [
    Case("sage_concat", ("mp_agg_dense_f32", "mp_agg_dense_add_f32", "mp_dense_fused_f32", "mp_dense_wgrad_relu_f32"),
         run_sage),
    Case("dense", ("mp_dense_fused_f32", "mp_dense_wgrad_f32", "mp_dense_wgrad_relu_f32"), bind(run_dense, False)),
    Case("dense_x3", ("mp_dense_x3_f32", "mp_split_w_bf16x3", "mp_dense_wgrad_relu_f32"), bind(run_dense, True),
         setup=setup_x3),
]
for _N, _d in BN_SHAPES:
    _s = f"-{_N}x{_d}"
    CASES += [
        Case("bn" + _s, ("mp_bn_train_fwd_f32", "mp_bn_train_bwd_f32", "mp_bn_train_bwd_relu_f32"), bind(run_bn, _N, _d)),
        Case("bn_act" + _s, ("mp_bn_train_fwd_act_f32", "mp_bn_train_bwd_act_f32"), bind(run_bn_act, _N, _d)),
        Case("bn_skip" + _s, ("mp_bn_train_fwd_skip_f32", "mp_bn_train_bwd_skip_f32", "mp_bn_train_fwd_skip_act_f32",
                              "mp_bn_train_bwd_skip_act_f32"), bind(run_bn_skip, _N, _d)),
        Case("bn_drop" + _s, ("mp_dropout_keyed_f32", "mp_bn_train_fwd_drop_act_f32", "mp_bn_train_bwd_drop_act_f32",
                              "mp_bn_train_fwd_drop_skip_act_f32", "mp_bn_train_bwd_drop_skip_act_f32"),
             bind(run_bn_drop, _N, _d)),
    ]
CASES += [
    Case("softmax_ce", ("mp_softmax_ce_rows_f32", "mp_softmax_ce_bwd_f32"), run_softmax_ce),
    Case("rows", ("mp_rows_gather_f32", "mp_rows_scatter_add_f32"), run_rows, oracle=oracle_rows),
    Case("codes_kernel", ("mp_embed_sum_f32", "mp_code_reduce_f32", "mp_spmm_csr_edge_f32", "mp_spmm_max_bwd_f32"),
         bind(run_codes, "kernel"), setup=setup_code_kernel, oracle=oracle_codes),
    Case("codes_operator", ("mp_embed_sum_f32", "mp_code_reduce_f32", "mp_spmm_csr_f32"), bind(run_codes, "operator"),
         oracle=oracle_codes),
    Case("softmax_tiers", ("mp_csr_row_softmax_f32", "mp_csr_row_softmax_bwd_f32", "mp_gat_alpha_f32",
                           "mp_edge_att_alpha_f32"), run_softmax_tiers, oracle=oracle_softmax_tiers),
    Case("sddmm", ("mp_sddmm_dot_stream_f32", "mp_sddmm_dot_f32", "mp_sddmm_add_f32", "mp_spmm_csr_heads_reduce_f32"),
         run_sddmm, oracle=oracle_sddmm),
    Case("edge_values", ("mp_spmm_csr_heads_reduce_f32", "mp_spmm_heads_max_bwd_f32", "mp_spmm_heads_max_da_f32",
                         "mp_sddmm_dot_stream_f32"), run_edge_values, oracle=oracle_edge_values),
    Case("spmm_edge", ("mp_spmm_csr_edge_f32", "mp_spmm_edge_bwd_f32", "mp_spmm_max_bwd_f32"), run_spmm_edge,
         oracle=oracle_spmm_edge),
    Case("spmm_edge_heads", ("mp_spmm_csr_edge_heads_f32", "mp_spmm_edge_heads_bwd_f32", "mp_spmm_heads_max_bwd_f32",
                             "mp_spmm_heads_max_da_f32", "mp_spmm_csr_edge_f32"), run_spmm_edge_heads,
         oracle=oracle_spmm_edge_heads),
    Case("ego", ("mp_ego_expand", "mp_csr_is_symmetric", "mp_csr_transpose"), run_ego),
    Case("edge_nets", ("mp_edge_expand", "mp_hop_distances"), run_edge_nets, oracle=oracle_edge_nets),
    Case("link_split", ("mp_pair_space_rows", "mp_sample_non_edges", "mp_edge_expand"), run_link),
    Case("samplers", ("mp_sample_parts", "mp_sample_entry_rows", "mp_sample_walks", "mp_bitmap_mark",
                      "mp_bitmap_word_counts", "mp_bitmap_nodes", "mp_induced_count", "mp_induced_fill"), run_samplers),
    Case("structure", ("mp_csr_triangles", "mp_hop_sums"), run_structure, oracle=oracle_structure),
    Case("identity_features", BUILD + ("mp_csr_transpose", "mp_csr_degree", "mp_csr_scale_f32", "mp_spmm_csr_f32"),
         run_identity),
    # 100 -> 64 transforms first (rows gathered and added for the identity nodes, then the plan aggregation with bias and
    # ReLU); 64 -> 64 is the one-kernel layer with the identity fix-up
    Case("idgcn_layer", ("mp_csr_from_coo", "mp_gcn_norm_edges", "mp_rows_gather_f32", "mp_rows_scatter_add_f32",
                         "mp_spmm_csr_f32", "mp_agg_dense_f32", "mp_id_fixup_f32", "mp_dense_wgrad_relu_f32"), run_layer),
    Case("collate", ("mp_collate_graphs", "mp_collate_check_entries", "mp_rows_gather_f32", "mp_ego_expand"), run_collate),
]

BYTES_SEEN = collections.Counter()      # case -> bytes that went through the shim (all three fills)


@pytest.fixture(autouse=True)
def small_graphs_reach_every_form(monkeypatch):
    import graphgym_amd as ga
    monkeypatch.setattr(ga.CSRGraph, "PLAN_CONFIG", PLAN_CONFIG)
    monkeypatch.setenv("MP_AGG_TILES", "0")       # the tile cases switch it on themselves
    monkeypatch.setenv("MP_X3", "1")
    monkeypatch.setenv("MP_FUSED", "1")
    monkeypatch.delenv("MP_CODE_REDUCE", raising=False)


def differential(run, dev, monkeypatch, entries=(), oracle=None, unspecified=None, what=""):
    """run `run(dev)` under the three fills, in order, with the checks of the module docstring; returns the bytes seen"""
    from graphgym_amd import _lib
    real = _lib.lib()
    real = real._real if isinstance(real, Recorder) else real
    masks = None if unspecified is None else unspecified[1](dev)
    base, seen_bytes = None, 0
    for word in FILLS:
        rec = Recorder(real)
        monkeypatch.setattr(_lib, "_lib", rec)
        try:
            with poisoned(word) as p:
                outs = run(dev)
                torch.cuda.synchronize()
        finally:
            monkeypatch.setattr(_lib, "_lib", real)
        tag = f"{what} fill {word:#010x}"
        p.check_guards()
        seen_bytes += p.bytes_seen
        assert p.allocations > 0, f"{tag}: nothing went through the shim"
        missing = sorted(set(entries) - rec.names())
        assert not missing, f"{tag}: the run never fetched {missing}"
        outs = tuple(o.detach() for o in outs)
        if base is None:
            base = outs
            for i, o in enumerate(outs):
                if o.is_floating_point():
                    ok = torch.isfinite(o)
                    if masks is not None and masks[i] is not None:
                        ok = ok | masks[i].to(o.device)
                    assert bool(ok.all()), f"{tag}: output {i} holds {int((~ok).sum())} non-finite values"
            if oracle is not None:
                oracle(outs)
            continue
        assert len(outs) == len(base), tag
        for i, (o, b) in enumerate(zip(outs, base)):
            assert o.shape == b.shape and o.dtype == b.dtype, f"{tag}: output {i} is {tuple(o.shape)} {o.dtype}"
            if masks is not None and masks[i] is not None:
                keep = ~masks[i].to(o.device)
                o, b = o[keep], b[keep]
            # (1-byte outputs — uint8 flags, bool masks — are filled by the 32-bit word: under the integer-1 fill only
            # every fourth byte is non-zero, and no single byte value marks the sentinel; held by bit equality alone)
            if o.element_size() > 1:
                hits = fill_hits(o, b, word)
                assert hits == 0, f"{tag}: output {i} holds the fill pattern in {hits} elements the baseline wrote"
            if not same_bits(o, b):
                diff = int((raw_bits(o) != raw_bits(b)).sum())
                raise AssertionError(f"{tag}: output {i} ({tuple(o.shape)} {o.dtype}) differs from the zero-filled run in "
                                     f"{diff} elements: the op read memory it had not written")
    return seen_bytes


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_no_op_depends_on_fresh_allocations(dev, monkeypatch, case):
    assert case.exact, "every case is held bit for bit (atomics get exactly summable operands)"
    if case.setup is not None:
        case.setup(monkeypatch)
    BYTES_SEEN[case.name] = differential(case.run, dev, monkeypatch, case.entries, case.oracle, case.unspecified,
                                         case.name)
    print(f"{case.name}: {BYTES_SEEN[case.name]} bytes through the shim")


def test_the_harness_can_fail(dev, monkeypatch):
    """torch only: a fake op that reads its fresh allocation is reported as depending on the fill, and one that writes one
    element past its tensor (inside the guard: in bounds of the real allocation) is reported by check_guards()"""
    x = torch.arange(64, dtype=torch.float32)

    def reads_its_allocation(dev):
        return (torch.empty(64, device=dev).add_(x.to(dev)),)

    def writes_past_the_end(dev):
        t = torch.empty(64, device=dev)
        t.copy_(x)
        torch.as_strided(t, (65,), (1,))[64] = 7.0
        return (t,)

    def fine(dev):
        return (torch.empty(64, device=dev).copy_(x), torch.empty_like(x.to(dev)).zero_(),
                x.to(dev).new_empty((3,), dtype=torch.int32).fill_(1))

    assert differential(fine, dev, monkeypatch, what="fine") == 3 * (256 + 256 + 12)
    with pytest.raises(AssertionError, match="fill pattern|differs from the zero-filled run"):
        differential(reads_its_allocation, dev, monkeypatch, what="reads")
    with pytest.raises(AssertionError, match="guard bytes overwritten"):
        differential(writes_past_the_end, dev, monkeypatch, what="writes past")
    # the three torch functions are back, whatever happened inside
    assert torch.empty.__name__ == "empty" and "new_empty" not in torch.Tensor.__dict__
    assert torch.empty(2).shape == (2,)
