"""The state that outlives a call: every cache that decides "is this still the tensor the structure was built for" by
graph.tensor_stamp, on the device.  One method throughout: warm the cache with A, ask for B (tests/_alias.py: same
address, element count and version, other contents), and compare B's answer with a COLD computation (a fresh CSRGraph
from copies of rowptr / col / val, or a fresh holder; structures bit for bit) and with a host reference that knows
nothing of the engine (numpy CSR selection, tests/_degenerate.numpy_csr, or the float64 / float32 oracle pair of
tests/_tol.py).  Every case also asserts the HIT: the same tensor again, and a fresh view of equal geometry, build
nothing (graphgym_amd.graph.BUILDS stays put).

The graph: one directed multigraph of 96 nodes and 1555 entries with repeated (r, c) entries, self loops, two rows of
more than 64 entries, empty rows, four columns far more popular than the rest, and weights that are not symmetric.
Widths 3 and 64 (128 on the tile path).  What is under test is the key, not the kernels' throughput."""
import gc
import types
import weakref

import numpy as np
import pytest
import torch

import _alias
import _ogb_ref as OR
from _degenerate import numpy_csr
from _tol import both, close, mag_of

pytestmark = pytest.mark.gpu

N = 96
EMPTY = (7, 13, 40, 41) + tuple(range(88, 96))
HOT = {10: 90, 20: 75, 30: 60, 60: 45}             # extra entries per column: the four most used columns, no ties
LONG = {3: 80, 50: 70}                             # extra entries per row: two rows of more than 64
LOOPS = (1, 2, 50, 60, 70)
WIDTHS = (3, 64)


def _make_graph():
    g = torch.Generator().manual_seed(96)
    live = torch.tensor([r for r in range(N) if r not in EMPTY])
    pick = lambda k: live[torch.randint(0, live.numel(), (k,), generator=g)]      # noqa: E731
    dst0, src0 = pick(1100), torch.randint(0, N, (1100,), generator=g)
    long_dst = torch.cat([torch.full((k,), r) for r, k in LONG.items()])
    long_src = torch.randint(0, N, (long_dst.numel(),), generator=g)
    hot_src = torch.cat([torch.full((k,), c) for c, k in HOT.items()])
    hot_dst = pick(hot_src.numel())
    loops = torch.tensor(LOOPS)
    dst = torch.cat([dst0, long_dst, hot_dst, loops, dst0[:30]])                  # the last 30: repeated entries
    src = torch.cat([src0, long_src, hot_src, loops, src0[:30]])
    perm = torch.randperm(dst.numel(), generator=g)
    dst, src = dst[perm].contiguous(), src[perm].contiguous()
    w = torch.rand(dst.numel(), generator=g) + 0.1
    return dst, src, w


DST, SRC, W = _make_graph()
NP_CSR = numpy_csr(DST, SRC, W, N)                   # (rowptr, col, val, eid) in the engine's order, by numpy
NP_ROWS = np.repeat(np.arange(N), np.diff(NP_CSR[0]))
_DEVICE = {}


def _parts(dev):
    """(rowptr, col, val) of the graph on the device, built once by the engine and checked against numpy"""
    if "parts" not in _DEVICE:
        import graphgym_amd as ga
        G = ga.CSRGraph.from_edge_index(torch.stack([DST, SRC]).to(dev), N, W.to(dev), dst_row=0)
        rp, col, val, eid = NP_CSR
        assert np.array_equal(G.rowptr.cpu().numpy(), rp) and np.array_equal(G.col.cpu().numpy(), col)
        assert np.array_equal(G.val.cpu().numpy(), val) and np.array_equal(G.eid.cpu().numpy(), eid)
        _DEVICE["parts"] = (G.rowptr, G.col, G.val)
    return _DEVICE["parts"]


def fresh(dev, val="own"):
    """a CSRGraph of the pattern that nothing has touched (CSRGraph.from_csr from copies)"""
    import graphgym_amd as ga
    rp, col, v = _parts(dev)
    v = v if isinstance(val, str) else val
    return ga.CSRGraph.from_csr(rp.clone(), col.clone(), None if v is None else v.clone(), N)


def again(t):
    """a new Python tensor object of the same geometry over the same memory (`ids[:k]` taken afresh)"""
    v = t[...]
    assert v is not t and v.data_ptr() == t.data_ptr() and v.stride() == t.stride() and v.shape == t.shape
    return v


def builds():
    from graphgym_amd import graph
    return dict(graph.BUILDS)


def x_of(d, seed=0):
    return torch.randn(N, d, generator=torch.Generator().manual_seed(100 + d + seed))


def dense(c, variant=0):
    """the operator (0), its transpose (1), the transposed mean operator (2) as a dense matrix in c's precision"""
    w = c(W)
    A = torch.zeros(N, N, dtype=w.dtype).index_put_((DST, SRC), w, accumulate=True)
    if variant == 2:
        cnt = torch.bincount(DST, minlength=N).clamp(min=1).to(w.dtype)
        A = A / cnt[:, None]
    return A if variant == 0 else A.t()


# ------------------------------------------------------------------------------------------------ comparisons
def same_graph(a, b, what=""):
    assert (a.num_nodes, a.num_cols, a.nnz) == (b.num_nodes, b.num_cols, b.nnz), what
    assert torch.equal(a.rowptr, b.rowptr) and torch.equal(a.col, b.col), what
    assert (a.val is None) == (b.val is None) and (a.val is None or torch.equal(a.val, b.val)), what


def same_branch(a, b, what=""):
    for f in ("rows", "crp", "slot", "val", "defer"):
        fa, fb = getattr(a, f), getattr(b, f)
        assert (fa is None) == (fb is None) and (fa is None or torch.equal(fa, fb)), (what, f)
    assert a.n_rows == b.n_rows, what
    same_graph(a.t, b.t, what + " t")


def np_select(rows, parts=None):
    rp, col, val = NP_CSR[:3] if parts is None else parts
    rows = np.asarray(rows, dtype=np.int64)
    deg = rp[rows + 1] - rp[rows]
    idx = np.concatenate([np.arange(rp[r], rp[r + 1]) for r in rows] + [np.zeros(0, np.int64)]).astype(np.int64)
    return np.concatenate([[0], np.cumsum(deg)]), col[idx], val[idx]


def graph_is(g, rowptr, col, val, what=""):
    assert np.array_equal(g.rowptr.cpu().numpy(), rowptr), what
    assert np.array_equal(g.col.cpu().numpy(), col), what
    assert np.array_equal(g.val.cpu().numpy(), val), what


def np_transpose(val=None):
    """A^T in the engine's order: rows ascending, columns ascending, equal pairs in stored order"""
    rp, col, v = NP_CSR[:3]
    v = v if val is None else val
    order = np.argsort(col, kind="stable")
    trp = np.concatenate([[0], np.cumsum(np.bincount(col, minlength=N))])
    return trp, NP_ROWS[order], v[order]


def np_marks(ids):
    col = NP_CSR[1].astype(np.int64)
    return np.where(np.isin(col, np.asarray(ids)), col - 2 ** 31, col).astype(np.int32)


def np_id_branch(ids):
    ids = np.asarray(ids, dtype=np.int64)
    rp, col, val = NP_CSR[:3]
    slot_of = np.full(N, -1, dtype=np.int64)
    slot_of[ids] = np.arange(ids.size)
    s = slot_of[col]
    e = np.nonzero(s >= 0)[0]
    rows_e, slot, v = NP_ROWS[e], s[e], val[e]
    rows, counts = np.unique(rows_e, return_counts=True)
    defer = np.zeros(N, np.uint8)
    defer[rows] = 1
    order = np.argsort(slot, kind="stable")
    trp = np.concatenate([[0], np.cumsum(np.bincount(slot, minlength=ids.size))])
    return dict(rows=rows, crp=np.concatenate([[0], np.cumsum(counts)]), slot=slot, val=v, defer=defer,
                t=(trp, rows_e[order], v[order]))


def branch_is(br, ids, what=""):
    want = np_id_branch(ids)
    for f in ("rows", "crp", "slot", "val", "defer"):
        assert np.array_equal(getattr(br, f).cpu().numpy(), want[f]), (what, f)
    graph_is(br.t, *want["t"], what=what + " t")
    assert br.t.num_nodes == len(ids) and br.t.num_cols == N


ROW_PAIRS = [("stride", 40, True, torch.int64), ("stride", 2, True, torch.int64), ("stride", 40, True, torch.int32),
             ("dtype", 40, False, torch.int64), ("dtype", 3, True, torch.int64)]
ID_PAIRS = [("stride", 40, torch.int64), ("stride", 2, torch.int64), ("stride", 40, torch.int32),
            ("dtype", 3, torch.int64), ("dtype", 2, torch.int64)]
_row_ids = [f"{s}-{n}-{str(t)[6:]}" for s, n, _, t in ROW_PAIRS]
_id_ids = [f"{s}-{n}-{str(t)[6:]}" for s, n, t in ID_PAIRS]


def id_pair(dev, sc, n, dtype):
    return _alias.index_pair(sc, dev, n, N, unique=True, dtype=dtype, seed=n)


def test_the_graph_is_what_the_cases_need(dev):
    rp, col, val, _ = NP_CSR
    deg = np.diff(rp)
    pairs = set()
    repeated = sum(1 for p in zip(NP_ROWS.tolist(), col.tolist()) if p in pairs or pairs.add(p))
    assert N == 96 and 1400 <= col.size <= 1600 and repeated >= 30
    assert int((NP_ROWS == col).sum()) >= len(LOOPS) and int((deg > 64).sum()) == 2
    assert all(deg[r] == 0 for r in EMPTY)
    counts = np.bincount(col, minlength=N)
    top = np.sort(counts)[::-1]
    assert sorted(np.argsort(counts)[-4:].tolist()) == sorted(HOT) and top[3] > top[4]         # the hot set has no tie
    A = dense(lambda t: t.double())
    assert not torch.equal(A, A.t())
    _parts(dev)


# =========================================================================================== alias pairs, site by site
@pytest.mark.parametrize("sc,n,unique,dtype", ROW_PAIRS, ids=_row_ids)
def test_select_rows_alias(dev, sc, n, unique, dtype):
    A, B = _alias.index_pair(sc, dev, n, N, unique=unique, dtype=dtype, seed=n)
    g = fresh(dev)
    graph_is(g.select_rows(A), *np_select(A.cpu().numpy()), what="A")
    sub = g.select_rows(B)
    same_graph(sub, fresh(dev).select_rows(B), "select_rows(B) after A against a cold graph")
    graph_is(sub, *np_select(B.cpu().numpy()), what="select_rows(B) after A against numpy")
    assert (sub.num_nodes, sub.num_cols) == (n, N)
    before = builds()
    assert g.select_rows(B) is sub and g.select_rows(again(B)) is sub and g.select_rows(again(A)) is not sub
    assert builds() == before


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("variant", [0, 1, 2])
@pytest.mark.parametrize("sc,n,unique,dtype", ROW_PAIRS[:1] + ROW_PAIRS[3:4], ids=_row_ids[:1] + _row_ids[3:4])
def test_spmm_rows_raw_alias(dev, sc, n, unique, dtype, variant, d):
    A, B = _alias.index_pair(sc, dev, n, N, unique=unique, dtype=dtype, seed=n)
    g, x = fresh(dev), x_of(d)
    xd = x.to(dev)
    torch.ops.mp.spmm_rows_raw(xd, g.handle, variant, A)
    y = torch.ops.mp.spmm_rows_raw(xd, g.handle, variant, B)
    cold = fresh(dev)
    assert torch.equal(y, torch.ops.mp.spmm_rows_raw(xd, cold.handle, variant, B))
    rows = B.cpu().long()
    close(y, both(lambda c: dense(c, variant)[rows] @ c(x)), what=f"spmm_rows_raw variant {variant} rows B after A")
    before = builds()
    assert torch.equal(torch.ops.mp.spmm_rows_raw(xd, g.handle, variant, B), y)
    assert torch.equal(torch.ops.mp.spmm_rows_raw(xd, g.handle, variant, again(B)), y)
    assert builds() == before


def _two_branch_refs(x, ids, dP, dQ):
    sel = torch.zeros(N, 1)
    sel[ids] = 1

    def ref(c):
        xr = c(x).clone().requires_grad_(True)
        A = dense(c)
        Pr, Qr = A @ xr, A @ (xr * c(sel))
        (Pr * c(dP) + Qr * c(dQ)).sum().backward()
        return Pr.detach(), Qr.detach(), xr.grad
    has = torch.zeros(N).index_add_(0, DST, sel[SRC].view(-1)) > 0
    return both(ref), has


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("sc,n,dtype", ID_PAIRS, ids=_id_ids)
def test_mark_ids_alias_through_idgnn_aggregate(dev, sc, n, dtype, d):
    """the plan path of ops.idgnn_aggregate (96 rows: far below the tile threshold) reads g.mark_ids(id_index); its
    backward selects the identity rows of the transposed operator (select_rows)"""
    from graphgym_amd import ops
    A, B = id_pair(dev, sc, n, dtype)
    g, x = fresh(dev), x_of(d)
    gen = torch.Generator().manual_seed(d)
    dP, dQ = torch.randn(N, d, generator=gen), torch.randn(N, d, generator=gen)

    def run(graph, ids):
        xg = x.to(dev).requires_grad_(True)
        P, Q = ops.idgnn_aggregate(graph, ids, xg)
        (P * dP.to(dev) + Q * dQ.to(dev)).sum().backward()
        return P.detach(), Q.detach(), xg.grad
    run(g, A)
    P, Q, dx = run(g, B)
    cold = fresh(dev)
    P0, Q0, dx0 = run(cold, B)
    assert torch.equal(P, P0) and torch.equal(Q, Q0) and torch.equal(dx, dx0)
    assert torch.equal(g.mark_ids(B), cold.mark_ids(B))
    assert np.array_equal(g.mark_ids(B).cpu().numpy(), np_marks(B.cpu().numpy()))
    (r64, r32), has = _two_branch_refs(x, B.cpu().long(), dP, dQ)
    close(P, (r64[0], r32[0]), what="two-branch P for B after A")
    close(Q, (r64[1], r32[1]), what="two-branch Q for B after A")
    close(dx, (r64[2], r32[2]), what="two-branch dx for B after A")
    assert bool((~has).any()) and float(Q.cpu()[~has].abs().max()) == 0.0       # zero off the neighbours of B's nodes
    before = builds()
    run(g, B)
    P2, _, _ = run(g, again(B))
    assert builds() == before and torch.equal(P2, P)


@pytest.mark.parametrize("sc,n,dtype", ID_PAIRS, ids=_id_ids)
def test_id_branch_alias_on_the_tile_path(dev, monkeypatch, sc, n, dtype):
    from graphgym_amd import ops
    A, B = id_pair(dev, sc, n, dtype)
    d = 128
    g, x = fresh(dev), x_of(d)
    xd = x.to(dev)
    monkeypatch.setenv("MP_AGG_TILES", "1")
    monkeypatch.setattr(ops, "AGG_TILES_MIN_ROWS", 1)          # (the product dispatches the tile kernels from 2^21 rows)
    calls = ops.AGG_TILES_CALLS
    ops.idgnn_aggregate(g, A, xd)
    P, Q = ops.idgnn_aggregate(g, B, xd)
    assert ops.AGG_TILES_CALLS == calls + 2                     # the tile path, which reads g.id_branch(id_index)
    cold = fresh(dev)
    P0, Q0 = ops.idgnn_aggregate(cold, B, xd)
    assert torch.equal(P, P0) and torch.equal(Q, Q0)
    same_branch(g.id_branch(B), cold.id_branch(B), "id_branch(B) after A")
    branch_is(g.id_branch(B), B.cpu().numpy(), "id_branch(B) after A")
    (r64, r32), has = _two_branch_refs(x, B.cpu().long(), torch.zeros(N, d), torch.zeros(N, d))
    close(P, (r64[0], r32[0]), what="tile two-branch P for B after A")
    close(Q, (r64[1], r32[1]), what="tile two-branch Q for B after A")
    assert float(Q.cpu()[~has].abs().max()) == 0.0
    before = builds()
    ops.idgnn_aggregate(g, B, xd)
    ops.idgnn_aggregate(g, again(B), xd)
    assert builds() == before


@pytest.mark.parametrize("sc,n,dtype", ID_PAIRS, ids=_id_ids)
def test_id_branch_alias_through_agg_dense_id(dev, sc, n, dtype):
    """ops.agg_dense's identity form: the one-kernel layer + the identity fix-up on g.id_branch(id_index), forward and
    backward (mp::id_branch_t_raw reads id_branch(id_index).t).  F = 64: the one-kernel layer has no width 3."""
    from graphgym_amd import ops
    A, B = id_pair(dev, sc, n, dtype)
    F = d = 64
    g, x = fresh(dev), x_of(F)
    gen = torch.Generator().manual_seed(5)
    Wm, Wid, b = torch.randn(F, d, generator=gen) / 8, torch.randn(F, d, generator=gen) / 8, torch.randn(d, generator=gen)
    up = torch.randn(N, d, generator=gen)

    def run(graph, ids):
        xd, Wd, Wi, bd = (t.to(dev).requires_grad_(True) for t in (x, Wm, Wid, b))
        out = ops.agg_dense_id(graph, xd, Wd, Wi, ids, bias=bd)
        assert out is not None
        out.backward(up.to(dev))
        return out.detach(), xd.grad, Wi.grad
    run(g, A)
    out, dx, dWi = run(g, B)
    o0, dx0, dWi0 = run(fresh(dev), B)
    assert torch.equal(out, o0) and torch.equal(dx, dx0) and torch.equal(dWi, dWi0)
    ids = B.cpu().long()

    def ref(c):
        xr, Wr, Wir, br = (c(t).clone().requires_grad_(True) for t in (x, Wm, Wid, b))
        h = xr @ Wr
        h = h.index_add(0, ids, xr[ids] @ Wir)
        o = dense(c) @ h + br
        o.backward(c(up))
        return o.detach(), xr.grad, Wir.grad
    r64, r32 = both(ref)
    close(out, (r64[0], r32[0]), what="agg_dense_id forward for B after A")
    close(dx, (r64[1], r32[1]), what="agg_dense_id dx for B after A")
    before = builds()
    run(g, B)
    run(g, again(B))
    assert builds() == before


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("sc,n,dtype", ID_PAIRS, ids=_id_ids)
def test_id_mlp_rows_alias(dev, sc, n, dtype, d):
    """layers._id_mlp_rows re-aggregates the identity nodes' rows over g.select_rows(id_index)"""
    from graphgym_amd import layers
    A, B = id_pair(dev, sc, n, dtype)
    g, x = fresh(dev), x_of(d)
    gen = torch.Generator().manual_seed(6)
    out0, Wm, bm = torch.randn(N, d, generator=gen), torch.randn(d, d, generator=gen) / d ** 0.5, torch.randn(d, generator=gen)
    mlp = torch.nn.Linear(d, d).to(dev)
    with torch.no_grad():
        mlp.weight.copy_(Wm.to(dev))
        mlp.bias.copy_(bm.to(dev))

    def run(graph, ids):
        with torch.no_grad():
            return layers._id_mlp_rows(out0.to(dev), graph, x.to(dev), ids, mlp, 1.5)
    run(g, A)
    y = run(g, B)
    assert torch.equal(y, run(fresh(dev), B))
    ids = B.cpu().long()

    def ref(c):
        h = dense(c)[ids] @ c(x) + 1.5 * c(x)[ids]
        return c(out0).index_add(0, ids, h @ c(Wm).t() + c(bm))
    close(y, both(ref), what="_id_mlp_rows for B after A")
    before = builds()
    run(g, B)
    run(g, again(B))
    assert builds() == before


@pytest.mark.parametrize("scenario", _alias.EDGE_SCENARIOS)
def test_get_graph_alias(dev, scenario):
    from graphgym_amd import layers
    A, B = _alias.edge_pair(scenario, dev, 200, N)
    holder = types.SimpleNamespace()
    gA = layers.get_graph(holder, A, N)
    gB = layers.get_graph(holder, B, N)
    cold = layers.get_graph(types.SimpleNamespace(), B, N)
    assert gB is not gA
    same_graph(gB, cold, "get_graph(B) after A against a fresh holder")
    assert torch.equal(gB.eid, cold.eid)
    Bc = B.cpu().long()
    rp, col, _, eid = numpy_csr(Bc[1].contiguous(), Bc[0].contiguous(), None, N)       # dst_row = 1: row = edge_index[1]
    assert np.array_equal(gB.rowptr.cpu().numpy(), rp) and np.array_equal(gB.col.cpu().numpy(), col)
    assert np.array_equal(gB.eid.cpu().numpy(), eid)
    before = builds()
    assert layers.get_graph(holder, B, N) is gB and layers.get_graph(holder, again(B), N) is gB
    assert builds() == before


def _tables(K, dim, d, seed=0):
    gen = torch.Generator().manual_seed(300 + seed)
    return [torch.rand(dim, d, generator=gen) * 2 - 1 for _ in range(K)]


def _embed_grad(dev, codes, tables, dy, dims):
    """dTables of ops.embed_sum on the device, list of K"""
    from graphgym_amd import ops
    leaves = [t.to(dev).requires_grad_(True) for t in tables]
    off = [sum(dims[:k]) for k in range(len(dims))]
    y = ops.embed_sum(codes, torch.cat(leaves), off)
    (y * dy.to(dev)).sum().backward()
    return y.detach(), [t.grad for t in leaves]


def _embed_refs(codes_cpu, tables, dy):
    def ref(c, sign=lambda t: t):
        leaves = [sign(c(t)).detach().clone().requires_grad_(True) for t in tables]
        (OR.encode(codes_cpu, leaves) * sign(c(dy))).sum().backward()
        return [t.grad for t in leaves]
    return both(ref), mag_of(lambda c: ref(c, torch.abs))


def _check_embed(got, codes_cpu, tables, dy, what):
    (r64, r32), m64 = _embed_refs(codes_cpu, tables, dy)
    for k, (a, g64, g32, mg) in enumerate(zip(got, r64, r32, m64)):
        close(a, (g64, g32), what=f"{what} dT{k}", mag=mg)


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("scenario", _alias.CODE_SCENARIOS)
def test_cached_codes_and_embed_sum_alias(dev, monkeypatch, scenario, d):
    """encoders.cached_codes on a holder, then mp::embed_sum's table gradient on the transposed one-hot operator
    (ops._ONEHOT_T, keyed on the checked codes)"""
    from graphgym_amd import encoders, ops
    monkeypatch.delenv("MP_CODE_REDUCE", raising=False)
    R = K = 6
    dims = [7] * K
    assert ops.code_reduce_path(sum(dims)) == "operator"
    A, B = _alias.code_pair(scenario, dev, R, K, 7)
    tables, dy = _tables(K, 7, d), torch.rand(R, d, generator=torch.Generator().manual_seed(d)) * 2 - 1
    holder = types.SimpleNamespace()
    ops._ONEHOT_T.clear()
    cA = encoders.cached_codes(holder, "node_feature", A, dims)
    _embed_grad(dev, cA, tables, dy, dims)
    cB = encoders.cached_codes(holder, "node_feature", B, dims)
    assert cB.dtype == torch.int32 and torch.equal(cB.cpu().long(), B.cpu().long()), "the codes of A were handed out for B"
    assert torch.equal(cB, encoders.cached_codes(types.SimpleNamespace(), "node_feature", B, dims))
    y, got = _embed_grad(dev, cB, tables, dy, dims)
    assert len(ops._ONEHOT_T) == 2
    _check_embed(got, B.cpu().long(), tables, dy, "embed_sum for B after A")
    assert torch.equal(y.cpu(), OR.encode(B.cpu().long(), tables))             # the forward has the bits of the fp32 loop
    ops._ONEHOT_T.clear()
    _, cold = _embed_grad(dev, cB, tables, dy, dims)
    assert all(torch.equal(a, b) for a, b in zip(got, cold))
    before, checked = builds(), []
    real = ops.check_codes
    monkeypatch.setattr(ops, "check_codes", lambda *a, **k: checked.append(1) or real(*a, **k))
    assert encoders.cached_codes(holder, "node_feature", B, dims) is cB
    assert encoders.cached_codes(holder, "node_feature", again(B), dims) is cB and not checked
    _embed_grad(dev, cB, tables, dy, dims)
    assert builds() == before and len(ops._ONEHOT_T) == 1
    # straight into ops.embed_sum, which checks (and copies) what is not a checked int32 tensor
    _embed_grad(dev, A, tables, dy, dims)
    _, direct = _embed_grad(dev, B, tables, dy, dims)
    assert all(torch.equal(a, b) for a, b in zip(got, direct))


def _code_graph(dev):
    import graphgym_amd as ga
    return ga.CSRGraph.from_edge_index(torch.stack([SRC, DST]).to(dev), N, W.to(dev))       # dst_row = 1, with eid


def _spmm_code_run(dev, g, q, x, table, dy, reduce):
    from graphgym_amd import ops
    xd, td = x.to(dev).requires_grad_(True), table.to(dev).requires_grad_(True)
    y = ops.spmm_code(g, xd, td, q, reduce)
    (y * dy.to(dev)).sum().backward()
    return y.detach(), td.grad


def _spmm_code_check(y, dT, q_cpu, x, table, dy, reduce, what):
    rows, cols, val = torch.from_numpy(NP_ROWS), torch.from_numpy(NP_CSR[1]).long(), torch.from_numpy(NP_CSR[2])
    qe = q_cpu.long()[torch.from_numpy(NP_CSR[3]).long()]

    def fwd(c, sign=lambda t: t):
        return OR.spmm_code(rows, cols, qe, sign(c(val)), sign(c(x)), sign(c(table)), None, N, reduce)

    def grad(c, sign=lambda t: t):
        tr = sign(c(table)).detach().clone().requires_grad_(True)
        out = OR.spmm_code(rows, cols, qe, sign(c(val)), sign(c(x)), tr, None, N, reduce)
        (out * sign(c(dy))).sum().backward()
        return tr.grad
    close(y, both(fwd), what=what + " y", mag=mag_of(lambda c: fwd(c, torch.abs)))
    close(dT, both(grad), what=what + " dtable", mag=mag_of(lambda c: grad(c, torch.abs)))


@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_spmm_code_alias(dev, monkeypatch, reduce, d):
    """spmm_code's table gradient on the one-hot operator of the entries (g._code_onehot_t): per-edge int32 codes, a
    prefix against every second element of one buffer; int64 codes are refused"""
    from graphgym_amd import ops
    monkeypatch.delenv("MP_CODE_REDUCE", raising=False)
    E, n_codes = DST.numel(), 12
    A2, B2 = _alias.code_pair("stride", dev, 1, E, n_codes, dtype=torch.int32)
    A, B = A2[0], B2[0]
    assert A.data_ptr() == B.data_ptr() and A.stride() == (1,) and B.stride() == (2,) and not torch.equal(A, B)
    g = _code_graph(dev)
    x, dy = x_of(d), x_of(d, seed=1)
    table = torch.rand(n_codes, d, generator=torch.Generator().manual_seed(d)) * 2 - 1
    _spmm_code_run(dev, g, A, x, table, dy, reduce)
    y, dT = _spmm_code_run(dev, g, B, x, table, dy, reduce)
    y0, dT0 = _spmm_code_run(dev, _code_graph(dev), B, x, table, dy, reduce)
    assert torch.equal(y, y0) and torch.equal(dT, dT0)
    _spmm_code_check(y, dT, B.cpu(), x, table, dy, reduce, f"spmm_code {reduce} for B after A")
    before = builds()
    _spmm_code_run(dev, g, B, x, table, dy, reduce)
    y2, dT2 = _spmm_code_run(dev, g, again(B), x, table, dy, reduce)
    assert builds() == before and torch.equal(dT2, dT)
    with pytest.raises(ValueError, match="int32"):
        ops.spmm_code(g, x.to(dev), table.to(dev), B.long(), reduce)


# ======================================================================================================== the ego shortcut
def _ego(dev):
    import graphgym_amd as ga
    from graphgym_amd.ego import ego_batch
    n0 = 40
    a = torch.arange(n0)
    und = torch.cat([torch.stack([a, (a + 1) % n0]), torch.stack([a[::3], (a[::3] + 7) % n0])], 1)
    ei = torch.cat([und, und.flip(0)], 1)
    base = ga.CSRGraph.from_edge_index(ei.to(dev), n0)
    centres = torch.tensor([0, 9, 17, 23, 31], device=dev)
    ei2, orig, ids, ego_of, g = ego_batch(base, centres, 2, csr="none")
    assert g is not None and g.symmetric and ids.numel() == 5 and g.num_nodes >= 10
    return g, ids


def _cold_of(g):
    import graphgym_amd as ga
    return ga.CSRGraph.from_csr(g.rowptr.clone(), g.col.clone(), None if g.val is None else g.val.clone(), g.num_nodes)


def test_ego_shortcut_and_an_aliasing_index(dev, monkeypatch):
    """id_branch(ids) of an ego batch's own CSR takes the shortcut; an index tensor with the legacy key of `ids` that
    lists other nodes takes the general build.  The `ids` ego_batch returns is a fresh arange(5): no view of ITS memory
    lists other nodes (its int32 words are 0 a 0 b ..: any five from the first address repeat 0 or are 0..4 again), so
    the colliding pair is made in a buffer of the test's own — buf[::2] = 0..4, the centres, against buf[:5] — and the
    graph is told that buf[::2] is its identity index, in the form ego_batch records it."""
    from graphgym_amd import graph
    CSR = graph.CSRGraph
    ran = []
    fast, slow = CSR._id_branch_of_ego_batch, CSR._id_branch_build
    monkeypatch.setattr(CSR, "_id_branch_of_ego_batch", lambda self, i: ran.append("ego") or fast(self, i))
    monkeypatch.setattr(CSR, "_id_branch_build", lambda self, i: ran.append("general") or slow(self, i))
    g, ids = _ego(dev)
    b0 = graph.BUILDS["id_branch"]
    br = g.id_branch(ids)
    assert ran == ["ego"] and graph.BUILDS["id_branch"] == b0 + 1
    same_branch(br, slow(g, ids), "the shortcut against _id_branch_build")
    same_branch(br, _cold_of(g).id_branch(ids), "the shortcut against a cold graph")
    ran.clear()
    before = builds()
    assert g.id_branch(ids) is br and g.id_branch(ids[:5]) is br and g.id_branch(again(ids)) is br
    assert builds() == before and not ran
    # the colliding pair
    g2, ids2 = _ego(dev)
    buf = torch.tensor([0, 9, 1, 7, 2, 8, 3, 6, 4, 5], device=dev)
    own, other = buf[::2], buf[:5]
    assert torch.equal(own, ids2) and _alias.legacy_index_key(own) == _alias.legacy_index_key(other)
    assert not torch.equal(own, other) and torch.unique(other).numel() == 5 and int(other.max()) < g2.num_nodes
    g2._ego_ids = (graph.tensor_stamp(own), own)
    ran.clear()
    br_own = g2.id_branch(own)
    assert ran == ["ego"]
    same_branch(br_own, br, "two expansions of the same centres")
    br_other = g2.id_branch(other)
    assert ran == ["ego", "general"], "an index that only aliases the centres was answered by the shortcut or the cache"
    same_branch(br_other, _cold_of(g2).id_branch(other), "the aliasing index against a cold graph")
    assert not torch.equal(br_other.slot, br_own.slot) or not torch.equal(br_other.rows, br_own.rows)


# ======================================================================================================= versioned updates
UPDATES = {
    "copy_": lambda t, new: t.copy_(new),
    "setitem": lambda t, new: t.__setitem__(slice(None), new),
    "add_": lambda t, new: t.add_(new - t),
}


@pytest.mark.parametrize("op", sorted(UPDATES))
@pytest.mark.parametrize("n", [1, 40])
def test_index_sites_rebuild_after_an_in_place_update(dev, op, n):
    from graphgym_amd import ops
    gen = torch.Generator().manual_seed(n)
    first, second = torch.randperm(N, generator=gen)[:n], torch.randperm(N, generator=gen)[:n]
    assert not torch.equal(first, second)
    ids = first.to(dev)
    g, x = fresh(dev), x_of(64).to(dev)
    g.select_rows(ids), g.mark_ids(ids), g.id_branch(ids)
    P_old, Q_old = ops.idgnn_aggregate(g, ids, x)
    UPDATES[op](ids, second.to(dev))
    assert torch.equal(ids.cpu(), second)
    cold = fresh(dev)
    same_graph(g.select_rows(ids), cold.select_rows(ids), "select_rows after " + op)
    graph_is(g.select_rows(ids), *np_select(second.numpy()), what="select_rows after " + op)
    assert torch.equal(g.mark_ids(ids), cold.mark_ids(ids))
    assert np.array_equal(g.mark_ids(ids).cpu().numpy(), np_marks(second.numpy()))
    same_branch(g.id_branch(ids), cold.id_branch(ids), "id_branch after " + op)
    branch_is(g.id_branch(ids), second.numpy(), "id_branch after " + op)
    P, Q = ops.idgnn_aggregate(g, ids, x)
    P0, Q0 = ops.idgnn_aggregate(cold, ids, x)
    assert torch.equal(Q, Q0) and torch.equal(P, P0) and torch.equal(P, P_old)
    before = builds()
    g.select_rows(ids), g.mark_ids(again(ids)), g.id_branch(again(ids))
    assert builds() == before


@pytest.mark.parametrize("op", sorted(UPDATES))
def test_holder_and_code_sites_rebuild_after_an_in_place_update(dev, monkeypatch, op):
    from graphgym_amd import encoders, layers, ops
    monkeypatch.delenv("MP_CODE_REDUCE", raising=False)
    gen = torch.Generator().manual_seed(11)
    # get_graph
    e1, e2 = torch.randint(0, N, (2, 150), generator=gen), torch.randint(0, N, (2, 150), generator=gen)
    ei, holder = e1.to(dev), types.SimpleNamespace()
    layers.get_graph(holder, ei, N)
    UPDATES[op](ei, e2.to(dev))
    gB = layers.get_graph(holder, ei, N)
    rp, col, _, eid = numpy_csr(e2[1].contiguous(), e2[0].contiguous(), None, N)
    assert np.array_equal(gB.rowptr.cpu().numpy(), rp) and np.array_equal(gB.col.cpu().numpy(), col)
    assert np.array_equal(gB.eid.cpu().numpy(), eid)
    before = builds()
    assert layers.get_graph(holder, again(ei), N) is gB and builds() == before
    # cached_codes, and embed_sum's one-hot operator on an int32 tensor the check hands back as it is
    K, dims, d = 3, [7, 7, 7], 64
    c1, c2 = torch.randint(0, 7, (30, K), generator=gen).int(), torch.randint(0, 7, (30, K), generator=gen).int()
    tables, dy = _tables(K, 7, d), torch.rand(30, d, generator=gen) * 2 - 1
    codes = c1.to(dev)
    ops._ONEHOT_T.clear()
    checked = encoders.cached_codes(holder, "node_feature", codes, dims)
    assert checked is codes                                        # int32, contiguous: no copy — the key IS the user's tensor
    _embed_grad(dev, checked, tables, dy, dims)
    UPDATES[op](codes, c2.to(dev))
    checked = encoders.cached_codes(holder, "node_feature", codes, dims)
    assert torch.equal(checked.cpu(), c2)
    _, got = _embed_grad(dev, checked, tables, dy, dims)
    assert len(ops._ONEHOT_T) == 2
    _check_embed(got, c2.long(), tables, dy, "embed_sum after " + op)
    ops._ONEHOT_T.clear()
    _, cold = _embed_grad(dev, checked, tables, dy, dims)
    assert all(torch.equal(a, b) for a, b in zip(got, cold))
    # spmm_code: the per-entry codes and the one-hot operator of the entries, both cached on the graph
    E, n_codes = DST.numel(), 12
    q1, q2 = torch.randint(0, n_codes, (E,), generator=gen).int(), torch.randint(0, n_codes, (E,), generator=gen).int()
    q, g = q1.to(dev), _code_graph(dev)
    x, dy2 = x_of(d), x_of(d, seed=1)
    table = torch.rand(n_codes, d, generator=gen) * 2 - 1
    _spmm_code_run(dev, g, q, x, table, dy2, "sum")
    UPDATES[op](q, q2.to(dev))
    y, dT = _spmm_code_run(dev, g, q, x, table, dy2, "sum")
    y0, dT0 = _spmm_code_run(dev, _code_graph(dev), q, x, table, dy2, "sum")
    assert torch.equal(y, y0) and torch.equal(dT, dT0), "spmm_code answered for the codes before " + op
    _spmm_code_check(y, dT, q2, x, table, dy2, "sum", "spmm_code after " + op)
    before = builds()
    _spmm_code_run(dev, g, q, x, table, dy2, "sum")
    assert builds() == before


def test_resampled_negatives_are_seen_by_a_cache(dev):
    """link_pred.run_negatives refills plan.out through its raw pointer on every call (resample_negative: one plan,
    another offset) and hands the same tensor out again: it moves the tensor's version, so a cache keyed on it rebuilds"""
    import graphgym_amd as ga
    from graphgym_amd import layers
    from graphgym_amd.link_pred import plan_negatives, run_negatives
    n = 30
    a = torch.arange(n)
    und = torch.stack([a, (a + 1) % n])
    base = ga.CSRGraph.from_edge_index(torch.cat([und, und.flip(0)], 1).to(dev), n)
    plan = plan_negatives(base, torch.tensor([0, n]), [40])
    holder = types.SimpleNamespace()
    out = run_negatives(plan, 3, 0)
    first = out.clone()
    g0 = layers.get_graph(holder, out, n)
    assert layers.get_graph(holder, out, n) is g0
    assert run_negatives(plan, 3, 1) is out and not torch.equal(out, first)
    g1 = layers.get_graph(holder, out, n)
    oc = out.cpu()
    rp, col, _, eid = numpy_csr(oc[1].contiguous(), oc[0].contiguous(), None, n)
    assert g1 is not g0 and np.array_equal(g1.rowptr.cpu().numpy(), rp) and np.array_equal(g1.col.cpu().numpy(), col)
    assert np.array_equal(g1.eid.cpu().numpy(), eid)


# ==================================================================================================== eviction and lifetime
LIMIT = 9           # `if len(cache) > 8: cache.clear()` before an insertion (graph.py): at most nine entries
ONEHOT_LIMIT = 8    # `if len(_ONEHOT_T) >= 8: _ONEHOT_T.clear()` (ops.py)

SITES = {
    "select_rows": ("_row_subsets", lambda g: g, lambda g, t: g.select_rows(t),
                    lambda a, b, w: same_graph(a, b, w)),
    "mark_ids": ("_id_marks", lambda g: g, lambda g, t: g.mark_ids(t),
                 lambda a, b, w: None if torch.equal(a, b) else pytest.fail(w)),
    "id_branch": ("_id_branch", lambda g: g, lambda g, t: g.id_branch(t),
                  lambda a, b, w: same_branch(a, b, w)),
}


@pytest.mark.parametrize("site", sorted(SITES))
def test_eleven_index_tensors_cycle_through_a_cache(dev, site):
    attr, owner, ask, same = SITES[site]
    gen = torch.Generator().manual_seed(7)
    keys = [torch.randperm(N, generator=gen)[:1 + 3 * k].to(dev) for k in range(11)]      # lengths 1, 4, .. 31
    g, cold = fresh(dev), fresh(dev)
    for k, t in enumerate(keys + keys[:1]):
        got = ask(g, t)
        assert len(owner(g).__dict__[attr]) <= LIMIT
        c = fresh(dev)
        same(got, ask(c, t), f"{site}: key {k} of the cycle against a cold graph")
    assert 1 <= len(owner(g).__dict__[attr]) <= LIMIT
    if site == "select_rows":
        graph_is(ask(g, keys[0]), *np_select(keys[0].cpu().numpy()), what="the first key again")
    del cold


@pytest.mark.parametrize("site", sorted(SITES))
def test_a_cached_key_tensor_lives_as_long_as_its_entry(dev, site):
    """holding the tensor is what keeps its address from being handed to another allocation while the entry lives"""
    attr, owner, ask, _ = SITES[site]
    g = fresh(dev)
    t = torch.arange(5, 25, device=dev)
    ask(g, t)
    alive = weakref.ref(t)
    del t
    gc.collect()
    assert alive() is not None and len(owner(g).__dict__[attr]) == 1
    for k in range(LIMIT):                                         # nine more keys: the tenth insertion clears the cache
        ask(g, torch.arange(k, k + 3, device=dev))
        assert len(owner(g).__dict__[attr]) <= LIMIT
    gc.collect()
    assert alive() is None, "the evicted key tensor is still referenced"


def test_onehot_operators_are_bounded_and_hold_their_codes(dev, monkeypatch):
    from graphgym_amd import ops
    monkeypatch.delenv("MP_CODE_REDUCE", raising=False)
    K, dims, d, R = 2, [5, 5], 3, 20
    gen = torch.Generator().manual_seed(9)
    tables, dy = _tables(K, 5, d), torch.rand(R, d, generator=gen) * 2 - 1
    ops._ONEHOT_T.clear()
    all_codes = [torch.randint(0, 5, (R, K), generator=gen) for _ in range(11)]
    first = ops.check_codes(all_codes[0].to(dev), dims)
    _, want = _embed_grad(dev, first, tables, dy, dims)
    alive = weakref.ref(first)
    del first
    gc.collect()
    assert alive() is not None and len(ops._ONEHOT_T) == 1
    for k, c in enumerate(all_codes[1:]):
        _, got = _embed_grad(dev, ops.check_codes(c.to(dev), dims), tables, dy, dims)
        assert len(ops._ONEHOT_T) <= ONEHOT_LIMIT
        _check_embed(got, c, tables, dy, f"codes {k + 1} of the cycle")
    gc.collect()
    assert alive() is None, "the evicted codes are still referenced"
    _, got = _embed_grad(dev, ops.check_codes(all_codes[0].to(dev), dims), tables, dy, dims)
    assert all(torch.equal(a, b) for a, b in zip(got, want)) and len(ops._ONEHOT_T) <= ONEHOT_LIMIT
    ops._ONEHOT_T.clear()


# ========================================================================================================== pattern sharing
def _derive(kind, g, dev):
    gen = torch.Generator().manual_seed(21)
    if kind == "gcn_row":
        return g.gcn_norm("row")
    if kind == "gcn_col":
        return g.gcn_norm("col")
    if kind == "scaled":
        return g.scaled((torch.rand(N, generator=gen) + 0.5).to(dev), (torch.rand(N, generator=gen) + 0.5).to(dev))
    return g.with_values((torch.rand(g.nnz, generator=gen) - 0.5).to(dev))


def _touch_all(g, ids, v2, row_bytes=256):
    t = g.transpose()
    return dict(plan=tuple(g.plan()[1]), t=t, t_mean=g.transpose_mean(), t_with=g.transpose_with(v2),
                row_ids=g.row_ids(), marks=g.mark_ids(ids), hot=g.hot_col(4 * row_bytes, row_bytes),
                id_t=g.id_branch(ids).t)


def _same_touch(a, b, what):
    assert a["plan"] == b["plan"], what + " plan counts"
    for k in ("t", "t_mean", "t_with", "id_t"):
        same_graph(a[k], b[k], f"{what} {k}")
    for k in ("row_ids", "marks", "hot"):
        assert torch.equal(a[k], b[k]), f"{what} {k}"


@pytest.mark.parametrize("order", ["base_first", "derived_first"])
@pytest.mark.parametrize("kind", ["gcn_row", "gcn_col", "scaled", "with_values"])
def test_graphs_of_one_pattern_share_structures_but_not_values(dev, kind, order):
    base = fresh(dev)
    b0 = builds()
    der = _derive(kind, base, dev)
    assert der.val is not None and not torch.equal(der.val, base.val)
    gen = torch.Generator().manual_seed(22)
    ids = torch.randperm(N, generator=gen)[:17].to(dev)
    v2 = (torch.rand(base.nnz, generator=gen) + 0.25).to(dev)
    if order == "base_first":
        got_base, got_der = _touch_all(base, ids, v2), _touch_all(der, ids, v2)
    else:
        got_der, got_base = _touch_all(der, ids, v2), _touch_all(base, ids, v2)
    b1 = builds()
    for shared in ("plan", "transpose", "id_marks", "hot_col"):    # built once for the pattern, whoever asked first
        assert b1.get(shared, 0) - b0.get(shared, 0) == 1, (shared, b0, b1)
    assert b1["id_branch"] - b0.get("id_branch", 0) == 2            # ... but one identity branch per graph: it holds values
    _same_touch(got_base, _touch_all(fresh(dev), ids, v2), f"{kind} {order}: base")
    _same_touch(got_der, _touch_all(fresh(dev, val=der.val), ids, v2), f"{kind} {order}: derived")
    # numpy: the transposes in the engine's order, the hot tag on the four most used columns, the marks
    for got, val in ((got_base, base.val), (got_der, der.val)):
        graph_is(got["t"], *np_transpose(val.cpu().numpy()), what=f"{kind} {order}: transpose against numpy")
        graph_is(got["t_with"], *np_transpose(v2.cpu().numpy()), what=f"{kind} {order}: transpose_with against numpy")
        assert np.array_equal(got["marks"].cpu().numpy(), np_marks(ids.cpu().numpy()))
        assert np.array_equal(got["hot"].cpu().numpy(), np_marks(sorted(HOT)))
        assert np.array_equal(got["row_ids"].cpu().numpy(), NP_ROWS)
    cnt = np.maximum(np.diff(NP_CSR[0]), 1).astype(np.float32)
    for got, val in ((got_base, base.val), (got_der, der.val)):
        want = (np.float32(1.0) / cnt)[NP_ROWS] * val.cpu().numpy()
        trp, tcol, tval = np_transpose(want)
        assert np.array_equal(got["t_mean"].rowptr.cpu().numpy(), trp) and np.array_equal(got["t_mean"].col.cpu().numpy(), tcol)
        assert np.array_equal(got["t_mean"].val.cpu().numpy(), tval)


# ============================================================================================================== flag caches
@pytest.mark.parametrize("order", ["graph_first", "sibling_first"])
def test_flag_caches_answer_for_the_graph_asked(dev, order):
    import graphgym_amd as ga
    n = 30
    a = torch.arange(n)
    und = torch.stack([a, (a + 1) % n])
    ei = torch.cat([und, und.flip(0), torch.tensor([[4, 11], [4, 11]])], 1)      # a symmetric pattern with two self loops
    wu = torch.rand(n, generator=torch.Generator().manual_seed(1)) + 0.5
    w = torch.cat([wu, wu, torch.tensor([2.0, 3.0])])
    g = ga.CSRGraph.from_edge_index(ei.to(dev), n, w.to(dev))
    asym = g.val * torch.linspace(1.0, 2.0, g.nnz, device=dev)
    sib = g.with_values(asym)
    asks = [(g, True), (sib, False)] if order == "graph_first" else [(sib, False), (g, True)]
    for graph, symmetric in asks + asks:                           # the second round is answered from the caches
        assert graph.is_symmetric(run=True) is symmetric
        assert graph.has_self_loops() is True and graph.max_row_entries() == 3
        t = graph.transpose()
        assert (t is graph) == symmetric
    plain = ga.CSRGraph.from_edge_index(torch.cat([und, und.flip(0)], 1).to(dev), n)
    sib2 = plain.with_values(torch.rand(plain.nnz, device=dev) + 0.5)
    for graph in (sib2, plain, sib2):
        assert graph.has_self_loops() is False and graph.max_row_entries() == 2
    assert plain.is_symmetric(run=True) is True and sib2.is_symmetric(run=True) is False
    tt = sib2.transpose()
    dense_of = lambda q: torch.zeros(n, n, device=dev).index_put_((q.row_ids().long(), q.col.long()), q.val)   # noqa: E731
    assert torch.equal(dense_of(tt), dense_of(sib2).t())
