"""ops.deterministic(): the backward forms without float atomics, on the device.

The pull-form max backward (mp_spmm_max_bwd_pull_f32 / _bf16 / mp_spmm_heads_max_bwd_pull_f32) against the scatter form
it stands in for (tests/_tol.py's regime), against float64, and — bit for bit — against the NumPy restatement of its
summation order (tests/_detref.py) and against itself over repeated calls and rebuilt graphs; the smaller sites (row
gather / scatter, the indexed cross-entropy, the by-node sums of the attention scores) against their default paths; the
proof that the switch alone decides (the atomic entry points replaced by functions that raise); two training runs from
one seed; and the gradient-subset sweeps of tests/test_grad_subsets_gpu.py once more under the switch.

Shapes are the smallest that reach every branch: d = 1, 3, 7 (W = 1, a scalar tail), 64 (W = 1 on full lanes), 260
(W = 4, two column tiles) — bf16 also 264 (W = 8); graphs of tests/_detref.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _detref as D
from _tol import assert_close_rows

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 7, 64, 260)


def same_bits(a, b):
    """equal shape, dtype and bytes (any dtype, any width, 0-dim included)"""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.reshape(-1).contiguous().view(torch.uint8),
                                                                     b.reshape(-1).contiguous().view(torch.uint8))


@pytest.fixture()
def switch():
    """the override as it was, whatever a test sets (torch's own flag too)"""
    from graphgym_amd import ops
    saved = ops._DETERMINISTIC
    t_on, t_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    yield ops
    ops._DETERMINISTIC = saved
    torch.use_deterministic_algorithms(t_on, warn_only=t_warn)


def _build(dev, kind, weighted, seed=0):
    """the operator of a tests/_detref.py graph on the device (a fresh build at every call) and the rows x must have"""
    import graphgym_amd as ga
    dst, src, N, w = D.edges(kind, seed)
    ei = torch.from_numpy(np.stack([src, dst])).to(dev)
    G = ga.CSRGraph.from_edge_index(ei, N, torch.from_numpy(w).to(dev) if weighted else None)
    if kind == "symmetric":
        G.symmetric = True
    if kind == "rect":
        G = G._select_rows(torch.arange(3, N, 2, device=dev))
        assert G.num_nodes != G.num_cols
    return G


def _cpu(G):
    rows = np.repeat(np.arange(G.num_nodes), np.diff(G.rowptr.cpu().numpy().astype(np.int64)))
    return rows, G.col.cpu().numpy().astype(np.int64), None if G.val is None else G.val.cpu().numpy()


def _boost(kind):
    return (0,) if kind == "star" else (4, 5, 6)


@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weighted"])
@pytest.mark.parametrize("kind", D.GRAPHS)
def test_pull_form_against_scatter_float64_and_host(dev, switch, monkeypatch, kind, weighted):
    import graphgym_amd as ga
    ops = switch
    if kind == "star":
        monkeypatch.setattr(ga.CSRGraph, "PLAN_CONFIG", D.STAR_PLAN)
    G = _build(dev, kind, weighted)
    rows, cols, val = _cpu(G)
    gt = G._transpose_sorted()
    assert gt is not G and gt.pos is not None
    if kind == "symmetric":
        assert G.transpose() is G                  # the flagged graph's own transpose has no pos: the pull form never asks it
    rp, gc, gp = (t.cpu().numpy() for t in (gt.rowptr, gt.col, gt.pos))
    n_hub = gt.plan()[1][1]
    assert (n_hub > 0) == (kind == "star")
    if kind == "star":
        assert 250 <= rp[1] - rp[0] <= 350 and gt.plan()[1][2] >= 4      # ~300 entries in >= 4 pieces
    if kind == "no_out":
        assert (np.diff(rp) == 0).sum() >= G.num_cols // 5
    hub = dict(hub_deg=D.STAR_PLAN[2], piece_edges=D.STAR_PLAN[3]) if kind == "star" else {}
    for d in WIDTHS:
        x = torch.from_numpy(D.features(G.num_cols, d, boost=_boost(kind))).to(dev)
        _, argmax = ops._raw_spmm(G, x, ops._lib.MAX, want_argmax=True)
        am = argmax.cpu().numpy()
        if kind == "empty_dst":
            assert (am == -1).all(axis=1).sum() >= G.num_nodes // 6
        dy = D.spread_dy((G.num_nodes, d))
        dyd = torch.from_numpy(dy).to(dev)
        scatter = torch.ops.mp.spmm_max_bwd_raw(dyd, argmax, G.handle)
        pull = torch.ops.mp.spmm_max_bwd_pull_raw(dyd, argmax, G.handle)
        assert pull.shape == (G.num_cols, d) and pull.dtype == torch.float32
        ref = D.max_bwd_dense64(rows, cols, val, am, dy, G.num_cols)
        mag = D.max_bwd_dense64(rows, cols, val, am, dy, G.num_cols, absolute=True)
        what = f"{kind} weighted={weighted} d={d}"
        # sums of either sign over magnitudes spread across 2^20: held to the sum of absolute terms (rule (d))
        assert_close_rows(pull, ref, mag=mag, what=what + " vs float64")
        assert_close_rows(pull, scatter.double().cpu(), mag=mag, what=what + " vs scatter")
        # the same bits: five calls, and a second build of the same edge list
        for _ in range(4):
            assert same_bits(torch.ops.mp.spmm_max_bwd_pull_raw(dyd, argmax, G.handle), pull), what
        G2 = _build(dev, kind, weighted)
        if kind == "star":
            assert G2._transpose_sorted().plan()[1][1] > 0
        _, argmax2 = ops._raw_spmm(G2, x, ops._lib.MAX, want_argmax=True)
        assert torch.equal(argmax2, argmax)
        assert same_bits(torch.ops.mp.spmm_max_bwd_pull_raw(dyd, argmax2, G2.handle), pull), what + " rebuilt"
        if d in (7, 260):
            host = D.max_bwd_pull_host(rp, gc, gp, val, am, dy, **hub)
            if not weighted:       # exact products, plain fp32 adds in the stated order: every row, hub rows included
                assert np.array_equal(host.view(np.uint32), pull.cpu().numpy().view(np.uint32)), what + " vs host"
            else:                  # (the fma of the host restatement may round twice: float64's regime)
                assert_close_rows(pull, host.astype(np.float64), mag=mag, what=what + " vs host")
            if not weighted and d == 7 and kind in ("multi", "star"):
                # the input shows an order: the host sum with every row's entries reversed has other bits somewhere
                rc, rpos = D.reversed_rows(rp, gc, gp)
                other = D.max_bwd_pull_host(rp, rc, rpos, val, am, dy)
                assert (other.view(np.uint32) != host.view(np.uint32)).any(axis=1).sum() >= 1


def test_second_backward_builds_nothing(dev, switch):
    from graphgym_amd import graph as gmod
    ops = switch
    ops.set_deterministic(True)
    G = _build(dev, "multi", True)
    x = torch.from_numpy(D.features(G.num_cols, 16)).to(dev).requires_grad_(True)
    ops.spmm(G, x, "max").sum().backward()
    before = dict(gmod.BUILDS)
    t, plan = G._t, G._t._plan
    assert t is not None and plan is not None
    ops.spmm(G, x, "max").sum().backward()
    assert G._t is t and G._t._plan is plan and dict(gmod.BUILDS) == before


@pytest.mark.parametrize("d", [64, 260, 264, 7])
def test_pull_form_bf16(dev, switch, d):
    """a bf16 dy gives a bf16 dx: the fp32 result on the widened dy, rounded once"""
    ops = switch
    G = _build(dev, "multi", True)
    x = torch.from_numpy(D.features(G.num_cols, d, boost=_boost("multi"))).to(dev)
    _, argmax = ops._raw_spmm(G, x, ops._lib.MAX, want_argmax=True)
    dy = torch.from_numpy(D.spread_dy((G.num_nodes, d))).to(dev).to(torch.bfloat16)
    lo = torch.ops.mp.spmm_max_bwd_pull_raw(dy, argmax, G.handle)
    hi = torch.ops.mp.spmm_max_bwd_pull_raw(dy.float(), argmax, G.handle)
    assert lo.dtype == torch.bfloat16 and lo.shape == hi.shape
    once = hi.to(torch.bfloat16)
    # one bf16 ulp of the fp32 value v = m 2^e (0.5 <= m < 1): 2^(e - 8)
    err = (lo.float() - once.float()).abs()
    ulp = torch.ldexp(torch.ones_like(hi), torch.frexp(hi).exponent - 8)
    print(f"bf16 d={d}: {int((err > 0).sum())} of {err.numel()} elements differ from the fp32 result rounded once")
    assert bool((err <= ulp).all())
    assert same_bits(torch.ops.mp.spmm_max_bwd_pull_raw(dy, argmax, G.handle), lo)
    scatter = torch.ops.mp.spmm_max_bwd_raw(dy, argmax, G.handle)
    assert scatter.dtype == torch.bfloat16
    # (the reference here is itself a bf16 rounding, which may exceed the sum of absolute terms by one rounding)
    mag = D.max_bwd_dense64(*_cpu(G), argmax.cpu().numpy(), dy.float().cpu().numpy(), G.num_cols, absolute=True)
    mag = mag * (1 + 2.0 ** -7)
    assert_close_rows(lo.float(), scatter.float().double().cpu(), tol=2.0 ** -7, mag=mag, what=f"bf16 d={d} vs scatter")


@pytest.mark.parametrize("kind", ["multi", "star"])
@pytest.mark.parametrize("heads", [1, 2, 4, 8, 3])
def test_heads_pull_form(dev, switch, monkeypatch, heads, kind):
    import graphgym_amd as ga
    ops = switch
    if kind == "star":
        monkeypatch.setattr(ga.CSRGraph, "PLAN_CONFIG", D.STAR_PLAN)
    G = _build(dev, kind, False)
    rows, cols, _ = _cpu(G)
    gt = G._transpose_sorted()
    rp, gc, gp = (t.cpu().numpy() for t in (gt.rowptr, gt.col, gt.pos))
    hub = dict(hub_deg=D.STAR_PLAN[2], piece_edges=D.STAR_PLAN[3]) if kind == "star" else {}
    g = torch.Generator().manual_seed(5 + heads)
    for d in (24, 96):
        V = torch.from_numpy(D.features(G.num_cols, d, boost=_boost(kind))).to(dev)
        wide = (torch.rand(G.nnz, 2 * heads, generator=g) + 0.25).to(dev)
        a = wide[:, ::2]                                   # not contiguous at the call site
        assert not a.is_contiguous()
        _, argmax = ops._raw_spmm_heads_reduce(G, a.contiguous(), V, heads, ops._lib.MAX)
        dy = D.spread_dy((G.num_nodes, d), seed=heads)
        dyd = torch.from_numpy(dy).to(dev)
        pull = torch.ops.mp.spmm_heads_max_bwd_pull_raw(dyd, argmax, a, G.handle, heads)
        ops.set_deterministic(False)
        scatter = ops._heads_grad_by_source(G, a.contiguous(), V, heads, True, dyd, argmax)
        ops.set_deterministic(True)
        chosen = ops._heads_grad_by_source(G, a, V, heads, True, dyd, argmax)
        am, an = argmax.cpu().numpy(), a.cpu().numpy()
        ref = D.max_bwd_dense64(rows, cols, an, am, dy, G.num_cols, heads=heads)
        mag = D.max_bwd_dense64(rows, cols, an, am, dy, G.num_cols, heads=heads, absolute=True)
        what = f"heads {heads} {kind} d={d}"
        assert_close_rows(pull, ref, mag=mag, what=what + " vs float64")
        assert_close_rows(pull, scatter.double().cpu(), mag=mag, what=what + " vs scatter")
        assert same_bits(chosen, pull)
        for _ in range(4):
            assert same_bits(torch.ops.mp.spmm_heads_max_bwd_pull_raw(dyd, argmax, a, G.handle, heads), pull), what
        if d == 24:
            host = D.max_bwd_pull_host(rp, gc, gp, an, am, dy, heads=heads, **hub)
            assert_close_rows(pull, host.astype(np.float64), mag=mag, what=what + " vs host")


# ---- the switch alone decides -------------------------------------------------------------------------------------------
ATOMIC_ENTRIES = ("mp_spmm_max_bwd_f32", "mp_spmm_max_bwd_bf16", "mp_spmm_heads_max_bwd_f32", "mp_rows_scatter_add_f32")


def _raiser(name):
    def f(*a, **k):
        raise AssertionError(f"{name} was launched")
    return f


def _steps(dev):
    """forward + backward of every op whose backward (or forward) has an atomic form, by name"""
    import graphgym_amd as ga
    from graphgym_amd import nn as _nn, ops  # noqa: F401  (nn registers mp::softmax_ce)
    dst, src, N, w = D.edges("multi")
    E = dst.size
    ei = torch.from_numpy(np.stack([src, dst])).to(dev)
    G = ga.CSRGraph.from_edge_index(ei, N, torch.from_numpy(w).to(dev))
    d, H = 16, 4
    g = torch.Generator().manual_seed(3)

    def leaf(*shape):
        return torch.randn(*shape, generator=g).to(dev).requires_grad_(True)

    def done(y, *leaves):
        y.sum().backward()
        torch.cuda.synchronize()
        assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in leaves)
    ids = torch.randint(0, 20, (64,), generator=g).to(dev)
    codes = torch.randint(0, 5, (E,), generator=g).to(torch.int32).to(dev)

    def spmm():
        x = leaf(N, d)
        done(ops.spmm(G, x, "max"), x)

    def spmm_bf16():
        x = torch.randn(N, d, generator=g).to(dev).to(torch.bfloat16).requires_grad_(True)
        done(ops.spmm(G, x, "max").float(), x)

    def spmm_edge():
        x, m = leaf(N, d), leaf(E, d)
        done(ops.spmm_edge(G, x, m, "max"), x, m)

    def spmm_code():
        x, table = leaf(N, d), leaf(5, d)
        done(ops.spmm_code(G, x, table, codes, "max"), x, table)

    def spmm_edge_values():
        a, V = leaf(G.nnz, H), leaf(N, d)
        done(ops.spmm_edge_values(G, a, V, H, "max"), a, V)

    def spmm_edge_heads():
        wt, x, m = leaf(G.nnz, H), leaf(N, d), leaf(E, d)
        done(ops.spmm_edge_heads(G, wt, x, m, heads=H, reduce="max"), wt, x, m)

    def gather_rows():
        x = leaf(N, d)
        done(ops.gather_rows(x, ids), x)

    def index_add_rows():
        h, u = leaf(N, d), leaf(ids.numel(), d)
        done(ops.index_add_rows(h, ids, u), h, u)

    def softmax_ce():
        z = leaf(N, 6)
        idx = torch.cat([torch.arange(40), torch.tensor([7, 7, 7])]).to(dev)        # row 7 four times over
        done(torch.ops.mp.softmax_ce(z, torch.randint(0, 6, (43,), generator=g).to(dev), idx), z)
    return [spmm, spmm_bf16, spmm_edge, spmm_code, spmm_edge_values, spmm_edge_heads, gather_rows, index_add_rows,
            softmax_ce]


def test_no_atomic_entry_is_launched_under_the_switch(dev, switch, monkeypatch):
    """with the four atomic entry points replaced by functions that raise, every op still runs forward and backward
    when the switch is on; with it off the same run raises — the default path is what it was"""
    from graphgym_amd import _lib
    ops = switch
    L = _lib.lib()
    for name in ATOMIC_ENTRIES:
        monkeypatch.setattr(L, name, _raiser(name))
    ops.set_deterministic(True)
    for step in _steps(dev):
        step()
    ops.set_deterministic(None)
    torch.use_deterministic_algorithms(True, warn_only=True)      # torch's flag alone turns it on as well
    for step in _steps(dev):
        step()
    torch.use_deterministic_algorithms(False)
    for step in _steps(dev):
        if step.__name__ == "softmax_ce":        # its atomic form lives inside mp_softmax_ce_bwd_f32 (checked by bits below)
            step()
            continue
        with pytest.raises(AssertionError, match="was launched"):
            step()
    ops.set_deterministic(False)
    torch.use_deterministic_algorithms(True, warn_only=True)      # ... and the override wins over torch's flag
    with pytest.raises(AssertionError, match="was launched"):
        _steps(dev)[0]()


# ---- the smaller sites --------------------------------------------------------------------------------------------------
def _both_ways(ops, run, n=3):
    """run() -> tuple of gradients: once on the default path, n times under the switch (equal bits among those)"""
    ops.set_deterministic(False)
    base = run()
    ops.set_deterministic(True)
    det = [run() for _ in range(n)]
    for other in det[1:]:
        for a, b in zip(det[0], other):
            assert same_bits(a, b)
    return base, det[0]


def _att_inputs(dev, heads, seed):
    import graphgym_amd as ga
    dst, src, N, _ = D.edges("multi", seed)
    ei = torch.from_numpy(np.stack([src, dst])).to(dev)
    G = ga.CSRGraph.from_edge_index(ei, N)
    g = torch.Generator().manual_seed(seed)
    return G, N, dst.size, g


def _abs_node_sums(G, terms):
    """(by destination, by source) sums of |terms| [nnz, H] in float64 on the CPU"""
    rows = torch.repeat_interleave(torch.arange(G.num_nodes), (G.rowptr[1:] - G.rowptr[:-1]).cpu().long())
    cols = G.col.cpu().long()
    t = terms.detach().abs().double().cpu()
    zero = torch.zeros(G.num_nodes, t.size(1), dtype=torch.float64)
    return zero.index_add(0, rows, t), zero.index_add(0, cols, t)


def test_sddmm_add_sums(dev, switch):
    ops = switch
    G, N, E, g = _att_inputs(dev, 1, 1)
    ai, aj = (torch.randn(N, generator=g).to(dev) for _ in range(2))
    ds = torch.from_numpy(D.spread_dy((G.nnz, 1), 1)).to(dev)

    def run():
        a, b = ai.clone().requires_grad_(True), aj.clone().requires_grad_(True)
        ops.sddmm_add(G, a, b, 0.2).backward(ds)
        return a.grad, b.grad
    base, det = _both_ways(ops, run)
    md, ms = _abs_node_sums(G, ds)               # lrelu' <= 1: the absolute terms bound the sums
    assert_close_rows(det[0][:, None], base[0].double().cpu()[:, None], mag=md, what="sddmm_add d_dst")
    assert_close_rows(det[1][:, None], base[1].double().cpu()[:, None], mag=ms, what="sddmm_add d_src")


@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("op", ["gat_alpha", "edge_att_alpha"])
def test_attention_score_sums(dev, switch, op, heads):
    ops = switch
    G, N, E, g = _att_inputs(dev, heads, 2)
    a_dst, a_src, a_edge = (torch.randn(n, heads, generator=g).to(dev) for n in (N, N, E))
    dal = torch.from_numpy(D.spread_dy((G.nnz, heads), 2)).to(dev)
    seen = {}

    def run():
        a, b, c = (t.clone().requires_grad_(True) for t in (a_dst, a_src, a_edge))
        alpha = ops.gat_alpha(G, a, b, 0.2) if op == "gat_alpha" else ops.edge_att_alpha(G, a, b, c, 0.2)
        alpha.backward(dal)
        seen["alpha"] = alpha.detach()
        return a.grad, b.grad
    base, det = _both_ways(ops, run)
    # |ds_e| <= alpha_e (|dalpha_e| + sum_row alpha |dalpha|) <= 2 max_row |dalpha| alpha_e: the absolute terms
    al = seen["alpha"].double().cpu()
    rows = torch.repeat_interleave(torch.arange(N), (G.rowptr[1:] - G.rowptr[:-1]).cpu().long())
    rowdot = torch.zeros(N, heads, dtype=torch.float64).index_add_(0, rows, al * dal.double().cpu().abs())
    md, ms = _abs_node_sums(G, al * (dal.double().cpu().abs() + rowdot[rows]))
    assert_close_rows(det[0], base[0].double().cpu(), mag=md, what=f"{op} H={heads} d_dst")
    assert_close_rows(det[1], base[1].double().cpu(), mag=ms, what=f"{op} H={heads} d_src")


def test_gather_rows_and_index_add_rows_with_repeats(dev, switch):
    ops = switch
    g = torch.Generator().manual_seed(4)
    n, d = 150, 33
    ids = torch.cat([torch.arange(0, 40), torch.tensor([3] * 3 + [9] * 5 + [11] * 17), torch.randint(0, 60, (100,),
                                                                                                    generator=g)]).to(dev)
    x = torch.randn(n, d, generator=g).to(dev)
    dout = torch.from_numpy(D.spread_dy((ids.numel(), d), 4)).to(dev)

    def run():
        t = x.clone().requires_grad_(True)
        ops.gather_rows(t, ids).backward(dout)
        return (t.grad,)
    base, det = _both_ways(ops, run)
    mag = torch.zeros(n, d, dtype=torch.float64).index_add_(0, ids.cpu(), dout.double().cpu().abs())
    ref = torch.zeros(n, d, dtype=torch.float64).index_add_(0, ids.cpu(), dout.double().cpu())
    assert_close_rows(det[0], ref, mag=mag, what="gather_rows dx vs float64")
    assert_close_rows(det[0], base[0].double().cpu(), mag=mag, what="gather_rows dx vs atomics")
    assert float(det[0][60:].abs().max()) == 0.0

    h = torch.randn(n, d, generator=g).to(dev)

    def run2():
        a, u = h.clone().requires_grad_(True), dout.clone().requires_grad_(True)
        y = ops.index_add_rows(a, ids, u)
        y.backward(torch.ones_like(y))
        return y.detach(), a.grad, u.grad
    base, det = _both_ways(ops, run2)
    ref = h.double().cpu().index_add(0, ids.cpu(), dout.double().cpu())
    assert_close_rows(det[0], ref, mag=mag + h.double().cpu().abs(), what="index_add_rows vs float64")
    assert_close_rows(det[0], base[0].double().cpu(), mag=mag + h.double().cpu().abs(), what="index_add_rows vs atomics")
    assert same_bits(det[1], base[1]) and same_bits(det[2], base[2])
    assert same_bits(det[0][60:], h[60:])


def test_cross_entropy_with_a_repeated_index(dev, switch):
    import graphgym_amd.nn  # noqa: F401  (registers mp::softmax_ce)
    ops = switch
    g = torch.Generator().manual_seed(6)
    n, Cn = 300, 7
    z = (torch.randn(n, Cn, generator=g) * 3).to(dev)
    idx = torch.cat([torch.randperm(n, generator=g)[:100], torch.tensor([5, 5, 5, 17, 17, 17, 17])]).to(dev)
    y = torch.randint(0, Cn, (idx.numel(),), generator=g).to(dev)

    def run():
        t = z.clone().requires_grad_(True)
        loss = torch.ops.mp.softmax_ce(t, y, idx)
        loss.backward()
        return t.grad, loss.detach()
    base, det = _both_ways(ops, run)
    t = z.double().cpu().requires_grad_(True)
    F.cross_entropy(t[idx.cpu()], y.cpu()).backward()
    terms = (torch.softmax(z.double().cpu()[idx.cpu()], 1) + F.one_hot(y.cpu(), Cn)) / idx.numel()
    mag = torch.zeros(n, Cn, dtype=torch.float64).index_add_(0, idx.cpu(), terms)
    assert_close_rows(det[0], t.grad, mag=mag, what="softmax_ce dlogits vs float64")
    assert_close_rows(det[0], base[0].double().cpu(), mag=mag, what="softmax_ce dlogits vs atomics")
    assert same_bits(det[1], base[1])
    out = torch.ones(n, dtype=torch.bool)
    out[idx.cpu()] = False
    assert float(det[0].cpu()[out].abs().max()) == 0.0
    # an index outside the matrix: no gradient for that row, as on the default path
    bad = idx.clone()
    bad[0] = n + 5
    ops.set_deterministic(True)
    d_bad = torch.ops.mp.softmax_ce_bwd_raw(z, y, bad, torch.ones((), device=dev), 1.0 / idx.numel())
    d_ok = torch.ops.mp.softmax_ce_bwd_raw(z, y, idx, torch.ones((), device=dev), 1.0 / idx.numel())
    keep = torch.ones(n, dtype=torch.bool, device=dev)
    keep[idx[0]] = False
    assert same_bits(d_bad[keep], d_ok[keep]) and float(d_bad[idx[0]].abs().max()) == 0.0


# ---- end to end -----------------------------------------------------------------------------------------------------------
@pytest.fixture()
def gcfg():
    from graphgym_amd.config import cfg
    import graphgym_amd.graphgym_plugin  # noqa: F401  (registers the layer keys)
    saved = {k: dict(vars(getattr(cfg, k))) for k in ("gnn", "dataset", "bn", "mem")}
    cfg.gnn.layers_pre_mp, cfg.gnn.dim_inner, cfg.gnn.layers_post_mp, cfg.gnn.layers_mp = 1, 16, 1, 3
    cfg.gnn.batchnorm, cfg.gnn.dropout, cfg.gnn.act, cfg.gnn.l2norm, cfg.gnn.stage_type = True, 0.0, "relu", True, "stack"
    cfg.gnn.agg, cfg.gnn.normalize_adj, cfg.gnn.att_heads = "max", False, 2
    cfg.dataset.task, cfg.dataset.transform = "node", "none"
    yield cfg
    for k, v in saved.items():
        ns = getattr(cfg, k)
        for name in list(vars(ns)):
            if name not in v:
                delattr(ns, name)
        for name, val in v.items():
            setattr(ns, name, val)


@pytest.mark.parametrize("layer_type", ["generalconv", "gaddconv"])
def test_two_training_runs_end_in_the_same_bits(dev, switch, gcfg, layer_type):
    """three Adam steps of a 3-layer max-aggregation model on a 200-node multigraph whose node_label_index lists fifty
    nodes twice, two times from one seed under torch's deterministic flag (which the switch follows and which covers
    torch's own indexing backward): the state dicts are equal bit for bit"""
    from graphgym_amd import harness as H
    ops = switch
    gcfg.gnn.layer_type = layer_type
    g = torch.Generator().manual_seed(8)
    n, f_in, classes = 200, 6, 4
    ei = torch.randint(0, n, (2, 900), generator=g)
    ei = torch.cat([ei, ei[:, :300]], 1).to(dev)                     # a third of the edges twice
    x = torch.randn(n, f_in, generator=g).to(dev)
    labels = torch.randint(0, classes, (n,), generator=g).to(dev)
    idx = torch.cat([torch.arange(n), torch.arange(0, n, 4)]).to(dev)
    ops.set_deterministic(None)
    torch.use_deterministic_algorithms(True, warn_only=True)
    assert ops.deterministic()

    def train():
        torch.manual_seed(0)
        model = H.GNN(f_in, classes).to(dev).train()
        opt = torch.optim.Adam(model.parameters(), lr=0.01)
        for _ in range(3):
            batch = H.Batch(node_feature=x.clone(), edge_index=ei, node_label=labels, node_label_index=idx)
            opt.zero_grad()
            pred, true = model(batch)
            F.cross_entropy(pred, true).backward()
            opt.step()
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in model.state_dict().items()}
    a, b = train(), train()
    assert a.keys() == b.keys() and len(a) > 6
    for k in a:
        assert same_bits(a[k], b[k]), k
    assert any(bool((v != 0).any()) for v in a.values())


# ---- every subset of differentiated inputs, under the switch ----------------------------------------------------------------
@pytest.mark.parametrize("case", ["spmm", "spmm_edge", "spmm_edge_values", "sddmm_add", "gat_alpha", "rows", "softmax_ce"])
def test_gradient_subsets_under_the_switch(dev, switch, case):
    """the sweeps of tests/test_grad_subsets_gpu.py (each formula under every non-empty subset of its inputs, against
    float64 autograd on the CPU) for the ops whose backward changes with the switch, with the switch on"""
    import test_grad_subsets_gpu as T
    switch.set_deterministic(True)
    if case == "spmm":
        for relu, ss in ((False, 0.0), (True, 0.5)):
            T.test_spmm(dev, "max", relu, ss)
        T.test_spmm_dy_layouts(dev, "slice")
    elif case == "spmm_edge":
        T.test_spmm_edge(dev, "max", True, True)
    elif case == "spmm_edge_values":
        for heads in (1, 4):
            T.test_spmm_edge_values(dev, "max", heads)
    elif case == "sddmm_add":
        T.test_sddmm_add(dev)
    elif case == "gat_alpha":
        for heads in (1, 4):
            T.test_gat_alpha(dev, heads)
    elif case == "rows":
        T.test_gather_rows_and_index_add_rows(dev)
    else:
        T.test_softmax_ce(dev, True)
