"""generaledgeconv / generalsampleedgeconv (graphgym/contrib/layer/generalconv.py:117-218, graphgym/models/layer.py:199-221)
and the two-gather aggregation under their max form, against the float64 restatement of tests/_edgeconv_ref.py at the
tolerances of tests/_tol.py: 1e-5 per output row (rules (a), (b), (d)), one scale per tensor for parameter gradients.
Max gradients are evaluated at the engine's argmax (a near-tie cannot flip a winner between the two evaluations); the max
VALUES are checked against the restatement's own maximum."""
import numpy as np
import pytest
import torch

import _edgeconv_ref as R
from _tol import both, close, close_all, mag_of

pytestmark = pytest.mark.gpu

WIDTHS = (36, 48, 64, 128, 256, 512)


def _graph_edges(n=300, seed=0):
    """[2, E] source -> destination, the graph of test_attconv_gpu._graph_edges: isolated destinations, one entry three
    times, self loops on some nodes, one hub destination of 200 entries (cut into pieces under PLAN_CONFIG (64, 1, 64,
    64))"""
    g = torch.Generator().manual_seed(seed)
    m = 4 * n
    src = torch.randint(0, n, (m,), generator=g)
    dst = torch.randint(0, n, (m,), generator=g)
    keep = dst % 7 != 3                                      # rows 3, 10, 17, ... receive nothing
    src, dst = src[keep], dst[keep]
    hub_src = torch.randint(0, n, (200,), generator=g)
    rep = torch.tensor([[5, 5, 5, 8], [1, 1, 1, 1]])         # entry (1 <- 5) three times
    return torch.cat([torch.stack([src, dst]), torch.stack([hub_src, torch.zeros(200, dtype=torch.long)]), rep], dim=1)


@pytest.fixture(params=["default_plan", "hub_plan"])
def plan(request, monkeypatch):
    import graphgym_amd as ga
    if request.param == "hub_plan":
        monkeypatch.setenv("MP_AGG_TILES", "0")
        monkeypatch.setattr(ga.CSRGraph, "PLAN_CONFIG", (64, 1, 64, 64))
    return request.param


def _struct(g):
    return (g.row_ids().cpu().long(), g.col.cpu().long(), g.eid.cpu().long(), None if g.val is None else g.val.cpu())


def _op_case(dev, d, full, seed, extra_rows=3, **build):
    """a graph and operands: full = entry values, T and bias present; M holds extra_rows rows no entry points at"""
    import graphgym_amd as ga
    n = 300
    ei = _graph_edges(n, seed)
    gen = torch.Generator().manual_seed(seed + 1)
    w = (torch.rand(ei.size(1), generator=gen) * 2 - 0.5) if full else None
    g = ga.CSRGraph.from_edge_index(ei.to(dev), n, None if w is None else w.to(dev), **build)
    X = torch.rand(n, d, generator=gen) * 2 - 1
    M = torch.rand(ei.size(1) + extra_rows, d, generator=gen) * 2 - 1
    T = torch.rand(n, d, generator=gen) * 2 - 1 if full else None
    b = torch.rand(d, generator=gen) - 0.5 if full else None
    dy = torch.rand(n, d, generator=gen) * 2 - 1
    return g, X, M, T, b, dy


def _dev(t, dev, grad=False):
    return None if t is None else t.to(dev).requires_grad_(grad)


@pytest.mark.parametrize("full", [False, True], ids=["plain", "val_T_bias"])
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
def test_spmm_edge(dev, plan, reduce, d, full):
    from graphgym_amd import ops
    # self loops removed: their input edges are not in the operator
    g, X, M, T, b, dy = _op_case(dev, d, full, seed=d + 7 * full, remove_self_loops=True)
    if plan == "hub_plan":
        assert g.plan()[1][1] > 0 and g.plan()[1][2] > 0          # the 200-entry row runs in pieces
    rows, cols, eids, val = _struct(g)
    n = g.num_nodes
    Xd, Md, Td, bd = _dev(X, dev, True), _dev(M, dev, True), _dev(T, dev, True), _dev(b, dev, True)
    y = ops.spmm_edge(g, Xd, Md, reduce, t=Td, bias=bd)
    (y * dy.to(dev)).sum().backward()
    what = f"{reduce} d={d} {'full' if full else 'plain'} {plan}"

    def fwd(c, sign=lambda t: t, win=None):
        o = lambda t: None if t is None else sign(c(t))          # noqa: E731
        return R.edge_agg(rows, cols, eids, o(val), o(X), o(M), o(T), o(b), n, reduce, win)
    close(y.detach(), both(fwd), what=what + " y", mag=mag_of(lambda c: fwd(c, torch.abs)))

    win = None
    if reduce == "max":
        win = ops._raw_spmm_edge(g, X.to(dev), M.to(dev), _dev(T, dev), _dev(b, dev), ops._lib.MAX, True)[1].cpu()
        deg = torch.diff(g.rowptr.cpu())
        assert bool((win[deg > 0] >= 0).all()) and bool((win[deg == 0] == -1).all())
        assert bool((win < g.nnz).all())

    def grads(c, sign=lambda t: t):
        leaf = lambda t: None if t is None else sign(c(t)).detach().clone().requires_grad_(True)    # noqa: E731
        Xr, Mr, Tr, br = leaf(X), leaf(M), leaf(T), leaf(b)
        out = R.edge_agg(rows, cols, eids, None if val is None else sign(c(val)), Xr, Mr, Tr, br, n, reduce, win)
        (out * sign(c(dy))).sum().backward()
        return [t.grad for t in (Xr, Mr, Tr, br) if t is not None]
    g64, g32 = both(grads)
    m64 = mag_of(lambda c: grads(c, torch.abs))
    got = [t.grad for t in (Xd, Md, Td, bd) if t is not None]
    names = [k for k, t in zip(("dX", "dM", "dT", "dbias"), (Xd, Md, Td, bd)) if t is not None]
    for k, a, r64, r32, mg in zip(names, got, g64, g32, m64):
        if k == "dbias":
            close_all(a, (r64, r32), what=f"{what} {k}")
        else:
            close(a, (r64, r32), what=f"{what} {k}", mag=mg)
    # input edges the operator does not hold (removed self loops, rows past the edge list) get exactly zero
    absent = torch.ones(M.size(0), dtype=torch.bool)
    absent[eids[eids >= 0]] = False
    assert int(absent.sum()) >= 3 and bool((Md.grad.cpu()[absent] == 0).all())


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
def test_two_runs_are_bit_equal(dev, plan, reduce):
    from graphgym_amd import ops
    g, X, M, T, b, dy = _op_case(dev, 64, True, seed=3)

    def run():
        Xd, Md, Td, bd = _dev(X, dev, True), _dev(M, dev, True), _dev(T, dev, True), _dev(b, dev, True)
        y = ops.spmm_edge(g, Xd, Md, reduce, t=Td, bias=bd)
        (y * dy.to(dev)).sum().backward()
        out = [y.detach(), Md.grad, Td.grad, bd.grad]
        return out + ([] if reduce == "max" else [Xd.grad])        # dX of max: float atomics (mp_spmm_max_bwd_f32)
    for a, c in zip(run(), run()):
        assert torch.equal(a, c)


@pytest.mark.parametrize("d", [48, 64])
def test_max_ties_go_to_the_first_csr_entry(dev, plan, d):
    """integer-valued X, M, T and entry values: every product and sum is exact in float32, equal candidates are exactly
    equal, and the maximum is the float32 maximum of the terms"""
    import graphgym_amd as ga
    from graphgym_amd import ops
    n = 200
    gen = torch.Generator().manual_seed(7)
    src = torch.randint(0, n, (1600,), generator=gen) % 8         # eight sources only: many repeats per row
    dst = torch.randint(0, n, (1600,), generator=gen)
    dst[:150] = 0                                                  # a hub row in pieces
    w = torch.randint(1, 3, (1600,), generator=gen).float()
    g = ga.CSRGraph.from_edge_index(torch.stack([src, dst]).to(dev), n, w.to(dev))
    X = torch.randint(-2, 3, (n, d), generator=gen).float()
    M = torch.randint(-1, 2, (1600, d), generator=gen).float()
    T = torch.randint(-2, 3, (n, d), generator=gen).float()
    y, win = ops._raw_spmm_edge(g, X.to(dev), M.to(dev), T.to(dev), None, ops._lib.MAX, True)
    rows, cols, eids, val = _struct(g)
    msg = val[:, None] * ((X[cols] + M[eids]) + T[rows])           # float32, exact
    assert torch.equal(y.cpu(), R.reduce_rows(rows, msg, n, "max"))
    rp, wl = g.rowptr.cpu().long(), win.cpu().long()
    ties = 0
    for i in range(n):
        e0, e1 = int(rp[i]), int(rp[i + 1])
        if e0 == e1:
            assert bool((wl[i] == -1).all()) and bool((y[i] == 0).all())
            continue
        block = msg[e0:e1]
        top = block == block.max(dim=0).values
        ties += int((top.sum(0) > 1).sum())
        assert torch.equal(wl[i], top.float().argmax(dim=0) + e0), i
    assert ties > 100


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
@pytest.mark.parametrize("d", [36, 64, 256])
def test_strided_offset_views(dev, plan, reduce, d):
    """X, M, T and the output as column windows of wider buffers: leading dimension d + 5, first element 4 bytes past a
    16-byte boundary; the same bits as on dense operands"""
    from graphgym_amd import ops
    g, X, M, T, b, _ = _op_case(dev, d, True, seed=d)
    red = ops._lib.REDUCE[reduce]

    def window(t):
        big = torch.full((t.size(0), d + 5), float("nan"), device=dev)
        big[:, 1:1 + d] = t.to(dev)
        v = big[:, 1:1 + d]
        assert v.stride() == (d + 5, 1) and v.data_ptr() % 16 == 4
        return v
    want, want_arg = ops._raw_spmm_edge(g, X.to(dev), M.to(dev), T.to(dev), b.to(dev), red, reduce == "max")
    out_big = torch.full((g.num_nodes, d + 5), 7.0, device=dev)
    out = out_big[:, 1:1 + d]
    _, arg = ops._raw_spmm_edge(g, window(X), window(M), window(T), b.to(dev), red, reduce == "max", out=out)
    assert torch.equal(out, want)
    assert bool((out_big[:, 0] == 7).all()) and bool((out_big[:, 1 + d:] == 7).all())     # nothing beside the window
    if reduce == "max":
        assert torch.equal(arg, want_arg)
    rows, cols, eids, val = _struct(g)
    close(out, both(lambda c: R.edge_agg(rows, cols, eids, c(val), c(X), c(M), c(T), c(b), g.num_nodes, reduce)),
          what=f"views {reduce} d={d}",
          mag=mag_of(lambda c: R.edge_agg(rows, cols, eids, c(val).abs(), c(X).abs(), c(M).abs(), c(T).abs(),
                                          c(b).abs(), g.num_nodes, reduce)))
    # the differentiable operator takes the same views
    y = ops.spmm_edge(g, window(X), window(M), reduce, t=window(T), bias=b.to(dev))
    assert torch.equal(y, want)


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
def test_inserted_self_loops_carry_no_edge_term(dev, plan, reduce):
    """add_self_loops: one entry per node with eid < 0, which contributes val * (X[r] + T[r]) only — also the gradient"""
    from graphgym_amd import ops
    g, X, M, T, b, dy = _op_case(dev, 64, True, seed=11, extra_rows=0, add_self_loops=True, fill=0.75)
    rows, cols, eids, val = _struct(g)
    assert int((eids < 0).sum()) == g.num_nodes
    Xd, Md, Td = _dev(X, dev, True), _dev(M, dev, True), _dev(T, dev, True)
    y = ops.spmm_edge(g, Xd, Md, reduce, t=Td)
    (y * dy.to(dev)).sum().backward()
    n = g.num_nodes
    close(y.detach(), both(lambda c: R.edge_agg(rows, cols, eids, c(val), c(X), c(M), c(T), None, n, reduce)),
          what=f"loops {reduce} y",
          mag=mag_of(lambda c: R.edge_agg(rows, cols, eids, c(val).abs(), c(X).abs(), c(M).abs(), c(T).abs(), None, n,
                                          reduce)))
    win = ops._raw_spmm_edge(g, X.to(dev), M.to(dev), T.to(dev), None, ops._lib.MAX, True)[1].cpu() \
        if reduce == "max" else None

    def dm(c, sign=lambda t: t):
        Mr = sign(c(M)).detach().clone().requires_grad_(True)
        out = R.edge_agg(rows, cols, eids, sign(c(val)), sign(c(X)), Mr, sign(c(T)), None, n, reduce, win)
        (out * sign(c(dy))).sum().backward()
        return Mr.grad
    close(Md.grad, both(dm), what=f"loops {reduce} dM", mag=mag_of(lambda c: dm(c, torch.abs)))


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
@pytest.mark.parametrize("d", [36, 64, 256])
@pytest.mark.parametrize("weighted", [True, False], ids=["val", "no_val"])
def test_without_edge_terms_it_is_the_plain_aggregation(dev, plan, reduce, d, weighted):
    """every entry with eid < 0, no T, no bias, a one-row M: each message is val * X[col], so the two-gather form gives the
    bits (and, for max, the winning entries) of the one-gather aggregation on the same operator"""
    import graphgym_amd as ga
    from graphgym_amd import ops
    g0, X, _, _, _, _ = _op_case(dev, d, weighted, seed=d + 1)
    assert (g0.val is not None) == weighted
    g = ga.CSRGraph(g0.rowptr, g0.col, g0.val, torch.full_like(g0.eid, -1), g0.num_nodes, g0.nnz)
    if plan == "hub_plan":
        assert g.plan()[1][1] > 0 and g.plan()[1][2] > 0
    Xd = X.to(dev)
    M = torch.full((1, d), float("nan"), device=dev)              # read and dropped, never added
    red = ops._lib.REDUCE[reduce]
    y, win = ops._raw_spmm_edge(g, Xd, M, None, None, red, reduce == "max")
    assert torch.equal(ops.spmm_edge(g, Xd, M, reduce), y)
    assert torch.equal(y, ops.spmm(g, Xd, reduce))
    if reduce == "max":
        want, want_win = ops._raw_spmm(g, Xd, red, want_argmax=True)
        assert torch.equal(y, want) and torch.equal(win, want_win)


def test_operand_checks(dev):
    import graphgym_amd as ga
    from graphgym_amd import ops
    g, X, M, T, b, _ = _op_case(dev, 64, True, seed=1)
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(TypeError, match="float32 only"):
            ops.spmm_edge(g, X.to(dev).to(dt), M.to(dev).to(dt), "max")
        with pytest.raises(TypeError, match="float32 only"):
            ops.spmm_edge(g, X.to(dev), M.to(dev).to(dt), "sum")
        with pytest.raises(TypeError, match="float32 only"):
            ops.spmm_edge(g, X.to(dev), M.to(dev), "sum", t=T.to(dev).to(dt))
    with pytest.raises(ValueError, match="rows"):
        ops.spmm_edge(g, X.to(dev), M[:100].to(dev), "sum")            # fewer rows than the largest input position
    plain = ga.CSRGraph.from_csr(g.rowptr, g.col, None, g.num_nodes)   # no eid
    with pytest.raises(ValueError, match="eid"):
        ops.spmm_edge(plain, X.to(dev), M.to(dev), "sum")


def test_opcheck(dev):
    from graphgym_amd import ops
    g, X, M, T, b, dy = _op_case(dev, 32, True, seed=2)
    h = g.handle
    t = lambda v, grad=True: v.to(dev).requires_grad_(grad)        # noqa: E731
    win = ops._raw_spmm_edge(g, X.to(dev), M.to(dev), T.to(dev), None, ops._lib.MAX, True)[1]
    none = torch.empty(0, dtype=torch.int32, device=dev)
    cases = [
        (torch.ops.mp.spmm_edge.default, (t(X), t(M), t(T), t(b), h, 0)),
        (torch.ops.mp.spmm_edge.default, (t(X), t(M), None, None, h, 1)),
        (torch.ops.mp.spmm_edge.default, (t(X), t(M), t(T), t(b), h, 2)),
        (torch.ops.mp.spmm_edge_raw.default, (t(X, False), t(M, False), t(T, False), None, h, 2, True)),
        (torch.ops.mp.spmm_edge_raw.default, (t(X, False), t(M, False), None, t(b, False), h, 0, False)),
        (torch.ops.mp.spmm_edge_bwd_raw.default, (t(dy, False), none, h, 1, M.size(0))),
        (torch.ops.mp.spmm_edge_bwd_raw.default, (t(dy, False), win, h, 2, M.size(0))),
        (torch.ops.mp.spmm_edge_dt_raw.default, (t(dy, False), none, h, 1)),
        (torch.ops.mp.spmm_edge_dt_raw.default, (t(dy, False), win, h, 2)),
    ]
    for op, args in cases:
        res = torch.library.opcheck(op, args, raise_exception=True)
        assert all(v == "SUCCESS" for v in res.values()), (op, res)


# ---- layers -------------------------------------------------------------------------------------------------------

# (dim_in, dim_out) by self_msg: 'add' needs equal widths; 32 -> 64 aggregates first, 48 -> 32 and 32 -> 32 transform first
DIMS = {"none": (32, 64), "add": (32, 32), "concat": (48, 32)}


def _layer_edges(n, normalize, seed):
    """normalize_adj: every node's self loop is in the input (once, closing the edge list in node order), so
    add_remaining_self_loops inserts nothing and leaves every edge in its place"""
    ei = _graph_edges(n, seed)
    if normalize:
        ei = torch.cat([ei[:, ei[0] != ei[1]], torch.arange(n).repeat(2, 1)], dim=1)
    return ei


def _set_cfg(monkeypatch, agg, msg_direction, self_msg, normalize, edge_dim, keep_edge=0.5):
    from graphgym_amd.config import cfg
    monkeypatch.setattr(cfg.gnn, "agg", agg)
    monkeypatch.setattr(cfg.gnn, "msg_direction", msg_direction)
    monkeypatch.setattr(cfg.gnn, "self_msg", self_msg)
    monkeypatch.setattr(cfg.gnn, "normalize_adj", normalize)
    monkeypatch.setattr(cfg.gnn, "keep_edge", keep_edge)
    monkeypatch.setattr(cfg.dataset, "edge_dim", edge_dim)


def _spy_argmax(monkeypatch):
    from graphgym_amd import ops
    seen = {}
    real = ops._raw_spmm_edge

    def spy(g, *a, **k):
        y, am = real(g, *a, **k)
        seen["g"], seen["win"] = g, am
        return y, am
    monkeypatch.setattr(ops, "_raw_spmm_edge", spy)
    return seen


def _check_layer(layer, out, xd, efd, x, ef, ei, dy, agg, msg_direction, self_msg, normalize, seen, what):
    """out and the gradients already accumulated on xd, efd and the layer's parameters, against the restatement on the
    edges ei with the feature rows ef"""
    n = x.size(0)
    win = None
    if agg == "max":
        # engine entry -> its input edge, the restatement's index
        e_of = seen["g"].eid.cpu().long()
        w = seen["win"].cpu().long()
        win = torch.where(w >= 0, e_of[w.clamp(min=0)], w)
    params = {k: v.detach().cpu() for k, v in layer.named_parameters()}

    def fn(c, sign=lambda t: t):
        xr, er = (sign(c(t)).detach().clone().requires_grad_(True) for t in (x, ef))
        pr = {k: sign(c(v)).detach().clone().requires_grad_(True) for k, v in params.items()}
        norm = R.norm_edges(ei, n, xr.dtype) if normalize else None
        o = R.edge_conv(xr, er, ei, norm, pr["linear_msg.weight"], pr.get("linear_self.weight"), pr.get("bias"),
                        msg_direction, self_msg, agg, win)
        (o * sign(c(dy))).sum().backward()
        return [o.detach(), xr.grad, er.grad] + [pr[k].grad for k in params]
    r64, r32 = both(fn)
    m64 = mag_of(lambda c: fn(c, torch.abs))
    close(out.detach(), (r64[0], r32[0]), what=what + " y", mag=m64[0])
    close(xd.grad, (r64[1], r32[1]), what=what + " dx", mag=m64[1])
    close(efd.grad, (r64[2], r32[2]), what=what + " def", mag=m64[2])
    grads = dict(layer.named_parameters())
    for k, g64, g32 in zip(params, r64[3:], r32[3:]):
        close_all(grads[k].grad, (g64, g32), what=f"{what} d{k}")


@pytest.mark.parametrize("edge_dim", [1, 8, 128])
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("self_msg", ["none", "add", "concat"])
@pytest.mark.parametrize("msg_direction", ["single", "both"])
@pytest.mark.parametrize("agg", ["add", "mean", "max"])
def test_generaledgeconv_layer(dev, monkeypatch, agg, msg_direction, self_msg, normalize, edge_dim):
    import graphgym_amd.graphgym_plugin as plugin
    from graphgym_amd.harness import Batch
    _set_cfg(monkeypatch, agg, msg_direction, self_msg, normalize, edge_dim)
    n, (din, dout), seed = 300, DIMS[self_msg], 3
    ei = _layer_edges(n, normalize, seed)
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(n, din, generator=gen) * 2 - 1
    ef = torch.rand(ei.size(1), edge_dim, generator=gen) * 2 - 1
    dy = torch.rand(n, dout, generator=gen) * 2 - 1
    torch.manual_seed(seed)
    layer = plugin.EDGE_KEYS["generaledgeconv"](din, dout, bias=True).to(dev)
    with torch.no_grad():
        layer.model.bias.uniform_(-0.5, 0.5)                      # a live bias
    seen = _spy_argmax(monkeypatch)
    xd, efd = x.to(dev).requires_grad_(True), ef.to(dev).requires_grad_(True)
    out = layer(Batch(node_feature=xd, edge_index=ei.to(dev), edge_feature=efd)).node_feature
    (out * dy.to(dev)).sum().backward()
    assert ("win" in seen) == (agg == "max")                      # add / mean never reach the two-gather kernel
    what = f"edgeconv {agg} {msg_direction} self={self_msg} norm={normalize} k={edge_dim}"
    _check_layer(layer.model, out, xd, efd, x, ef, ei, dy, agg, msg_direction, self_msg, normalize, seen, what)


@pytest.mark.parametrize("agg", ["add", "max"])
def test_generalsampleedgeconv_follows_the_cpu_generator(dev, monkeypatch, agg):
    import graphgym_amd.graphgym_plugin as plugin
    from graphgym_amd.harness import Batch
    _set_cfg(monkeypatch, agg, "both", "concat", False, 8, keep_edge=0.6)
    n, din, dout, seed = 300, 32, 64, 5
    ei = _layer_edges(n, False, seed)
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(n, din, generator=gen) * 2 - 1
    ef = torch.rand(ei.size(1), 8, generator=gen) * 2 - 1
    dy = torch.rand(n, dout, generator=gen) * 2 - 1
    layer = plugin.EDGE_KEYS["generalsampleedgeconv"](din, dout, bias=True).to(dev)
    seen = _spy_argmax(monkeypatch)
    xd, efd = x.to(dev).requires_grad_(True), ef.to(dev).requires_grad_(True)
    torch.manual_seed(17)
    out = layer(Batch(node_feature=xd, edge_index=ei.to(dev), edge_feature=efd)).node_feature
    (out * dy.to(dev)).sum().backward()
    torch.manual_seed(17)
    mask = torch.rand(ei.size(1)) < 0.6                           # layer.py:216
    assert 0 < int(mask.sum()) < ei.size(1)
    ef_grad_full = efd.grad
    assert bool((ef_grad_full.cpu()[~mask] == 0).all())           # dropped edges take no part
    efd_kept = ef[mask].to(dev).requires_grad_(True)
    efd_kept.grad = ef_grad_full[mask.to(dev)]
    _check_layer(layer.model, out, xd, efd_kept, x, ef[mask], ei[:, mask], dy, agg, "both", "concat", False, seen,
                 f"sampleedgeconv {agg}")


def test_edge_feature_must_line_up_with_the_entries(dev, monkeypatch):
    from graphgym_amd.edgeconv import GeneralEdgeConvLayer
    n = 300
    for agg in ("add", "max"):
        _set_cfg(monkeypatch, agg, "single", "none", True, 8)
        layer = GeneralEdgeConvLayer(32, 64).to(dev)
        x = torch.rand(n, 32, device=dev)
        ei = _graph_edges(n, 3).to(dev)                           # most nodes have no self loop: loops are inserted
        with pytest.raises(RuntimeError, match="the reference fails here too"):
            layer(x, ei, edge_feature=torch.rand(ei.size(1), 8, device=dev))
        ok = _layer_edges(n, True, 3).to(dev)
        layer(x, ok, edge_feature=torch.rand(ok.size(1), 8, device=dev))
        with pytest.raises(RuntimeError, match="the reference fails here too"):
            layer(x, ok, edge_feature=torch.rand(ok.size(1) - 1, 8, device=dev))
        twice = ok.clone()
        twice[:, -1] = 0                                          # node 0's loop twice, the last node's never:
        with pytest.raises(RuntimeError, match="the reference fails here too"):    # as many entries as edges, one inserted
            layer(x, twice, edge_feature=torch.rand(ok.size(1), 8, device=dev))
        _set_cfg(monkeypatch, agg, "single", "none", False, 8)
        layer = GeneralEdgeConvLayer(32, 64).to(dev)
        with pytest.raises(RuntimeError, match="the reference fails here too"):
            layer(x, ei, edge_feature=torch.rand(ei.size(1) + 1, 8, device=dev))


def test_cached_layer_checks_the_edge_count(dev, monkeypatch):
    from graphgym_amd.edgeconv import GeneralEdgeConvLayer
    _set_cfg(monkeypatch, "max", "single", "none", False, 8)
    layer = GeneralEdgeConvLayer(32, 64, cached=True).to(dev)
    x = torch.rand(300, 32, device=dev)
    ei = _graph_edges(300, 3).to(dev)
    ef = torch.rand(ei.size(1), 8, device=dev)
    a = layer(x, ei, edge_feature=ef)
    assert layer.cached_result is not None and torch.equal(layer(x, ei, edge_feature=ef), a)
    with pytest.raises(RuntimeError, match="Cached {} number of edges, but found {}".format(ei.size(1), ei.size(1) - 1)):
        layer(x, ei[:, :-1], edge_feature=ef[:-1])


def test_bf16_refused(dev, monkeypatch):
    import graphgym_amd.graphgym_plugin as plugin
    from graphgym_amd.harness import Batch
    _set_cfg(monkeypatch, "max", "single", "none", False, 8)
    for key in plugin.EDGE_KEYS:
        layer = plugin.EDGE_KEYS[key](8, 16).to(dev)
        batch = Batch(node_feature=torch.rand(50, 8, device=dev, dtype=torch.bfloat16),
                      edge_index=torch.randint(0, 50, (2, 200), device=dev),
                      edge_feature=torch.rand(200, 8, device=dev, dtype=torch.bfloat16))
        with pytest.raises(TypeError, match="generaledgeconv and generalsampleedgeconv"):
            layer(batch)


@pytest.mark.parametrize("agg", ["add", "max"])
@pytest.mark.parametrize("key", ["generaledgeconv", "generalsampleedgeconv"])
def test_graphgym_stack_trains(dev, monkeypatch, key, agg):
    from graphgym_amd import harness as H
    from graphgym_amd.config import cfg
    import graphgym_amd.graphgym_plugin  # noqa: F401
    from test_harness_gpu import make_batch
    for k, v in (("layer_type", key), ("layers_mp", 2), ("dim_inner", 16), ("layers_pre_mp", 1), ("agg", agg),
                 ("normalize_adj", False), ("msg_direction", "both"), ("self_msg", "concat"), ("keep_edge", 0.8),
                 ("batchnorm", True)):
        monkeypatch.setattr(cfg.gnn, k, v)
    monkeypatch.setattr(cfg.dataset, "edge_dim", 8)
    batch, _ = make_batch(dev, seed=2)
    batch.edge_feature = torch.rand(batch.edge_index.size(1), 8, generator=torch.Generator().manual_seed(1)).to(dev)
    x0 = batch.node_feature.clone()
    torch.manual_seed(0)
    model = H.GNNStack(6, 4).to(dev)
    assert any("BatchNorm" in type(m).__name__ for m in model.modules())
    opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4)

    def fl():
        batch.node_feature = x0
        pred, true = model(batch)
        return torch.nn.functional.cross_entropy(pred, true)
    losses = [float(H.train_step(model, opt, fl)) for _ in range(5)]
    assert np.isfinite(losses).all(), losses
    if key == "generaledgeconv":                                  # (the sampled key sees another graph every step)
        assert losses[-1] < losses[0], losses


# ---- no per-entry tensor ------------------------------------------------------------------------------------------
# N = 2e4, E = 2e6, dim_in = dim_out = 64, edge_dim = 8: the operands take 69 MB, one [E, 64] tensor 512 MB.  The bounds
# are a condition on the design: add / mean may not allocate anything of that size, max the edge term M and its gradient
# and nothing else.
@pytest.mark.parametrize("agg,budget", [("add", 0.5), ("mean", 0.5), ("max", 2.5)])
def test_no_per_entry_tensor(dev, monkeypatch, agg, budget):
    from graphgym_amd.edgeconv import GeneralEdgeConvLayer
    from graphgym_amd.harness import Batch
    _set_cfg(monkeypatch, agg, "both", "concat", False, 8)
    n, E, d = 20000, 2000000, 64
    gen = torch.Generator().manual_seed(0)
    ei = torch.randint(0, n, (2, E), generator=gen).to(dev)
    x = (torch.rand(n, d, generator=gen) * 2 - 1).to(dev).requires_grad_(True)
    ef = (torch.rand(E, 8, generator=gen) * 2 - 1).to(dev).requires_grad_(True)
    torch.manual_seed(0)
    layer = GeneralEdgeConvLayer(d, d).to(dev)
    batch = Batch(node_feature=x, edge_index=ei, edge_feature=ef)

    def step():
        layer(x, ei, edge_feature=ef, holder=batch).sum().backward()
    step()                                                        # builds and caches the graph, its plan and transposes
    nnz = batch._mp_graph_cache[(1, "none", None, 1.0)].nnz
    assert nnz == E
    for t in [x, ef] + list(layer.parameters()):
        t.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - base
    print(f"agg={agg}: peak rise {rise / 2 ** 20:.1f} MiB, budget {budget * nnz * d * 4 / 2 ** 20:.1f} MiB")
    assert rise < budget * nnz * d * 4, (agg, rise)
