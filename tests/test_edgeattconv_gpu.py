"""generaledgeattconvv1 / generaledgeattconvv2 (graphgym/contrib/layer/attconv.py:243-543) and the two operators under them
(ops.edge_att_alpha, ops.spmm_edge_heads), against the float64 restatement of tests/_edgeatt_ref.py at the tolerances of
tests/_tol.py: 1e-5 per output row (rules (a), (b), (d)), one scale per tensor for parameter gradients.  Max gradients are
evaluated at the engine's argmax (a near-tie cannot flip a winner between the two evaluations); the max VALUES are
checked against the restatement's own amax."""
import pytest
import torch

import _edgeatt_ref as R
from _tol import both, close, close_all, mag_of

pytestmark = pytest.mark.gpu

LONG = 2100      # one destination above kSmLong = 2048: the whole-workgroup tier of the row softmax


def _graph_edges(n=300, seed=0, long_row=True):
    """[2, E] source -> destination, the recipe of test_attconv_gpu._graph_edges (isolated destinations, one entry three
    times, self loops on some nodes, a hub destination of 200 entries cut into pieces under PLAN_CONFIG (64, 1, 64, 64))
    plus one destination of 2 100 entries, in a shuffled input order: eid is not the identity"""
    g = torch.Generator().manual_seed(seed)
    m = 4 * n
    src = torch.randint(0, n, (m,), generator=g)
    dst = torch.randint(0, n, (m,), generator=g)
    keep = dst % 7 != 3                                      # rows 3, 10, 17, ... receive nothing
    src, dst = src[keep], dst[keep]
    hub_src = torch.randint(0, n, (200,), generator=g)
    rep = torch.tensor([[5, 5, 5, 8], [1, 1, 1, 1]])         # entry (1 <- 5) three times
    parts = [torch.stack([src, dst]), torch.stack([hub_src, torch.zeros(200, dtype=torch.long)]), rep]
    if long_row:
        parts.append(torch.stack([torch.randint(0, n, (LONG,), generator=g), torch.full((LONG,), 2)]))
    ei = torch.cat(parts, dim=1)
    return ei[:, torch.randperm(ei.size(1), generator=g)]


@pytest.fixture
def hub_plan(monkeypatch):
    import graphgym_amd as ga
    monkeypatch.setenv("MP_AGG_TILES", "0")
    monkeypatch.setattr(ga.CSRGraph, "PLAN_CONFIG", (64, 1, 64, 64))


def _struct(g):
    return g.row_ids().cpu().long(), g.col.cpu().long(), g.eid.cpu().long()


def _graph(dev, seed, **build):
    import graphgym_amd as ga
    n = 300
    ei = _graph_edges(n, seed)
    g = ga.CSRGraph.from_edge_index(ei.to(dev), n, **build)
    return g, ei


def _check_row_tiers(g):
    deg = torch.diff(g.rowptr.cpu())
    assert int(deg.max()) > 2048 and bool(((deg > 16) & (deg <= 2048)).any()) and bool(((deg > 0) & (deg <= 16)).any())
    assert g.plan()[1][2] > 0                                 # hub rows run in pieces
    assert not torch.equal(g.eid.cpu().long(), torch.arange(g.nnz))


def _dev(t, dev, grad=False):
    return None if t is None else t.to(dev).requires_grad_(grad)


# ---- ops.edge_att_alpha ---------------------------------------------------------------------------------------------

def _softmax_terms(alpha64, dl64, rows, n):
    """|alpha_e| (|dalpha_e| + sum_row |alpha dalpha|): the absolute terms of a softmax row's gradient"""
    rowdot = torch.zeros(n, alpha64.size(1), dtype=torch.float64).index_add_(0, rows, (alpha64 * dl64).abs())
    return alpha64.abs() * (dl64.abs() + rowdot[rows])


def _alpha_check(dev, g, E, heads, has_dst, seed, what):
    from graphgym_amd import ops
    n = g.num_nodes
    rows, cols, eids = _struct(g)
    gen = torch.Generator().manual_seed(seed)
    a_dst = torch.randn(n, heads, generator=gen) if has_dst else None
    a_src = torch.randn(n, heads, generator=gen)
    a_edge = torch.randn(E + 3, heads, generator=gen)         # three rows no entry points at
    dl = torch.randn(g.nnz, heads, generator=gen)
    dd, sd, ed = _dev(a_dst, dev, True), _dev(a_src, dev, True), _dev(a_edge, dev, True)
    alpha = ops.edge_att_alpha(g, dd, sd, ed, 0.2)
    assert alpha.shape == (g.nnz, heads)
    (alpha * dl.to(dev)).sum().backward()

    def fn(c):
        leaf = lambda t: None if t is None else c(t).detach().clone().requires_grad_(True)    # noqa: E731
        ad, asr, ae = leaf(a_dst), leaf(a_src), leaf(a_edge)
        al = R.edge_att_alpha(rows, cols, eids, ad, asr, ae, n, 0.2)
        (al * c(dl)).sum().backward()
        return [al.detach(), asr.grad, ae.grad] + ([ad.grad] if ad is not None else [])
    r64, r32 = both(fn)
    close(alpha.detach(), (r64[0], r32[0]), what=what + " alpha")
    # the gradients sum terms of either sign (the softmax backward cancels by construction): held to 1e-5 of the sums
    # of their absolute terms with lrelu' <= 1 (tests/_tol.py rule (d))
    terms = _softmax_terms(r64[0], dl.double(), rows, n)
    zero = torch.zeros(n, heads, dtype=torch.float64)
    has = eids >= 0
    mag_e = torch.zeros(E + 3, heads, dtype=torch.float64)
    mag_e[eids[has]] = terms[has]
    close(sd.grad, (r64[1], r32[1]), what=what + " d_src", mag=zero.index_add(0, cols, terms))
    close(ed.grad, (r64[2], r32[2]), what=what + " d_edge", mag=mag_e)
    absent = torch.ones(E + 3, dtype=torch.bool)
    absent[eids[has]] = False
    assert int(absent.sum()) >= 3 and bool((ed.grad.cpu()[absent] == 0).all())
    if has_dst:
        close(dd.grad, (r64[3], r32[3]), what=what + " d_dst", mag=zero.index_add(0, rows, terms))


@pytest.mark.parametrize("has_dst", [True, False], ids=["dst", "nodst"])
@pytest.mark.parametrize("heads", [1, 2, 3, 4, 8])
def test_edge_att_alpha(dev, hub_plan, heads, has_dst):
    g, ei = _graph(dev, seed=heads)
    _check_row_tiers(g)
    _alpha_check(dev, g, ei.size(1), heads, has_dst, 10 + heads, f"alpha H={heads} dst={has_dst}")


@pytest.mark.parametrize("heads", [1, 4])
def test_edge_att_alpha_entries_without_an_input_edge(dev, hub_plan, heads):
    """loops="remaining" on an edge list where most nodes lack a loop: the self entries (eid < 0) score without an edge
    term, and the rows of a_edge of the loops that were replaced receive no gradient"""
    from graphgym_amd.layers import get_graph
    n = 300
    ei = _graph_edges(n, 4)
    assert 0 < int((ei[0] == ei[1]).sum()) < n
    g = get_graph(None, ei.to(dev), n, loops="remaining")
    assert int((g.eid < 0).sum()) == n
    _alpha_check(dev, g, ei.size(1), heads, True, 20 + heads, f"alpha loops H={heads}")


# ---- ops.spmm_edge_heads --------------------------------------------------------------------------------------------

HEAD_CASES = [(h, d) for h in (1, 2, 4, 8) for d in (64, 256)] + [(3, 48), (6, 48)]


def _count_per_head_launches(monkeypatch):
    """count the calls of the per-head entry from here on"""
    from graphgym_amd import ops
    calls, real = [], ops._raw_spmm_edge

    def spy(*a, **k):
        calls.append(1)
        return real(*a, **k)
    monkeypatch.setattr(ops, "_raw_spmm_edge", spy)
    return calls


def _op_case(dev, heads, d, has_t, seed, **build):
    g, ei = _graph(dev, seed, **build)
    gen = torch.Generator().manual_seed(seed + 1)
    n = g.num_nodes
    t = {"w": torch.rand(g.nnz, heads, generator=gen) * 2 - 0.5, "x": torch.rand(n, d, generator=gen) * 2 - 1,
         "m": torch.rand(ei.size(1) + 3, d, generator=gen) * 2 - 1,
         "t": torch.rand(n, d, generator=gen) * 2 - 1 if has_t else None, "bias": torch.rand(d, generator=gen) - 0.5}
    dy = torch.rand(n, d, generator=gen) * 2 - 1
    return g, t, dy


def _refuses_one_launch(dev, g, t, heads, d):
    """the C entry itself returns MP_ERR_UNSUPPORTED for this head count"""
    from graphgym_amd import ops
    plan, counts, ws, ws_bytes = ops._plan_ws(g, dev, d, 0, False)
    x, m, w = t["x"].to(dev), t["m"].to(dev), t["w"].to(dev)
    y = torch.empty_like(x)
    return ops.lib().mp_spmm_csr_edge_heads_f32(ops.ptr(g.rowptr), ops.ptr(g.col), ops.ptr(g.eid), ops.ptr(w),
                                                g.num_nodes, ops.ptr(plan), counts, heads, ops.ptr(x), d, ops.ptr(m), d,
                                                None, 0, ops.ptr(y), d, d, 0, None, None, ops.ptr(ws), ws_bytes, None)


def _heads_check(dev, g, t, dy, heads, reduce, what, make=lambda v, dev: v.to(dev)):
    """forward and the five gradients of ops.spmm_edge_heads on the operands t (made device tensors by `make`) against the
    restatement; returns the engine's (y, dw, dm)"""
    from graphgym_amd import ops
    rows, cols, eids = _struct(g)
    n = g.num_nodes
    d = {k: (None if v is None else make(v, dev).detach().requires_grad_(True)) for k, v in t.items()}
    y = ops.spmm_edge_heads(g, d["w"], d["x"], d["m"], t=d["t"], heads=heads, reduce=reduce, bias=d["bias"])
    (y * dy.to(dev)).sum().backward()

    def fwd(c, sign=lambda v: v, win=None):
        o = lambda v: None if v is None else sign(c(v))          # noqa: E731
        return R.edge_heads_agg(rows, cols, eids, o(t["w"]), o(t["x"]), o(t["m"]), o(t["t"]), o(t["bias"]), n, heads,
                                reduce, win)
    close(y.detach(), both(fwd), what=what + " y", mag=mag_of(lambda c: fwd(c, torch.abs)))
    win = None
    if reduce == "max":
        dv = {k: (None if v is None else v.to(dev)) for k, v in t.items()}
        win = ops._raw_spmm_edge_heads(g, dv["w"], dv["x"], dv["m"], dv["t"], dv["bias"], heads, ops._lib.MAX, True)[1].cpu()
        deg = torch.diff(g.rowptr.cpu())
        assert bool((win[deg > 0] >= 0).all()) and bool((win[deg == 0] == -1).all()) and bool((win < g.nnz).all())
    names = [k for k in ("w", "x", "m", "t", "bias") if t[k] is not None]

    def grads(c, sign=lambda v: v):
        leaf = {k: (None if t[k] is None else sign(c(t[k])).detach().clone().requires_grad_(True)) for k in t}
        out = R.edge_heads_agg(rows, cols, eids, leaf["w"], leaf["x"], leaf["m"], leaf["t"], leaf["bias"], n, heads,
                               reduce, win)
        (out * sign(c(dy))).sum().backward()
        return [leaf[k].grad for k in names]
    g64, g32 = both(grads)
    m64 = mag_of(lambda c: grads(c, torch.abs))
    for k, r64, r32, mg in zip(names, g64, g32, m64):
        if k == "bias":
            close_all(d[k].grad, (r64, r32), what=f"{what} dbias")
        else:
            close(d[k].grad, (r64, r32), what=f"{what} d{k}", mag=mg)
    # input edges the operator does not hold get exactly zero
    absent = torch.ones(t["m"].size(0), dtype=torch.bool)
    absent[eids[eids >= 0]] = False
    assert int(absent.sum()) >= 3 and bool((d["m"].grad.cpu()[absent] == 0).all())
    return y.detach(), d["w"].grad, d["m"].grad


@pytest.mark.parametrize("has_t", [True, False], ids=["t", "not"])
@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
@pytest.mark.parametrize("heads,d", HEAD_CASES)
def test_spmm_edge_heads(dev, hub_plan, monkeypatch, heads, d, reduce, has_t):
    g, t, dy = _op_case(dev, heads, d, has_t, seed=heads * 31 + d)
    _check_row_tiers(g)
    if heads in (3, 6):
        assert _refuses_one_launch(dev, g, t, heads, d) == 2      # the per-head path ran
    calls = _count_per_head_launches(monkeypatch)
    _heads_check(dev, g, t, dy, heads, reduce, f"edge_heads {reduce} H={heads} d={d} t={has_t}")
    # the operator's forward and, for max, the argmax run of the check: 2, 4 and 8 heads take the one-launch kernel, the
    # other head counts one launch of mp_spmm_csr_edge_f32 per head
    assert len(calls) == (0 if heads in (2, 4, 8) else (1 + (reduce == "max")) * heads), len(calls)


@pytest.mark.parametrize("heads,d", [(1, 64), (2, 64), (4, 64), (8, 64), (3, 48), (6, 48)])
def test_max_ties_go_to_the_first_csr_entry(dev, hub_plan, heads, d):
    """integer-valued X, M, T and weights: every product and sum is exact in float32, equal candidates are exactly equal
    (repeated entries, eight sources only), and the winner is the first of them in CSR order"""
    import graphgym_amd as ga
    from graphgym_amd import ops
    n = 200
    gen = torch.Generator().manual_seed(7)
    src = torch.randint(0, n, (1600,), generator=gen) % 8         # eight sources only: many repeats per row
    dst = torch.randint(0, n, (1600,), generator=gen)
    dst[:150] = 0                                                  # a hub row in pieces
    g = ga.CSRGraph.from_edge_index(torch.stack([src, dst]).to(dev), n)
    assert g.plan()[1][2] > 0
    w = torch.randint(1, 3, (g.nnz, heads), generator=gen).float()
    X = torch.randint(-2, 3, (n, d), generator=gen).float()
    M = torch.randint(-1, 2, (1600, d), generator=gen).float()
    T = torch.randint(-2, 3, (n, d), generator=gen).float()
    y, win = ops._raw_spmm_edge_heads(g, w.to(dev), X.to(dev), M.to(dev), T.to(dev), None, heads, ops._lib.MAX, True)
    rows, cols, eids = _struct(g)
    msg = w.repeat_interleave(d // heads, dim=1) * ((X[cols] + M[eids]) + T[rows])     # float32, exact
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
@pytest.mark.parametrize("heads", [1, 4, 3])
def test_inserted_self_loops_carry_no_edge_term(dev, hub_plan, reduce, heads):
    """add_self_loops: one entry per node with eid < 0, which contributes w (X[r] + T[r]) only: its row of dm stays zero
    (there is none) and the M term of its dw is zero — both are in the restatement the gradients are held against"""
    d = 48
    g, t, dy = _op_case(dev, heads, d, True, seed=11 + heads, add_self_loops=True)
    assert int((g.eid < 0).sum()) == g.num_nodes
    _heads_check(dev, g, t, dy, heads, reduce, f"edge_heads loops {reduce} H={heads}")
    # dw of an inserted loop is <dy[r], X[r] + T[r]>_h whatever M holds
    from graphgym_amd import ops
    loop = (g.eid < 0).cpu()
    wd = t["w"].to(dev).requires_grad_(True)
    y = ops.spmm_edge_heads(g, wd, t["x"].to(dev), t["m"].to(dev), t=t["t"].to(dev), heads=heads, reduce="sum")
    (y * dy.to(dev)).sum().backward()
    rows = g.row_ids().cpu().long()
    hw = d // heads
    x64, t64, dy64 = t["x"].double(), t["t"].double(), dy.double()
    want = (dy64 * (x64 + t64)).view(-1, heads, hw).sum(-1)[rows][loop]
    mag = (dy64.abs() * (x64.abs() + t64.abs())).view(-1, heads, hw).sum(-1)[rows][loop]
    close(wd.grad.cpu()[loop], want, what=f"dw of inserted loops H={heads}", mag=mag)


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
@pytest.mark.parametrize("heads,d", [(1, 64), (4, 64), (3, 48)])
def test_two_runs_are_bit_equal(dev, hub_plan, reduce, heads, d):
    from graphgym_amd import ops
    g, t, dy = _op_case(dev, heads, d, True, seed=3)

    def run():
        v = {k: x.to(dev).requires_grad_(True) for k, x in t.items()}
        y = ops.spmm_edge_heads(g, v["w"], v["x"], v["m"], t=v["t"], heads=heads, reduce=reduce, bias=v["bias"])
        (y * dy.to(dev)).sum().backward()
        return [y.detach(), v["m"].grad, v["w"].grad]
    for a, c in zip(run(), run()):
        assert torch.equal(a, c)


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
@pytest.mark.parametrize("heads,d", [(4, 64), (8, 256), (3, 48)])
def test_operand_views(dev, hub_plan, reduce, heads, d):
    """x, m and t as column windows of wider buffers: leading dimension d + 5, first element 4 bytes past a 16-byte
    boundary (one column per lane, ld > d); the forward gives the bits of the dense operands, the gradients hold"""
    from graphgym_amd import ops
    g, t, dy = _op_case(dev, heads, d, True, seed=d + heads)

    def window(v, dev):
        if v.dim() != 2 or v.size(1) != d:
            return v.to(dev)
        big = torch.full((v.size(0), d + 5), float("nan"), device=dev)
        big[:, 1:1 + d] = v.to(dev)
        out = big[:, 1:1 + d]
        assert out.stride() == (d + 5, 1) and out.data_ptr() % 16 == 4
        return out
    dv = {k: v.to(dev) for k, v in t.items()}
    want = ops.spmm_edge_heads(g, dv["w"], dv["x"], dv["m"], t=dv["t"], heads=heads, reduce=reduce, bias=dv["bias"])
    y, _, _ = _heads_check(dev, g, t, dy, heads, reduce, f"edge_heads views {reduce} H={heads} d={d}", make=window)
    assert torch.equal(y, want)


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
@pytest.mark.parametrize("heads,d", [(2, 64), (4, 256), (8, 64)])
def test_the_two_forms_give_the_same_bits(dev, hub_plan, reduce, heads, d):
    """all heads in one launch and one launch per head add the same terms in the same order"""
    from graphgym_amd import ops
    g, t, _ = _op_case(dev, heads, d, True, seed=5)
    v = {k: x.to(dev) for k, x in t.items()}
    red = ops._lib.REDUCE[reduce]
    a = ops._raw_spmm_edge_heads(g, v["w"], v["x"], v["m"], v["t"], v["bias"], heads, red, reduce == "max", one_launch=True)
    b = ops._raw_spmm_edge_heads(g, v["w"], v["x"], v["m"], v["t"], v["bias"], heads, red, reduce == "max", one_launch=False)
    assert torch.equal(a[0], b[0])
    if reduce == "max":
        assert torch.equal(a[1], b[1])


def test_operand_checks(dev):
    import graphgym_amd as ga
    from graphgym_amd import ops
    g, t, _ = _op_case(dev, 4, 64, True, seed=1)
    v = {k: x.to(dev) for k, x in t.items()}
    for dt in (torch.bfloat16, torch.float16):
        with pytest.raises(TypeError, match="spmm_edge_heads is float32 only"):
            ops.spmm_edge_heads(g, v["w"], v["x"].to(dt), v["m"], heads=4)
        with pytest.raises(TypeError, match="spmm_edge_heads is float32 only"):
            ops.spmm_edge_heads(g, v["w"].to(dt), v["x"], v["m"], heads=4)
        with pytest.raises(TypeError, match="edge_att_alpha is float32 only"):
            ops.edge_att_alpha(g, None, v["w"][:300].to(dt), v["w"])
    with pytest.raises(ValueError, match="rows"):
        ops.spmm_edge_heads(g, v["w"], v["x"], v["m"][:100], heads=4)     # fewer rows than the largest input position
    with pytest.raises(ValueError, match="multiple of heads"):
        ops.spmm_edge_heads(g, v["w"][:, :3], v["x"], v["m"], heads=3)
    plain = ga.CSRGraph.from_csr(g.rowptr, g.col, None, g.num_nodes)       # no eid
    with pytest.raises(ValueError, match="eid"):
        ops.spmm_edge_heads(plain, v["w"], v["x"], v["m"], heads=4)


# ---- layers ---------------------------------------------------------------------------------------------------------

DIN, EDIM, DOUT = 32, 8, 64


def _layer_edges(n, normalize, seed):
    """normalize_adj: every node's self loop is in the input (once, closing the edge list in node order), so
    add_remaining_self_loops inserts nothing and leaves every edge in its place"""
    ei = _graph_edges(n, seed, long_row=False)
    if normalize:
        ei = torch.cat([ei[:, ei[0] != ei[1]], torch.arange(n).repeat(2, 1)], dim=1)
    return ei


def _set_cfg(monkeypatch, agg, msg_direction, heads, normalize, final=False, final_bn=False):
    from graphgym_amd.config import cfg
    monkeypatch.setattr(cfg.gnn, "agg", agg)
    monkeypatch.setattr(cfg.gnn, "msg_direction", msg_direction)
    monkeypatch.setattr(cfg.gnn, "att_heads", heads)
    monkeypatch.setattr(cfg.gnn, "normalize_adj", normalize)
    monkeypatch.setattr(cfg.gnn, "att_final_linear", final, raising=False)
    monkeypatch.setattr(cfg.gnn, "att_final_linear_bn", final_bn, raising=False)
    monkeypatch.setattr(cfg.dataset, "edge_dim", EDIM)


def _spy_argmax(monkeypatch):
    from graphgym_amd import ops
    seen = {}
    real = ops._raw_spmm_edge_heads

    def spy(g, *a, **k):
        y, am = real(g, *a, **k)
        seen["g"], seen["win"] = g, am
        return y, am
    monkeypatch.setattr(ops, "_raw_spmm_edge_heads", spy)
    return seen


def _run_layer(dev, monkeypatch, version, agg, msg_direction, heads, bias, normalize=False, final=False, final_bn=False,
               task_channels=None, state=None, seed=3):
    """one forward + backward of the Layer against the restatement: output, x.grad, edge_feature.grad, every parameter
    gradient.  state: reference-named tensors loaded into the layer before the run"""
    from graphgym_amd import edgeattconv as EA
    from graphgym_amd.config import cfg
    _set_cfg(monkeypatch, agg, msg_direction, heads, normalize, final, final_bn)
    n = 300
    ei = _layer_edges(n, normalize, seed)
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(n, DIN, generator=gen) * 2 - 1
    ef = torch.rand(ei.size(1), EDIM, generator=gen) * 2 - 1
    dy = torch.rand(n, DOUT, generator=gen) * 2 - 1
    task = torch.rand(task_channels, generator=gen) * 2 - 1 if task_channels else None
    torch.manual_seed(seed)
    Layer = EA.GeneralEdgeAttConvv1Layer if version == 1 else EA.GeneralEdgeAttConvv2Layer
    layer = Layer(DIN, DOUT, task_channels=task_channels, bias=bias)
    if state is not None:
        layer.load_state_dict(state, strict=True)
    layer = layer.to(dev).train()
    if state is None:
        with torch.no_grad():
            for p in layer.parameters():                           # non-zero biases: every term of the layer is live
                if p.dim() == 1:
                    p.uniform_(-0.5, 0.5)
    seen = _spy_argmax(monkeypatch)
    xd, efd = x.to(dev).requires_grad_(True), ef.to(dev).requires_grad_(True)
    out = layer(xd, ei.to(dev), edge_feature=efd, task_emb=None if task is None else task.to(dev))
    (out * dy.to(dev)).sum().backward()
    win = None
    if agg == "max":
        e_of = seen["g"].eid.cpu().long()                          # engine entry -> its input edge, the restatement's index
        w = seen["win"].cpu().long()
        win = torch.where(w >= 0, e_of[w.clamp(min=0)], w)
    ei_ref, norm = R.att_edges(ei, n, normalize)
    assert torch.equal(ei_ref, ei)
    params = {k: v.detach().cpu() for k, v in layer.named_parameters()}
    bn = (cfg.bn.eps, cfg.bn.mom) if final_bn else None
    args = (version, heads, agg, msg_direction)

    def fn(c):
        xr, er = (c(v).detach().clone().requires_grad_(True) for v in (x, ef))
        pr = {k: c(v).detach().clone().requires_grad_(True) for k, v in params.items()}
        o = R.edge_att_conv(xr, er, ei, None if norm is None else c(norm), pr, *args,
                            task_emb=None if task is None else c(task), bn=bn, win=win)
        (o * c(dy)).sum().backward()
        return [o.detach(), xr.grad, er.grad] + [pr[k].grad for k in params]
    r64, r32 = both(fn)
    p64 = {k: v.double() for k, v in params.items()}
    mag_x, mag_ef = R.input_magnitudes(x.double(), ef.double(), ei, norm, p64, *args, dy.double(),
                                       task_emb=None if task is None else task.double(), bn=bn, win=win)
    what = f"edgeattconvv{version} {agg} {msg_direction} H={heads} bias={bias} norm={normalize} final={final}/{final_bn}"
    close(out.detach(), (r64[0], r32[0]), what=what + " y")
    if agg == "max":     # the values once more against the restatement's own amax, not at the engine's winners

        def own_amax(c):
            with torch.no_grad():
                return R.edge_att_conv(c(x), c(ef), ei, None if norm is None else c(norm),
                                       {k: c(v) for k, v in params.items()}, *args,
                                       task_emb=None if task is None else c(task), bn=bn, win=None)
        close(out.detach(), both(own_amax), what=what + " y against the restatement's amax")
    # x.grad and edge_feature.grad sum terms of either sign (the softmax backward cancels by construction): held to 1e-5
    # of the sums of their absolute per-edge terms (tests/_tol.py rule (d))
    close(xd.grad, (r64[1], r32[1]), what=what + " dx", mag=mag_x)
    close(efd.grad, (r64[2], r32[2]), what=what + " def", mag=mag_ef)
    grads = dict(layer.named_parameters())
    for k, g64, g32 in zip(params, r64[3:], r32[3:]):
        if k.startswith("linear_key"):                             # constructed, never used (attconv.py:402-408)
            assert grads[k].grad is None and g64 is None, k
            continue
        close_all(grads[k].grad, (g64, g32), what=f"{what} d{k}")
    if version == 2:
        assert "linear_key.weight" in params
    return layer


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("heads", [1, 2, 4])
@pytest.mark.parametrize("agg", ["add", "mean", "max"])
@pytest.mark.parametrize("msg_direction", ["single", "both"])
@pytest.mark.parametrize("version", [1, 2])
def test_layer(dev, hub_plan, monkeypatch, version, msg_direction, agg, heads, bias):
    _run_layer(dev, monkeypatch, version, agg, msg_direction, heads, bias)


@pytest.mark.parametrize("version", [1, 2])
def test_layer_final_linear_and_batchnorm(dev, hub_plan, monkeypatch, version):
    """update(): training-mode BatchNorm, then the final linear, then the bias (attconv.py:362-370)"""
    _run_layer(dev, monkeypatch, version, "add", "both", 4, True, final=True, final_bn=True)


@pytest.mark.parametrize("version", [1, 2])
def test_layer_task_embedding(dev, hub_plan, monkeypatch, version):
    _run_layer(dev, monkeypatch, version, "max", "single", 2, True, task_channels=8)


@pytest.mark.parametrize("agg", ["add", "max"])
@pytest.mark.parametrize("version", [1, 2])
def test_layer_normalize_adj(dev, hub_plan, monkeypatch, version, agg):
    """an edge list that already holds every self loop matches; one that does not raises, as the reference fails"""
    from graphgym_amd import edgeattconv as EA
    _run_layer(dev, monkeypatch, version, agg, "both", 4, True, normalize=True)
    Layer = EA.GeneralEdgeAttConvv1Layer if version == 1 else EA.GeneralEdgeAttConvv2Layer
    layer = Layer(DIN, DOUT).to(dev)
    ei = _layer_edges(300, False, 3).to(dev)                      # most nodes have no self loop: loops are inserted
    with pytest.raises(RuntimeError, match="the reference fails here too"):
        layer(torch.rand(300, DIN, device=dev), ei, edge_feature=torch.rand(ei.size(1), EDIM, device=dev))


@pytest.mark.parametrize("msg_direction", ["single", "both"])
@pytest.mark.parametrize("version", [1, 2])
def test_state_dict_from_reference_names(dev, hub_plan, monkeypatch, version, msg_direction):
    """tensors named and shaped as the reference names them load strictly, and the layer computes the reference's formula
    with them: the column order [W_i | W_j | W_e] of the message linear"""
    gen = torch.Generator().manual_seed(9)
    k = (DIN if msg_direction == "single" else 2 * DIN) + EDIM
    r = lambda *s: torch.rand(*s, generator=gen) - 0.5            # noqa: E731
    if version == 1:
        state = {"linear_msg.weight": r(DOUT, k)}
    else:
        state = {"linear_value.weight": r(DOUT, k), "linear_value.bias": r(DOUT), "linear_key.weight": r(DOUT, k),
                 "linear_key.bias": r(DOUT)}
    state.update({"att_msg": r(1, 4, DOUT // 4), "bias": r(DOUT)})
    layer = _run_layer(dev, monkeypatch, version, "add", msg_direction, 4, True, state=state)
    for name, v in state.items():
        assert torch.equal(layer.state_dict()[name].cpu(), v), name


@pytest.mark.parametrize("agg", ["add", "max"])
@pytest.mark.parametrize("key", ["generaledgeattconvv1", "generaledgeattconvv2"])
def test_registered_keys_run_a_batch(dev, monkeypatch, key, agg):
    from graphgym_amd.harness import Batch
    from graphgym_amd.registry import layer_dict
    import graphgym_amd.graphgym_plugin  # noqa: F401
    _set_cfg(monkeypatch, agg, "both", 2, False)
    ei = _graph_edges(100, 1, long_row=False) % 100
    batch = Batch(node_feature=torch.rand(100, 8, device=dev), edge_index=ei.to(dev),
                  edge_feature=torch.rand(ei.size(1), EDIM, device=dev))
    layer = layer_dict[key](8, 16).to(dev)
    out = layer(batch).node_feature
    assert out.shape == (100, 16) and bool(torch.isfinite(out).all())
    assert (1, "none", None, 1.0) in batch._mp_graph_cache           # holder=batch: the graph is cached on the batch
