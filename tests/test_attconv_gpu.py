"""gaddconv / gmulconv (graphgym/contrib/layer/attconv.py) and the multi-head weighted mean / max under them, against
the float64 restatement of tests/_att_ref.py, at the tolerances of tests/_tol.py: 1e-5 per output row, per tensor for
parameter gradients.  Max gradients are evaluated at the engine's argmax (near-ties cannot flip a winner between the
two evaluations); the max VALUES are checked against the restatement's own amax."""
import numpy as np
import pytest
import torch

import _att_ref as R
from _tol import both, close, close_all, mag_of

pytestmark = pytest.mark.gpu


def _graph_edges(n=300, seed=0):
    """[2, E] source -> destination: isolated destinations, repeated entries, one hub destination of 200 entries (cut
    into pieces under PLAN_CONFIG (64, 1, 64, 64)), self loops on some nodes"""
    g = torch.Generator().manual_seed(seed)
    m = 4 * n
    src = torch.randint(0, n, (m,), generator=g)
    dst = torch.randint(0, n, (m,), generator=g)
    keep = dst % 7 != 3                                      # rows 3, 10, 17, ... receive nothing
    src, dst = src[keep], dst[keep]
    hub_src = torch.randint(0, n, (200,), generator=g)
    rep = torch.tensor([[5, 5, 5, 8], [1, 1, 1, 1]])         # entry (1 <- 5) three times
    ei = torch.cat([torch.stack([src, dst]), torch.stack([hub_src, torch.zeros(200, dtype=torch.long)]), rep], dim=1)
    return ei


@pytest.fixture
def hub_plan(monkeypatch):
    import graphgym_amd as ga
    monkeypatch.setenv("MP_AGG_TILES", "0")
    monkeypatch.setattr(ga.CSRGraph, "PLAN_CONFIG", (64, 1, 64, 64))


def _op_case(dev, heads, d, seed):
    import graphgym_amd as ga
    n = 300
    ei = _graph_edges(n, seed)
    g = ga.CSRGraph.from_edge_index(ei.to(dev), n)
    gen = torch.Generator().manual_seed(seed + 1)
    a = torch.rand(g.nnz, heads, generator=gen) * 2 - 0.5
    V = torch.rand(n, d, generator=gen) * 2 - 1
    dy = torch.rand(n, d, generator=gen) * 2 - 1
    rows, cols = g.row_ids().cpu().long(), g.col.cpu().long()
    return g, a, V, dy, rows, cols


CASES = [(h, d) for d in (48, 64, 256) for h in (1, 2, 3, 4, 6, 8) if d % h == 0 and (h in (1, 2, 4, 8) or d == 48)]
# d = 36 with 3 or 6 heads: 12 / 6 lanes per head, not a power of two — the masked da dot runs per head on column slices
CASES += [(3, 36), (6, 36)]
FALLBACK_DA = {(3, 36), (6, 36)}


@pytest.mark.parametrize("reduce", ["mean", "max"])
@pytest.mark.parametrize("heads,d", CASES)
def test_spmm_edge_values_reduce(dev, hub_plan, reduce, heads, d):
    from graphgym_amd import ops
    g, a, V, dy, rows, cols = _op_case(dev, heads, d, seed=heads * 31 + d)
    assert g.plan()[1][2] > 0                                # the hub row runs in pieces
    ad, Vd = a.to(dev).requires_grad_(True), V.to(dev).requires_grad_(True)
    y = ops.spmm_edge_values(g, ad, Vd, heads, reduce=reduce)
    (y * dy.to(dev)).sum().backward()
    n = g.num_nodes
    close(y.detach(), both(lambda c: R.edge_values_agg(rows, cols, c(a), c(V), n, heads, reduce)),
          what=f"{reduce} y H={heads} d={d}")
    win = None
    if reduce == "max":
        win = ops._raw_spmm_heads_reduce(g, a.to(dev), V.to(dev), heads, ops._lib.MAX)[1].cpu()
        assert bool((win[rows.unique()] >= 0).all()) and bool((win[torch.diff(g.rowptr.cpu()) == 0] == -1).all())
        if (heads, d) in FALLBACK_DA:     # the one-launch masked dot refuses this layout: the per-head path ran
            L, wd, s = ops.lib(), win.to(dev), torch.empty((g.nnz, heads), device=dev)
            assert L.mp_spmm_heads_max_da_f32(ops.ptr(g.row_ids()), ops.ptr(g.col), g.nnz, ops.ptr(wd), d,
                                              ops.ptr(dy.to(dev)), d, ops.ptr(V.to(dev)), d, d, heads, ops.ptr(s),
                                              None) == 2

    def grads(c, sign=lambda t: t):
        ar, Vr = sign(c(a)).detach().clone().requires_grad_(True), sign(c(V)).detach().clone().requires_grad_(True)
        (R.edge_values_agg(rows, cols, ar, Vr, n, heads, reduce, win) * sign(c(dy))).sum().backward()
        return ar.grad, Vr.grad
    g64, g32 = both(grads)
    # da and dV are sums of products of either sign (one dot product per entry and head): held to 1e-5 of their sums of
    # absolute terms (tests/_tol.py rule (d)), the same gradients evaluated on |a|, |V|, |dy|
    m64 = mag_of(lambda c: grads(c, torch.abs))
    close(ad.grad, (g64[0], g32[0]), what=f"{reduce} da H={heads} d={d}", mag=m64[0])
    close(Vd.grad, (g64[1], g32[1]), what=f"{reduce} dV H={heads} d={d}", mag=m64[1])


@pytest.mark.parametrize("heads,d", [(1, 64), (2, 64), (4, 64), (8, 64), (3, 48), (6, 48)])
def test_max_ties_go_to_the_first_csr_entry(dev, hub_plan, heads, d):
    """exactly equal candidates: repeated entries and distinct sources with equal rows of V under equal weights; 3 and 6
    heads run one launch per head on column slices"""
    from graphgym_amd import ops
    import graphgym_amd as ga
    n = 200
    gen = torch.Generator().manual_seed(7)
    src = torch.randint(0, n, (1600,), generator=gen) % 8         # eight sources only: many repeats per row
    dst = torch.randint(0, n, (1600,), generator=gen)
    dst[:150] = 0                                                  # a hub row in pieces
    g = ga.CSRGraph.from_edge_index(torch.stack([src, dst]).to(dev), n)
    V = torch.rand(n, d, generator=gen)
    V[4] = V[2]                                                   # sources 2 and 4 tie everywhere
    V[6, : d // 2] = V[1, : d // 2]
    a = torch.ones(g.nnz, heads)
    y, win = ops._raw_spmm_heads_reduce(g, a.to(dev), V.to(dev), heads, ops._lib.MAX)
    rows, cols = g.row_ids().cpu().long(), g.col.cpu().long()
    msg = V[cols]                                                 # [nnz, d]; all weights 1
    ref = R.reduce_rows(rows, msg, n, "max")
    assert torch.equal(y.cpu(), ref)
    rp = g.rowptr.cpu().long()
    w = win.cpu().long()
    for i in range(n):
        e0, e1 = int(rp[i]), int(rp[i + 1])
        if e0 == e1:
            assert bool((w[i] == -1).all())
            continue
        block = msg[e0:e1]                                        # [deg, d]
        first = (block == block.max(dim=0).values).float().argmax(dim=0) + e0
        assert torch.equal(w[i], first), i


@pytest.mark.parametrize("reduce", ["mean", "max"])
@pytest.mark.parametrize("heads,width", [(4, 8), (1, 2)])
def test_strided_edge_values(dev, hub_plan, reduce, heads, width):
    """a column slice of a wider [nnz, width] tensor as the weights (row stride width, not heads): the forward and both
    gradients equal those of the dense weights"""
    from graphgym_amd import ops
    d = 64
    g, _, V, dy, rows, cols = _op_case(dev, heads, d, seed=11 * heads + width)
    gen = torch.Generator().manual_seed(5)
    big = torch.rand(g.nnz, width, generator=gen) * 2 - 0.5
    bd, Vd = big.to(dev).requires_grad_(True), V.to(dev).requires_grad_(True)
    a_view = bd[:, :heads]
    assert a_view.stride() == (width, 1)
    y = ops.spmm_edge_values(g, a_view, Vd, heads, reduce=reduce)
    (y * dy.to(dev)).sum().backward()
    a = big[:, :heads].contiguous()
    n = g.num_nodes
    close(y.detach(), both(lambda c: R.edge_values_agg(rows, cols, c(a), c(V), n, heads, reduce)),
          what=f"strided {reduce} y H={heads}")
    win = None
    if reduce == "max":
        win = ops._raw_spmm_heads_reduce(g, a.to(dev), V.to(dev), heads, ops._lib.MAX)[1].cpu()

    def grads(c, sign=lambda t: t):
        ar, Vr = sign(c(a)).detach().clone().requires_grad_(True), sign(c(V)).detach().clone().requires_grad_(True)
        (R.edge_values_agg(rows, cols, ar, Vr, n, heads, reduce, win) * sign(c(dy))).sum().backward()
        return ar.grad, Vr.grad
    g64, g32 = both(grads)
    m64 = mag_of(lambda c: grads(c, torch.abs))
    assert bool((bd.grad[:, heads:] == 0).all())
    close(bd.grad[:, :heads], (g64[0], g32[0]), what=f"strided {reduce} da H={heads}", mag=m64[0])
    close(Vd.grad, (g64[1], g32[1]), what=f"strided {reduce} dV H={heads}", mag=m64[1])


def _layer_refs(kind, layer, x, ei, heads, agg, normalize, dy, win_engine, g):
    """float64 / float32 evaluations of the restated layer: output and the gradients of x and every parameter"""
    n = x.size(0)
    ei_ref, norm = R.att_edges(ei, n, normalize)
    win = None
    if agg == "max":
        # engine entry e -> an edge of the restatement with the same (destination, source): duplicates carry equal
        # messages and equal gradients, so any one of them stands for the engine's winner
        key_ref = ei_ref[1] * n + ei_ref[0]
        order = torch.argsort(key_ref)
        key_eng = g.row_ids().cpu().long() * n + g.col.cpu().long()
        pos = torch.searchsorted(key_ref[order], key_eng)
        assert torch.equal(key_ref[order][pos], key_eng)
        e_ref = order[pos]
        w = win_engine.long()
        win = torch.where(w >= 0, e_ref[w.clamp(min=0)], w)
    m = layer.model
    params = {k: v.detach().cpu() for k, v in m.named_parameters()}

    def fn(c):
        xr = c(x).detach().clone().requires_grad_(True)
        pr = {k: c(v).detach().clone().requires_grad_(True) for k, v in params.items()}
        out, _ = R.att_conv(kind, xr, pr["linear_msg.weight"], pr.get("att"), pr.get("bias_att"), pr.get("bias"),
                            ei_ref, None if norm is None else c(norm), heads, agg, win)
        (out * c(dy)).sum().backward()
        return [out.detach(), xr.grad] + [pr[k].grad for k in params]
    p64 = {k: v.double() for k, v in params.items()}
    mag = R.dx_magnitude(kind, x.double(), p64["linear_msg.weight"], p64.get("att"), p64.get("bias_att"),
                         p64.get("bias"), ei_ref, norm, heads, agg, dy.double(), win)
    return list(params), both(fn), mag


def _run_layer(dev, monkeypatch, kind, agg, heads, normalize, seed=3):
    import graphgym_amd.graphgym_plugin as plugin
    from graphgym_amd import ops
    from graphgym_amd.config import cfg
    from graphgym_amd.harness import Batch
    monkeypatch.setattr(cfg.gnn, "att_heads", heads)
    monkeypatch.setattr(cfg.gnn, "agg", agg)
    monkeypatch.setattr(cfg.gnn, "normalize_adj", normalize)
    n, din, dout = 300, 32, 64
    ei = _graph_edges(n, seed)
    gen = torch.Generator().manual_seed(seed)
    x = torch.rand(n, din, generator=gen) * 2 - 1
    dy = torch.rand(n, dout, generator=gen) * 2 - 1
    torch.manual_seed(seed)
    layer = plugin.DESIGN_KEYS["gaddconv" if kind == "add" else "gmulconv"](din, dout, bias=True).to(dev)
    with torch.no_grad():
        for p in layer.parameters():                               # non-zero biases: every term of the layer is live
            if p.dim() == 1:
                p.uniform_(-0.5, 0.5)
    seen = {}
    real = ops._raw_spmm_heads_reduce

    def spy(g, a, V, h, r):
        y, am = real(g, a, V, h, r)
        seen["g"], seen["win"] = g, am
        return y, am
    monkeypatch.setattr(ops, "_raw_spmm_heads_reduce", spy)
    xd = x.to(dev).requires_grad_(True)
    batch = Batch(node_feature=xd, edge_index=ei.to(dev))
    out = layer(batch).node_feature
    (out * dy.to(dev)).sum().backward()
    names, (r64, r32), mag = _layer_refs(kind, layer, x, ei, heads, agg, normalize, dy,
                                    None if seen.get("win") is None else seen["win"].cpu(), seen.get("g"))
    what = f"{kind} agg={agg} H={heads} norm={normalize}"
    close(out.detach(), (r64[0], r32[0]), what=what + " y")
    # x.grad sums terms of either sign over a node's edges (the softmax backward cancels by construction): held to 1e-5 of
    # the sum of their absolute values (tests/_tol.py rule (d))
    close(xd.grad, (r64[1], r32[1]), what=what + " dx", mag=mag)
    grads = dict(layer.model.named_parameters())
    for k, g64, g32 in zip(names, r64[2:], r32[2:]):
        if k == "bias_att":      # zero in exact arithmetic: the softmax is blind to a shift shared by a row
            assert float(grads[k].grad.abs().max()) <= 1e-6 * float(dy.norm()), (what, k)
            continue
        close_all(grads[k].grad, (g64, g32), what=f"{what} d{k}")


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("heads", [1, 4])
@pytest.mark.parametrize("agg", ["add", "mean", "max"])
def test_gaddconv_layer(dev, monkeypatch, agg, heads, normalize):
    _run_layer(dev, monkeypatch, "add", agg, heads, normalize)


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("agg", ["add", "mean", "max"])
def test_gmulconv_layer(dev, monkeypatch, agg, normalize):
    _run_layer(dev, monkeypatch, "mul", agg, 1, normalize)


@pytest.mark.parametrize("key", ["gaddconv", "gmulconv"])
def test_graphgym_stack_trains_with_max(dev, monkeypatch, key):
    from graphgym_amd import harness as H
    from graphgym_amd.config import cfg
    import graphgym_amd.graphgym_plugin  # noqa: F401
    from test_harness_gpu import make_batch
    for k, v in (("layer_type", key), ("layers_mp", 2), ("dim_inner", 16), ("layers_pre_mp", 1), ("agg", "max"),
                 ("att_heads", 1), ("normalize_adj", False)):
        monkeypatch.setattr(cfg.gnn, k, v)
    batch, _ = make_batch(dev, seed=2)
    x0 = batch.node_feature.clone()
    torch.manual_seed(0)
    model = H.GNNStack(6, 4).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=0.01, weight_decay=5e-4)

    def fl():
        batch.node_feature = x0
        pred, true = model(batch)
        return torch.nn.functional.cross_entropy(pred, true)
    losses = [float(H.train_step(model, opt, fl)) for _ in range(25)]
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses


@pytest.mark.parametrize("agg", ["add", "mean", "max"])
@pytest.mark.parametrize("key", ["gaddconv", "gmulconv"])
def test_registered_keys_run_a_batch(dev, monkeypatch, key, agg):
    from graphgym_amd.config import cfg
    from graphgym_amd.harness import Batch
    from graphgym_amd.registry import layer_dict
    import graphgym_amd.graphgym_plugin  # noqa: F401
    monkeypatch.setattr(cfg.gnn, "agg", agg)
    monkeypatch.setattr(cfg.gnn, "att_heads", 1)
    ei = _graph_edges(100, 1) % 100
    batch = Batch(node_feature=torch.rand(100, 8, device=dev), edge_index=ei.to(dev))
    out = layer_dict[key](8, 16).to(dev)(batch).node_feature
    assert out.shape == (100, 16) and bool(torch.isfinite(out).all())


@pytest.mark.parametrize("key", ["gaddconv", "gmulconv"])
def test_bf16_refused(dev, monkeypatch, key):
    from graphgym_amd.config import cfg
    from graphgym_amd.harness import Batch
    import graphgym_amd.graphgym_plugin as plugin
    monkeypatch.setattr(cfg.gnn, "att_heads", 1)
    layer = plugin.DESIGN_KEYS[key](8, 16).to(dev)
    batch = Batch(node_feature=torch.rand(50, 8, device=dev, dtype=torch.bfloat16),
                  edge_index=torch.randint(0, 50, (2, 200), device=dev))
    with pytest.raises(TypeError, match="gaddconv and gmulconv"):
        layer(batch)
