"""harness.GNN with stage_type skipsum / skipconcat, and graphgym_plugin.accelerate() on the reference's skip block.

Whole models (pre_mp -> blocks -> row L2-normalisation -> node head) against the float64 / float32 restatement of
tests/_skip_ref.py; the block's fused pass (conv -> one mp::bn_skip_act) against the composition act(x . f(x)) evaluated
with the same modules; the fallbacks (eval mode, dropout, no BatchNorm) and what a dispatch-mode tracer sees.
Common setting: a Barabasi-Albert graph of 3000 nodes, 32 input features, dim_inner 64."""
import copy

import pytest
import torch
import torch.nn as nn
from torch.utils._python_dispatch import TorchDispatchMode

from _skip_ref import RefStyleSkipBlock, skip_gnn
from _tol import both, close, close_all

pytestmark = pytest.mark.gpu

N, F_IN, D, CLASSES = 3000, 32, 64, 5
STAGES = ["skipsum", "skipconcat"]


@pytest.fixture()
def gcfg():
    from graphgym_amd.config import cfg
    import graphgym_amd.graphgym_plugin  # noqa: F401  (registers the layer keys)
    saved = {k: dict(vars(getattr(cfg, k))) for k in ("gnn", "dataset", "bn", "mem")}
    cfg.gnn.layers_pre_mp, cfg.gnn.dim_inner, cfg.gnn.layers_post_mp, cfg.gnn.layers_mp = 1, D, 1, 4
    cfg.gnn.batchnorm, cfg.gnn.dropout, cfg.gnn.act, cfg.gnn.l2norm, cfg.gnn.skip_every = True, 0.0, "relu", True, 1
    cfg.gnn.agg, cfg.gnn.normalize_adj, cfg.gnn.self_msg = "add", False, "concat"
    cfg.dataset.task, cfg.dataset.transform = "node", "none"
    yield cfg
    for k, v in saved.items():
        ns = getattr(cfg, k)
        for name in list(vars(ns)):
            if name not in v:
                delattr(ns, name)
        for name, val in v.items():
            setattr(ns, name, val)


@pytest.fixture(scope="module")
def graph():
    from graphgym_amd import graphgen
    g = torch.Generator().manual_seed(11)
    ei = graphgen.ba_edge_index(N, 4, seed=5)
    x = torch.randn(N, F_IN, generator=g)
    idx = torch.randperm(N, generator=g)[: N // 2].sort().values
    up = torch.randn(idx.numel(), CLASSES, generator=g)
    return ei, x, idx, up


def _batch(dev, x, ei, idx=None, grad=False):
    from graphgym_amd import harness as H
    b = H.Batch(node_feature=x.to(dev).requires_grad_(grad), edge_index=ei.to(dev))
    if idx is not None:
        b.node_label_index = idx.to(dev)
        b.node_label = torch.zeros(idx.numel(), dtype=torch.int64, device=dev)
    return b


class Spy(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        if str(func).startswith("mp."):
            self.seen.append(str(func).split(".")[1])
        return func(*args, **(kwargs or {}))


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("layer_type", ["gcnconv", "generalconv"])
@pytest.mark.parametrize("skip_every", [1, 2])
def test_model_against_the_restatement(dev, gcfg, graph, stage, layer_type, skip_every):
    """Whole models, rows through close(deep=True), parameter gradients through close_all.

    Measured on an MI355X, worst err / allowed over the parameter gradients of a case: 0.13-0.31 over the eight cases.
    With the forward statistics shifted by row 0 (node 0 of a Barabasi-Albert graph is its largest hub: 12 standard
    deviations from the column mean behind generalconv's unnormalised add aggregation, the variance then off by 6.5e-6)
    the same figures were 0.19-0.68 and 1.008 for skipsum / generalconv / skip_every 2; csrc/bn.hip: bn_pivot."""
    from graphgym_amd import harness as H
    ei, x, idx, up = graph
    gcfg.gnn.stage_type, gcfg.gnn.layer_type, gcfg.gnn.skip_every = stage, layer_type, skip_every
    torch.manual_seed(3)
    model = H.GNN(F_IN, CLASSES).to(dev).train()
    with torch.no_grad():
        for m in model.modules():
            if isinstance(m, nn.BatchNorm1d):
                m.weight.uniform_(0.5, 1.5); m.bias.uniform_(-0.3, 0.3)
    # the engine's ReLU patterns in forward order: pre_mp, then per block the inner layers' and the block's own
    masks = []
    hooks = [model.pre_mp.Layer_0.post_layer.register_forward_hook(lambda m, i, o: masks.append(o.detach() > 0))]
    for blk in model.mp.children():
        for layer in list(blk.f)[:-1]:
            hooks.append(layer.post_layer.register_forward_hook(lambda m, i, o: masks.append(o.detach() > 0)))
        hooks.append(blk.register_forward_hook(lambda m, i, o: masks.append(o.node_feature.detach() > 0)))
    with Spy() as spy:
        pred, _ = model(_batch(dev, x, ei, idx))
    for h in hooks:
        h.remove()
    n_blocks = 4 // skip_every
    assert spy.seen.count("bn_skip_act") == n_blocks and len(masks) == 1 + 4
    pred.backward(up.to(dev))
    params = dict(model.named_parameters())

    def ref(c):     # the whole model: several layers, BatchNorm, l2norm and a head
        p, P = skip_gnn(c, params, x, ei, idx, list(masks), stage, layer_type, 4, skip_every)
        p.backward(c(up))
        return [p.detach()] + [P[k].grad for k in params]
    r64, r32 = both(ref)
    what = f"{stage} {layer_type} skip_every {skip_every}"
    close(pred, (r64[0], r32[0]), what=what + " pred", deep=True)
    for j, (k, p) in enumerate(params.items()):
        assert p.grad is not None, k
        close_all(p.grad, (r64[1 + j], r32[1 + j]), what=f"{what} grad {k}")
    for blk in model.mp.children():
        assert int(blk.f[-1].post_layer[0].num_batches_tracked) == 1


def _block(dev, gcfg, stage, skip_every=2, layer_type="gcnconv", **over):
    from graphgym_amd import harness as H
    gcfg.gnn.stage_type, gcfg.gnn.layer_type, gcfg.gnn.skip_every = stage, layer_type, skip_every
    for k, v in over.items():
        setattr(gcfg.gnn, k, v)
    torch.manual_seed(7)
    blk = H.GNNSkipBlock(D, D, skip_every).to(dev)
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, nn.BatchNorm1d):
                m.weight.uniform_(0.5, 1.5); m.bias.uniform_(-0.3, 0.3)
    return blk


def _composed(blk, batch, stage):
    """act(x . block.f(batch)) with the block's own modules: the plain, unfused layers"""
    x = batch.node_feature
    h = blk.f(batch).node_feature
    return blk.act(x + h if stage == "skipsum" else torch.cat((x, h), 1))


def _run(dev, blk, fn, x0, ei, up):
    blk.zero_grad()
    b = _batch(dev, x0, ei, grad=True)
    xin = b.node_feature
    with Spy() as spy:
        out = fn(b)
    out.backward(up.to(dev))
    return out.detach(), xin.grad, {k: p.grad.clone() for k, p in blk.named_parameters()}, spy.seen


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("layer_type", ["gcnconv", "generalconv"])
def test_fused_block_against_the_composition(dev, gcfg, graph, stage, layer_type):
    ei = graph[0]
    g = torch.Generator().manual_seed(2)
    x0 = torch.randn(N, D, generator=g)
    up = torch.randn(N, D if stage == "skipsum" else 2 * D, generator=g)
    blk = _block(dev, gcfg, stage, layer_type=layer_type).train()
    out, dx, grads, seen = _run(dev, blk, lambda b: blk(b).node_feature, x0, ei, up)
    ref, rdx, rgrads, rseen = _run(dev, blk, lambda b: _composed(blk, b, stage), x0, ei, up)
    assert seen.count("bn_skip_act") == 1 and "bn_skip_act" not in rseen and "bn_act" in rseen
    assert torch.equal(out, ref)                # the sum, or both slabs: the same arithmetic on the same bits
    close(dx, rdx.double(), what=f"{stage} fused dx")
    for k in grads:
        close_all(grads[k], rgrads[k].double(), what=f"{stage} fused grad {k}")
    assert int(blk.f[-1].post_layer[0].num_batches_tracked) == 2


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("case", ["eval", "dropout", "no-batchnorm"])
def test_fallbacks_give_the_composition(dev, gcfg, graph, stage, case):
    ei = graph[0]
    x0 = torch.randn(N, D, generator=torch.Generator().manual_seed(4))
    over = {"dropout": dict(dropout=0.5), "no-batchnorm": dict(batchnorm=False)}.get(case, {})
    blk = _block(dev, gcfg, stage, **over)
    post = blk.f[-1].post_layer
    if case == "dropout":
        assert [type(m).__name__ for m in post] == ["BatchNorm1d", "Dropout"]
    if case == "no-batchnorm":
        assert len(post) == 0 and blk.f[-1].layer.model.bias is not None
    if case == "no-batchnorm":
        blk.train()
    else:
        with torch.no_grad():       # running statistics that are not the initial ones
            blk.train()
            blk(_batch(dev, x0, ei))
        blk.eval()
    with Spy() as spy, torch.no_grad():
        out = blk(_batch(dev, x0, ei)).node_feature
        ref = _composed(blk, _batch(dev, x0, ei), stage)
    assert "bn_skip_act" not in spy.seen
    assert out.shape == (N, D if stage == "skipsum" else 2 * D) and torch.equal(out, ref)


@pytest.mark.parametrize("stage", STAGES)
def test_accelerate_on_the_references_block(dev, gcfg, graph, stage):
    """the accelerated block against the same block left as torch modules, training and eval"""
    import graphgym_amd.graphgym_plugin as plugin
    from graphgym_amd import layers as L
    ei = graph[0]
    gcfg.gnn.stage_type = stage
    g = torch.Generator().manual_seed(9)
    x0 = torch.randn(N, D, generator=g)
    up = torch.randn(N, D if stage == "skipsum" else 2 * D, generator=g)
    torch.manual_seed(5)
    plain = RefStyleSkipBlock(L.GCNConv, D, D, 2).to(dev)
    with torch.no_grad():
        for m in plain.modules():
            if isinstance(m, nn.BatchNorm1d):
                m.weight.uniform_(0.5, 1.5); m.bias.uniform_(-0.3, 0.3)
    fast = copy.deepcopy(plain)
    assert plugin.accelerate(fast) == 2
    plain.train(), fast.train()
    ref, rdx, rgrads, rseen = _run(dev, plain, lambda b: plain(b).node_feature, x0, ei, up)
    out, dx, grads, seen = _run(dev, fast, lambda b: fast(b).node_feature, x0, ei, up)
    assert seen.count("bn_skip_act") == 1 and "bn_skip_act" not in rseen
    what = f"accelerate {stage}"
    close(out, ref.double(), what=what + " out")
    close(dx, rdx.double(), what=what + " dx")
    for k in grads:
        close_all(grads[k], rgrads[k].double(), what=f"{what} grad {k}")
    for (ka, a), (kb, b) in zip(fast.named_buffers(), plain.named_buffers()):
        assert ka == kb
        close_all(a.float(), b.double(), what=f"{what} buffer {ka}")
    plain.eval(), fast.eval()
    with Spy() as spy, torch.no_grad():
        out = fast(_batch(dev, x0, ei)).node_feature
        ref = plain(_batch(dev, x0, ei)).node_feature
    assert "bn_skip_act" not in spy.seen
    close(out, ref.double(), what=what + " eval out")
    # another block activation stays on the original forward
    other = RefStyleSkipBlock(L.GCNConv, D, D, 1, act=nn.PReLU()).to(dev).train()
    plugin.accelerate(other)
    with Spy() as spy:
        other(_batch(dev, x0, ei))
    assert "bn_skip_act" not in spy.seen
