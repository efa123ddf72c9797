"""The skip stages restated for tests/test_skip_stage_gpu.py and tests/test_bn_skip_host.py.

`skip_gnn` is harness.GNN with stage_type skipsum / skipconcat (graphgym/models/gnn.py:30-60, 84-109, 123-168) as plain
tensor arithmetic on the CPU, built from oracle/ref_layers.py: Linear -> BN -> ReLU (pre_mp), blocks of
conv -> BN [-> ReLU] with `act(x + f(x))` / `act(cat(x, f(x)))` behind them, row L2-normalisation, a Linear head on the
labelled rows.  It is dtype-generic (tests/_tol.py: both) and differentiates every ReLU through the engine's own pattern
(tests/_gradsub.py: relu_like, which also asserts that the patterns agree away from zero).

RefStyleGeneralLayer / RefStyleSkipBlock are the reference's layer wrapper and skip block written with plain torch
modules — what create_model() produces when the engine's conv classes sit in layer_dict — for accelerate()."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from _gradsub import relu_like
from oracle import ref_layers as RL


def _bn(h, P, prefix, eps):
    return F.batch_norm(h, None, None, P[prefix + ".weight"], P[prefix + ".bias"], True, 0.1, eps)


def _conv(h, ei, P, prefix, layer_type):
    if layer_type == "gcnconv":
        return RL.pyg_gcn_conv(h, ei, P[prefix + ".weight"], P.get(prefix + ".bias"))
    assert layer_type == "generalconv"          # cfg defaults: agg add, no adjacency normalisation, self_msg concat
    return RL.general_conv(h, ei, P[prefix + ".weight"], P[prefix + ".weight_self"], P.get(prefix + ".bias"))


def skip_block(h, ei, P, prefix, masks, stage, layer_type, skip_every, eps=1e-5, has_bn=True):
    """one GNNSkipBlock under `prefix` (its `f.{j}` children); masks: the engine's patterns of the inner activations, then
    of the block's own — consumed from the front"""
    x0 = h
    for j in range(skip_every):
        p = f"{prefix}f.{j}"
        h = _conv(h, ei, P, p + ".layer.model", layer_type)
        if has_bn:
            h = _bn(h, P, p + ".post_layer.0", eps)
        if j < skip_every - 1:
            h = relu_like(h, masks.pop(0))
    h = x0 + h if stage == "skipsum" else torch.cat((x0, h), 1)
    return relu_like(h, masks.pop(0))


def skip_gnn(c, params, x, ei, label_index, masks, stage, layer_type, layers_mp, skip_every, eps=1e-5, l2norm=True):
    """(pred on the labelled rows, P): c casts the inputs; params: the model's named parameters; masks: the engine's
    ReLU patterns in forward order (pre_mp, then per block the inner layers' and the block's own)"""
    P = {k: c(v.detach().cpu()).clone().requires_grad_(True) for k, v in params.items()}
    masks = [m.cpu() for m in masks]
    h = c(x) @ P["pre_mp.Layer_0.layer.model.weight"].t()
    h = relu_like(_bn(h, P, "pre_mp.Layer_0.post_layer.0", eps), masks.pop(0))
    for i in range(layers_mp // skip_every):
        h = skip_block(h, ei, P, f"mp.block{i}.", masks, stage, layer_type, skip_every, eps)
    assert not masks
    if l2norm:
        h = F.normalize(h, p=2, dim=-1)
    pred = h @ P["post_mp.layer_post_mp.model.0.model.weight"].t() + P["post_mp.layer_post_mp.model.0.model.bias"]
    return pred[label_index], P


class RefStyleGeneralLayer(nn.Module):
    """layer.py:16-47 as written in the reference"""

    def __init__(self, conv_cls, dim_in, dim_out, has_act=True, has_bn=True, has_l2norm=False, dropout=0.0):
        super().__init__()
        self.has_l2norm = has_l2norm
        self.layer = conv_cls(dim_in, dim_out, bias=not has_bn)
        wrapper = []
        if has_bn:
            wrapper.append(nn.BatchNorm1d(dim_out, eps=1e-5, momentum=0.1))
        if dropout > 0:
            wrapper.append(nn.Dropout(p=dropout))
        if has_act:
            wrapper.append(nn.ReLU())
        self.post_layer = nn.Sequential(*wrapper)

    def forward(self, batch):
        batch = self.layer(batch)
        batch.node_feature = self.post_layer(batch.node_feature)
        if self.has_l2norm:
            batch.node_feature = F.normalize(batch.node_feature, p=2, dim=1)
        return batch


class RefStyleSkipBlock(nn.Module):
    """gnn.py:30-60 as written in the reference: cfg.gnn.stage_type is read when the block runs"""

    def __init__(self, conv_cls, dim_in, dim_out, num_layers, act=None, **kw):
        super().__init__()
        f = [RefStyleGeneralLayer(conv_cls, dim_in if i == 0 else dim_out, dim_out, **kw) for i in range(num_layers - 1)]
        f.append(RefStyleGeneralLayer(conv_cls, dim_in if num_layers == 1 else dim_out, dim_out, has_act=False, **kw))
        self.f = nn.Sequential(*f)
        self.act = nn.ReLU() if act is None else act

    def forward(self, batch):
        from graphgym_amd.config import cfg
        stage = cfg.gnn.stage_type
        if stage not in ("skipsum", "skipconcat"):
            raise ValueError(f"no skip stage {stage!r}")
        x = batch.node_feature
        h = self.f(batch).node_feature
        batch.node_feature = self.act(x + h if stage == "skipsum" else torch.cat((x, h), 1))
        return batch
