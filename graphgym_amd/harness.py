"""The callers on either side of the hot path, restated just far enough to drive it:
model shapes of the reference's two entry points and its training step order.

    TfgNodeModel   the eight keras models of main_zd.py:28-243 (n conv layers -> Flatten ->
                   Dense(256, relu) -> Dense(num_labels)); GCN / GAT families hard-code 3 layers
                   (main_zd.py:33-35,82-84), SAGE / GIN use cfg.gnn.layers_mp (:131-132,178-187)
    GNN            graphgym/models/gnn.py:123-168, module for module (the reference's own state dicts load with
                   strict=True): pre_mp.Layer_i -> mp.layer{i} (stage 'stack'; GeneralLayer: conv -> BN -> dropout ->
                   act, layer.py:16-47) or mp.block{i}.f.{j} (stages 'skipsum' / 'skipconcat', gnn.py:30-60, 84-109)
                   -> row L2-normalise (gnn.py:79-80, 107-108) -> post_mp.layer_post_mp
                   (node head + label gather head.py:19-37, or graph head with ego add-pool head.py:96-119)
    train_step     zero_grad -> forward -> loss -> backward -> [gradient all-reduce] -> step
                   (graphgym/train.py:18-25, 47-56)
    eval_epoch     model.eval() -> forward -> loss and statistics into a metrics.Meter, nothing read on the host
                   (graphgym/train.py:67-80)
    tfg_loss       mean softmax-CE over node_label_index + 5e-4 * sum ||kernel||^2 / 2
                   (graphgym/loss.py:53-68)
"""
import os
import types

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import layers as L
from . import nn as mpnn
from .config import cfg
from .registry import layer_dict


class Batch(types.SimpleNamespace):
    """the fields of a DeepSNAP batch the path reads (idconv.py:390-441, head.py:27-32)"""

    def to(self, device):
        for k, v in list(vars(self).items()):
            if isinstance(v, torch.Tensor):
                setattr(self, k, v.to(device))
        return self


# ---- TF path: main_zd.py model shapes ----------------------------------------------------
_TF_LAYER = {
    "gcn": (L.GCN, False), "idgcn": (L.IDGCN, True), "gat": (L.GAT, False), "idgat": (L.IDGAT, True),
    "sage": (L.MeanGraphSage, False), "idsage": (L.IDSAGE, True), "gin": (L.GIN, False), "idgin": (L.IDGIN, True),
}


def _keras_gin_mlp(dim_in, dim):
    # main_zd.py:181-186: Dense(d, relu) -> Dense(d) -> BatchNormalization -> relu
    # BatchNormalization + relu run as one engine op (graphgym_amd.nn.BatchNorm1d(relu=True))
    # Dense(d, relu): the ReLU rides in the transform kernel's store; nn.Identity keeps the module indices (and so the
    # state-dict keys) of Linear -> ReLU -> Linear -> BatchNorm
    return nn.Sequential(mpnn.Linear(dim_in, dim, relu=True), nn.Identity(), mpnn.Linear(dim, dim),
                         mpnn.BatchNorm1d(dim, eps=1e-3, momentum=0.01, relu=True))


class TfgNodeModel(nn.Module):
    def __init__(self, kind, dim_in, dim_inner, num_labels, layers_mp=3):
        super().__init__()
        cls, self.with_id = _TF_LAYER[kind]
        self.kind = kind
        n_layers = 3 if kind in ("gcn", "idgcn", "gat", "idgat") else layers_mp
        convs = []
        for i in range(n_layers):
            d_in = dim_in if i == 0 else dim_inner
            if kind in ("gin", "idgin"):
                mlps = [_keras_gin_mlp(d_in, dim_inner)] + ([_keras_gin_mlp(d_in, dim_inner)] if self.with_id else [])
                convs.append(cls(*mlps))
            else:
                convs.append(cls(dim_inner, activation=torch.relu, in_features=d_in))
        self.convs = nn.ModuleList(convs)
        self.mlp = nn.Sequential(nn.Flatten(), mpnn.Linear(dim_inner, 256, relu=True), nn.Identity(),
                                 mpnn.Linear(256, num_labels))

    def kernel_parameters(self):
        """the variables compute_loss_Tfg regularises: every keras variable whose name contains "kernel"
        (loss.py:65) — conv kernels and Dense kernels, not biases / BN"""
        out = []
        for name, p in self.named_parameters():
            leaf = name.split(".")[-1]
            if "kernel" in leaf or (leaf == "weight" and p.dim() == 2):
                out.append(p)
        return out

    def prepare(self, inputs, holder):
        """build the batch's graph structures ahead of the step (every conv layer's prepare(); layers of one model share
        them through `holder`'s cache).  Returns False when a layer family has no prepare(): the step then builds lazily."""
        ok = True
        feats, edge_index = inputs[0], inputs[1]
        rest = [inputs[2]] if self.with_id else []
        for conv in self.convs:
            if not hasattr(conv, "prepare"):
                ok = False
                continue
            conv.prepare([feats, edge_index] + rest, holder)
            width = getattr(conv, "units", None)
            if width is not None and width != feats.size(1):     # later layers see the hidden width (order selection);
                feats = torch.empty((feats.size(0), width), device="meta")      # only its shape is read
        return ok

    def forward(self, inputs, holder=None):
        x, edge_index = inputs[0], inputs[1]
        id_index = inputs[2] if self.with_id else None
        h = x
        for conv in self.convs:
            args = [h, edge_index] + ([id_index] if self.with_id else [])
            h = conv(args, training=self.training, holder=holder)
        return self.mlp(h)


def tfg_loss(logits, node_label_index, labels, kernel_params, ego=False):
    """graphgym/loss.py:53-68"""
    if ego:
        labels = labels[node_label_index]
    ce = mpnn.softmax_cross_entropy(logits, labels, node_label_index)   # == F.cross_entropy(logits[idx], labels)
    l2 = sum((p * p).sum() / 2 for p in kernel_params)     # tf.nn.l2_loss = sum(t^2) / 2
    return ce + 5e-4 * l2


# ---- torch path: GraphGym's GNN, module for module ------------------------------------------
# The module tree (attribute names, nesting, which layers carry a bias) is the reference's, so that its state dicts load
# with strict=True: tests/test_reference_checkpoint.py loads the two trained gcnidconv checkpoints the reference holds
# (run/results/node*/1/ckpt/999.ckpt -> tests/golden/ref_ckpt_*.npz) into this class and into nothing else.
#
#   pre_mp.Layer_{i}.layer.model.weight            GeneralMultiLayer('linear', ...)      layer.py:50-67, gnn.py:23-25
#   pre_mp.Layer_{i}.post_layer.0.*                BatchNorm1d of GeneralLayer           layer.py:26-35
#   mp.layer{i}.layer.model.{weight,weight_id}     GNNStackStage -> GeneralLayer -> conv  gnn.py:65-74, idconv.py:396-404
#   post_mp.layer_post_mp.model.{j}...             GNNNodeHead / GNNGraphHead -> MLP      head.py:19-37,96-119, layer.py:107-132
class GeneralLayer(nn.Module):
    """graphgym/models/layer.py:16-47"""

    def __init__(self, name, dim_in, dim_out, has_act=True, has_bn=True, has_l2norm=False, **kwargs):
        super().__init__()
        self.has_l2norm = has_l2norm
        has_bn = has_bn and cfg.gnn.batchnorm
        self.layer = layer_dict[name](dim_in, dim_out, bias=not has_bn, **kwargs)
        post = []
        fuse_relu = has_bn and has_act and cfg.gnn.act == "relu" and not cfg.gnn.dropout > 0
        if has_bn:   # BN (+ the ReLU right behind it) on the engine's HBM-bound passes
            post.append(mpnn.BatchNorm1d(dim_out, eps=cfg.bn.eps, momentum=cfg.bn.mom, relu=fuse_relu))
        if cfg.gnn.dropout > 0:
            # gnn.keyed_dropout (ours, off by default: the keyed mask is not torch's generator, so a seeded run's numbers
            # change): the mask rides the BatchNorm passes and nothing of it is stored
            make = mpnn.Dropout if getattr(cfg.gnn, "keyed_dropout", False) else nn.Dropout
            post.append(make(p=cfg.gnn.dropout, inplace=cfg.mem.inplace))
        if has_act and not fuse_relu:
            post.append(_act_module())
        self.post_layer = nn.Sequential(*post)

    def _post(self, x):
        """post_layer; [BatchNorm1d, an activation graphgym_amd.nn.act_spec knows] in training mode on a device fp32
        tensor is ONE engine op (nn.bn_act_module), and so are [BatchNorm1d, graphgym_amd.nn.Dropout, activation] and
        [BatchNorm1d, graphgym_amd.nn.Dropout] (gnn.keyed_dropout).  The modules stay where they are: a PReLU's slope
        is post_layer.1.weight (post_layer.2.weight behind a dropout) in the state dict either way."""
        post = self.post_layer
        if (len(post) > 1 and type(post[0]) is mpnn.BatchNorm1d and not post[0].relu and post[0].training
                and x.dim() == 2 and x.is_cuda and x.dtype == torch.float32):
            rest = list(post)[1:]
            drop = rest.pop(0) if type(rest[0]) is mpnn.Dropout else None
            act = rest.pop(0) if rest else None
            if not rest and (act is None or mpnn.act_spec(act) is not None):
                return mpnn.bn_act_module(post[0], x, act, drop=drop)
        return post(x)

    def forward(self, batch):
        batch = self.layer(batch)
        if isinstance(batch, torch.Tensor):                      # layer.py:39-42 (the head's MLP passes tensors)
            batch = self._post(batch)
            return F.normalize(batch, p=2, dim=1) if self.has_l2norm else batch
        batch.node_feature = self._post(batch.node_feature)
        if self.has_l2norm:
            batch.node_feature = F.normalize(batch.node_feature, p=2, dim=1)
        return batch


class GeneralMultiLayer(nn.Module):
    """graphgym/models/layer.py:50-67: children named Layer_{i}"""

    def __init__(self, name, num_layers, dim_in, dim_out, dim_inner=None, final_act=True, **kwargs):
        super().__init__()
        dim_inner = dim_in if dim_inner is None else dim_inner
        for i in range(num_layers):
            d_in = dim_in if i == 0 else dim_inner
            d_out = dim_out if i == num_layers - 1 else dim_inner
            has_act = final_act if i == num_layers - 1 else True
            self.add_module('Layer_{}'.format(i), GeneralLayer(name, d_in, d_out, has_act, **kwargs))

    def forward(self, batch):
        for layer in self.children():
            batch = layer(batch)
        return batch


class Linear(nn.Module):
    """graphgym/models/layer.py:70-82 (the 'linear' key): the nn.Linear sits under `.model`"""

    def __init__(self, dim_in, dim_out, bias=False, **kwargs):
        super().__init__()
        self.model = mpnn.Linear(dim_in, dim_out, bias=bias)     # nn.Linear's parameters and state dict, engine kernels

    def forward(self, batch):
        if isinstance(batch, torch.Tensor):
            return self.model(batch)
        batch.node_feature = self.model(batch.node_feature)
        return batch


layer_dict.setdefault("linear", Linear)


class MLP(nn.Module):
    """graphgym/models/layer.py:107-132: model = Sequential([GeneralMultiLayer('linear', n - 1), Linear]) or
    Sequential([Linear]) for n <= 1"""

    def __init__(self, dim_in, dim_out, bias=True, dim_inner=None, num_layers=2, **kwargs):
        super().__init__()
        dim_inner = dim_in if dim_inner is None else dim_inner
        layers = []
        if num_layers > 1:
            layers.append(GeneralMultiLayer('linear', num_layers - 1, dim_in, dim_inner, dim_inner, final_act=True))
            layers.append(Linear(dim_inner, dim_out, bias))
        else:
            layers.append(Linear(dim_in, dim_out, bias))
        self.model = nn.Sequential(*layers)

    def forward(self, batch):
        if isinstance(batch, torch.Tensor):
            return self.model(batch)
        batch.node_feature = self.model(batch.node_feature)
        return batch


def GNNLayer(dim_in, dim_out, has_act=True):       # gnn.py:19-20
    return GeneralLayer(cfg.gnn.layer_type, dim_in, dim_out, has_act)


def GNNPreMP(dim_in, dim_out):                     # gnn.py:23-25
    return GeneralMultiLayer('linear', cfg.gnn.layers_pre_mp, dim_in, dim_out, dim_inner=dim_out, final_act=True)


class GNNStackStage(nn.Module):
    """graphgym/models/gnn.py:65-81: children named layer{i}; row L2-normalisation behind the last one"""

    def __init__(self, dim_in, dim_out, num_layers):
        super().__init__()
        for i in range(num_layers):
            self.add_module('layer{}'.format(i), GNNLayer(dim_in if i == 0 else dim_out, dim_out))
        self.dim_out = dim_out

    def forward(self, batch):
        for layer in self.children():
            batch = layer(batch)
        if cfg.gnn.l2norm:
            batch.node_feature = F.normalize(batch.node_feature, p=2, dim=-1)
        return batch


# graphgym/models/act.py:6-14, built per use (the reference shares one module instance per key)
act_dict = {
    'relu': lambda: nn.ReLU(inplace=cfg.mem.inplace),
    'selu': lambda: nn.SELU(inplace=cfg.mem.inplace),
    'prelu': lambda: nn.PReLU(),
    'elu': lambda: nn.ELU(inplace=cfg.mem.inplace),
    'lrelu_01': lambda: nn.LeakyReLU(negative_slope=0.1, inplace=cfg.mem.inplace),
    'lrelu_025': lambda: nn.LeakyReLU(negative_slope=0.25, inplace=cfg.mem.inplace),
    'lrelu_05': lambda: nn.LeakyReLU(negative_slope=0.5, inplace=cfg.mem.inplace),
}


def _act_module():
    """cfg.gnn.act through the reference's act_dict keys; a name that is none of them is taken as a torch.nn class, as
    before"""
    make = act_dict.get(cfg.gnn.act)
    return make() if make is not None else getattr(nn, cfg.gnn.act)()


def skip_block_forward(block, batch, stage_type, orig=None):
    """GNNSkipBlock.forward (gnn.py:49-60) for a block `f` of layer wrappers (`.layer`, `.post_layer`, `.has_l2norm`) and
    an activation `act`.  When the last layer's post-ops are exactly one BatchNorm1d in training mode (no dropout, no
    fused ReLU of its own) and the block's activation is ReLU — or, for the harness's own block (`orig` None), any
    activation graphgym_amd.nn.act_spec knows — the BatchNorm, the skip add / concatenation and the activation are ONE
    graphgym_amd.nn.bn_skip_act call behind the last conv; anything else is the reference's composition
    (`orig(batch)` when given: the forward graphgym_plugin.accelerate() replaced).  With gnn.keyed_dropout the harness's
    own block also takes a last post_layer of [BatchNorm1d, graphgym_amd.nn.Dropout]: the mask is drawn in the same call,
    on the BatchNorm term, before the skip operand."""
    if stage_type not in ("skipsum", "skipconcat"):
        raise ValueError("cfg.gnn.stage_type must in [skipsum, skipconcat]")
    last = block.f[-1]
    post = list(last.post_layer)
    # the harness's own block (orig None) takes any activation graphgym_amd.nn.act_spec knows; a block accelerate()
    # rewired keeps its original forward unless its activation is ReLU
    relu = type(block.act) is nn.ReLU
    act_ok = relu or (orig is None and mpnn.act_spec(block.act) is not None)
    # gnn.keyed_dropout, the harness's own block only: the last layer's [BatchNorm1d, graphgym_amd.nn.Dropout] rides along
    drop = post.pop() if (orig is None and len(post) == 2 and type(post[1]) is mpnn.Dropout) else None
    fused = (len(post) == 1 and isinstance(post[0], nn.BatchNorm1d) and not getattr(post[0], "relu", False)
             and (post[0].training or not post[0].track_running_stats) and act_ok and not last.has_l2norm
             and isinstance(batch.node_feature, torch.Tensor) and batch.node_feature.is_cuda)
    if not fused and orig is not None:
        return orig(batch)
    x = batch.node_feature
    if not fused:
        h = block.f(batch).node_feature
        batch.node_feature = block.act(x + h if stage_type == "skipsum" else torch.cat((x, h), 1))
        return batch
    for layer in list(block.f)[:-1]:
        batch = layer(batch)
    batch = last.layer(batch)
    batch.node_feature = mpnn.bn_skip_act(post[0], batch.node_feature, x, stage_type, relu=True,
                                          act=None if relu else block.act, drop=drop)
    return batch


class GNNSkipBlock(nn.Module):
    """graphgym/models/gnn.py:30-60: `f` = Sequential of GNNLayers, the last without activation; forward =
    act(x + f(x)) (skipsum) or act(cat(x, f(x))) (skipconcat), with the last BatchNorm, the skip operand and the
    activation in one engine pass where skip_block_forward's conditions hold.  `self.f(batch)` alone stays the plain,
    unfused layers."""

    def __init__(self, dim_in, dim_out, num_layers):
        super().__init__()
        layers = []
        for i in range(num_layers - 1):
            layers.append(GNNLayer(dim_in if i == 0 else dim_out, dim_out))
        layers.append(GNNLayer(dim_in if num_layers == 1 else dim_out, dim_out, has_act=False))
        self.f = nn.Sequential(*layers)
        self.act = _act_module()
        if cfg.gnn.stage_type == 'skipsum':
            assert dim_in == dim_out, 'Sum skip must have same dim_in, dim_out'

    def forward(self, batch):
        return skip_block_forward(self, batch, cfg.gnn.stage_type)


class GNNSkipStage(nn.Module):
    """graphgym/models/gnn.py:84-109: children named block{i}, each cfg.gnn.skip_every layers; skipconcat widens the
    input of block i to dim_in + i * dim_out; row L2-normalisation behind the last one"""

    def __init__(self, dim_in, dim_out, num_layers):
        super().__init__()
        assert num_layers % cfg.gnn.skip_every == 0, \
            'cfg.gnn.skip_every must be multiples of cfg.gnn.layer_mp(excluding head layer)'
        d_in = dim_in
        for i in range(num_layers // cfg.gnn.skip_every):
            if cfg.gnn.stage_type == 'skipsum':
                d_in = dim_in if i == 0 else dim_out
            elif cfg.gnn.stage_type == 'skipconcat':
                d_in = dim_in if i == 0 else dim_in + i * dim_out
            self.add_module('block{}'.format(i), GNNSkipBlock(d_in, dim_out, cfg.gnn.skip_every))
        self.dim_out = d_in + dim_out if cfg.gnn.stage_type == 'skipconcat' else dim_out

    def forward(self, batch):
        for layer in self.children():
            batch = layer(batch)
        if cfg.gnn.l2norm:
            batch.node_feature = F.normalize(batch.node_feature, p=2, dim=-1)
        return batch


stage_dict = {'stack': GNNStackStage, 'skipsum': GNNSkipStage, 'skipconcat': GNNSkipStage}      # gnn.py:112-116


class GNNNodeHead(nn.Module):
    """graphgym/models/head.py:19-37"""

    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.layer_post_mp = MLP(dim_in, dim_out, num_layers=cfg.gnn.layers_post_mp, bias=True)

    def _apply_index(self, batch):
        idx = batch.node_label_index
        if idx.shape[0] == batch.node_label.shape[0]:
            return batch.node_feature[idx], batch.node_label
        return batch.node_feature[idx], batch.node_label[idx]

    def forward(self, batch):
        batch = self.layer_post_mp(batch)
        return self._apply_index(batch)


class GNNGraphHead(nn.Module):
    """graphgym/models/head.py:96-119: pool (ego batches: the centre rows only, pooling.py:12-17), then the MLP"""

    def __init__(self, dim_in, dim_out):
        super().__init__()
        from .pooling import pooling_dict
        self.layer_post_mp = MLP(dim_in, dim_out, num_layers=cfg.gnn.layers_post_mp, bias=True)
        self.pooling_fun = pooling_dict[cfg.model.graph_pooling]

    def forward(self, batch):
        operator = getattr(batch, "pool_operator", None)      # a loader batch brings its own (graph_loader.collate)
        if cfg.dataset.transform == 'ego':
            graph_emb = self.pooling_fun(batch.node_feature, batch.batch, batch.node_id_index, operator=operator)
        else:
            graph_emb = self.pooling_fun(batch.node_feature, batch.batch, operator=operator)
        batch.graph_feature = self.layer_post_mp(graph_emb)
        return batch.graph_feature, batch.graph_label


# GNNEdgeHead sends its pairs to the engine's pair decoders (graphgym_amd/pair_ops.py: no [2, K, d] gather in either
# direction) when the node features are fp32 on the device, K * d >= PAIR_DECODE_MIN and MP_PAIR_DECODE is not "0";
# everything else (CPU tensors, bf16, small batches, PAIR_DECODE_MIN = None) is the reference's composition, unchanged.
# The value is MEASURED: the smallest power of two at which the engine route, forward + backward with the index build
# included, is no slower than the composition at d = 64 and at d = 256 (scripts/pair_decode_ab.py on link_batch of
# BA(1e6, 5), profiles/pair_decode_ab.jsonl): dot and cosine_similarity lose up to K d = 2^24
# (cosine at d = 256: 3.62 against 3.27 ms) and win from 2^25 on (1.2 x at d = 256, 1.8 - 2.5 x at d = 64).  The concat
# decoding crosses sixteen times later — its two products over the N nodes and its three index builds cost 8 - 9 ms
# whatever K is: it loses at 2^28 at d = 256 (9.19 against 7.78 ms) and wins from 2^29 on — so it takes the route from
# PAIR_DECODE_MIN * PAIR_DECODE_CONCAT on; one number for all three would either send concat batches to a slower route or
# keep score batches that run 2 - 5 x faster off it.
# The floor is a condition, not a measurement: the threshold exceeds K * d of every test that ran a GNNEdgeHead before
# the route existed, so that those keep seeing the composition — the largest is PAIR_DECODE_FLOOR = 1514 pairs x 32 (the
# train batch of tests/test_link_pred_gpu.py::test_edge_head_without_the_transform; test_eval_gpu.py reaches 1388 x 32,
# test_edge_nets_gpu.py 30 x 16, test_poison_gpu.py runs no head).
PAIR_DECODE_MIN = 1 << 25
PAIR_DECODE_CONCAT = 16
PAIR_DECODE_FLOOR = 48448


def pair_decode_route(on_device, dtype, K, d, concat=False):
    """the route rule of GNNEdgeHead on the facts it depends on: True -> the engine's pair decoders"""
    if PAIR_DECODE_MIN is None or os.environ.get("MP_PAIR_DECODE", "1") == "0":
        return False
    least = PAIR_DECODE_MIN * (PAIR_DECODE_CONCAT if concat else 1)
    return bool(on_device and dtype == torch.float32 and K * d >= least)


class GNNEdgeHead(nn.Module):
    """graphgym/models/head.py:40-85: decode the label pairs batch.edge_label_index [2, K] from the node embeddings.
    cfg.model.edge_decoding 'concat': MLP(2 dim_in, dim_out) on cat(h[a], h[b]); 'dot' / 'cosine_similarity': MLP(dim_in,
    dim_in) over the batch, then the pair's dot product / cosine similarity (binary only: dim_out > 1 raises).
    transform: edge batches (edge_nets.edge_batch) are node classification and train through GNNNodeHead instead."""

    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.decoding = getattr(cfg.model, "edge_decoding", "dot")
        if self.decoding == 'concat':
            self.layer_post_mp = MLP(dim_in * 2, dim_out, num_layers=cfg.gnn.layers_post_mp, bias=True)
            return
        if dim_out > 1:
            raise ValueError('Binary edge decoding ({}) is used for multi-class edge/link prediction.'.format(
                self.decoding))
        if self.decoding not in ('dot', 'cosine_similarity'):
            raise ValueError('Unknown edge decoding {}.'.format(self.decoding))
        self.layer_post_mp = MLP(dim_in, dim_in, num_layers=cfg.gnn.layers_post_mp, bias=True)

    def _apply_index(self, batch):
        return batch.node_feature[batch.edge_label_index], batch.edge_label

    def _pair_route(self, h, index):
        """whether the pairs go to graphgym_amd.pair_ops (pair_decode_route, above the class)"""
        if not (isinstance(h, torch.Tensor) and isinstance(index, torch.Tensor) and h.dim() == 2
                and index.dim() == 2 and index.size(0) == 2 and index.dtype == torch.int64
                and (index.size(1) <= 1 or index.stride(1) == 1)):
            return False
        return pair_decode_route(h.is_cuda and index.is_cuda, h.dtype, index.size(1), h.size(1),
                                 concat=self.decoding == 'concat')

    def _concat_pairs(self, batch, pair_index):
        """the concat decoding without cat((h[a], h[b]), -1): the first nn.Linear of layer_post_mp, weight [m, 2d],
        distributes over the halves, cat(h[a], h[b]) W^T = (h W[:, :d]^T)[a] + (h W[:, d:]^T)[b] — two products over the N
        nodes instead of one over the K pairs, then ops.pair_sum; whatever follows that Linear in the MLP (BatchNorm,
        activation and the later layers for layers_post_mp > 1) runs on the [K, m] rows as it is.  The state dict is
        unchanged: the column halves of the weight are views."""
        from . import ops
        h = batch.node_feature
        d = h.size(1)
        first, *rest = list(self.layer_post_mp.model)
        inner = list(first.children()) if isinstance(first, GeneralMultiLayer) else []
        lin = (inner[0].layer if inner else first).model
        W = lin.weight
        # the two half products take the dispatch of the module's own forward (graphgym_amd.nn.linear: the narrow-output
        # weight gradient, the engine's transform on wide outputs); the bias joins in pair_sum
        z = ops.pair_sum(mpnn.linear(h, W[:, :d]), mpnn.linear(h, W[:, d:]), batch.edge_label_index, lin.bias,
                         pair_index=pair_index)
        if inner:
            z = inner[0]._post(z)
            if inner[0].has_l2norm:
                z = F.normalize(z, p=2, dim=1)
            for layer in inner[1:]:
                z = layer(z)
        for layer in rest:
            z = layer(z)
        return z

    def forward(self, batch):
        if self.decoding != 'concat':
            batch = self.layer_post_mp(batch)
        if self._pair_route(batch.node_feature, batch.edge_label_index):
            from . import ops
            pi = getattr(batch, "pair_index", None)     # a PairIndex built ahead; used when its stamp matches
            if self.decoding == 'concat':
                return self._concat_pairs(batch, pi), batch.edge_label
            return ops.pair_score(batch.node_feature, batch.edge_label_index, cosine=self.decoding != 'dot',
                                  pair_index=pi), batch.edge_label
        pred, label = self._apply_index(batch)
        a, b = pred[0], pred[1]
        if self.decoding == 'concat':
            return self.layer_post_mp(torch.cat((a, b), dim=-1)), label
        if self.decoding == 'dot':
            return (a * b).sum(dim=-1), label
        return F.cosine_similarity(a, b, dim=-1), label


head_dict = {'node': GNNNodeHead, 'graph': GNNGraphHead,      # head.py:122-127
             'edge': GNNEdgeHead, 'link_pred': GNNEdgeHead}


class BatchNorm1dNode(nn.Module):
    """graphgym/models/layer.py:85-94, the BatchNorm on the engine's passes (same parameters and buffers under `.bn`)"""

    def __init__(self, dim_in):
        super().__init__()
        self.bn = mpnn.BatchNorm1d(dim_in, eps=cfg.bn.eps, momentum=cfg.bn.mom)

    def forward(self, batch):
        batch.node_feature = self.bn(batch.node_feature)
        return batch


class BatchNorm1dEdge(nn.Module):
    """graphgym/models/layer.py:97-106"""

    def __init__(self, dim_in):
        super().__init__()
        self.bn = mpnn.BatchNorm1d(dim_in, eps=cfg.bn.eps, momentum=cfg.bn.mom)

    def forward(self, batch):
        batch.edge_feature = self.bn(batch.edge_feature)
        return batch


class GNN(nn.Module):
    """graphgym/models/gnn.py:123-168: cfg.gnn.stage_type picks the message-passing stage from stage_dict — 'stack'
    (mp.layer{i}), or 'skipsum' / 'skipconcat' (mp.block{i}.f.{j}: cfg.gnn.skip_every layers per block, the block's last
    BatchNorm + skip add / concatenation + ReLU as one engine pass); an unknown key raises ValueError.  cfg.dataset.node_encoder /
    edge_encoder put node_encoder (+ node_encoder_bn) and edge_encoder (+ edge_encoder_bn) ahead of pre_mp and set dim_in
    to cfg.dataset.encoder_dim (gnn.py:136-150; graphgym_amd.encoders).  The feature-augmentation `preprocess` module of the
    reference holds no parameters and is outside the path: inputs arrive already assembled (the structural features and labels it
    concatenates: graphgym_amd.structure.augment)."""

    def __init__(self, dim_in, dim_out, **kwargs):
        super().__init__()
        stage_type = getattr(cfg.gnn, "stage_type", "stack")
        if stage_type not in stage_dict:
            raise ValueError("cfg.gnn.stage_type must be one of {}, got {!r}".format(sorted(stage_dict), stage_type))
        ds = cfg.dataset
        if getattr(ds, "node_encoder", False):       # gnn.py:136-143
            from .encoders import node_encoder_dict
            self.node_encoder = node_encoder_dict[ds.node_encoder_name](ds.encoder_dim)
            if ds.node_encoder_bn:
                self.node_encoder_bn = BatchNorm1dNode(ds.encoder_dim)
            dim_in = ds.encoder_dim
        if getattr(ds, "edge_encoder", False):       # gnn.py:144-149
            from .encoders import edge_encoder_dict
            self.edge_encoder = edge_encoder_dict[ds.edge_encoder_name](ds.encoder_dim)
            if ds.edge_encoder_bn:
                self.edge_encoder_bn = BatchNorm1dEdge(ds.edge_dim)
        d_in = dim_in
        if cfg.gnn.layers_pre_mp > 0:
            self.pre_mp = GNNPreMP(d_in, cfg.gnn.dim_inner)
            d_in = cfg.gnn.dim_inner
        if cfg.gnn.layers_mp > 0:
            self.mp = stage_dict[stage_type](dim_in=d_in, dim_out=cfg.gnn.dim_inner, num_layers=cfg.gnn.layers_mp)
            d_in = self.mp.dim_out
        self.post_mp = head_dict[getattr(cfg.dataset, "task", "node")](dim_in=d_in, dim_out=dim_out)

    def forward(self, batch):
        for module in self.children():
            batch = module(batch)
        return batch


GNNStack = GNN      # the name rounds 1-2 used


def train_step(model, optimizer, forward_loss, bucket=None):
    """train.py:18-25 / 47-56 with the data-parallel exchange added between backward and step"""
    optimizer.zero_grad()
    loss = forward_loss()
    loss.backward()
    if bucket is not None:
        bucket.all_reduce_mean()
    optimizer.step()
    return loss.detach()


@torch.no_grad()
def eval_epoch(model, loader, meter):
    """train.py:67-80 on a graphgym_amd.metrics.Meter: the model's raw outputs go into meter.update_logits, which
    accumulates the statistics and the loss on the device — no copy of `true` / `pred_score` to the host and no
    loss.item() per batch.  The epoch's numbers are meter.compute() (one device-to-host copy)."""
    model.eval()
    for batch in loader:
        pred, true = model(batch)
        meter.update_logits(pred, true)
    return meter


class GraphedTrainStep:
    """The whole step (forward, loss, backward, optimizer) captured once into a HIP graph and replayed.

    The reference trains full-batch on small graphs (batch_size >= dataset in config/*_tf/*.yaml), where a
    step is ~100 short kernels and launch overhead dominates; shapes repeat every epoch, so one capture
    serves the run.  Requirements: the batch's CSR / plan / transpose are already cached (run a few eager
    steps first — done here), the optimizer is capture-safe (torch.optim.Adam(capturable=True)), and
    forward_loss() reads only tensors that stay at fixed addresses.  Engine ops are capture-safe: they
    enqueue on torch's current stream and never synchronise once the graph structures are cached."""

    def __init__(self, model, optimizer, forward_loss, warmup=3):
        self.optimizer = optimizer
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(warmup):
                train_step(model, optimizer, forward_loss)
        torch.cuda.current_stream().wait_stream(side)
        self.graph = torch.cuda.CUDAGraph()
        optimizer.zero_grad(set_to_none=True)
        with torch.cuda.graph(self.graph):
            self.loss = forward_loss()
            self.loss.backward()
            optimizer.step()

    def __call__(self):
        self.graph.replay()
        return self.loss
