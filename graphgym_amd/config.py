"""Minimal stand-in for the keys of GraphGym's global ``cfg`` that the hot path reads
(graphgym/config.py:313-372,409-420).  When the real ``graphgym.config`` is importable
(a deployment with yacs installed) that object is used instead, so the layers see the
experiment's actual configuration; otherwise the same YAML files are read with PyYAML.
"""
import types

import yaml


def _defaults():
    cfg = types.SimpleNamespace()
    cfg.device = "auto"                      # config.py:33
    cfg.num_threads = 6                      # config.py:57
    cfg.round = 4                            # config.py:60 (metrics.py: the digits an epoch's statistics are rounded to)
    cfg.metric_best = "auto"                 # config.py:45
    cfg.dataset = types.SimpleNamespace(transform="none", augment_feature=[], task="node",
                                        edge_dim=128,                    # config.py:145
                                        edge_train_mode="all", edge_message_ratio=0.8,
                                        edge_negative_sampling_ratio=1.0, resample_disjoint=False,
                                        resample_negative=False,         # config.py:147-163 (link_pred.py)
                                        node_encoder=False, node_encoder_name="Atom", node_encoder_bn=True,
                                        edge_encoder=False, edge_encoder_name="Bond", edge_encoder_bn=True,
                                        encoder_dim=128)                 # config.py:121-142 (encoders.py)
    cfg.model = types.SimpleNamespace(graph_pooling="add", loss_fun="cross_entropy",      # config.py:285-301
                                      size_average="mean", thresh=0.5)                    # config.py:284,287 (metrics.py)
    # config.py:212-248 (samplers.py); train.train_parts (read by loader_pyg.py:218) has no default there or here
    cfg.train = types.SimpleNamespace(batch_size=16, sampler="full_batch", iter_per_epoch=32, walk_length=4,
                                      neighbor_sizes=[20, 15, 10, 5])
    cfg.val = types.SimpleNamespace(sampler="full_batch")                 # config.py:254-261
    cfg.gnn = types.SimpleNamespace(
        layers_pre_mp=0, layers_mp=2, layers_post_mp=1, dim_inner=16,
        layer_type="generalconv", stage_type="stack", batchnorm=True, act="relu",
        dropout=0.0, agg="add", flow="source_to_target", normalize_adj=False,
        self_msg="concat", att_heads=1, l2norm=True,
        msg_direction="single", keep_edge=0.5,
        att_final_linear=False, att_final_linear_bn=False,
        skip_every=1,                                                     # config.py:313-372 (:363-366, :331)
        keyed_dropout=False)              # ours: gnn.dropout through graphgym_amd.nn.Dropout, fused into the BatchNorm passes
    cfg.bn = types.SimpleNamespace(eps=1e-5, mom=0.1)                     # config.py:409-412
    cfg.mem = types.SimpleNamespace(inplace=False)                        # config.py:420
    cfg.optim = types.SimpleNamespace(base_lr=0.01, max_epoch=200, weight_decay=5e-4)
    return cfg


try:  # a real GraphGym install wins
    from graphgym.config import cfg  # noqa: F401
    HAVE_GRAPHGYM_CFG = True
except Exception:  # yacs / graphgym absent: same keys, plain namespace
    cfg = _defaults()
    HAVE_GRAPHGYM_CFG = False


def load_cfg(path, target=None):
    """merge a GraphGym YAML (e.g. config/gcnconv_tf/gcnconv_node_scalefree.yaml) into cfg"""
    target = cfg if target is None else target
    with open(path) as f:
        data = yaml.safe_load(f) or {}
    for k, v in data.items():
        if isinstance(v, dict):
            node = getattr(target, k, None)
            if node is None:
                node = types.SimpleNamespace()
                setattr(target, k, node)
            for kk, vv in v.items():
                setattr(node, kk, vv)
        else:
            setattr(target, k, v)
    return target
