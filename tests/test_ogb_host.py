"""The OGB encoders, generalogbconv and sageinitconv: everything that needs no device — parameter names and shapes, the
feature dims, the combined bond code, the range check, the registration, the config defaults and the module tree the two
shipped configs (tests/golden/cfg_idgnn_graph_ogb.yaml = run/configs/IDGNN/graph_ogb.yaml, cfg_design_v2ogb.yaml =
run/configs/design/design_v2ogb.yaml) build."""
import copy
import os

import pytest
import torch

import _ogb_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ATOM = [119, 4, 12, 12, 10, 6, 6, 2, 2]
BOND = [5, 6, 2]


@pytest.fixture
def fresh_cfg():
    """the global cfg, restored afterwards"""
    from graphgym_amd.config import cfg
    saved = copy.deepcopy(vars(cfg))
    yield cfg
    for k in list(vars(cfg)):
        if k not in saved:
            delattr(cfg, k)
    for k, v in saved.items():
        setattr(cfg, k, v)


def test_feature_dims():
    from graphgym_amd import encoders as E
    try:
        from ogb.utils.features import get_atom_feature_dims, get_bond_feature_dims
        atom, bond = list(get_atom_feature_dims()), list(get_bond_feature_dims())
    except ImportError:
        atom, bond = ATOM, BOND
    assert E.full_atom_feature_dims == atom and E.full_bond_feature_dims == bond
    assert E.ATOM_FEATURE_DIMS == ATOM and E.BOND_FEATURE_DIMS == BOND
    assert sum(ATOM) == 173 and sum(BOND) == 13 and 5 * 6 * 2 == 60
    assert E.table_offsets(BOND) == [0, 5, 11]


def test_state_dict_keys_and_shapes():
    from graphgym_amd import encoders as E
    from graphgym_amd import ogbconv as O
    from graphgym_amd.config import cfg
    d = 24
    assert {k: tuple(v.shape) for k, v in E.IntegerFeatureEncoder(d, num_classes=7).state_dict().items()} == \
        {"encoder.weight": (7, d)}
    assert {k: tuple(v.shape) for k, v in E.SingleAtomEncoder(d).state_dict().items()} == \
        {"atom_type_embedding.weight": (E.full_atom_feature_dims[0], d)}
    assert {k: tuple(v.shape) for k, v in E.AtomEncoder(d).state_dict().items()} == \
        {f"atom_embedding_list.{i}.weight": (n, d) for i, n in enumerate(E.full_atom_feature_dims)}
    assert {k: tuple(v.shape) for k, v in E.BondEncoder(d).state_dict().items()} == \
        {f"bond_embedding_list.{i}.weight": (n, d) for i, n in enumerate(E.full_bond_feature_dims)}
    assert set(E.node_encoder_dict) == {"Integer", "SingleAtom", "Atom"} and set(E.edge_encoder_dict) == {"Bond"}
    # xavier_uniform_: within sqrt(6 / (fan_in + fan_out)), and not the N(0, 1) nn.Embedding starts from
    w = E.AtomEncoder(d).atom_embedding_list[0].weight.detach()
    bound = (6.0 / (w.size(0) + w.size(1))) ** 0.5
    assert float(w.abs().max()) <= bound and float(w.abs().max()) > 0.5 * bound
    assert cfg.gnn.agg in ("add", "mean", "max")
    layer = O.GeneralOGBConv(16, d, bias=True)
    want = {"model.weight": (16, d), "model.bias": (d,)}
    want.update({f"model.bond_encoder.bond_embedding_list.{i}.weight": (n, d)
                 for i, n in enumerate(E.full_bond_feature_dims)})
    assert {k: tuple(v.shape) for k, v in layer.state_dict().items()} == want
    assert "model.bias" not in O.GeneralOGBConv(16, d).state_dict()
    sage = O.SAGEinitConv(16, d, bias=True)
    assert {k: tuple(v.shape) for k, v in sage.state_dict().items()} == {"model.weight": (32, d), "model.bias": (d,)}
    assert sage.model.concat is True


def test_combined_bond_code_round_trips():
    from graphgym_amd import ogbconv as O
    q = torch.arange(60)
    c = O.unpack_bond_codes(q)
    assert c.shape == (60, 3)
    for k, n in enumerate(BOND):
        assert int(c[:, k].min()) == 0 and int(c[:, k].max()) == n - 1
    assert len({tuple(r) for r in c.tolist()}) == 60
    assert torch.equal(O.pack_bond_codes(c), q)
    assert torch.equal(O.pack_bond_codes(c.to(torch.int32)), q.to(torch.int32))
    # the combined table of a layer is the reference's loop over the unpacked codes
    from graphgym_amd.config import cfg  # noqa: F401
    layer = O.GeneralOGBConvLayer(8, 12)
    tables = [e.weight.detach() for e in layer.bond_encoder.bond_embedding_list]
    assert torch.equal(layer.combined_table().detach(), R.encode(c, tables))


@pytest.mark.parametrize("dims", [ATOM, BOND, [7]])
def test_codes_out_of_range_raise_index_error(dims):
    from graphgym_amd import ops
    gen = torch.Generator().manual_seed(0)
    good = torch.stack([torch.randint(0, n, (20,), generator=gen) for n in dims], dim=1)
    for k, n in enumerate(dims):
        for bad in (-1, n):
            c = good.clone()
            c[7, k] = bad
            with pytest.raises(IndexError, match="out of range"):
                ops.check_codes(c, dims)
        c = good.clone()
        c[3, k] = n - 1
        c[4, k] = 0
        with pytest.raises(Exception) as info:      # in range: the only complaint left is that this is no device tensor
            ops.check_codes(c, dims)
        assert not isinstance(info.value, IndexError)


def test_ogb_keys_are_installed():
    import graphgym_amd.graphgym_plugin as P
    from graphgym_amd import ogbconv as O
    from graphgym_amd import registry
    assert P.OGB_KEYS == {"generalogbconv": O.GeneralOGBConv, "sageinitconv": O.SAGEinitConv}
    assert sorted(P.installed_ogb_keys) == sorted(P.OGB_KEYS) == sorted(P.install_ogb())
    for k, cls in P.OGB_KEYS.items():
        assert registry.layer_dict[k] is cls
        with pytest.raises(KeyError):
            registry.register_layer(k, cls)
    assert not set(P.OGB_KEYS) & (set(P.ALL_KEYS) | set(P.DESIGN_KEYS) | set(P.EDGE_KEYS) | set(P.EDGE_ATT_KEYS))


def test_config_defaults():
    from graphgym_amd import config
    ds = config._defaults().dataset
    assert (ds.node_encoder, ds.node_encoder_name, ds.node_encoder_bn) == (False, "Atom", True)
    assert (ds.edge_encoder, ds.edge_encoder_name, ds.edge_encoder_bn) == (False, "Bond", True)
    assert ds.encoder_dim == 128 and ds.edge_dim == 128


@pytest.mark.parametrize("name,encoder,layer,act", [
    ("cfg_idgnn_graph_ogb.yaml", "SingleAtomEncoder", "GeneralIDConv", "relu"),
    ("cfg_design_v2ogb.yaml", "AtomEncoder", "GeneralOGBConv", "prelu")])
def test_shipped_configs_build_the_reference_module_tree(fresh_cfg, name, encoder, layer, act):
    import graphgym_amd.graphgym_plugin  # noqa: F401
    from graphgym_amd import config, harness as H
    cfg = config.load_cfg(os.path.join(GOLDEN, name), target=fresh_cfg)
    assert cfg.gnn.act == act
    model = H.GNN(dim_in=9, dim_out=2)
    tree = R.module_tree(cfg)
    assert [n for n, _ in model.named_children()] == [n for n, _ in tree]
    assert type(model.node_encoder).__name__ == encoder
    assert model.node_encoder_bn.bn.num_features == cfg.dataset.encoder_dim
    assert not hasattr(model, "edge_encoder")
    assert len(list(model.mp.children())) == cfg.gnn.layers_mp
    first = model.pre_mp.Layer_0.layer.model
    assert first.weight.shape == (cfg.gnn.dim_inner, cfg.dataset.encoder_dim)      # dim_in = encoder_dim (gnn.py:143)
    for lay in model.mp.children():
        assert type(lay.layer).__name__ == layer
    acts = [m for m in model.modules() if isinstance(m, torch.nn.PReLU)]
    assert bool(acts) == (act == "prelu")
    keys = set(model.state_dict())
    assert any(k.startswith("node_encoder.") for k in keys) and "node_encoder_bn.bn.weight" in keys
    if act == "prelu":
        assert "mp.layer0.layer.model.bond_encoder.bond_embedding_list.2.weight" in keys
        assert "node_encoder.atom_embedding_list.8.weight" in keys
    else:
        assert "node_encoder.atom_type_embedding.weight" in keys


def test_act_dict_keys(fresh_cfg):
    from graphgym_amd import harness as H
    assert set(H.act_dict) == {"relu", "selu", "prelu", "elu", "lrelu_01", "lrelu_025", "lrelu_05"}
    fresh_cfg.gnn.act = "lrelu_025"
    m = H._act_module()
    assert isinstance(m, torch.nn.LeakyReLU) and m.negative_slope == 0.25
