"""The host side of the activation-fused BatchNorm passes: graphgym_amd.nn.act_spec, the argument checks of the new C
entries (csrc/bn.hip: mp_bn_train_*_act_f32) before anything is launched, and the harness's module tree with
gnn.act = prelu.  No device work here."""
import ctypes as C
import os

import pytest
import torch
import torch.nn as nn

from graphgym_amd import _lib
from test_ogb_host import fresh_cfg  # noqa: F401

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
INVALID, WORKSPACE = 1, 3
FAKE = C.c_void_p(4096)         # never dereferenced: every call below is refused before a launch
NONE, RELU, LRELU, PRELU, ELU, SELU, SILU = range(7)
SUM, CONCAT = 0, 1


def test_act_spec_knows_exact_types_only():
    from graphgym_amd import nn as mpnn
    assert (mpnn.ACT_NONE, mpnn.ACT_RELU, mpnn.ACT_LRELU, mpnn.ACT_PRELU, mpnn.ACT_ELU, mpnn.ACT_SELU,
            mpnn.ACT_SILU) == (NONE, RELU, LRELU, PRELU, ELU, SELU, SILU)
    assert mpnn.act_spec(nn.ReLU()) == (RELU, None) and mpnn.act_spec(nn.ReLU(inplace=True)) == (RELU, None)
    assert mpnn.act_spec(nn.LeakyReLU(0.25)) == (LRELU, 0.25) and mpnn.act_spec(nn.LeakyReLU()) == (LRELU, 0.01)
    assert mpnn.act_spec(nn.ELU()) == (ELU, 1.0) and mpnn.act_spec(nn.ELU(alpha=0.5)) == (ELU, 0.5)
    assert mpnn.act_spec(nn.SELU()) == (SELU, None) and mpnn.act_spec(nn.SiLU()) == (SILU, None)
    p = nn.PReLU()
    kind, slope = mpnn.act_spec(p)
    assert kind == PRELU and slope is p.weight

    class MyReLU(nn.ReLU):
        pass

    class MyPReLU(nn.PReLU):
        pass

    class Mine(nn.Module):
        def forward(self, x):
            return x
    for m in (MyReLU(), MyPReLU(), Mine(), nn.PReLU(8), nn.Tanh(), nn.GELU(), nn.Identity(), torch.relu, None):
        assert mpnn.act_spec(m) is None, m


def test_the_header_declares_the_kinds():
    text = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "mp_engine.h")).read()
    for name, v in (("NONE", NONE), ("RELU", RELU), ("LRELU", LRELU), ("PRELU", PRELU), ("ELU", ELU), ("SELU", SELU),
                    ("SILU", SILU)):
        assert f"#define MP_ACT_{name} {v}\n" in text


# ---- the C entries, before anything is launched ----------------------------------------------------------------------
def _fwd(N=10, d=8, act=ELU, slope=None, x=FAKE, y=FAKE, ldx=8, ldy=8, ws=FAKE, nb=1 << 30):
    return _lib.lib().mp_bn_train_fwd_act_f32(x, ldx, N, d, FAKE, FAKE, 1e-5, act, 1.0, slope, y, ldy, FAKE, FAKE, FAKE,
                                              ws, nb, None)


def _bwd(N=10, d=8, act=ELU, slope=None, dy=FAKE, x=FAKE, dx=FAKE, lddy=8, ws=FAKE, nb=1 << 30):
    return _lib.lib().mp_bn_train_bwd_act_f32(dy, lddy, x, 8, N, d, FAKE, FAKE, FAKE, FAKE, act, 1.0, slope, dx, 8,
                                              FAKE, FAKE, FAKE, ws, nb, None)


def _fwd_skip(N=10, d=8, d_skip=8, mode=SUM, act=ELU, slope=None, skip=FAKE, ldo=16, ws=FAKE, nb=1 << 30):
    return _lib.lib().mp_bn_train_fwd_skip_act_f32(FAKE, 8, skip, 8, N, d, d_skip, mode, FAKE, FAKE, 1e-5, act, 1.0,
                                                   slope, FAKE, ldo, FAKE, FAKE, FAKE, ws, nb, None)


def _bwd_skip(N=10, d=8, d_skip=8, mode=SUM, act=ELU, slope=None, skip=FAKE, lddy=16, dskip=FAKE, lddskip=8, ws=FAKE,
              nb=1 << 30):
    return _lib.lib().mp_bn_train_bwd_skip_act_f32(FAKE, lddy, FAKE, 8, skip, 8, N, d, d_skip, mode, FAKE, FAKE, FAKE,
                                                   FAKE, act, 1.0, slope, FAKE, 8, dskip, lddskip, FAKE, FAKE, FAKE, ws,
                                                   nb, None)


ENTRIES = {"fwd": _fwd, "bwd": _bwd, "fwd_skip": _fwd_skip, "bwd_skip": _bwd_skip}


@pytest.mark.parametrize("name", list(ENTRIES))
def test_entries_validate_their_arguments(name):
    call = ENTRIES[name]
    sym = {"fwd": "mp_bn_train_fwd_act_f32", "bwd": "mp_bn_train_bwd_act_f32",
           "fwd_skip": "mp_bn_train_fwd_skip_act_f32", "bwd_skip": "mp_bn_train_bwd_skip_act_f32"}[name]
    assert sym in _lib.PROTOTYPES and hasattr(_lib.lib(), sym)
    for act in (-1, 7, 100):
        assert call(act=act) == INVALID, act                   # an unknown kind
    assert call(act=PRELU, slope=None) == INVALID              # PRELU without its slope
    assert call(N=0) == INVALID and call(d=0) == INVALID
    # every kind passes the argument checks: the calls stop at the workspace they were not given
    for act in range(7):
        assert call(act=act, slope=FAKE if act == PRELU else None, nb=16) == WORKSPACE, act
        assert call(act=act, slope=FAKE if act == PRELU else None, ws=None) == WORKSPACE, act


def test_plain_entries_reject_short_rows_and_null_operands():
    assert _fwd(x=None) == INVALID and _fwd(y=None) == INVALID and _fwd(ldx=7) == INVALID and _fwd(ldy=7) == INVALID
    assert _bwd(dy=None) == INVALID and _bwd(x=None) == INVALID and _bwd(dx=None) == INVALID and _bwd(lddy=7) == INVALID


def test_skip_entries_reject_shapes_that_do_not_fit():
    for call in (_fwd_skip, _bwd_skip):
        assert call(mode=2) == INVALID and call(mode=-1) == INVALID
        assert call(mode=SUM, d_skip=4) == INVALID              # SUM needs d_skip == d
        assert call(d_skip=0) == INVALID and call(skip=None) == INVALID
    assert _fwd_skip(mode=CONCAT, ldo=15) == INVALID            # a row of out holds both slabs
    assert _fwd_skip(mode=SUM, ldo=7) == INVALID
    assert _bwd_skip(mode=CONCAT, lddy=15) == INVALID
    assert _bwd_skip(mode=CONCAT, d_skip=4, lddskip=3) == INVALID
    assert _bwd_skip(mode=CONCAT, d_skip=4, lddy=12, nb=16) == WORKSPACE


def test_workspace_query():
    lib = _lib.lib()
    nb, nb0 = C.c_size_t(0), C.c_size_t(0)
    assert lib.mp_bn_act_ws_bytes(-1, 8, C.byref(nb)) == INVALID and lib.mp_bn_act_ws_bytes(10, 0, C.byref(nb)) == INVALID
    assert lib.mp_bn_act_ws_bytes(10, 8, None) == INVALID
    for N, d in ((10, 8), (10 ** 7, 256), (333, 7)):
        assert lib.mp_bn_act_ws_bytes(N, d, C.byref(nb)) == 0 and lib.mp_bn_ws_bytes(N, d, C.byref(nb0)) == 0
        assert nb0.value < nb.value <= nb0.value + (1 << 16)      # the BatchNorm workspace plus PRELU's partial sums


# ---- the harness ------------------------------------------------------------------------------------------------------
def test_prelu_keeps_the_module_tree_and_the_state_dict(fresh_cfg):  # noqa: F811
    import graphgym_amd.graphgym_plugin  # noqa: F401
    from graphgym_amd import config, harness as H, nn as mpnn
    cfg = config.load_cfg(os.path.join(GOLDEN, "cfg_design_v2ogb.yaml"), target=fresh_cfg)
    assert cfg.gnn.act == "prelu"
    model = H.GNN(dim_in=9, dim_out=2)
    keys = set(model.state_dict())
    for i in range(cfg.gnn.layers_mp):
        post = getattr(model.mp, f"layer{i}").post_layer
        assert [type(m) for m in post] == [mpnn.BatchNorm1d, nn.PReLU] and post[0].relu is False
        assert mpnn.act_spec(post[1]) == (mpnn.ACT_PRELU, post[1].weight)
        assert {f"mp.layer{i}.post_layer.0.weight", f"mp.layer{i}.post_layer.0.running_mean",
                f"mp.layer{i}.post_layer.1.weight"} <= keys
    assert "pre_mp.Layer_0.post_layer.1.weight" in keys
    # on the host the layer is the composition: Sequential's own result
    layer = H.GeneralLayer("linear", 6, 5).train()
    x = torch.randn(12, 6)
    ref = layer.post_layer(layer.layer(x))
    layer.post_layer[0].reset_running_stats()
    assert torch.equal(layer(x), ref)
    # relu keeps its fused BatchNorm and no activation module
    cfg.gnn.act = "relu"
    post = H.GeneralLayer("linear", 6, 5).post_layer
    assert len(post) == 1 and post[0].relu is True


def test_bn_act_module_on_the_host_is_the_composition():
    from graphgym_amd import nn as mpnn
    torch.manual_seed(0)
    x, skip = torch.randn(20, 6), torch.randn(20, 6)
    for act in (nn.PReLU(), nn.ELU(), nn.SiLU(), nn.PReLU(6), nn.Tanh()):
        a, b = mpnn.BatchNorm1d(6), nn.BatchNorm1d(6)
        assert torch.equal(mpnn.bn_act_module(a, x, act), act(b(x)))
        assert torch.equal(a.running_mean, b.running_mean) and int(a.num_batches_tracked) == 1
        a, b = mpnn.BatchNorm1d(6), nn.BatchNorm1d(6)
        assert torch.equal(mpnn.bn_skip_act(a, x, skip, "skipsum", act=act), act(skip + b(x)))
        if not (isinstance(act, nn.PReLU) and act.num_parameters > 1):      # six slopes do not fit twelve columns
            assert torch.equal(mpnn.bn_skip_act(a, x, skip, "skipconcat", act=act), act(torch.cat((skip, b(x)), 1)))
