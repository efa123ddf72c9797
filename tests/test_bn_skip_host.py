"""The skip stages without a device: argument validation of mp_bn_train_fwd_skip_f32 / mp_bn_train_bwd_skip_f32 on the C
ABI (every refusal happens before a launch), schemas and fake kernels of mp::bn_skip_fwd_raw / bn_skip_bwd_raw /
bn_skip_act, the schemas of every other BatchNorm op and what the four *actx_bwd_raw ops return empty,
cfg.gnn.skip_every, the module tree of harness.GNN with stage_type skipsum / skipconcat against key lists written
from graphgym/models/gnn.py:30-44, 84-102, and graphgym_plugin.accelerate() on a reference-style skip block."""
import ctypes as C
import itertools

import pytest
import torch
import torch.nn as nn

from _skip_ref import RefStyleSkipBlock
from graphgym_amd import _lib

INVALID, WORKSPACE = 1, 3
SUM, CONCAT = 0, 1


@pytest.fixture()
def fake():
    """non-NULL operands that no refused call touches: the addresses of small host buffers"""
    bufs = [(C.c_float * 64)() for _ in range(10)]
    return [C.c_void_p(C.addressof(b)) for b in bufs]


def _ws_bytes(N, d):
    nb = C.c_size_t(0)
    assert _lib.lib().mp_bn_ws_bytes(N, d, C.byref(nb)) == 0
    return nb.value


def _fwd(p, **kw):
    a = dict(x=p[0], ldx=8, skip=p[1], ldskip=8, N=4, d=8, d_skip=8, mode=SUM, gamma=p[2], beta=p[3], relu=1, out=p[4],
             ldo=8, mean=p[5], invstd=p[6], var=p[7], ws=p[8], ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = _ws_bytes(max(a["N"], 1), max(a["d"], 1))
    return _lib.lib().mp_bn_train_fwd_skip_f32(a["x"], a["ldx"], a["skip"], a["ldskip"], a["N"], a["d"], a["d_skip"],
                                               a["mode"], a["gamma"], a["beta"], 1e-5, a["relu"], a["out"], a["ldo"],
                                               a["mean"], a["invstd"], a["var"], a["ws"], a["ws_bytes"], None)


def _bwd(p, **kw):
    a = dict(dy=p[0], lddy=8, out=p[1], ldo=8, x=p[2], ldx=8, N=4, d=8, gamma=p[3], mean=p[4], invstd=p[5], dx=p[6],
             lddx=8, dskip=p[7], lddskip=8, dgamma=p[8], dbeta=p[9], ws=p[8], ws_bytes=None)
    a.update(kw)
    if a["ws_bytes"] is None:
        a["ws_bytes"] = _ws_bytes(max(a["N"], 1), max(a["d"], 1))
    return _lib.lib().mp_bn_train_bwd_skip_f32(a["dy"], a["lddy"], a["out"], a["ldo"], a["x"], a["ldx"], a["N"], a["d"],
                                               a["gamma"], a["mean"], a["invstd"], a["dx"], a["lddx"], a["dskip"],
                                               a["lddskip"], a["dgamma"], a["dbeta"], a["ws"], a["ws_bytes"], None)


@pytest.mark.parametrize("bad", [dict(x=None), dict(skip=None), dict(out=None), dict(mean=None), dict(invstd=None),
                                 dict(var=None), dict(N=0), dict(N=-3), dict(d=0), dict(d_skip=0), dict(d_skip=-1),
                                 dict(ldx=7), dict(ldskip=7), dict(ldo=7), dict(mode=2), dict(mode=-1),
                                 dict(mode=SUM, d_skip=4, ldskip=4),                       # SUM needs d_skip == d
                                 dict(mode=CONCAT, d_skip=4, ldo=11),                      # CONCAT: ldo >= d_skip + d
                                 dict(mode=CONCAT, ldo=8)])
def test_forward_refuses_bad_arguments_before_any_launch(fake, bad):
    assert _fwd(fake, **bad) == INVALID


def test_forward_refuses_a_short_workspace(fake):
    need = _ws_bytes(4, 8)
    assert _fwd(fake, ws_bytes=need - 1) == WORKSPACE
    assert _fwd(fake, ws=None) == WORKSPACE
    assert _fwd(fake, mode=CONCAT, d_skip=4, ldo=12, ws_bytes=0) == WORKSPACE      # valid arguments get this far
    assert _fwd(fake, N=0, ws_bytes=0) == INVALID                                  # the arguments are judged first


@pytest.mark.parametrize("bad", [dict(dy=None), dict(x=None), dict(mean=None), dict(invstd=None), dict(dx=None),
                                 dict(dskip=None),                                         # required with out (ReLU)
                                 dict(N=0), dict(d=0), dict(lddy=7), dict(ldo=7), dict(ldx=7), dict(lddx=7),
                                 dict(lddskip=7)])
def test_backward_refuses_bad_arguments_before_any_launch(fake, bad):
    assert _bwd(fake, **bad) == INVALID


def test_backward_refuses_a_short_workspace(fake):
    need = _ws_bytes(4, 8)
    assert _bwd(fake, ws_bytes=need - 1) == WORKSPACE
    assert _bwd(fake, ws=None) == WORKSPACE
    # without the activation (out NULL) d(skip) is dy itself: dskip may be NULL and its stride is not looked at
    assert _bwd(fake, out=None, ldo=0, dskip=None, lddskip=0, ws_bytes=0) == WORKSPACE


_T4, _T5 = " -> (Tensor, Tensor, Tensor, Tensor)", " -> (Tensor, Tensor, Tensor, Tensor, Tensor)"
_ACTX = "Tensor? weight, Tensor? bias, Tensor? slope, float eps, SymInt kind, float param"
_ACTX_BWD = "Tensor? weight, Tensor? bias, Tensor? slope, Tensor mean, Tensor invstd"
_KEY = "SymInt T, SymInt seed, SymInt offset"
# the public signatures of the other BatchNorm ops and of dropout_keyed, without the "mp::<name>"
_OTHER_SCHEMAS = {
    "bn_fwd_raw": "(Tensor x, Tensor? weight, Tensor? bias, float eps, bool relu)" + _T4,
    "bn_bwd_raw": "(Tensor dy, Tensor? y, Tensor x, Tensor? weight, Tensor mean, Tensor invstd, Tensor? bias=None, "
                  "bool relu_from_x=False) -> (Tensor, Tensor, Tensor)",
    "bn_act": "(Tensor x, Tensor? weight, Tensor? bias, float eps, bool relu)" + _T4,
    "bn_actx_fwd_raw": f"(Tensor x, {_ACTX})" + _T4,
    "bn_actx_bwd_raw": f"(Tensor dy, Tensor x, {_ACTX_BWD}, SymInt kind, float param, bool want_dslope=True)" + _T4,
    "bn_actx": f"(Tensor x, {_ACTX})" + _T4,
    "bn_skip_actx_fwd_raw": f"(Tensor x, Tensor skip, {_ACTX}, SymInt mode)" + _T4,
    "bn_skip_actx_bwd_raw": f"(Tensor dy, Tensor x, Tensor skip, {_ACTX_BWD}, SymInt mode, SymInt kind, float param, "
                            "bool want_dskip=True, bool want_dslope=True)" + _T5,
    "bn_skip_actx": f"(Tensor x, Tensor skip, {_ACTX}, SymInt mode)" + _T4,
    "bn_drop_actx_fwd_raw": f"(Tensor x, {_ACTX}, {_KEY})" + _T4,
    "bn_drop_actx_bwd_raw": f"(Tensor dy, Tensor x, {_ACTX_BWD}, SymInt kind, float param, {_KEY}, "
                            "bool want_dslope=True)" + _T4,
    "bn_drop_actx": f"(Tensor x, {_ACTX}, {_KEY})" + _T4,
    "bn_drop_skip_actx_fwd_raw": f"(Tensor x, Tensor skip, {_ACTX}, SymInt mode, {_KEY})" + _T4,
    "bn_drop_skip_actx_bwd_raw": f"(Tensor dy, Tensor x, Tensor skip, {_ACTX_BWD}, SymInt mode, SymInt kind, "
                                 f"float param, {_KEY}, bool want_dskip=True, bool want_dslope=True)" + _T5,
    "bn_drop_skip_actx": f"(Tensor x, Tensor skip, {_ACTX}, SymInt mode, {_KEY})" + _T4,
    "dropout_keyed": "(Tensor x, SymInt T, SymInt seed, SymInt offset) -> Tensor",
}


def test_schemas_and_fake_kernels():
    from torch._subclasses.fake_tensor import FakeTensorMode
    import graphgym_amd.nn as mpnn
    assert (mpnn.SKIP_SUM, mpnn.SKIP_CONCAT) == (SUM, CONCAT)
    ops = torch.ops.mp
    assert str(ops.bn_skip_fwd_raw.default._schema) == (
        "mp::bn_skip_fwd_raw(Tensor x, Tensor skip, Tensor? weight, Tensor? bias, float eps, bool relu, SymInt mode) -> "
        "(Tensor, Tensor, Tensor, Tensor)")
    assert str(ops.bn_skip_act.default._schema) == (
        "mp::bn_skip_act(Tensor x, Tensor skip, Tensor? weight, Tensor? bias, float eps, bool relu, SymInt mode) -> "
        "(Tensor, Tensor, Tensor, Tensor)")
    assert str(ops.bn_skip_bwd_raw.default._schema) == (
        "mp::bn_skip_bwd_raw(Tensor dy, Tensor? out, Tensor x, Tensor? weight, Tensor mean, Tensor invstd, SymInt mode, "
        "bool want_dskip=True) -> (Tensor, Tensor, Tensor, Tensor)")
    fake_mode = FakeTensorMode()
    with fake_mode:
        N, d, ds = 11, 8, 6
        x, w, b = torch.empty(N, d, device="cuda"), torch.empty(d, device="cuda"), torch.empty(d, device="cuda")
        for op in (ops.bn_skip_fwd_raw, ops.bn_skip_act):
            out, mean, invstd, var = op(x, torch.empty(N, d, device="cuda"), w, b, 1e-5, True, SUM)
            assert out.shape == (N, d) and mean.shape == invstd.shape == var.shape == (d,)
            out, mean, invstd, var = op(x, torch.empty(N, ds, device="cuda"), None, None, 1e-5, False, CONCAT)
            assert out.shape == (N, ds + d) and out.dtype == torch.float32 and mean.shape == (d,)
        st = torch.empty(d, device="cuda")
        dy = torch.empty(N, d, device="cuda")
        dx, dg, db, dskip = ops.bn_skip_bwd_raw(dy, dy, x, w, st, st, SUM)
        assert dx.shape == (N, d) and dg.shape == db.shape == (d,) and dskip.shape == (N, d)
        assert ops.bn_skip_bwd_raw(dy, None, x, w, st, st, SUM)[3].numel() == 0          # d(skip) is dy itself
        assert ops.bn_skip_bwd_raw(dy, dy, x, w, st, st, SUM, False)[3].numel() == 0
        dyc = torch.empty(N, ds + d, device="cuda")
        dx, dg, db, dskip = ops.bn_skip_bwd_raw(dyc, dyc, x, w, st, st, CONCAT)
        assert dx.shape == (N, d) and dskip.shape == (N, ds)
    for name, schema in _OTHER_SCHEMAS.items():
        assert str(getattr(ops, name).default._schema) == f"mp::{name}{schema}", name
    # the four *actx_bwd_raw ops: dskip comes back EMPTY unless asked for AND there is an activation, dslope unless asked
    # for AND the kind is PRELU; everything else has its shape whatever is asked
    NONE, RELU, PRELU = mpnn.ACT_NONE, mpnn.ACT_RELU, mpnn.ACT_PRELU
    key = (20000, 5, 7)
    with fake_mode:
        sl = torch.empty(1, device="cuda")
        for fam, extra in (("bn_actx", ()), ("bn_drop_actx", key)):         # the forward fakes of the other families
            for op in (getattr(ops, fam), getattr(ops, fam + "_fwd_raw")):
                res = op(x, w, b, None, 1e-5, RELU, 0.0, *extra)
                assert [tuple(t.shape) for t in res] == [(N, d), (d,), (d,), (d,)], fam
                assert all(t.dtype == torch.float32 for t in res), fam
        for fam, extra in (("bn_skip_actx", ()), ("bn_drop_skip_actx", key)):
            for op, mode in itertools.product((getattr(ops, fam), getattr(ops, fam + "_fwd_raw")), (SUM, CONCAT)):
                skip = torch.empty(N, d if mode == SUM else ds, device="cuda")
                res = op(x, skip, w, b, sl, 1e-5, PRELU, 0.0, mode, *extra)
                assert [tuple(t.shape) for t in res] == [(N, skip.size(1) + (d if mode == CONCAT else 0)), (d,), (d,), (d,)]
        assert [tuple(t.shape) for t in ops.bn_bwd_raw(dy, None, x, w, st, st)] == [(N, d), (d,), (d,)]
        for kind, want_dskip, want_dslope, mode in itertools.product((NONE, RELU, PRELU), (True, False), (True, False),
                                                                     (SUM, CONCAT)):
            s = sl if kind == PRELU else None
            skip = torch.empty(N, d if mode == SUM else ds, device="cuda")
            dyk = dy if mode == SUM else dyc
            plain = [ops.bn_actx_bwd_raw(dy, x, w, b, s, st, st, kind, 0.0, want_dslope),
                     ops.bn_drop_actx_bwd_raw(dy, x, w, b, s, st, st, kind, 0.0, *key, want_dslope)]
            wants = (want_dskip, want_dslope)
            skipped = [ops.bn_skip_actx_bwd_raw(dyk, x, skip, w, b, s, st, st, mode, kind, 0.0, *wants),
                       ops.bn_drop_skip_actx_bwd_raw(dyk, x, skip, w, b, s, st, st, mode, kind, 0.0, *key, *wants)]
            for res, n_results in [(r, 4) for r in plain] + [(r, 5) for r in skipped]:
                what = (kind, want_dskip, want_dslope, mode, n_results)
                assert len(res) == n_results, what
                assert all(isinstance(t, torch.Tensor) and t.dtype == torch.float32 and t.is_cuda for t in res), what
                dx, dg, db, dslope = res[0], res[1], res[2], res[-1]
                assert dx.shape == (N, d) and dg.shape == db.shape == (d,), what
                assert dslope.shape == ((1,) if (kind == PRELU and want_dslope) else (0,)), what
            for res in skipped:
                assert res[3].shape == (skip.shape if (want_dskip and kind != NONE) else (0,)), (kind, want_dskip, mode)


def test_bn_skip_act_outside_the_kernels_domain_is_the_torch_composition():
    """CPU tensors, eval mode, another activation: act(skip + bn(x)) / act(cat(skip, bn(x))), running statistics
    updated by the module itself"""
    import graphgym_amd.nn as mpnn
    g = torch.Generator().manual_seed(0)
    x, s = torch.randn(9, 4, generator=g), torch.randn(9, 4, generator=g)
    for cls in (nn.BatchNorm1d, mpnn.BatchNorm1d):
        for mode, comb in (("skipsum", lambda a, b: a + b), ("skipconcat", lambda a, b: torch.cat((a, b), 1))):
            bn, ref = cls(4), nn.BatchNorm1d(4)
            got = mpnn.bn_skip_act(bn, x, s, mode)
            assert torch.equal(got, torch.relu(comb(s, ref(x))))
            assert torch.equal(bn.running_mean, ref.running_mean) and int(bn.num_batches_tracked) == 1
            assert torch.equal(mpnn.bn_skip_act(bn, x, s, mode, relu=False), comb(s, ref(x)))
            assert torch.equal(mpnn.bn_skip_act(bn, x, s, mode, act=torch.tanh), torch.tanh(comb(s, ref(x))))
            bn.eval(), ref.eval()
            assert torch.equal(mpnn.bn_skip_act(bn, x, s, mode), torch.relu(comb(s, ref(x))))
    with pytest.raises(ValueError):
        mpnn.bn_skip_act(nn.BatchNorm1d(4), x, torch.randn(9, 5), "skipsum")
    with pytest.raises(KeyError):
        mpnn.bn_skip_act(nn.BatchNorm1d(4), x, s, "stack")


def test_skip_every_default():
    from graphgym_amd.config import _defaults
    assert _defaults().gnn.skip_every == 1


# ---- the module tree ------------------------------------------------------------------------------------------------
@pytest.fixture()
def gcfg():
    from graphgym_amd.config import cfg
    saved = {k: dict(vars(getattr(cfg, k))) for k in ("gnn", "dataset", "bn", "mem")}
    cfg.gnn.layers_pre_mp, cfg.gnn.dim_inner, cfg.gnn.layers_post_mp = 1, 16, 1
    cfg.gnn.batchnorm, cfg.gnn.dropout, cfg.gnn.act = True, 0.0, "relu"
    cfg.dataset.task = "node"
    yield cfg
    for k, v in saved.items():
        ns = getattr(cfg, k)
        for name in list(vars(ns)):
            if name not in v:
                delattr(ns, name)
        for name, val in v.items():
            setattr(ns, name, val)


_BN = [("weight", (16,)), ("bias", (16,)), ("running_mean", (16,)), ("running_var", (16,)), ("num_batches_tracked", ())]


def _expected_keys(stage, layers_mp, skip_every, layer_type, F_in=8, D=16, C_out=3):
    """gnn.py:30-44 (block: f = Sequential of skip_every GeneralLayers, every one conv -> BatchNorm1d since
    cfg.gnn.batchnorm), gnn.py:84-102 (stage: block{i}; skipconcat feeds block i with D + i * D columns and hands
    d_in_last + D to the head); conv weights are [dim_in, dim_out], generalconv adds weight_self (self_msg = concat)"""
    keys = [("pre_mp.Layer_0.layer.model.weight", (D, F_in))] + [(f"pre_mp.Layer_0.post_layer.0.{n}", s) for n, s in _BN]
    d_in = D
    for i in range(layers_mp // skip_every):
        d_in = D if (stage == "skipsum" or i == 0) else D + i * D
        for j in range(skip_every):
            w_in = d_in if j == 0 else D
            keys.append((f"mp.block{i}.f.{j}.layer.model.weight", (w_in, D)))
            if layer_type == "generalconv":
                keys.append((f"mp.block{i}.f.{j}.layer.model.weight_self", (w_in, D)))
            keys += [(f"mp.block{i}.f.{j}.post_layer.0.{n}", s) for n, s in _BN]
    head_in = d_in + D if stage == "skipconcat" else D
    return keys + [("post_mp.layer_post_mp.model.0.model.weight", (C_out, head_in)),
                   ("post_mp.layer_post_mp.model.0.model.bias", (C_out,))]


@pytest.mark.parametrize("stage,layers_mp,skip_every,layer_type",
                         list(itertools.product(["skipsum", "skipconcat"], [2, 4], [1, 2], ["gcnconv", "generalconv"])))
def test_state_dict_keys_are_the_references(gcfg, stage, layers_mp, skip_every, layer_type):
    from graphgym_amd import harness
    import graphgym_amd.graphgym_plugin  # noqa: F401  (registers the layer keys)
    gcfg.gnn.stage_type, gcfg.gnn.layers_mp, gcfg.gnn.skip_every, gcfg.gnn.layer_type = stage, layers_mp, skip_every, layer_type
    model = harness.GNN(8, 3)
    got = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    assert got == _expected_keys(stage, layers_mp, skip_every, layer_type)
    blocks = list(model.mp.children())
    assert len(blocks) == layers_mp // skip_every and all(type(b) is harness.GNNSkipBlock for b in blocks)
    for b in blocks:        # the last layer of a block has no activation of its own, the others fuse theirs
        assert [bool(l.post_layer[0].relu) for l in b.f] == [True] * (skip_every - 1) + [False]
        assert isinstance(b.act, nn.ReLU)


def test_the_explicit_key_list_of_one_case():
    """the generator above, spelled out once: skipconcat, 2 layers, skip_every 1, gcnconv"""
    bn = lambda p: [p + ".weight", p + ".bias", p + ".running_mean", p + ".running_var", p + ".num_batches_tracked"]  # noqa: E731
    want = (["pre_mp.Layer_0.layer.model.weight"] + bn("pre_mp.Layer_0.post_layer.0")
            + ["mp.block0.f.0.layer.model.weight"] + bn("mp.block0.f.0.post_layer.0")
            + ["mp.block1.f.0.layer.model.weight"] + bn("mp.block1.f.0.post_layer.0")
            + ["post_mp.layer_post_mp.model.0.model.weight", "post_mp.layer_post_mp.model.0.model.bias"])
    exp = _expected_keys("skipconcat", 2, 1, "gcnconv")
    assert [k for k, _ in exp] == want
    assert dict(exp)["mp.block1.f.0.layer.model.weight"] == (32, 16)
    assert dict(exp)["post_mp.layer_post_mp.model.0.model.weight"] == (3, 48)


def test_stage_assertions_and_unknown_key(gcfg):
    from graphgym_amd import harness
    import graphgym_amd.graphgym_plugin  # noqa: F401
    gcfg.gnn.layer_type, gcfg.gnn.stage_type = "gcnconv", "skipsum"
    gcfg.gnn.layers_mp, gcfg.gnn.skip_every = 3, 2
    with pytest.raises(AssertionError):
        harness.GNN(8, 3)
    gcfg.gnn.layers_mp, gcfg.gnn.skip_every = 2, 1
    with pytest.raises(AssertionError):
        harness.GNNSkipStage(dim_in=8, dim_out=16, num_layers=2)          # skipsum: dim_in == dim_out
    with pytest.raises(AssertionError):
        harness.GNNSkipBlock(8, 16, 1)
    assert set(harness.stage_dict) == {"stack", "skipsum", "skipconcat"}
    gcfg.gnn.stage_type = "stack"
    assert type(harness.GNN(8, 3).mp) is harness.GNNStackStage
    gcfg.gnn.stage_type = "skipmul"
    with pytest.raises(ValueError):
        harness.GNN(8, 3)


# ---- accelerate() on the reference's block, written with plain torch modules ------------------------------------------
def test_accelerate_patches_a_skip_block_once_and_keeps_the_state_dict():
    import graphgym_amd.graphgym_plugin as plugin
    from graphgym_amd import layers as L, nn as mpnn
    model = nn.Sequential(RefStyleSkipBlock(L.GCNConv, 16, 16, 2), RefStyleSkipBlock(L.GCNConv, 16, 16, 1))
    keys = list(model.state_dict().keys())
    params = list(model.parameters())
    bn = model[0].f[1].post_layer[0]
    w, rm = bn.weight, bn.running_mean
    assert plugin.accelerate(model) == 3                     # the three layer wrappers; the two blocks are not counted
    for blk in model:
        assert "forward" in vars(blk) and hasattr(blk, "_mp_orig_block_forward")
    first = [vars(blk)["forward"] for blk in model]
    origs = [blk._mp_orig_block_forward for blk in model]
    assert plugin.accelerate(model) == 3                     # idempotent: nothing is patched twice
    assert all(vars(blk)["forward"] is f and blk._mp_orig_block_forward is o for blk, f, o in zip(model, first, origs))
    assert list(model.state_dict().keys()) == keys
    assert all(a is b for a, b in zip(model.parameters(), params))
    new = model[0].f[1].post_layer[0]
    assert isinstance(new, mpnn.BatchNorm1d) and new.relu is False and new.weight is w and new.running_mean is rm
    assert model[0].f[0].post_layer[0].relu is True
    # a module that merely has `.f` is no skip block
    plain = nn.Sequential(nn.Linear(4, 4))
    holder = nn.Module()
    holder.f, holder.act = plain, nn.ReLU()
    assert plugin.accelerate(holder) == 0 and "forward" not in vars(holder)
