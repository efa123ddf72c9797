"""The host side of the keyed dropout (csrc/draws.h keep(), csrc/bn_drop.hip): graphgym_amd.nn.dropout_keep_host against a
scalar restatement of the definition, the statistics of the draw, graphgym_amd.nn.Dropout on CPU tensors, the argument
checks of the three C entries before anything is launched, and the harness's module tree under gnn.keyed_dropout.  No
device work here."""
import ctypes as C
import math

import pytest
import torch
import torch.nn as nn

from graphgym_amd import _lib
from test_ogb_host import fresh_cfg  # noqa: F401

INVALID, WORKSPACE = 1, 3
FAKE = C.c_void_p(4096)         # never dereferenced: every call below is refused before a launch
NONE, RELU, LRELU, PRELU, ELU, SELU, SILU = range(7)
SUM, CONCAT = 0, 1
M64 = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
SEED = 20240613                 # the seed of the statistical checks: test_zero_rate shows it satisfies them
N, D = 4096, 256


def _mix(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _keep_scalar(seed, offset, r, c, d, T):
    """csrc/draws.h, one element at a time in Python integers"""
    q = (d + 3) // 4
    key = _mix((_mix((seed + G) & M64) ^ offset) + G & M64)
    h = _mix(((key ^ ((r * q + c // 4) & M64)) + G) & M64)
    return ((h >> (16 * (c % 4))) & 0xFFFF) >= T


def _sigma(p, n):
    return math.sqrt(n * p * (1 - p)) / n


# ---- the draw ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N_,d,seed,offset,p", [(5, 7, 1, 0, 0.3), (3, 8, 2 ** 63 + 5, 2 ** 64 - 1, 0.6), (4, 1, 7, 3, 0.5),
                                                (2, 1028, 99, 12345678901234, 0.1), (9, 5, 0, 0, 0.9)])
def test_keep_host_is_the_definition(N_, d, seed, offset, p):
    from graphgym_amd import nn as mpnn
    T = mpnn.dropout_threshold(p)
    got = mpnn.dropout_keep_host(seed, offset, N_, d, p)
    assert got.dtype == torch.bool and got.shape == (N_, d)
    want = torch.tensor([[_keep_scalar(seed & M64, offset & M64, r, c, d, T) for c in range(d)] for r in range(N_)])
    assert torch.equal(got, want)


def test_threshold_and_scale():
    from graphgym_amd import nn as mpnn
    assert mpnn.dropout_threshold(0.0) == 0 and mpnn.dropout_threshold(1.0) == 65536
    assert mpnn.dropout_threshold(0.5) == 32768 and mpnn.dropout_threshold(0.1) == 6554
    assert mpnn.dropout_scale(0.0) == 1.0 and mpnn.dropout_scale(1.0) == 0.0 and mpnn.dropout_scale(0.5) == 2.0
    s = mpnn.dropout_scale(0.1)
    assert s == float(torch.tensor(65536.0 / (65536 - 6554), dtype=torch.float64).float())     # fp32, rounded once
    for bad in (-0.1, 1.5):
        with pytest.raises(ValueError):
            mpnn.dropout_threshold(bad)


@pytest.mark.parametrize("p", [0.1, 0.3, 0.6])
def test_zero_rate(p):
    from graphgym_amd import nn as mpnn
    keep = mpnn.dropout_keep_host(SEED, 0, N, D, p)
    pe = mpnn.dropout_threshold(p) / 65536
    rate = 1.0 - float(keep.double().mean())
    assert abs(rate - pe) <= 5 * _sigma(pe, N * D), (rate, pe)


@pytest.mark.parametrize("p", [0.1, 0.3, 0.6])
def test_no_structure(p):
    from graphgym_amd import nn as mpnn
    keep = mpnn.dropout_keep_host(SEED, 0, N, D, p)
    pe = mpnn.dropout_threshold(p) / 65536
    # every column at its own n
    col = 1.0 - keep.double().mean(0)
    assert float((col - pe).abs().max()) <= 5 * _sigma(pe, N), float((col - pe).abs().max())
    # the four columns of one hash: two independent draws agree with probability p^2 + q^2
    agree = pe * pe + (1 - pe) * (1 - pe)
    lanes = keep.reshape(N, D // 4, 4)
    n = N * (D // 4)
    for i in range(4):
        for j in range(i + 1, 4):
            got = float((lanes[:, :, i] == lanes[:, :, j]).double().mean())
            assert got <= agree + 5 * _sigma(agree, n), (i, j, got, agree)
    # consecutive call offsets
    nxt = mpnn.dropout_keep_host(SEED, 1, N, D, p)
    got = float((keep == nxt).double().mean())
    assert got <= agree + 5 * _sigma(agree, N * D), (got, agree)
    # and consecutive rows, consecutive groups
    for a, b in ((keep[1:], keep[:-1]), (lanes[:, 1:], lanes[:, :-1])):
        got = float((a == b).double().mean())
        assert got <= agree + 5 * _sigma(agree, a.numel()), (got, agree)


def test_edges():
    from graphgym_amd import nn as mpnn
    assert bool(mpnn.dropout_keep_host(SEED, 0, 64, 12, 0.0).all())
    assert not bool(mpnn.dropout_keep_host(SEED, 0, 64, 12, 1.0).any())
    # the mask at width d is the function of ceil(d / 4): 5 and 8 share their groups, 7 and 9 do not
    a, b = mpnn.dropout_keep_host(SEED, 3, 50, 5, 0.5), mpnn.dropout_keep_host(SEED, 3, 50, 8, 0.5)
    assert torch.equal(a, b[:, :5])
    a, b = mpnn.dropout_keep_host(SEED, 3, 50, 7, 0.5), mpnn.dropout_keep_host(SEED, 3, 50, 9, 0.5)
    assert torch.equal(a[0], b[0, :7]) and not torch.equal(a[1:], b[1:, :7])      # row 0 starts at group 0 either way
    # the seed and the offset both move the mask
    base = mpnn.dropout_keep_host(SEED, 3, 50, 8, 0.5)
    assert not torch.equal(base, mpnn.dropout_keep_host(SEED + 1, 3, 50, 8, 0.5))
    assert not torch.equal(base, mpnn.dropout_keep_host(SEED, 4, 50, 8, 0.5))
    assert not torch.equal(mpnn.dropout_keep_host(3, 4, 50, 8, 0.5), mpnn.dropout_keep_host(4, 3, 50, 8, 0.5))


# ---- the module on CPU tensors -----------------------------------------------------------------------------------------
def test_dropout_module_on_the_host():
    from graphgym_amd import nn as mpnn
    x = torch.randn(37, 7)
    drop = mpnn.Dropout(0.3, seed=11)
    assert isinstance(drop, nn.Dropout) and drop.p == 0.3 and drop.p_effective == 19661 / 65536 and drop.step == 0
    assert drop.eval()(x) is x and drop.step == 0                      # eval: the identity, no counter value taken
    drop.train()
    out = drop(x)
    keep = mpnn.dropout_keep_host(11, 0, 37, 7, 0.3)
    assert torch.equal(out, x * keep.float() * mpnn.dropout_scale(0.3)) and drop.step == 1
    assert 0 < int(keep.sum()) < keep.numel()
    out2 = drop(x)
    assert drop.step == 2 and not torch.equal(out2, out)
    assert torch.equal(out2, x * mpnn.dropout_keep_host(11, 1, 37, 7, 0.3).float() * mpnn.dropout_scale(0.3))
    drop.set_stream(11, 0)
    assert torch.equal(drop(x), out) and drop.step == 1                # a call reproduced
    # p = 0: the identity, no counter; p = 1: zeros
    zero = mpnn.Dropout(0.0).train()
    assert zero(x) is x and zero.step == 0
    assert not bool(mpnn.Dropout(1.0, seed=1).train()(x).any())
    # float64 input keeps its dtype; autograd sees the mask
    xd = x.double().requires_grad_(True)
    drop.set_stream(11, 0)
    y = drop(xd)
    assert y.dtype == torch.float64
    y.sum().backward()
    assert torch.equal(xd.grad, keep.double() * mpnn.dropout_scale(0.3))


def test_seeds_come_from_the_default_generator():
    from graphgym_amd import nn as mpnn
    torch.manual_seed(5)
    a, b = mpnn.Dropout(0.1), mpnn.Dropout(0.1)
    torch.manual_seed(5)
    c, d = mpnn.Dropout(0.1), mpnn.Dropout(0.1)
    assert a.seed != b.seed and (a.seed, b.seed) == (c.seed, d.seed)
    assert all(isinstance(m.seed, int) and 0 <= m.seed < 2 ** 63 for m in (a, b))
    assert mpnn.Dropout(0.1, seed=42).seed == 42
    assert list(mpnn.Dropout(0.1).state_dict()) == []                 # no parameters, no buffers: state-dict keys unchanged


# ---- the C entries, before anything is launched ------------------------------------------------------------------------
def _fwd(N=10, d=8, act=ELU, slope=None, T=100, x=FAKE, y=FAKE, ldx=8, ldy=8, ws=FAKE, nb=1 << 30):
    return _lib.lib().mp_bn_train_fwd_drop_act_f32(x, ldx, N, d, FAKE, FAKE, 1e-5, act, 1.0, slope, T, 1, 2, y, ldy, FAKE,
                                                   FAKE, FAKE, ws, nb, None)


def _bwd(N=10, d=8, act=ELU, slope=None, T=100, dy=FAKE, x=FAKE, dx=FAKE, lddy=8, ws=FAKE, nb=1 << 30):
    return _lib.lib().mp_bn_train_bwd_drop_act_f32(dy, lddy, x, 8, N, d, FAKE, FAKE, FAKE, FAKE, act, 1.0, slope, T, 1, 2,
                                                   dx, 8, FAKE, FAKE, FAKE, ws, nb, None)


def _fwd_skip(N=10, d=8, d_skip=8, mode=SUM, act=ELU, slope=None, T=100, skip=FAKE, ldo=16, ws=FAKE, nb=1 << 30):
    return _lib.lib().mp_bn_train_fwd_drop_skip_act_f32(FAKE, 8, skip, 8, N, d, d_skip, mode, FAKE, FAKE, 1e-5, act, 1.0,
                                                        slope, T, 1, 2, FAKE, ldo, FAKE, FAKE, FAKE, ws, nb, None)


def _bwd_skip(N=10, d=8, d_skip=8, mode=SUM, act=ELU, slope=None, T=100, skip=FAKE, lddy=16, dskip=FAKE, lddskip=8,
              ws=FAKE, nb=1 << 30):
    return _lib.lib().mp_bn_train_bwd_drop_skip_act_f32(FAKE, lddy, FAKE, 8, skip, 8, N, d, d_skip, mode, FAKE, FAKE, FAKE,
                                                        FAKE, act, 1.0, slope, T, 1, 2, FAKE, 8, dskip, lddskip, FAKE,
                                                        FAKE, FAKE, ws, nb, None)


def _mask(N=10, d=8, T=100, x=FAKE, out=FAKE, ldx=8, ldo=8):
    return _lib.lib().mp_dropout_keyed_f32(x, ldx, N, d, T, 1, 2, out, ldo, None)


ENTRIES = {"fwd": (_fwd, "mp_bn_train_fwd_drop_act_f32"), "bwd": (_bwd, "mp_bn_train_bwd_drop_act_f32"),
           "fwd_skip": (_fwd_skip, "mp_bn_train_fwd_drop_skip_act_f32"),
           "bwd_skip": (_bwd_skip, "mp_bn_train_bwd_drop_skip_act_f32")}


@pytest.mark.parametrize("name", list(ENTRIES))
def test_entries_validate_their_arguments(name):
    call, sym = ENTRIES[name]
    assert sym in _lib.PROTOTYPES and hasattr(_lib.lib(), sym)
    for act in (-1, 7, 100):
        assert call(act=act) == INVALID, act                   # an unknown kind
    assert call(act=PRELU, slope=None) == INVALID              # PRELU without its slope
    assert call(N=0) == INVALID and call(d=0) == INVALID
    for T in (-1, 65537, 1 << 20):
        assert call(T=T) == INVALID, T                         # a rate outside [0, 1]
    # every kind — MP_ACT_NONE too — and both ends of T pass the argument checks: the calls stop at the workspace
    for act in range(7):
        for T in (0, 100, 65536):
            assert call(act=act, T=T, slope=FAKE if act == PRELU else None, nb=16) == WORKSPACE, (act, T)
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


def test_the_mask_entry_validates_its_arguments():
    assert "mp_dropout_keyed_f32" in _lib.PROTOTYPES and hasattr(_lib.lib(), "mp_dropout_keyed_f32")
    assert _mask(x=None) == INVALID and _mask(out=None) == INVALID
    assert _mask(N=0) == INVALID and _mask(d=0) == INVALID and _mask(d=-3) == INVALID
    assert _mask(ldx=7) == INVALID and _mask(ldo=7) == INVALID
    for T in (-1, 65537):
        assert _mask(T=T) == INVALID


def test_workspace_query():
    lib = _lib.lib()
    assert "mp_bn_drop_ws_bytes" in _lib.PROTOTYPES
    nb, nb0 = C.c_size_t(0), C.c_size_t(0)
    assert lib.mp_bn_drop_ws_bytes(-1, 8, C.byref(nb)) == INVALID and lib.mp_bn_drop_ws_bytes(10, 0, C.byref(nb)) == INVALID
    assert lib.mp_bn_drop_ws_bytes(10, 8, None) == INVALID
    for N_, d in ((10, 8), (10 ** 7, 256), (333, 7)):
        assert lib.mp_bn_drop_ws_bytes(N_, d, C.byref(nb)) == 0 and lib.mp_bn_act_ws_bytes(N_, d, C.byref(nb0)) == 0
        assert nb0.value <= nb.value <= 2 * nb0.value     # a second partial slab per statistics workgroup (256-byte units)
    assert lib.mp_bn_drop_ws_bytes(10, 8, C.byref(nb)) == 0
    assert _bwd(N=10, d=8, nb=nb.value - 1) == WORKSPACE and _fwd(N=10, d=8, nb=nb.value - 1) == WORKSPACE     # one byte short
    assert lib.mp_bn_act_ws_bytes(10 ** 7, 256, C.byref(nb0)) == 0       # the *_act entries' workspace keeps its value
    assert lib.mp_bn_drop_ws_bytes(10 ** 7, 256, C.byref(nb)) == 0 and nb.value > nb0.value


def test_the_header_declares_the_entries():
    import os
    text = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "include", "mp_engine.h")).read()
    for _, sym in ENTRIES.values():
        assert f"int {sym}(" in text
    assert "int mp_dropout_keyed_f32(" in text


# ---- the harness --------------------------------------------------------------------------------------------------------
def test_the_route_is_opt_in(fresh_cfg):  # noqa: F811
    import graphgym_amd.graphgym_plugin  # noqa: F401
    from graphgym_amd import config, harness as H, nn as mpnn
    cfg = fresh_cfg
    assert config._defaults().gnn.keyed_dropout is False
    cfg.gnn.dropout, cfg.gnn.act, cfg.gnn.batchnorm = 0.1, "prelu", True
    for absent in (True, False):
        if absent and hasattr(cfg.gnn, "keyed_dropout"):
            delattr(cfg.gnn, "keyed_dropout")                   # a real GraphGym cfg does not have the key
        elif not absent:
            cfg.gnn.keyed_dropout = False
        post = H.GeneralLayer("linear", 6, 5).post_layer
        assert [type(m) for m in post] == [mpnn.BatchNorm1d, nn.Dropout, nn.PReLU] and post[0].relu is False
        assert post[1].p == 0.1
    cfg.gnn.keyed_dropout = True
    layer = H.GeneralLayer("linear", 6, 5)
    post = layer.post_layer
    assert [type(m) for m in post] == [mpnn.BatchNorm1d, mpnn.Dropout, nn.PReLU] and post[0].relu is False
    assert post[1].p == 0.1 and post[1].T == 6554
    assert set(layer.state_dict()) == set(H.GeneralLayer("linear", 6, 5).state_dict())
    assert "post_layer.2.weight" in layer.state_dict()           # the slope stays where the reference has it
    cfg.gnn.act = "relu"                                         # dropout keeps the ReLU out of the BatchNorm, as before
    post = H.GeneralLayer("linear", 6, 5).post_layer
    assert [type(m) for m in post] == [mpnn.BatchNorm1d, mpnn.Dropout, nn.ReLU] and post[0].relu is False
    post = H.GeneralLayer("linear", 6, 5, has_act=False).post_layer
    assert [type(m) for m in post] == [mpnn.BatchNorm1d, mpnn.Dropout]
    # on the host the layer is the composition with the module's own counter
    layer = H.GeneralLayer("linear", 6, 5).train()
    x = torch.randn(12, 6)
    out = layer(x)
    assert layer.post_layer[1].step == 1
    layer.post_layer[1].set_stream(layer.post_layer[1].seed, 0)
    layer.post_layer[0].reset_running_stats()
    assert torch.equal(out, layer.post_layer(layer.layer(x)))


def test_bn_act_module_with_a_dropout_on_the_host_is_the_composition():
    from graphgym_amd import nn as mpnn
    torch.manual_seed(0)
    x, skip = torch.randn(20, 6), torch.randn(20, 6)
    for drop in (mpnn.Dropout(0.3, seed=4), nn.Dropout(0.3)):
        for act in (nn.PReLU(), None):
            a, b = mpnn.BatchNorm1d(6), nn.BatchNorm1d(6)
            keyed = isinstance(drop, mpnn.Dropout)
            if keyed:
                drop.set_stream(4, 0)
            torch.manual_seed(1)
            got = mpnn.bn_act_module(a, x, act, drop=drop)
            if keyed:
                assert drop.step == 1
                drop.set_stream(4, 0)
            torch.manual_seed(1)
            want = drop(b(x))
            assert torch.equal(got, want if act is None else act(want))
            if keyed:
                drop.set_stream(4, 0)
            torch.manual_seed(1)
            got = mpnn.bn_skip_act(a, x, skip, "skipsum", act=act, relu=False, drop=drop)
            if keyed:
                drop.set_stream(4, 0)
            torch.manual_seed(1)
            want = skip + drop(b(x))
            assert torch.equal(got, want if act is None else act(want))
