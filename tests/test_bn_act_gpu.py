"""Every gnn.act activation fused into the BatchNorm and skip passes (csrc/act.h, csrc/bn.hip: mp_bn_train_*_act_f32, the ops
mp::bn_actx / mp::bn_skip_actx, graphgym_amd.nn.bn_act_module / bn_skip_act(act=...), and the harness's routing) against the
torch composition on the CPU — BatchNorm1d in training mode -> [add | cat] -> activation — in float64 and float32
(tests/_tol.py: both), judged by close (rows) and close_all (parameter gradients) at their defaults.

For the kinked kinds (ReLU, LeakyReLU, PReLU, SELU) the oracle takes the engine's branch pattern: z > 0 on the bits of
mp::bn_act(relu=False) on the same input (plus skip), which the fused pass must reproduce; the pattern may disagree with the
float64 pre-activation only within 1e-5 of the largest magnitude (the _check_pattern idea of tests/test_bn_skip_gpu.py)."""
import ctypes as C
import os

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.utils._python_dispatch import TorchDispatchMode

import _gradsub
from _bigview import IDS, N_WIDE, WIDE, Kept, assert_beside, need, sample_rows, wide_empty, wide_of
from _bigview import assert_written as wide_written
from _layout import LAYOUTS, OFF1, Unchanged, assert_untouched, assert_written, out_view, same_bits, view_of
from _tol import both, close, close_all
from test_ogb_gpu import _molecules, shipped_cfg  # noqa: F401

pytestmark = pytest.mark.gpu

SUM, CONCAT = 0, 1
NONE, RELU, LRELU, PRELU, ELU, SELU, SILU = range(7)
EPS, MOM = 1e-5, 0.1
SELU_ALPHA, SELU_SCALE = 1.6732632423543772848170429916717, 1.0507009873554804934193349852946
# name -> (module factory, kind, host parameter, kinked)
ACTS = {
    "relu": (lambda: nn.ReLU(), RELU, 0.0, True),
    "lrelu_01": (lambda: nn.LeakyReLU(0.1), LRELU, 0.1, True),
    "lrelu_05": (lambda: nn.LeakyReLU(0.5), LRELU, 0.5, True),
    "prelu": (lambda: nn.PReLU(init=0.25), PRELU, 0.0, True),
    "elu": (lambda: nn.ELU(alpha=1.0), ELU, 1.0, False),
    "selu": (lambda: nn.SELU(), SELU, 0.0, True),
    "silu": (lambda: nn.SiLU(), SILU, 0.0, False),
}
PLAIN_SHAPES = [(2, 4), (100, 4), (333, 7), (4097, 100), (1000, 256), (600, 257), (300, 1028)]
SUM_SHAPES = [(2, 4, 4), (333, 7, 7), (4097, 100, 100), (1000, 256, 256)]
CAT_SHAPES = [(2, 4, 4), (333, 7, 5), (4097, 6, 8), (1000, 100, 36), (1000, 256, 64)]      # (N, d_skip, d)
SKIP_CASES = [(SUM,) + s for s in SUM_SHAPES] + [(CONCAT,) + s for s in CAT_SHAPES]
SKIP_IDS = [f"{'sum' if m == SUM else 'cat'}-{n}-{ds}-{d}" for m, n, ds, d in SKIP_CASES]


def _inputs(N, d_skip, d, mode):
    """mode None: the plain form (skip is drawn and unused).  dy = randn + 0.5: a sum over it is not noise around zero"""
    g = torch.Generator().manual_seed(N + d)
    x = torch.randn(N, d, generator=g) * (torch.rand(d, generator=g) * 3 + 0.1) + torch.randn(d, generator=g) * 5
    skip = torch.randn(N, d_skip, generator=g)
    dy = torch.randn(N, d_skip + d if mode == CONCAT else d, generator=g) + 0.5
    w, b = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g)
    return x, skip, dy, w, b


def _combine(skip, y, mode):
    return y if mode is None else (skip + y if mode == SUM else torch.cat((skip, y), 1))


def _engine_pre(x, skip, w, b, mode, dev):
    """the pre-activation's bits: mp::bn_act(relu=False) on the same input, then the skip pass's own add / placement"""
    z = torch.ops.mp.bn_act(x.to(dev), w.to(dev), b.to(dev), EPS, False)[0]
    return _combine(skip.to(dev), z, mode)


def _check_pattern(x, skip, w, b, mode, pos):
    pre = _combine(skip.double(), F.batch_norm(x.double(), None, None, w.double(), b.double(), True, MOM, EPS), mode)
    off = (pre > 0) != pos
    assert not bool(off.any()) or float(pre.abs()[off].max()) <= 1e-5 * float(pre.abs().max())


def _act_ref(name, pre, pos, slope):
    """the activation on the reference's pre-activation; kinked kinds through the engine's branch pattern `pos`"""
    if name == "relu":
        return pre * pos.to(pre.dtype)
    if name.startswith("lrelu") or name == "prelu":
        return torch.where(pos, pre, slope * pre)
    if name == "selu":
        return SELU_SCALE * torch.where(pos, pre, SELU_ALPHA * torch.expm1(pre))
    return {"elu": F.elu, "silu": F.silu}[name](pre)


def _oracle(name, x, skip, dy, w, b, mode, pos, slope=None):
    """(out, dx, dskip, dgamma, dbeta, dslope, running_mean, running_var) of the composition in float64 and float32"""
    if slope is None:
        slope = 0.25 if name == "prelu" else ACTS[name][2]
    slope32 = torch.tensor([slope], dtype=torch.float32)       # the fp32 value the engine multiplies by

    def fn(c):
        ref = torch.nn.BatchNorm1d(x.size(1), eps=EPS, momentum=MOM).to(c(x).dtype)
        with torch.no_grad():
            ref.weight.copy_(c(w)); ref.bias.copy_(c(b))
        xr, sr = c(x).clone().requires_grad_(True), c(skip).clone().requires_grad_(True)
        sl = c(slope32).clone().requires_grad_(True)
        out = _act_ref(name, _combine(sr, ref(xr), mode), pos, sl)
        out.backward(c(dy))
        return (out.detach(), xr.grad, sr.grad if mode is not None else None, ref.weight.grad, ref.bias.grad,
                sl.grad if name == "prelu" else None, ref.running_mean.clone(), ref.running_var.clone())
    return both(fn)


def _pair(r, i):
    return (r[0][i], r[1][i])


def _module_run(name, x, skip, dy, w, b, mode, dev, slope=None):
    from graphgym_amd import nn as mpnn
    act = ACTS[name][0]().to(dev)
    if slope is not None:
        with torch.no_grad():
            act.weight.fill_(slope)
    bn = mpnn.BatchNorm1d(x.size(1), eps=EPS, momentum=MOM).to(dev)
    with torch.no_grad():
        bn.weight.copy_(w); bn.bias.copy_(b)
    xg, sg = x.to(dev).requires_grad_(True), skip.to(dev).requires_grad_(True)
    out = mpnn.bn_act_module(bn, xg, act) if mode is None else mpnn.bn_skip_act(bn, xg, sg, mode, act=act)
    assert out.shape == dy.shape
    out.backward(dy.to(dev))
    return out.detach(), xg.grad, sg.grad, bn, act


def _check_parity(name, N, d_skip, d, mode, dev, slope=None):
    x, skip, dy, w, b = _inputs(N, d_skip, d, mode)
    out, dx, dskip, bn, act = _module_run(name, x, skip, dy, w, b, mode, dev, slope)
    pos = None
    if ACTS[name][3]:
        pos = (_engine_pre(x, skip, w, b, mode, dev) > 0).cpu()
        _check_pattern(x, skip, w, b, mode, pos)
    r = _oracle(name, x, skip, dy, w, b, mode, pos, slope)
    what = f"bn + {name} {'plain' if mode is None else ('sum' if mode == SUM else 'cat')} {N}x{d}"
    close(out, _pair(r, 0), what=what + " out")
    if N >= 8:
        close(dx, _pair(r, 1), what=what + " dx")
    else:       # a batch of two: dx is the rounding residue of terms that cancel exactly (tests/test_bn_gpu.py)
        close_all(dx, _pair(r, 1), what=what + " dx (degenerate batch)")
    if mode is not None:
        close(dskip, _pair(r, 2), what=what + " dskip")
    close_all(bn.weight.grad, _pair(r, 3), what=what + " dgamma")
    close_all(bn.bias.grad, _pair(r, 4), what=what + " dbeta")
    if name == "prelu":
        assert act.weight.grad is not None and act.weight.grad.shape == (1,)
        close_all(act.weight.grad, _pair(r, 5), what=what + " dslope")
    col = lambda t: t.detach().reshape(-1, 1)      # noqa: E731  one statistic per column: each its own scale
    # a column mean cancels (a column may be centred near zero: (600, 257) holds one whose mean is 0.002 of its spread),
    # so beside its own magnitude a column is held to its sum of absolute terms, 0.1 * mean |x| (tests/_tol.py rule (d))
    close(col(bn.running_mean), (col(r[0][6]), col(r[1][6])), what=what + " running_mean",
          mag=col(MOM * x.double().abs().mean(0)))
    close(col(bn.running_var), (col(r[0][7]), col(r[1][7])), what=what + " running_var")
    assert int(bn.num_batches_tracked) == 1


# ---- 1, 2: parity ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,d", PLAIN_SHAPES, ids=[f"{n}-{d}" for n, d in PLAIN_SHAPES])
@pytest.mark.parametrize("name", list(ACTS))
def test_parity_plain(dev, name, N, d):
    """nn.bn_act_module: out, dx, dgamma, dbeta, dslope and the running statistics after a step.  The shapes: a degenerate
    batch, fewer rows than a workgroup's row lanes, the scalar form, ragged row blocks, two column tiles in the scalar and
    in the 4-wide form"""
    _check_parity(name, N, d, d, None, dev)


@pytest.mark.parametrize("mode,N,d_skip,d", SKIP_CASES, ids=SKIP_IDS)
@pytest.mark.parametrize("name", list(ACTS))
def test_parity_skip(dev, name, mode, N, d_skip, d):
    """nn.bn_skip_act(act=module): the above and dskip"""
    _check_parity(name, N, d_skip, d, mode, dev)


# ---- 3: bit identities ---------------------------------------------------------------------------------------------------
def _grads(fn, leaves, dy):
    for t in leaves:
        t.grad = None
    out = fn()
    out.backward(dy)
    return [out.detach()] + [t.grad for t in leaves]


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("mode,N,d_skip,d", [(None, 333, 7, 7), (None, 1000, 256, 256), (SUM, 333, 7, 7),
                                             (SUM, 1000, 256, 256), (CONCAT, 333, 7, 5), (CONCAT, 1000, 256, 64),
                                             (CONCAT, 4097, 6, 8)])
def test_none_and_relu_have_the_bits_of_the_existing_ops(dev, mode, N, d_skip, d, relu):
    ops = torch.ops.mp
    x, skip, dy, w, b = (t.to(dev) for t in _inputs(N, d_skip, d, mode))
    for t in (x, skip, w, b):
        t.requires_grad_(True)
    kind = RELU if relu else NONE
    if mode is None:
        old = _grads(lambda: ops.bn_act(x, w, b, EPS, relu)[0], (x, w, b), dy)
        new = _grads(lambda: ops.bn_actx(x, w, b, None, EPS, kind, 0.0)[0], (x, w, b), dy)
    else:
        old = _grads(lambda: ops.bn_skip_act(x, skip, w, b, EPS, relu, mode)[0], (x, skip, w, b), dy)
        new = _grads(lambda: ops.bn_skip_actx(x, skip, w, b, None, EPS, kind, 0.0, mode)[0], (x, skip, w, b), dy)
    for i, (a, c) in enumerate(zip(old, new)):
        assert same_bits(a, c), f"result {i} of mode {mode} relu {relu} differs"
    if relu:
        assert 0.2 < float((new[0] > 0).float().mean()) < 0.8


@pytest.mark.parametrize("mode,N,d_skip,d", [(None, 333, 7, 7), (None, 1000, 256, 256), (SUM, 1000, 256, 256),
                                             (CONCAT, 333, 7, 5)])
@pytest.mark.parametrize("name", ["lrelu_01", "lrelu_05", "prelu"])
def test_leaky_outputs_are_the_branches_on_the_batchnorm_bits(dev, name, mode, N, d_skip, d):
    x, skip, dy, w, b = (t.to(dev) for t in _inputs(N, d_skip, d, mode))
    _, kind, param, _ = ACTS[name]
    slope = torch.tensor([0.25], device=dev) if kind == PRELU else None
    z = _engine_pre(x, skip, w, b, mode, dev)
    want = torch.where(z > 0, z, z * (slope if kind == PRELU else param))
    if mode is None:
        out = torch.ops.mp.bn_actx(x, w, b, slope, EPS, kind, param)[0]
    else:
        out = torch.ops.mp.bn_skip_actx(x, skip, w, b, slope, EPS, kind, param, mode)[0]
    assert same_bits(out, want)


@pytest.mark.parametrize("mode,N,d_skip,d", [(None, 333, 7, 7), (SUM, 1000, 256, 256), (CONCAT, 333, 7, 5)])
@pytest.mark.parametrize("slope", [0.0, -0.5])
def test_prelu_backward_recomputes_the_pre_activation(dev, slope, mode, N, d_skip, d):
    """slope 0 and -0.5: the sign of the output says nothing about z; dx and dslope come from the recomputed z"""
    _check_parity("prelu", N, d_skip, d, mode, dev, slope=slope)


@pytest.mark.parametrize("mode", [None, SUM, CONCAT])
def test_prelu_dslope_is_deterministic(dev, mode):
    N, d_skip, d = 4097, 36, 36
    x, skip, dy, w, b = (t.to(dev) for t in _inputs(N, d_skip, d, mode))
    slope = torch.tensor([0.25], device=dev)
    mean, invstd = torch.ops.mp.bn_actx_fwd_raw(x, w, b, slope, EPS, PRELU, 0.0)[1:3]
    runs = []
    for _ in range(2):
        if mode is None:
            runs.append(torch.ops.mp.bn_actx_bwd_raw(dy, x, w, b, slope, mean, invstd, PRELU, 0.0))
        else:
            runs.append(torch.ops.mp.bn_skip_actx_bwd_raw(dy, x, skip, w, b, slope, mean, invstd, mode, PRELU, 0.0))
    for a, c in zip(*runs):
        assert same_bits(a, c)
    assert runs[0][-1].shape == (1,) and float(runs[0][-1].abs()) > 0


# ---- 4: operand views ----------------------------------------------------------------------------------------------------
def _ws(N, d, dev):
    from graphgym_amd import _lib
    nb = C.c_size_t(0)
    _lib.check(_lib.lib().mp_bn_act_ws_bytes(N, d, C.byref(nb)))
    return torch.empty(nb.value, dtype=torch.uint8, device=dev), nb.value


def _c_fwd(xv, sv, gd, bd, kind, param, slope, mode, ov, stats, ws, nb, what):
    from graphgym_amd import _lib
    from graphgym_amd.graph import _stream
    p = _lib.ptr
    N, d = xv.shape
    if mode is None:
        rc = _lib.lib().mp_bn_train_fwd_act_f32(p(xv), xv.stride(0), N, d, p(gd), p(bd), EPS, kind, param, p(slope), p(ov),
                                                ov.stride(0), p(stats[0]), p(stats[1]), p(stats[2]), p(ws), nb, _stream())
    else:
        rc = _lib.lib().mp_bn_train_fwd_skip_act_f32(p(xv), xv.stride(0), p(sv), sv.stride(0), N, d, sv.size(1), mode,
                                                     p(gd), p(bd), EPS, kind, param, p(slope), p(ov), ov.stride(0),
                                                     p(stats[0]), p(stats[1]), p(stats[2]), p(ws), nb, _stream())
    _lib.check(rc, what)


def _c_bwd(gv, xv, sv, gd, bd, stats, kind, param, slope, mode, dxv, dsv, dgamma, dbeta, dslope, ws, nb, what):
    from graphgym_amd import _lib
    from graphgym_amd.graph import _stream
    p = _lib.ptr
    N, d = xv.shape
    if mode is None:
        rc = _lib.lib().mp_bn_train_bwd_act_f32(p(gv), gv.stride(0), p(xv), xv.stride(0), N, d, p(gd), p(bd), p(stats[0]),
                                                p(stats[1]), kind, param, p(slope), p(dxv), dxv.stride(0), p(dgamma),
                                                p(dbeta), p(dslope), p(ws), nb, _stream())
    else:
        rc = _lib.lib().mp_bn_train_bwd_skip_act_f32(p(gv), gv.stride(0), p(xv), xv.stride(0), p(sv), sv.stride(0), N, d,
                                                     sv.size(1), mode, p(gd), p(bd), p(stats[0]), p(stats[1]), kind, param,
                                                     p(slope), p(dxv), dxv.stride(0), p(dsv),
                                                     dsv.stride(0) if dsv is not None else 0, p(dgamma), p(dbeta),
                                                     p(dslope), p(ws), nb, _stream())
    _lib.check(rc, what)


_LAYOUT_REF = {}


def _layout_ref(dev, mode, N, d_skip, d):
    """the contiguous run of the ops and the composition's oracle, computed once per mode (PRELU at 0.25)"""
    key = (mode, N, d_skip, d)
    if key not in _LAYOUT_REF:
        ops = torch.ops.mp
        x, skip, dy, w, b = _inputs(N, d_skip, d, mode)
        xd, sd, gd, wd, bd = (t.to(dev) for t in (x, skip, dy, w, b))
        slope = torch.tensor([0.25], device=dev)
        if mode is None:
            out, mean, invstd, _ = ops.bn_actx_fwd_raw(xd, wd, bd, slope, EPS, PRELU, 0.0)
            dx, dg, db, ds = ops.bn_actx_bwd_raw(gd, xd, wd, bd, slope, mean, invstd, PRELU, 0.0)
            dskip = None
        else:
            out, mean, invstd, _ = ops.bn_skip_actx_fwd_raw(xd, sd, wd, bd, slope, EPS, PRELU, 0.0, mode)
            dx, dg, db, dskip, ds = ops.bn_skip_actx_bwd_raw(gd, xd, sd, wd, bd, slope, mean, invstd, mode, PRELU, 0.0)
        pos = (_engine_pre(x, skip, w, b, mode, dev) > 0).cpu()
        _check_pattern(x, skip, w, b, mode, pos)
        _LAYOUT_REF[key] = ((x, skip, dy, w, b), (out, dx, dskip, dg, db, ds),
                            _oracle("prelu", x, skip, dy, w, b, mode, pos))
    return _LAYOUT_REF[key]


@pytest.mark.parametrize("mode,d_skip", [(None, 8), (SUM, 8), (CONCAT, 8), (CONCAT, 6)],
                         ids=["plain", "sum", "cat", "cat-dskip6"])
@pytest.mark.parametrize("lay", [LAYOUTS[2], OFF1], ids=["aligned-offset", "misaligned-offset"])
def test_operands_as_column_slices(dev, mode, d_skip, lay):
    """x, skip, out, dy, dx and dskip at an aligned (16-byte) and a misaligned (4-byte) offset of wider buffers, PRELU:
    inputs keep their bits, nothing beside an output slice is written, the aligned layout has the contiguous run's bits"""
    N, d = 777, 8
    (x, skip, dy, w, b), cont, r = _layout_ref(dev, mode, N, d_skip, d)
    what = f"bn act layouts mode {mode} d_skip {d_skip} [{lay[0]}]"
    width = d_skip + d if mode == CONCAT else d
    gd, bd, slope = w.to(dev), b.to(dev), torch.tensor([0.25], device=dev)
    ws, nb = _ws(N, d, dev)
    stats = [torch.empty(d, device=dev) for _ in range(3)]
    xb, xv = view_of(x, lay, dev, seed=1)
    sb, sv = view_of(skip, lay, dev, seed=2)
    gb, gv = view_of(dy, lay, dev, seed=3)
    ob, ov = out_view(N, width, lay, dev)
    with Unchanged(xb, sb, slope):
        _c_fwd(xv, sv, gd, bd, PRELU, 0.0, slope, mode, ov, stats, ws, nb, what)
    assert_untouched(ob, lay[2], width, what)
    assert_written(ov, what)
    close(ov, _pair(r, 0), what=what + " out")
    dxb, dxv = out_view(N, d, lay, dev)
    dsb, dsv = out_view(N, d_skip, lay, dev)
    dgamma, dbeta, dslope = torch.empty(d, device=dev), torch.empty(d, device=dev), torch.empty(1, device=dev)
    with Unchanged(xb, sb, gb, slope):
        _c_bwd(gv, xv, sv, gd, bd, stats, PRELU, 0.0, slope, mode, dxv, dsv, dgamma, dbeta, dslope, ws, nb, what)
    assert_untouched(dxb, lay[2], d, what + " dx")
    assert_written(dxv, what + " dx")
    close(dxv, _pair(r, 1), what=what + " dx")
    close_all(dgamma, _pair(r, 3), what=what + " dgamma")
    close_all(dbeta, _pair(r, 4), what=what + " dbeta")
    close_all(dslope, _pair(r, 5), what=what + " dslope")
    if mode is not None:
        assert_untouched(dsb, lay[2], d_skip, what + " dskip")
        assert_written(dsv, what + " dskip")
        close(dsv, _pair(r, 2), what=what + " dskip")
    if lay is LAYOUTS[2] and d_skip % 4 == 0:      # rows on 16-byte boundaries: the same vector kernels as the contiguous run
        assert same_bits(ov, cont[0]) and same_bits(dxv, cont[1]), what
        assert same_bits(dgamma, cont[3]) and same_bits(dbeta, cont[4]) and same_bits(dslope, cont[5]), what
        assert mode is None or same_bits(dsv, cont[2]), what
    # the ops on the same views (no copy is made of a column slice): the C entries' bits
    with Unchanged(xb, sb, gb):
        if mode is None:
            out, mean, invstd, _ = torch.ops.mp.bn_actx_fwd_raw(xv, gd, bd, slope, EPS, PRELU, 0.0)
            dx, dg, db, ds = torch.ops.mp.bn_actx_bwd_raw(gv, xv, gd, bd, slope, mean, invstd, PRELU, 0.0)
        else:
            out, mean, invstd, _ = torch.ops.mp.bn_skip_actx_fwd_raw(xv, sv, gd, bd, slope, EPS, PRELU, 0.0, mode)
            dx, dg, db, dskip, ds = torch.ops.mp.bn_skip_actx_bwd_raw(gv, xv, sv, gd, bd, slope, mean, invstd, mode,
                                                                      PRELU, 0.0)
            close(dskip, _pair(r, 2), what=what + " dskip of the op")
    # (the ops' outputs are contiguous: aligned whatever the inputs' offset, so only the aligned layout shares a form)
    close(out, _pair(r, 0), what=what + " out of the op")
    close(dx, _pair(r, 1), what=what + " dx of the op")
    close_all(ds, _pair(r, 5), what=what + " dslope of the op")
    if lay is LAYOUTS[2] and d_skip % 4 == 0:
        assert same_bits(out, ov) and same_bits(dx, dxv) and same_bits(dg, dgamma) and same_bits(db, dbeta), what
        assert same_bits(ds, dslope), what


@pytest.mark.parametrize("lay", WIDE, ids=IDS)
def test_wide_buffers(dev, lay):
    """PRELU in SUM mode (the new read of skip and the new partial sums): x, skip, out, dy, dx and dskip as 8-column slices
    of [70 000, 32 768 (+3)] buffers, rows past 2^32 bytes and 2^31 elements"""
    N, d, mode = N_WIDE, 8, SUM
    need(6 * N * 32_771 * 4 + (1 << 30), "bn act skip, wide")
    what = f"wide bn act sum [{lay[0]}]"
    x, skip, dy, w, b = _inputs(N, d, d, mode)
    rows = sample_rows(N, seed=6)
    rd = rows.to(dev)
    gd, bd, slope = w.to(dev), b.to(dev), torch.tensor([0.25], device=dev)
    ws, nb = _ws(N, d, dev)
    stats = [torch.empty(d, device=dev) for _ in range(3)]
    xb, xv = wide_of(x, lay, dev)
    sb, sv = wide_of(skip, lay, dev)
    ob, ov = wide_empty(N, d, lay, dev)
    with Kept((xb, xv, lay), (sb, sv, lay)):
        _c_fwd(xv, sv, gd, bd, PRELU, 0.0, slope, mode, ov, stats, ws, nb, what)
    assert_beside(ob, lay, d, what)
    wide_written(ov, what)
    pos = (_engine_pre(x, skip, w, b, mode, dev) > 0).cpu()
    _check_pattern(x, skip, w, b, mode, pos)
    r = _oracle("prelu", x, skip, dy, w, b, mode, pos)
    take = lambda i: (r[0][i][rows], r[1][i][rows])     # noqa: E731
    got = ov[rd]
    assert bool(torch.isfinite(got).all()), what
    close(got, take(0), what=what + " out")
    del ob, ov
    gb, gv = wide_of(dy, lay, dev)
    dxb, dxv = wide_empty(N, d, lay, dev)
    dsb, dsv = wide_empty(N, d, lay, dev)
    dgamma, dbeta, dslope = torch.empty(d, device=dev), torch.empty(d, device=dev), torch.empty(1, device=dev)
    with Kept((gb, gv, lay), (xb, xv, lay), (sb, sv, lay)):
        _c_bwd(gv, xv, sv, gd, bd, stats, PRELU, 0.0, slope, mode, dxv, dsv, dgamma, dbeta, dslope, ws, nb, what)
    assert_beside(dsb, lay, d, what + " dskip")
    wide_written(dsv, what + " dskip")
    close(dsv[rd], take(2), what=what + " dskip")
    assert_beside(dxb, lay, d, what + " dx")
    wide_written(dxv, what + " dx")
    got = dxv[rd]
    assert bool(torch.isfinite(got).all()), what
    close(got, take(1), what=what + " dx")
    close_all(dgamma, _pair(r, 3), what=what + " dgamma")
    close_all(dbeta, _pair(r, 4), what=what + " dbeta")
    close_all(dslope, _pair(r, 5), what=what + " dslope")


# ---- 5: autograd -----------------------------------------------------------------------------------------------------------
class Spy(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        self.seen.append(str(func))
        return func(*args, **(kwargs or {}))

    def mp(self):
        return [s.split(".")[1] for s in self.seen if s.startswith("mp.")]

    def prelu(self):
        return [s for s in self.seen if "prelu" in s.lower()]


@pytest.mark.parametrize("mode,d_skip", [(None, 12), (SUM, 12), (CONCAT, 6)], ids=["plain", "sum", "cat"])
def test_every_subset_of_differentiated_inputs(dev, mode, d_skip):
    """PRELU: gradients of a subset of {x, skip, weight, bias, slope} are the all-inputs run's bit for bit, nothing outside
    the subset receives a .grad, and every run is one backward op"""
    N, d = 257, 12
    x, skip, dy, w, b = _inputs(N, d_skip, d, mode)
    inputs = {"x": x, "weight": w, "bias": b, "slope": torch.tensor([0.25])}
    if mode is not None:
        inputs["skip"] = skip

    def op(t):
        if mode is None:
            return torch.ops.mp.bn_actx(t["x"], t["weight"], t["bias"], t["slope"], EPS, PRELU, 0.0)[0]
        return torch.ops.mp.bn_skip_actx(t["x"], t["skip"], t["weight"], t["bias"], t["slope"], EPS, PRELU, 0.0, mode)[0]

    def oracle(c, t, eng):
        pre = _combine(t.get("skip"), F.batch_norm(t["x"], None, None, t["weight"], t["bias"], True, MOM, EPS), mode)
        pos = eng[0] > 0                       # slope 0.25: the output has the pre-activation's sign
        p = pre.detach()
        far = p.abs() > 1e-5 * float(p.abs().max())
        assert bool(((p > 0) == pos)[far].all()), "activation pattern differs away from zero"
        return torch.where(pos, pre, t["slope"] * pre)
    full = None
    for s in _gradsub.subsets(list(inputs)):
        with Spy() as spy:
            res = _gradsub.run(op, inputs, oracle, s, dy, dev, params=("weight", "bias", "slope"),
                               what=f"bn_actx mode {mode}")
        bwd = [n for n in spy.mp() if n.endswith("_bwd_raw")]
        assert bwd == ["bn_actx_bwd_raw" if mode is None else "bn_skip_actx_bwd_raw"], (s, bwd)
        if full is None:
            full = res
        else:
            _gradsub.hold_bits(full, res, ("y", "x", "skip", "weight", "bias", "slope"), f"mode {mode} {s}")


def test_kinds_without_a_slope_return_no_slope_gradient(dev):
    x, skip, dy, w, b = (t.to(dev) for t in _inputs(257, 12, 12, SUM))
    slope = torch.tensor([0.25], device=dev, requires_grad=True)
    xg = x.clone().requires_grad_(True)
    torch.ops.mp.bn_skip_actx(xg, skip, w, b, slope, EPS, ELU, 1.0, SUM)[0].backward(dy)
    assert slope.grad is None and xg.grad is not None
    mean, invstd = torch.ops.mp.bn_actx_fwd_raw(x, w, b, None, EPS, ELU, 1.0)[1:3]
    assert torch.ops.mp.bn_actx_bwd_raw(dy, x, w, b, None, mean, invstd, ELU, 1.0)[3].numel() == 0
    none = torch.ops.mp.bn_skip_actx_bwd_raw(dy, x, skip, w, b, None, mean, invstd, SUM, NONE, 0.0)
    assert none[3].numel() == 0 and none[4].numel() == 0       # d(skip) is dy itself: nothing is written
    with pytest.raises(ValueError):
        torch.ops.mp.bn_actx_fwd_raw(x, w, b, None, EPS, PRELU, 0.0)
    with pytest.raises(ValueError):
        torch.ops.mp.bn_actx_fwd_raw(x, w, b, None, EPS, 7, 0.0)


def test_opcheck(dev):
    gen = torch.Generator().manual_seed(0)

    def t(*shape):
        return torch.randn(*shape, generator=gen).to(dev).requires_grad_(True)
    n, d = 300, 32
    slope = lambda: torch.tensor([0.25], device=dev, requires_grad=True)      # noqa: E731
    for args in [(t(n, d), t(d), t(d), slope(), EPS, PRELU, 0.0), (t(n, d), t(d), t(d), None, EPS, ELU, 1.0),
                 (t(n, d), None, None, None, EPS, SILU, 0.0), (t(n, d), t(d), t(d), None, EPS, NONE, 0.0)]:
        res = torch.library.opcheck(torch.ops.mp.bn_actx.default, args, raise_exception=True)
        assert all(v == "SUCCESS" for v in res.values()), res
    for args in [(t(n, d), t(n, d), t(d), t(d), slope(), EPS, PRELU, 0.0, SUM),
                 (t(n, d), t(n, 20), t(d), t(d), slope(), EPS, PRELU, 0.0, CONCAT),
                 (t(n, d), t(n, 20), t(d), t(d), None, EPS, SELU, 0.0, CONCAT),
                 (t(n, d), t(n, d), None, None, None, EPS, NONE, 0.0, SUM)]:
        res = torch.library.opcheck(torch.ops.mp.bn_skip_actx.default, args, raise_exception=True)
        assert all(v == "SUCCESS" for v in res.values()), res


# ---- 6: dispatch -------------------------------------------------------------------------------------------------------------
D = 64


@pytest.fixture()
def gcfg():
    from graphgym_amd.config import cfg
    import graphgym_amd.graphgym_plugin  # noqa: F401  (registers the layer keys)
    saved = {k: dict(vars(getattr(cfg, k))) for k in ("gnn", "dataset", "bn", "mem")}
    cfg.gnn.layers_pre_mp, cfg.gnn.dim_inner, cfg.gnn.layers_post_mp, cfg.gnn.layers_mp = 1, D, 1, 4
    cfg.gnn.batchnorm, cfg.gnn.dropout, cfg.gnn.act, cfg.gnn.l2norm, cfg.gnn.skip_every = True, 0.0, "prelu", True, 1
    cfg.gnn.agg, cfg.gnn.normalize_adj, cfg.gnn.self_msg, cfg.gnn.layer_type = "add", False, "concat", "gcnconv"
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
    n = 500
    return graphgen.ba_edge_index(n, 4, seed=5), torch.randn(n, D, generator=g)


def _batch(dev, x, ei):
    from graphgym_amd import harness as H
    return H.Batch(node_feature=x.to(dev), edge_index=ei.to(dev))


def test_a_prelu_layer_is_one_op(dev, gcfg, graph):
    from graphgym_amd import harness as H
    x = graph[1].to(dev)
    torch.manual_seed(1)
    layer = H.GeneralLayer("linear", D, D).to(dev).train()
    assert [type(m).__name__ for m in layer.post_layer] == ["BatchNorm1d", "PReLU"]
    with Spy() as spy:
        out = layer(x)
        out.sum().backward()
    assert spy.mp().count("bn_actx") == 1 and spy.mp().count("bn_actx_bwd_raw") == 1 and not spy.prelu(), spy.seen
    assert "bn_act" not in spy.mp() and "bn_bwd_raw" not in spy.mp()
    got = [out.detach()] + [p.grad.clone() for p in layer.parameters()]
    assert layer.post_layer[1].weight.grad is not None and int(layer.post_layer[0].num_batches_tracked) == 1
    layer.zero_grad()
    ref = layer.post_layer(layer.layer(x))          # the Sequential: BatchNorm on the engine, then torch's PReLU
    ref.sum().backward()
    close(got[0], ref.detach().double(), what="prelu layer out")
    for g, p in zip(got[1:], layer.parameters()):
        close_all(g, p.grad.double(), what="prelu layer grads")


@pytest.mark.parametrize("stage", ["skipsum", "skipconcat"])
def test_a_prelu_skip_block_is_one_op(dev, gcfg, graph, stage):
    from graphgym_amd import harness as H
    ei, x = graph
    gcfg.gnn.stage_type = stage
    torch.manual_seed(2)
    blk = H.GNNSkipBlock(D, D, 2).to(dev).train()
    with Spy() as spy:
        out = blk(_batch(dev, x, ei)).node_feature
        out.sum().backward()
    assert spy.mp().count("bn_skip_actx") == 1 and spy.mp().count("bn_actx") == 1, spy.mp()     # the block's tail, its inner layer
    assert "bn_skip_act" not in spy.mp() and not spy.prelu(), spy.seen
    got = [out.detach()] + [p.grad.clone() for p in blk.parameters()]
    blk.zero_grad()
    b = _batch(dev, x, ei)
    h = blk.f(b).node_feature                       # the inner layers as they are, then the unfused tail
    x0 = x.to(dev)
    ref = blk.act(x0 + h if stage == "skipsum" else torch.cat((x0, h), 1))
    ref.sum().backward()
    assert out.shape == (x.size(0), D if stage == "skipsum" else 2 * D)
    close(got[0], ref.detach().double(), what=f"prelu {stage} out")
    for g, p in zip(got[1:], blk.parameters()):
        close_all(g, p.grad.double(), what=f"prelu {stage} grads")


@pytest.mark.parametrize("case", ["dropout", "eval", "per-channel"])
def test_fallbacks_are_the_composition(dev, gcfg, graph, case):
    from graphgym_amd import harness as H
    ei, x = graph
    gcfg.gnn.stage_type = "skipsum"
    if case == "dropout":
        gcfg.gnn.dropout = 0.1
    torch.manual_seed(3)
    layer = H.GeneralLayer("linear", D, D).to(dev).train()
    blk = H.GNNSkipBlock(D, D, 1).to(dev).train()
    if case == "per-channel":
        layer.post_layer[1] = nn.PReLU(D).to(dev)
        blk.act = nn.PReLU(D).to(dev)
    if case == "eval":
        with torch.no_grad():                       # running statistics that are not the initial ones
            layer(x.to(dev)); blk(_batch(dev, x, ei))
        layer.eval(); blk.eval()
    with Spy() as spy, torch.no_grad():
        torch.manual_seed(5)
        out = layer(x.to(dev))
        torch.manual_seed(6)
        sk = blk(_batch(dev, x, ei)).node_feature
    assert "bn_actx" not in spy.mp() and "bn_skip_actx" not in spy.mp(), spy.mp()
    # (in training mode the reference calls below update the running statistics again; the outputs do not depend on them)
    with torch.no_grad():
        torch.manual_seed(5)
        ref = layer.post_layer(layer.layer(x.to(dev)))
        torch.manual_seed(6)
        rsk = blk.act(x.to(dev) + blk.f(_batch(dev, x, ei)).node_feature)
    assert torch.equal(out, ref) and torch.equal(sk, rsk)


def test_accelerate_leaves_a_prelu_skip_block_alone(dev, gcfg, graph):
    import graphgym_amd.graphgym_plugin as plugin
    from graphgym_amd import layers as L
    from _skip_ref import RefStyleSkipBlock
    ei, x = graph
    gcfg.gnn.stage_type = "skipsum"
    other = RefStyleSkipBlock(L.GCNConv, D, D, 1, act=nn.PReLU()).to(dev).train()
    plugin.accelerate(other)
    with Spy() as spy:
        other(_batch(dev, x, ei))
    assert "bn_skip_act" not in spy.mp() and "bn_skip_actx" not in spy.mp(), spy.mp()


# ---- 7: a model ------------------------------------------------------------------------------------------------------------------
class _PlainPReLU(nn.PReLU):
    """no spec: the composition"""


def test_design_v2ogb_takes_a_step_on_the_fused_route(dev, shipped_cfg):  # noqa: F811
    import graphgym_amd.graphgym_plugin  # noqa: F401
    from graphgym_amd import config, harness as H, nn as mpnn
    cfg = config.load_cfg(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cfg_design_v2ogb.yaml"),
                          target=shipped_cfg)
    gen = torch.Generator().manual_seed(0)
    ei, nodes, bonds, owner, label = _molecules(gen, graphs=16)
    batch = H.Batch(node_feature=nodes.to(dev), edge_index=ei.to(dev), edge_feature=bonds.to(dev), batch=owner.to(dev),
                    graph_label=label.to(dev))
    x0 = batch.node_feature
    torch.manual_seed(0)
    model = H.GNN(dim_in=9, dim_out=2).to(dev).train()
    layers = [m for m in model.modules() if isinstance(m, H.GeneralLayer) and len(m.post_layer) == 2]
    assert len(layers) >= cfg.gnn.layers_mp and all(type(m.post_layer[1]) is nn.PReLU for m in layers)

    def step():
        model.zero_grad()
        batch.node_feature = x0
        with Spy() as spy:
            pred, true = model(batch)
            loss = F.cross_entropy(pred, true)
            loss.backward()
        return loss.detach(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}, spy
    loss, grads, spy = step()
    assert spy.mp().count("bn_actx") == len(layers) and spy.mp().count("bn_actx_bwd_raw") == len(layers), spy.mp()
    assert not spy.prelu(), spy.prelu()
    # the same model with the fused route off: an activation subclass has no spec
    for m in layers:
        plain = _PlainPReLU().to(dev)
        plain.weight = m.post_layer[1].weight
        assert mpnn.act_spec(plain) is None
        m.post_layer[1] = plain
    rloss, rgrads, rspy = step()
    assert "bn_actx" not in rspy.mp() and rspy.prelu()
    assert set(grads) == set(rgrads) and any(k.endswith("post_layer.1.weight") for k in grads)
    close_all(loss, rloss.double(), what="design_v2ogb loss")
    for k in grads:
        close_all(grads[k], rgrads[k].double(), what=f"design_v2ogb grad {k}")
