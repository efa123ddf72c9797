"""gnn.dropout fused into the BatchNorm and skip passes through the keyed mask (csrc/draws.h, csrc/bn_drop.hip: the entries
mp_bn_train_*_drop_*_f32 and mp_dropout_keyed_f32; the ops mp::bn_drop_actx, mp::bn_drop_skip_actx, mp::dropout_keyed;
graphgym_amd.nn.Dropout, bn_act_module / bn_skip_act(drop=...), and the harness's routing under gnn.keyed_dropout).

The mask is held bit for bit against graphgym_amd.nn.dropout_keep_host; values against the torch composition on the CPU —
BatchNorm1d in training mode -> the host mask times scale -> [add | cat] -> activation — in float64 and float32
(tests/_tol.py: both), by close (rows) and close_all (parameter gradients) at their defaults.  For the kinked kinds the
oracle takes the engine's branch pattern: z > 0 on the bits of the fused op with MP_ACT_NONE and the same key, which may
disagree with the float64 pre-activation only within 1e-5 of the largest magnitude."""
import ctypes as C

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import _gradsub
from _bigview import IDS, N_WIDE, WIDE, Kept, assert_beside, need, sample_rows, wide_empty, wide_of
from _bigview import assert_written as wide_written
from _layout import LAYOUTS, OFF1, Unchanged, assert_untouched, assert_written, out_view, same_bits, view_of
from _tol import both, close, close_all
from test_bn_act_gpu import (ACTS, CAT_SHAPES, CONCAT, ELU, EPS, LRELU, MOM, NONE, PRELU, RELU, SELU, SILU, SUM,  # noqa: F401
                             SUM_SHAPES, Spy, _act_ref, _batch, _combine, _inputs, _pair, gcfg, graph)

pytestmark = pytest.mark.gpu

SEED = 0x5EED5EED1234
MASK_SHAPES = [(2, 4), (333, 7), (100, 5), (4097, 100), (600, 257), (300, 1028)]
MASK_LAYOUTS = [LAYOUTS[0], LAYOUTS[2], OFF1]       # contiguous, a column slice of a wider buffer, a misaligned offset view
KINDS = {"none": (None, NONE, 0.0, False), **ACTS}  # name -> (module factory, kind, host parameter, kinked)
SKIP_CASES = [(SUM,) + s for s in SUM_SHAPES] + [(CONCAT,) + s for s in CAT_SHAPES]
SKIP_IDS = [f"{'sum' if m == SUM else 'cat'}-{n}-{ds}-{d}" for m, n, ds, d in SKIP_CASES]


def _T(p):
    from graphgym_amd import nn as mpnn
    return mpnn.dropout_threshold(p)


def _keep(step, N, d, p, seed=SEED):
    from graphgym_amd import nn as mpnn
    return mpnn.dropout_keep_host(seed, step, N, d, p)


def _scale(p):
    from graphgym_amd import nn as mpnn
    return mpnn.dropout_scale(p)


# ---- 1: the mask, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lay", MASK_LAYOUTS, ids=[l[0] for l in MASK_LAYOUTS])
@pytest.mark.parametrize("N,d", MASK_SHAPES, ids=[f"{n}-{d}" for n, d in MASK_SHAPES])
def test_the_mask_is_the_host_mask(dev, N, d, lay):
    """mp_dropout_keyed_f32 on ones: keep_host * scale exactly, whatever the leading dimension and the offset of the views
    (the mask follows the LOGICAL index); nothing beside the output slice is written; the op on the same view agrees"""
    from graphgym_amd import _lib
    from graphgym_amd.graph import _stream
    p, step = 0.3, 7
    what = f"dropout_keyed {N}x{d} [{lay[0]}]"
    want = (_keep(step, N, d, p).float() * _scale(p)).to(dev)
    xb, xv = view_of(torch.ones(N, d), lay, dev, seed=1)
    ob, ov = out_view(N, d, lay, dev)
    with Unchanged(xb):
        _lib.check(_lib.lib().mp_dropout_keyed_f32(_lib.ptr(xv), xv.stride(0), N, d, _T(p), SEED, step, _lib.ptr(ov),
                                                   ov.stride(0), _stream()), what)
    assert_untouched(ob, lay[2], d, what)
    assert_written(ov, what)
    assert torch.equal(ov, want), what
    assert torch.equal(torch.ops.mp.dropout_keyed(xv, _T(p), SEED, step), want), what
    assert 0.1 < float((want == 0).float().mean()) < 0.6 or N * d < 64


def test_the_mask_edges_and_its_backward(dev):
    x = torch.randn(257, 12, generator=torch.Generator().manual_seed(0)).to(dev)
    assert torch.equal(torch.ops.mp.dropout_keyed(x, 0, SEED, 0), x)                   # T = 0: everything kept, scale 1
    assert not bool(torch.ops.mp.dropout_keyed(x, 65536, SEED, 0).any())              # T = 65536: nothing kept
    with pytest.raises(ValueError):
        torch.ops.mp.dropout_keyed(x, 65537, SEED, 0)
    xg = x.clone().requires_grad_(True)
    dy = torch.randn_like(x)
    torch.ops.mp.dropout_keyed(xg, _T(0.6), SEED, 3).backward(dy)
    assert torch.equal(xg.grad, dy * (_keep(3, 257, 12, 0.6).float() * _scale(0.6)).to(dev))


def test_the_module_draws_one_mask_on_every_path(dev):
    """graphgym_amd.nn.Dropout: fp32 and fp64 device tensors and a CPU tensor get the mask of (seed, step)"""
    from graphgym_amd import nn as mpnn
    x = torch.randn(100, 7, generator=torch.Generator().manual_seed(1))
    drop = mpnn.Dropout(0.3, seed=5).train()
    host = drop(x)
    for t in (x.to(dev), x.double().to(dev), x.half().to(dev)):
        drop.set_stream(5, 0)
        out = drop(t)
        assert out.dtype == t.dtype and drop.step == 1
        assert torch.equal(out == 0, (host == 0).to(dev))
    drop.set_stream(5, 0)
    assert torch.equal(drop(x.to(dev)).cpu(), host)
    y = x.to(dev)
    assert drop.eval()(y) is y and drop.step == 1                                      # eval: the identity


# ---- 2: the fused passes draw the same mask ----------------------------------------------------------------------------
@pytest.mark.parametrize("N,d", [(333, 7), (4097, 100), (600, 257), (300, 1028)])
def test_the_fused_pass_draws_the_host_mask(dev, N, d):
    x, _, _, w, b = _inputs(N, d, d, None)
    p, step = 0.3, 2
    out = torch.ops.mp.bn_drop_actx(x.to(dev), w.to(dev), b.to(dev), None, EPS, NONE, 0.0, _T(p), SEED, step)[0].cpu()
    bn = F.batch_norm(x.double(), None, None, w.double(), b.double(), True, MOM, EPS)
    far = bn.abs() > 1e-6
    keep = _keep(step, N, d, p)
    assert torch.equal((out == 0)[far], ~keep[far]) and int(far.sum()) > 0.99 * far.numel()


@pytest.mark.parametrize("mode,N,d_skip,d", [(SUM, 333, 7, 7), (SUM, 1000, 256, 256), (CONCAT, 333, 7, 5),
                                             (CONCAT, 4097, 6, 8), (CONCAT, 1000, 100, 36)])
def test_the_skip_pass_draws_the_host_mask(dev, mode, N, d_skip, d):
    """SUM: out == skip exactly where dropped; CONCAT: the right slab is zero there and the left slab is skip's bits.
    The mask is indexed by x's own row and column in both forms."""
    x, skip, _, w, b = _inputs(N, d_skip, d, mode)
    p, step = 0.6, 4
    out = torch.ops.mp.bn_drop_skip_actx(x.to(dev), skip.to(dev), w.to(dev), b.to(dev), None, EPS, NONE, 0.0, mode, _T(p),
                                         SEED, step)[0].cpu()
    bn = F.batch_norm(x.double(), None, None, w.double(), b.double(), True, MOM, EPS)
    far = bn.abs() > 1e-3            # SUM: a kept term this large is not absorbed by the skip operand's rounding
    keep = _keep(step, N, d, p)
    if mode == SUM:
        assert torch.equal((out == skip)[far], ~keep[far])
    else:
        assert same_bits(out[:, :d_skip], skip)
        assert torch.equal((out[:, d_skip:] == 0)[far], ~keep[far])


# ---- 3: parity ---------------------------------------------------------------------------------------------------------
def _pre_bits(x, skip, w, b, mode, dev, T, step):
    """the fused op's pre-activation bits: the same op with MP_ACT_NONE and the same key"""
    if mode is None:
        return torch.ops.mp.bn_drop_actx(x.to(dev), w.to(dev), b.to(dev), None, EPS, NONE, 0.0, T, SEED, step)[0]
    return torch.ops.mp.bn_drop_skip_actx(x.to(dev), skip.to(dev), w.to(dev), b.to(dev), None, EPS, NONE, 0.0, mode, T,
                                          SEED, step)[0]


def _masked_pre(c, x, skip, w, b, mode, ms):
    y = F.batch_norm(c(x), None, None, c(w), c(b), True, MOM, EPS) * c(ms)
    return _combine(None if skip is None else c(skip), y, mode)


def _check_pattern(x, skip, w, b, mode, ms, pos):
    pre = _masked_pre(lambda t: t.double(), x, skip, w, b, mode, ms)
    off = (pre > 0) != pos
    assert not bool(off.any()) or float(pre.abs()[off].max()) <= 1e-5 * float(pre.abs().max())


def _oracle(name, x, skip, dy, w, b, mode, ms, pos, slope=0.25):
    """(out, dx, dskip, dgamma, dbeta, dslope, running_mean, running_var) of the composition in float64 and float32;
    ms = keep_host * scale, multiplied in behind the BatchNorm"""
    slope = slope if name == "prelu" else KINDS[name][2]
    slope32 = torch.tensor([slope], dtype=torch.float32)

    def fn(c):
        ref = torch.nn.BatchNorm1d(x.size(1), eps=EPS, momentum=MOM).to(c(x).dtype)
        with torch.no_grad():
            ref.weight.copy_(c(w)); ref.bias.copy_(c(b))
        xr, sr = c(x).clone().requires_grad_(True), c(skip).clone().requires_grad_(True)
        sl = c(slope32).clone().requires_grad_(True)
        pre = _combine(sr, ref(xr) * c(ms), mode)
        out = pre if name == "none" else _act_ref(name, pre, pos, sl)
        out.backward(c(dy))
        return (out.detach(), xr.grad, sr.grad if mode is not None else None, ref.weight.grad, ref.bias.grad,
                sl.grad if name == "prelu" else None, ref.running_mean.clone(), ref.running_var.clone())
    return both(fn)


def _module_run(name, x, skip, dy, w, b, mode, dev, p, step):
    from graphgym_amd import nn as mpnn
    make = KINDS[name][0]
    act = None if make is None else make().to(dev)
    bn = mpnn.BatchNorm1d(x.size(1), eps=EPS, momentum=MOM).to(dev)
    with torch.no_grad():
        bn.weight.copy_(w); bn.bias.copy_(b)
    drop = mpnn.Dropout(p, seed=SEED).train()
    drop.set_stream(SEED, step)
    xg, sg = x.to(dev).requires_grad_(True), skip.to(dev).requires_grad_(True)
    with Spy() as spy:
        if mode is None:
            out = mpnn.bn_act_module(bn, xg, act, drop=drop)
        else:
            out = mpnn.bn_skip_act(bn, xg, sg, mode, relu=False, act=act, drop=drop)
        out.backward(dy.to(dev))
    want = "bn_drop_actx" if mode is None else "bn_drop_skip_actx"
    assert spy.mp().count(want) == 1 and spy.mp().count(want + "_bwd_raw") == 1, spy.mp()
    assert drop.step == step + 1                       # ONE counter value, the one the module's forward would have taken
    assert out.shape == dy.shape
    return out.detach(), xg.grad, sg.grad, bn, act


def _check_parity(name, N, d_skip, d, mode, dev, p, step=1):
    x, skip, dy, w, b = _inputs(N, d_skip, d, mode)
    ms = _keep(step, N, d, p).float() * _scale(p)
    out, dx, dskip, bn, act = _module_run(name, x, skip, dy, w, b, mode, dev, p, step)
    pos = None
    if KINDS[name][3]:
        pos = (_pre_bits(x, skip, w, b, mode, dev, _T(p), step) > 0).cpu()
        _check_pattern(x, skip, w, b, mode, ms, pos)
    r = _oracle(name, x, skip, dy, w, b, mode, ms, pos)
    what = f"bn + drop {p} + {name} {'plain' if mode is None else ('sum' if mode == SUM else 'cat')} {N}x{d}"
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
    close(col(bn.running_mean), (col(r[0][6]), col(r[1][6])), what=what + " running_mean",
          mag=col(MOM * x.double().abs().mean(0)))
    close(col(bn.running_var), (col(r[0][7]), col(r[1][7])), what=what + " running_var")
    assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("p", [0.3, 0.6])
@pytest.mark.parametrize("N,d", MASK_SHAPES, ids=[f"{n}-{d}" for n, d in MASK_SHAPES])
@pytest.mark.parametrize("name", list(KINDS))
def test_parity_plain(dev, name, N, d, p):
    """The six shapes of the mask test, eight kinds, two rates.  Two of the shapes are where the backward's own precision
    measures (csrc/bn_drop.hip) show: (300, 1028) holds a column of mean -12.3 and deviation 0.12, where half an ulp of the
    fp32 mean is 4e-6 of a deviation and the smooth kinds' dx needs the mean's residue; (2, 4), a batch of two, has a dx that
    is the residue of terms of size 2 cancelling to 1e-4 and needs the column sums' low-order parts and the unrounded
    product with the scale."""
    _check_parity(name, N, d, d, None, dev, p)


@pytest.mark.parametrize("p", [0.3, 0.6])
@pytest.mark.parametrize("mode,N,d_skip,d", SKIP_CASES, ids=SKIP_IDS)
@pytest.mark.parametrize("name", list(KINDS))
def test_parity_skip(dev, name, mode, N, d_skip, d, p):
    _check_parity(name, N, d_skip, d, mode, dev, p)


# ---- 4: identity with the composition on the engine --------------------------------------------------------------------
def _fused_fwd(x, skip, w, b, slope, kind, param, mode, T, step):
    if mode is None:
        return torch.ops.mp.bn_drop_actx(x, w, b, slope, EPS, kind, param, T, SEED, step)[0]
    return torch.ops.mp.bn_drop_skip_actx(x, skip, w, b, slope, EPS, kind, param, mode, T, SEED, step)[0]


@pytest.mark.parametrize("mode,N,d_skip,d", [(None, 333, 7, 7), (None, 1000, 256, 256), (CONCAT, 333, 7, 5),
                                             (CONCAT, 1000, 256, 64), (SUM, 333, 7, 7), (SUM, 1000, 256, 256)])
@pytest.mark.parametrize("name", ["relu", "lrelu_01", "prelu"])
def test_the_forward_is_the_composition_on_the_engine(dev, name, mode, N, d_skip, d):
    """act([skip +|cat] Dropout(bn_act(relu=False)(x))) with the same (seed, step), under torch.equal — SUM included: the
    product with the scale is never contracted into the skip add"""
    from graphgym_amd import nn as mpnn
    x, skip, _, w, b = (t.to(dev) for t in _inputs(N, d_skip, d, mode))
    make, kind, param, _ = ACTS[name]
    act = make().to(dev)
    slope = act.weight.detach() if kind == PRELU else None
    p, step = 0.3, 9
    got = _fused_fwd(x, skip, w, b, slope, kind, param, mode, _T(p), step)
    drop = mpnn.Dropout(p, seed=SEED).train()
    drop.set_stream(SEED, step)
    with torch.no_grad():
        y = drop(torch.ops.mp.bn_act(x, w, b, EPS, False)[0])
        want = act(_combine(skip, y, mode))
    assert torch.equal(got, want)


@pytest.mark.parametrize("mode,N,d_skip,d", [(None, 333, 7, 7), (None, 1000, 256, 256), (SUM, 1000, 256, 256),
                                             (CONCAT, 333, 7, 5), (CONCAT, 1000, 256, 64)])
@pytest.mark.parametrize("name", list(KINDS))
def test_threshold_zero_has_the_bits_of_the_undropped_ops(dev, name, mode, N, d_skip, d):
    x, skip, _, w, b = (t.to(dev) for t in _inputs(N, d_skip, d, mode))
    _, kind, param, _ = KINDS[name]
    slope = torch.tensor([0.25], device=dev) if kind == PRELU else None
    got = _fused_fwd(x, skip, w, b, slope, kind, param, mode, 0, 5)
    if mode is None:
        want = torch.ops.mp.bn_actx(x, w, b, slope, EPS, kind, param)[0]
    else:
        want = torch.ops.mp.bn_skip_actx(x, skip, w, b, slope, EPS, kind, param, mode)[0]
    assert same_bits(got, want)


# ---- 5: determinism ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [None, SUM, CONCAT])
def test_two_runs_give_the_same_bits(dev, mode):
    N, d_skip, d = 4097, 36, 36
    x, skip, dy, w, b = (t.to(dev) for t in _inputs(N, d_skip, d, mode))
    slope = torch.tensor([0.25], device=dev)
    T = _T(0.3)

    def run(step):
        if mode is None:
            out, mean, invstd, _ = torch.ops.mp.bn_drop_actx_fwd_raw(x, w, b, slope, EPS, PRELU, 0.0, T, SEED, step)
            return (out,) + tuple(torch.ops.mp.bn_drop_actx_bwd_raw(dy, x, w, b, slope, mean, invstd, PRELU, 0.0, T, SEED,
                                                                    step))
        out, mean, invstd, _ = torch.ops.mp.bn_drop_skip_actx_fwd_raw(x, skip, w, b, slope, EPS, PRELU, 0.0, mode, T, SEED,
                                                                      step)
        return (out,) + tuple(torch.ops.mp.bn_drop_skip_actx_bwd_raw(dy, x, skip, w, b, slope, mean, invstd, mode, PRELU,
                                                                     0.0, T, SEED, step))
    a, c, other = run(3), run(3), run(4)
    for u, v in zip(a, c):
        assert same_bits(u, v)
    assert a[-1].shape == (1,) and float(a[-1].abs()) > 0                      # PRELU's dslope
    assert not torch.equal(a[0] == (skip if mode == SUM else 0), other[0] == (skip if mode == SUM else 0))


# ---- 6: autograd -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode,d_skip", [(None, 12), (SUM, 12), (CONCAT, 6)], ids=["plain", "sum", "cat"])
def test_every_subset_of_differentiated_inputs(dev, mode, d_skip):
    """PRELU, p = 0.3: gradients of a subset of {x, skip, weight, bias, slope} are the all-inputs run's bit for bit, nothing
    outside the subset receives a .grad, and every run is one backward op"""
    N, d, p, step = 257, 12, 0.3, 6
    x, skip, dy, w, b = _inputs(N, d_skip, d, mode)
    ms = _keep(step, N, d, p).float() * _scale(p)
    inputs = {"x": x, "weight": w, "bias": b, "slope": torch.tensor([0.25])}
    if mode is not None:
        inputs["skip"] = skip

    def op(t):
        if mode is None:
            return torch.ops.mp.bn_drop_actx(t["x"], t["weight"], t["bias"], t["slope"], EPS, PRELU, 0.0, _T(p), SEED,
                                             step)[0]
        return torch.ops.mp.bn_drop_skip_actx(t["x"], t["skip"], t["weight"], t["bias"], t["slope"], EPS, PRELU, 0.0,
                                              mode, _T(p), SEED, step)[0]

    def oracle(c, t, eng):
        pre = _combine(t.get("skip"), F.batch_norm(t["x"], None, None, t["weight"], t["bias"], True, MOM, EPS) * c(ms),
                       mode)
        pos = eng[0] > 0                       # slope 0.25: the output has the pre-activation's sign
        q = pre.detach()
        far = q.abs() > 1e-5 * float(q.abs().max())
        assert bool(((q > 0) == pos)[far].all()), "activation pattern differs away from zero"
        return torch.where(pos, pre, t["slope"] * pre)
    full = None
    for s in _gradsub.subsets(list(inputs)):
        with Spy() as spy:
            res = _gradsub.run(op, inputs, oracle, s, dy, dev, params=("weight", "bias", "slope"),
                               what=f"bn_drop_actx mode {mode}")
        bwd = [n for n in spy.mp() if n.endswith("_bwd_raw")]
        assert bwd == ["bn_drop_actx_bwd_raw" if mode is None else "bn_drop_skip_actx_bwd_raw"], (s, bwd)
        if full is None:
            full = res
        else:
            _gradsub.hold_bits(full, res, ("y", "x", "skip", "weight", "bias", "slope"), f"mode {mode} {s}")


def test_nothing_of_the_mask_is_saved(dev):
    """the autograd context keeps x, the parameters and the statistics: no [N, d] tensor beside x (and skip)"""
    N, d = 300, 32
    x, skip, dy, w, b = (t.to(dev) for t in _inputs(N, d, d, SUM))
    saved = []
    with torch.autograd.graph.saved_tensors_hooks(lambda t: saved.append(t) or t, lambda t: t):
        xg = x.clone().requires_grad_(True)
        torch.ops.mp.bn_drop_skip_actx(xg, skip, w, b, None, EPS, ELU, 1.0, SUM, _T(0.3), SEED, 0)
    big = [t for t in saved if t.numel() >= N * d]
    assert len(big) == 2 and {t.data_ptr() for t in big} == {xg.data_ptr(), skip.data_ptr()}


def test_opcheck(dev):
    gen = torch.Generator().manual_seed(0)

    def t(*shape):
        return torch.randn(*shape, generator=gen).to(dev).requires_grad_(True)
    n, d, T = 300, 32, _T(0.3)
    slope = lambda: torch.tensor([0.25], device=dev, requires_grad=True)      # noqa: E731
    for args in [(t(n, d), t(d), t(d), slope(), EPS, PRELU, 0.0, T, SEED, 1), (t(n, d), t(d), t(d), None, EPS, ELU, 1.0, T, SEED, 2),
                 (t(n, d), None, None, None, EPS, SILU, 0.0, T, SEED, 3), (t(n, d), t(d), t(d), None, EPS, NONE, 0.0, T, SEED, 4)]:
        res = torch.library.opcheck(torch.ops.mp.bn_drop_actx.default, args, raise_exception=True)
        assert all(v == "SUCCESS" for v in res.values()), res
    for args in [(t(n, d), t(n, d), t(d), t(d), slope(), EPS, PRELU, 0.0, SUM, T, SEED, 1),
                 (t(n, d), t(n, 20), t(d), t(d), slope(), EPS, PRELU, 0.0, CONCAT, T, SEED, 2),
                 (t(n, d), t(n, 20), t(d), t(d), None, EPS, SELU, 0.0, CONCAT, T, SEED, 3),
                 (t(n, d), t(n, d), None, None, None, EPS, NONE, 0.0, SUM, T, SEED, 4)]:
        res = torch.library.opcheck(torch.ops.mp.bn_drop_skip_actx.default, args, raise_exception=True)
        assert all(v == "SUCCESS" for v in res.values()), res
    for args in [(t(n, d), T, SEED, 1), (t(n, 7), 0, SEED, 2), (t(n, d), 65536, SEED, 3)]:
        res = torch.library.opcheck(torch.ops.mp.dropout_keyed.default, args, raise_exception=True)
        assert all(v == "SUCCESS" for v in res.values()), res


# ---- 7: wide views -----------------------------------------------------------------------------------------------------
def _ws(N, d, dev):
    from graphgym_amd import _lib
    nb = C.c_size_t(0)
    _lib.check(_lib.lib().mp_bn_drop_ws_bytes(N, d, C.byref(nb)))
    return torch.empty(nb.value, dtype=torch.uint8, device=dev), nb.value


@pytest.mark.parametrize("lay", WIDE, ids=IDS)
def test_wide_mask(dev, lay):
    """mp_dropout_keyed_f32 on an 8-column slice of a [70 000, 32 768 (+3)] buffer: rows past 2^32 bytes and 2^31 elements"""
    from graphgym_amd import _lib
    from graphgym_amd.graph import _stream
    N, d, p, step = N_WIDE, 8, 0.3, 1
    need(2 * N * 32_771 * 4 + (1 << 30), "dropout_keyed, wide")
    what = f"wide dropout_keyed [{lay[0]}]"
    xb, xv = wide_of(torch.ones(N, d), lay, dev)
    ob, ov = wide_empty(N, d, lay, dev)
    with Kept((xb, xv, lay)):
        _lib.check(_lib.lib().mp_dropout_keyed_f32(_lib.ptr(xv), xv.stride(0), N, d, _T(p), SEED, step, _lib.ptr(ov),
                                                   ov.stride(0), _stream()), what)
    assert_beside(ob, lay, d, what)
    wide_written(ov, what)
    assert torch.equal(ov.cpu(), _keep(step, N, d, p).float() * _scale(p)), what


@pytest.mark.parametrize("lay,mode", [(WIDE[1], None), (WIDE[0], SUM)], ids=[f"plain-{IDS[1]}", f"sum-{IDS[0]}"])
def test_wide_buffers(dev, lay, mode):
    """PRELU — the plain entries in their scalar form, the skip entries (SUM) in their 4-wide form: x, skip, out, dy, dx and
    dskip as 8-column slices of [70 000, 32 768 (+3)] buffers, rows past 2^32 bytes and 2^31 elements"""
    from graphgym_amd import _lib
    from graphgym_amd.graph import _stream
    pt = _lib.ptr
    N, d, p, step = N_WIDE, 8, 0.3, 2
    need(6 * N * 32_771 * 4 + (1 << 30), "bn drop, wide")
    what = f"wide bn drop {mode} [{lay[0]}]"
    T = _T(p)
    x, skip, dy, w, b = _inputs(N, d, d, mode)
    ms = _keep(step, N, d, p).float() * _scale(p)
    rows = sample_rows(N, seed=6)
    rd = rows.to(dev)
    gd, bd, slope = w.to(dev), b.to(dev), torch.tensor([0.25], device=dev)
    ws, nb = _ws(N, d, dev)
    mean, invstd, var = (torch.empty(d, device=dev) for _ in range(3))
    xb, xv = wide_of(x, lay, dev)
    sb, sv = wide_of(skip, lay, dev) if mode is not None else (None, None)
    ob, ov = wide_empty(N, d, lay, dev)
    kept = [(xb, xv, lay)] + ([(sb, sv, lay)] if mode is not None else [])
    with Kept(*kept):
        if mode is None:
            rc = _lib.lib().mp_bn_train_fwd_drop_act_f32(pt(xv), xv.stride(0), N, d, pt(gd), pt(bd), EPS, PRELU, 0.0,
                                                         pt(slope), T, SEED, step, pt(ov), ov.stride(0), pt(mean),
                                                         pt(invstd), pt(var), pt(ws), nb, _stream())
        else:
            rc = _lib.lib().mp_bn_train_fwd_drop_skip_act_f32(pt(xv), xv.stride(0), pt(sv), sv.stride(0), N, d, d, mode,
                                                              pt(gd), pt(bd), EPS, PRELU, 0.0, pt(slope), T, SEED, step,
                                                              pt(ov), ov.stride(0), pt(mean), pt(invstd), pt(var), pt(ws),
                                                              nb, _stream())
        _lib.check(rc, what)
    assert_beside(ob, lay, d, what)
    wide_written(ov, what)
    pos = (_pre_bits(x, skip, w, b, mode, dev, T, step) > 0).cpu()
    _check_pattern(x, skip, w, b, mode, ms, pos)
    r = _oracle("prelu", x, skip, dy, w, b, mode, ms, pos)
    take = lambda i: (r[0][i][rows], r[1][i][rows])     # noqa: E731
    got = ov[rd]
    assert bool(torch.isfinite(got).all()), what
    close(got, take(0), what=what + " out")
    del ob, ov
    gb, gv = wide_of(dy, lay, dev)
    dxb, dxv = wide_empty(N, d, lay, dev)
    dsb, dsv = wide_empty(N, d, lay, dev) if mode is not None else (None, None)
    dgamma, dbeta, dslope = torch.empty(d, device=dev), torch.empty(d, device=dev), torch.empty(1, device=dev)
    with Kept((gb, gv, lay), *kept):
        if mode is None:
            rc = _lib.lib().mp_bn_train_bwd_drop_act_f32(pt(gv), gv.stride(0), pt(xv), xv.stride(0), N, d, pt(gd), pt(bd),
                                                         pt(mean), pt(invstd), PRELU, 0.0, pt(slope), T, SEED, step,
                                                         pt(dxv), dxv.stride(0), pt(dgamma), pt(dbeta), pt(dslope),
                                                         pt(ws), nb, _stream())
        else:
            rc = _lib.lib().mp_bn_train_bwd_drop_skip_act_f32(pt(gv), gv.stride(0), pt(xv), xv.stride(0), pt(sv),
                                                              sv.stride(0), N, d, d, mode, pt(gd), pt(bd), pt(mean),
                                                              pt(invstd), PRELU, 0.0, pt(slope), T, SEED, step, pt(dxv),
                                                              dxv.stride(0), pt(dsv), dsv.stride(0), pt(dgamma),
                                                              pt(dbeta), pt(dslope), pt(ws), nb, _stream())
        _lib.check(rc, what)
    if mode is not None:
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


# ---- 8: routing --------------------------------------------------------------------------------------------------------
D = 64


def _aten_dropout(spy):
    return [s for s in spy.seen if "dropout" in s.lower() and not s.startswith("mp.")]


def test_a_keyed_dropout_layer_is_one_op(dev, gcfg, graph):  # noqa: F811
    from graphgym_amd import harness as H, nn as mpnn
    x = graph[1].to(dev)
    gcfg.gnn.dropout, gcfg.gnn.keyed_dropout = 0.1, True
    torch.manual_seed(1)
    layer = H.GeneralLayer("linear", D, D).to(dev).train()
    assert [type(m) for m in layer.post_layer] == [mpnn.BatchNorm1d, mpnn.Dropout, nn.PReLU]
    drop = layer.post_layer[1]
    with Spy() as spy:
        out = layer(x)
        out.sum().backward()
    assert spy.mp().count("bn_drop_actx") == 1 and spy.mp().count("bn_drop_actx_bwd_raw") == 1, spy.mp()
    assert not _aten_dropout(spy) and "bn_actx" not in spy.mp() and "dropout_keyed" not in spy.mp(), spy.seen
    assert not spy.prelu() and drop.step == 1
    got = [out.detach()] + [q.grad.clone() for q in layer.parameters()]
    assert layer.post_layer[2].weight.grad is not None and int(layer.post_layer[0].num_batches_tracked) == 1
    # the Sequential with the same counter value: BatchNorm on the engine, mp::dropout_keyed, torch's PReLU
    layer.zero_grad()
    drop.set_stream(drop.seed, 0)
    ref = layer.post_layer(layer.layer(x))
    ref.sum().backward()
    assert torch.equal(got[0], ref.detach())
    assert 0.05 < float((ref == 0).float().mean()) < 0.15
    for g, q in zip(got[1:], layer.parameters()):
        close_all(g, q.grad.double(), what="keyed dropout layer grads")
    # a layer without activation
    bare = H.GeneralLayer("linear", D, D, has_act=False).to(dev).train()
    with Spy() as spy:
        bare(x).sum().backward()
    assert spy.mp().count("bn_drop_actx") == 1 and not _aten_dropout(spy) and "dropout_keyed" not in spy.mp(), spy.mp()


@pytest.mark.parametrize("stage", ["skipsum", "skipconcat"])
def test_a_keyed_dropout_skip_block_is_one_op(dev, gcfg, graph, stage):  # noqa: F811
    from graphgym_amd import harness as H, nn as mpnn
    ei, x = graph
    gcfg.gnn.stage_type, gcfg.gnn.dropout, gcfg.gnn.keyed_dropout = stage, 0.1, True
    torch.manual_seed(2)
    blk = H.GNNSkipBlock(D, D, 2).to(dev).train()
    assert [type(m) for m in blk.f[-1].post_layer] == [mpnn.BatchNorm1d, mpnn.Dropout]
    with Spy() as spy:
        out = blk(_batch(dev, x, ei)).node_feature
        out.sum().backward()
    assert spy.mp().count("bn_drop_skip_actx") == 1 and spy.mp().count("bn_drop_actx") == 1, spy.mp()   # the tail, the inner layer
    assert spy.mp().count("bn_drop_skip_actx_bwd_raw") == 1
    assert not _aten_dropout(spy) and "bn_skip_actx" not in spy.mp() and not spy.prelu(), spy.seen
    drops = [m for m in blk.modules() if isinstance(m, mpnn.Dropout)]
    assert len(drops) == 2 and all(m.step == 1 for m in drops)
    got = [out.detach()] + [q.grad.clone() for q in blk.parameters()]
    blk.zero_grad()
    for m in drops:
        m.set_stream(m.seed, 0)
    h = blk.f(_batch(dev, x, ei)).node_feature              # the layers as they are (each one op), then the unfused tail
    x0 = x.to(dev)
    ref = blk.act(x0 + h if stage == "skipsum" else torch.cat((x0, h), 1))
    ref.sum().backward()
    assert out.shape == (x.size(0), D if stage == "skipsum" else 2 * D)
    assert torch.equal(got[0], ref.detach())
    for g, q in zip(got[1:], blk.parameters()):
        close_all(g, q.grad.double(), what=f"keyed dropout {stage} grads")


def test_eval_mode_is_the_composition(dev, gcfg, graph):  # noqa: F811
    from graphgym_amd import harness as H
    ei, x = graph
    gcfg.gnn.stage_type, gcfg.gnn.dropout, gcfg.gnn.keyed_dropout = "skipsum", 0.1, True
    torch.manual_seed(3)
    layer = H.GeneralLayer("linear", D, D).to(dev).train()
    blk = H.GNNSkipBlock(D, D, 1).to(dev).train()
    with torch.no_grad():                       # running statistics that are not the initial ones
        layer(x.to(dev)); blk(_batch(dev, x, ei))
    layer.eval(); blk.eval()
    with Spy() as spy, torch.no_grad():
        out = layer(x.to(dev))
        sk = blk(_batch(dev, x, ei)).node_feature
    assert not [n for n in spy.mp() if "drop" in n], spy.mp()
    assert layer.post_layer[1].step == 1        # the one training call above; eval takes no counter value
    with torch.no_grad():
        ref = layer.post_layer(layer.layer(x.to(dev)))
        rsk = blk.act(x.to(dev) + blk.f(_batch(dev, x, ei)).node_feature)
    assert torch.equal(out, ref) and torch.equal(sk, rsk)


# ---- 9: a model --------------------------------------------------------------------------------------------------------
def test_example_node_shape_trains_on_the_keyed_route(dev, gcfg, graph):  # noqa: F811
    """run/configs/pyg/example_node.yaml's shape — sageconv, skipsum, 1 / 3 / 1 layers, prelu, dropout 0.1 — on BA(500, 4)"""
    from graphgym_amd import harness as H, nn as mpnn
    ei, x = graph
    c = gcfg
    c.gnn.layer_type, c.gnn.stage_type, c.gnn.act, c.gnn.dropout, c.gnn.keyed_dropout = "sageconv", "skipsum", "prelu", 0.1, True
    c.gnn.layers_pre_mp, c.gnn.layers_mp, c.gnn.layers_post_mp, c.gnn.agg = 1, 3, 1, "mean"
    torch.manual_seed(0)
    model = H.GNN(dim_in=D, dim_out=4).to(dev).train()
    drops = [m for m in model.modules() if isinstance(m, nn.Dropout)]
    assert len(drops) >= 4 and all(type(m) is mpnn.Dropout for m in drops)
    assert len({m.seed for m in drops}) == len(drops)                    # every layer its own seed
    label = torch.randint(0, 4, (x.size(0),), generator=torch.Generator().manual_seed(3)).to(dev)
    opt = torch.optim.SGD(model.parameters(), lr=0.01)
    losses = []
    for _ in range(3):
        batch = H.Batch(node_feature=x.to(dev), edge_index=ei.to(dev), node_label=label,
                        node_label_index=torch.arange(x.size(0), device=dev))
        opt.zero_grad()
        with Spy() as spy:
            pred, true = model(batch)
            loss = F.cross_entropy(pred, true)
            loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        assert not _aten_dropout(spy), _aten_dropout(spy)
        assert spy.mp().count("bn_drop_skip_actx") == 3 and spy.mp().count("bn_drop_actx") >= 1, spy.mp()
    assert all(m.step == 3 for m in drops), [m.step for m in drops]
    assert all(torch.isfinite(torch.tensor(losses))), losses
