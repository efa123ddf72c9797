"""The skip block's fused pass (csrc/bn.hip: mp_bn_train_fwd_skip_f32 / mp_bn_train_bwd_skip_f32, the ops
mp::bn_skip_fwd_raw / bn_skip_bwd_raw / bn_skip_act and graphgym_amd.nn.bn_skip_act) against the torch composition on the
CPU — torch.nn.BatchNorm1d in training mode -> add / cat -> ReLU (graphgym/models/gnn.py:49-60 behind a last layer
without activation) — in float64 and float32 (tests/_tol.py: both), through the engine's own ReLU pattern as
tests/test_bn_gpu.py does; bit for bit against the existing BatchNorm kernels; on strided, offset and misaligned operand
views; under every subset of differentiated inputs; and on buffers whose rows lie past 2^32 bytes."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import _gradsub
from _bigview import IDS, N_WIDE, WIDE, Kept, assert_beside, need, sample_rows, wide_empty, wide_of
from _bigview import assert_written as wide_written
from _layout import LAYOUTS, OFF1, Unchanged, assert_untouched, assert_written, out_view, same_bits, view_of
from _tol import both, close, close_all

pytestmark = pytest.mark.gpu

SUM, CONCAT = 0, 1
EPS, MOM = 1e-5, 0.1
SUM_SHAPES = [(2, 4, 4), (333, 7, 7), (4097, 100, 100), (1000, 256, 256), (50000, 64, 64)]
CAT_SHAPES = [(2, 4, 4), (333, 7, 5), (4097, 6, 8), (1000, 100, 36), (1000, 256, 64), (50000, 64, 64)]   # (N, d_skip, d)
CASES = [(SUM,) + s for s in SUM_SHAPES] + [(CONCAT,) + s for s in CAT_SHAPES]
CASE_IDS = [f"{'sum' if m == SUM else 'cat'}-{n}-{ds}-{d}" for m, n, ds, d in CASES]


def _inputs(N, d_skip, d, mode):
    g = torch.Generator().manual_seed(N + d)
    x = torch.randn(N, d, generator=g) * (torch.rand(d, generator=g) * 3 + 0.1) + torch.randn(d, generator=g) * 5
    skip = torch.randn(N, d_skip, generator=g)
    dy = torch.randn(N, d if mode == SUM else d_skip + d, generator=g)
    w, b = torch.rand(d, generator=g) + 0.5, torch.randn(d, generator=g)
    return x, skip, dy, w, b


def _combine(skip, y, mode):
    return skip + y if mode == SUM else torch.cat((skip, y), 1)


def _check_pattern(x, skip, w, b, mode, mask):
    """the float64 pre-activation disagrees with the engine's ReLU pattern only within 1e-5 of the largest magnitude"""
    pre = _combine(skip.double(), F.batch_norm(x.double(), None, None, w.double(), b.double(), True, MOM, EPS), mode)
    off = (pre > 0) != mask
    assert not bool(off.any()) or float(pre.abs()[off].max()) <= 1e-5 * float(pre.abs().max())


def _oracle(x, skip, dy, w, b, mode, mask):
    """(out, dx, dskip, dgamma, dbeta, running_mean, running_var) of the composition in float64 and float32; mask: the
    engine's ReLU pattern (None: no activation)"""
    def fn(c):
        ref = torch.nn.BatchNorm1d(x.size(1), eps=EPS, momentum=MOM).to(c(x).dtype)
        with torch.no_grad():
            ref.weight.copy_(c(w)); ref.bias.copy_(c(b))
        xr, sr = c(x).clone().requires_grad_(True), c(skip).clone().requires_grad_(True)
        z = _combine(sr, ref(xr), mode)
        if mask is not None:
            z = z * mask.to(z.dtype)
        z.backward(c(dy))
        return (z.detach(), xr.grad, sr.grad, ref.weight.grad, ref.bias.grad, ref.running_mean.clone(),
                ref.running_var.clone())
    return both(fn)


def _pair(r, i):
    return (r[0][i], r[1][i])


@pytest.mark.parametrize("mode,N,d_skip,d", CASES, ids=CASE_IDS)
@pytest.mark.parametrize("relu", [False, True])
def test_parity_with_the_torch_composition(dev, mode, N, d_skip, d, relu):
    """graphgym_amd.nn.bn_skip_act on a BatchNorm1d module: forward, the four gradients, running statistics after a step"""
    from graphgym_amd import nn as mpnn
    x, skip, dy, w, b = _inputs(N, d_skip, d, mode)
    bn = mpnn.BatchNorm1d(d, eps=EPS, momentum=MOM).to(dev)
    with torch.no_grad():
        bn.weight.copy_(w); bn.bias.copy_(b)
    xg, sg = x.to(dev).requires_grad_(True), skip.to(dev).requires_grad_(True)
    out = mpnn.bn_skip_act(bn, xg, sg, mode, relu=relu)
    assert out.shape == dy.shape
    out.backward(dy.to(dev))
    mask = (out.detach() > 0).cpu() if relu else None
    if relu:
        _check_pattern(x, skip, w, b, mode, mask)
    r = _oracle(x, skip, dy, w, b, mode, mask)
    what = f"skip {'sum' if mode == SUM else 'cat'} relu={relu}"
    close(out, _pair(r, 0), what=what + " out")
    if N >= 8:
        close(xg.grad, _pair(r, 1), what=what + " dx")
    else:       # a batch of two: dx is the rounding residue of terms that cancel exactly (tests/test_bn_gpu.py)
        close_all(xg.grad, _pair(r, 1), what=what + " dx (degenerate batch)")
    close(sg.grad, _pair(r, 2), what=what + " dskip")
    close_all(bn.weight.grad, _pair(r, 3), what=what + " dgamma")
    close_all(bn.bias.grad, _pair(r, 4), what=what + " dbeta")
    col = lambda t: t.detach().reshape(-1, 1)      # noqa: E731  one statistic per column: each its own scale
    close(col(bn.running_mean), (col(r[0][5]), col(r[1][5])), what=what + " running_mean")
    close(col(bn.running_var), (col(r[0][6]), col(r[1][6])), what=what + " running_var")
    assert int(bn.num_batches_tracked) == 1


@pytest.mark.parametrize("N,d", [(333, 7), (4097, 100), (1000, 256)])
@pytest.mark.parametrize("relu", [False, True])
def test_sum_has_the_bits_of_the_batchnorm_kernels(dev, N, d, relu):
    """SUM with skip = 0 is mp_bn_train_fwd_f32; its backward is mp_bn_train_bwd_f32(dy, y = out) plus dskip"""
    ops = torch.ops.mp
    x, skip, dy, w, b = (t.to(dev) for t in _inputs(N, d, d, SUM))
    y0, m0, i0, v0 = ops.bn_fwd_raw(x, w, b, EPS, relu)
    out, mean, invstd, var = ops.bn_skip_fwd_raw(x, torch.zeros_like(skip), w, b, EPS, relu, SUM)
    assert torch.equal(out, y0) and torch.equal(mean, m0) and torch.equal(invstd, i0) and torch.equal(var, v0)
    out, mean, invstd, var = ops.bn_skip_fwd_raw(x, skip, w, b, EPS, relu, SUM)          # a real skip operand
    assert torch.equal(mean, m0) and torch.equal(invstd, i0)
    if relu:
        assert 0.2 < float((out > 0).float().mean()) < 0.8
    dx0, dg0, db0 = ops.bn_bwd_raw(dy, out if relu else None, x, w, mean, invstd)
    dx, dg, db, dskip = ops.bn_skip_bwd_raw(dy, out if relu else None, x, w, mean, invstd, SUM)
    assert torch.equal(dx, dx0) and torch.equal(dg, dg0) and torch.equal(db, db0)
    if relu:
        assert torch.equal(dskip, dy * (out > 0))
    else:
        assert dskip.numel() == 0                       # d(skip) is dy itself: nothing is written
    dx, dg, db, none = ops.bn_skip_bwd_raw(dy, out if relu else None, x, w, mean, invstd, SUM, False)
    assert torch.equal(dx, dx0) and torch.equal(dg, dg0) and torch.equal(db, db0) and none.numel() == 0


@pytest.mark.parametrize("N,d_skip,d", [(333, 7, 5), (4097, 6, 8), (1000, 100, 36), (1000, 256, 64)])
@pytest.mark.parametrize("relu", [False, True])
def test_concat_slabs_have_the_bits_of_their_parts(dev, N, d_skip, d, relu):
    """CONCAT: the right slab is mp_bn_train_fwd_f32's y (also where out + d_skip is misaligned: (4097, 6, 8)), the left
    slab is relu(skip); the backward is mp_bn_train_bwd_f32 on the right-hand column views"""
    ops = torch.ops.mp
    x, skip, dy, w, b = (t.to(dev) for t in _inputs(N, d_skip, d, CONCAT))
    y0, m0, i0, v0 = ops.bn_fwd_raw(x, w, b, EPS, relu)
    out, mean, invstd, var = ops.bn_skip_fwd_raw(x, skip, w, b, EPS, relu, CONCAT)
    assert out.shape == (N, d_skip + d)
    assert torch.equal(out[:, d_skip:], y0) and torch.equal(out[:, :d_skip], torch.relu(skip) if relu else skip)
    assert torch.equal(mean, m0) and torch.equal(invstd, i0) and torch.equal(var, v0)
    dx0, dg0, db0 = ops.bn_bwd_raw(dy[:, d_skip:].contiguous(), y0 if relu else None, x, w, mean, invstd)
    dx, dg, db, dskip = ops.bn_skip_bwd_raw(dy, out if relu else None, x, w, mean, invstd, CONCAT)
    if d % 4 != 0 or d_skip % 4 == 0:       # the views take the form (4-wide or scalar) the contiguous operands take
        assert torch.equal(dx, dx0) and torch.equal(dg, dg0) and torch.equal(db, db0)
    else:       # (4097, 6, 8): dy + d_skip is misaligned, the scalar kernels sum their partial slabs in another order
        close(dx, dx0.double(), what="cat dx on misaligned views")
        close_all(dg, dg0.double(), what="cat dgamma on misaligned views")
        close_all(db, db0.double(), what="cat dbeta on misaligned views")
    if relu:
        assert torch.equal(dskip, dy[:, :d_skip] * (out[:, :d_skip] > 0))
    else:
        assert dskip.numel() == 0


# ---- layouts: every operand of the C entries a column slice of a wider buffer ----------------------------------------
def _ws(N, d, dev):
    from graphgym_amd import _lib
    nb = C.c_size_t(0)
    _lib.check(_lib.lib().mp_bn_ws_bytes(N, d, C.byref(nb)))
    return torch.empty(nb.value, dtype=torch.uint8, device=dev), nb.value


def _c_fwd(xv, sv, gd, bd, relu, mode, ov, stats, ws, nb, what):
    from graphgym_amd import _lib
    from graphgym_amd.graph import _stream
    p = _lib.ptr
    N, d = xv.shape
    _lib.check(_lib.lib().mp_bn_train_fwd_skip_f32(p(xv), xv.stride(0), p(sv), sv.stride(0), N, d, sv.size(1), mode, p(gd),
                                                   p(bd), EPS, int(relu), p(ov), ov.stride(0), p(stats[0]), p(stats[1]),
                                                   p(stats[2]), p(ws), nb, _stream()), what)


def _c_bwd_sum(gv, ov, xv, gd, stats, dxv, dsv, dgamma, dbeta, ws, nb, what):
    from graphgym_amd import _lib
    from graphgym_amd.graph import _stream
    p = _lib.ptr
    N, d = xv.shape
    _lib.check(_lib.lib().mp_bn_train_bwd_skip_f32(p(gv), gv.stride(0), p(ov), ov.stride(0) if ov is not None else 0,
                                                   p(xv), xv.stride(0), N, d, p(gd), p(stats[0]), p(stats[1]), p(dxv),
                                                   dxv.stride(0), p(dsv), dsv.stride(0) if dsv is not None else 0,
                                                   p(dgamma), p(dbeta), p(ws), nb, _stream()), what)


def _c_bwd_plain(gv, yv, xv, gd, stats, dxv, dgamma, dbeta, ws, nb, what):
    from graphgym_amd import _lib
    from graphgym_amd.graph import _stream
    p = _lib.ptr
    N, d = xv.shape
    _lib.check(_lib.lib().mp_bn_train_bwd_f32(p(gv), gv.stride(0), p(yv), yv.stride(0), p(xv), xv.stride(0), N, d, p(gd),
                                              p(stats[0]), p(stats[1]), p(dxv), dxv.stride(0), p(dgamma), p(dbeta),
                                              p(ws), nb, _stream()), what)


_LAYOUT_REF = {}


def _layout_ref(dev, mode, N, d_skip, d):
    """the contiguous run of the ops and the composition's oracle, computed once per mode"""
    key = (mode, N, d_skip, d)
    if key not in _LAYOUT_REF:
        ops = torch.ops.mp
        x, skip, dy, w, b = _inputs(N, d_skip, d, mode)
        out, mean, invstd, var = ops.bn_skip_fwd_raw(x.to(dev), skip.to(dev), w.to(dev), b.to(dev), EPS, True, mode)
        dx, dg, db, dskip = ops.bn_skip_bwd_raw(dy.to(dev), out, x.to(dev), w.to(dev), mean, invstd, mode)
        mask = (out > 0).cpu()
        _check_pattern(x, skip, w, b, mode, mask)
        _LAYOUT_REF[key] = ((x, skip, dy, w, b), (out, dx, dskip, dg, db), _oracle(x, skip, dy, w, b, mode, mask))
    return _LAYOUT_REF[key]


@pytest.mark.parametrize("mode,d_skip", [(SUM, 8), (CONCAT, 8), (CONCAT, 6)], ids=["sum", "cat", "cat-dskip6"])
@pytest.mark.parametrize("lay", [LAYOUTS[2], OFF1], ids=["aligned-offset", "misaligned-offset"])
def test_operands_as_column_slices(dev, mode, d_skip, lay):
    """x, skip, out, dy, dx and dskip at an aligned (16-byte) and a misaligned (4-byte) offset of wider buffers: inputs
    keep their bits, nothing beside an output slice is written, the aligned layout has the contiguous run's bits"""
    N, d = 777, 8
    (x, skip, dy, w, b), cont, r = _layout_ref(dev, mode, N, d_skip, d)
    what = f"skip layouts mode {mode} d_skip {d_skip} [{lay[0]}]"
    width = d if mode == SUM else d_skip + d
    gd, bd = w.to(dev), b.to(dev)
    ws, nb = _ws(N, d, dev)
    stats = [torch.empty(d, device=dev) for _ in range(3)]
    xb, xv = view_of(x, lay, dev, seed=1)
    sb, sv = view_of(skip, lay, dev, seed=2)
    gb, gv = view_of(dy, lay, dev, seed=3)
    ob, ov = out_view(N, width, lay, dev)
    with Unchanged(xb, sb):
        _c_fwd(xv, sv, gd, bd, True, mode, ov, stats, ws, nb, what)
    assert_untouched(ob, lay[2], width, what)
    assert_written(ov, what)
    close(ov, _pair(r, 0), what=what + " out")
    dxb, dxv = out_view(N, d, lay, dev)
    dsb, dsv = out_view(N, d_skip, lay, dev)
    dgamma, dbeta = torch.empty(d, device=dev), torch.empty(d, device=dev)
    with Unchanged(xb, gb, ob):
        if mode == SUM:
            _c_bwd_sum(gv, ov, xv, gd, stats, dxv, dsv, dgamma, dbeta, ws, nb, what)
        else:       # the existing backward on the right-hand column views of dy and out
            _c_bwd_plain(gv[:, d_skip:], ov[:, d_skip:], xv, gd, stats, dxv, dgamma, dbeta, ws, nb, what)
    assert_untouched(dxb, lay[2], d, what + " dx")
    assert_written(dxv, what + " dx")
    close(dxv, _pair(r, 1), what=what + " dx")
    close_all(dgamma, _pair(r, 3), what=what + " dgamma")
    close_all(dbeta, _pair(r, 4), what=what + " dbeta")
    if mode == SUM:
        assert_untouched(dsb, lay[2], d_skip, what + " dskip")
        assert_written(dsv, what + " dskip")
        assert torch.equal(dsv, gv * (ov > 0)), what
        close(dsv, _pair(r, 2), what=what + " dskip")
    if lay is LAYOUTS[2] and d_skip % 4 == 0:      # rows on 16-byte boundaries: the same vector kernels as the contiguous run
        assert same_bits(ov, cont[0]) and same_bits(dxv, cont[1]), what
        assert same_bits(dgamma, cont[3]) and same_bits(dbeta, cont[4]), what
    # the ops on the same views (no copy is made of a column slice): the C entries' bits
    with Unchanged(xb, sb, gb):
        out, mean, invstd, _ = torch.ops.mp.bn_skip_fwd_raw(xv, sv, gd, bd, EPS, True, mode)
        dx, dg, db, dskip = torch.ops.mp.bn_skip_bwd_raw(gv, out, xv, gd, mean, invstd, mode)
    assert same_bits(out, ov) and same_bits(dx, dxv) and same_bits(dg, dgamma) and same_bits(db, dbeta), what
    assert torch.equal(dskip, gv[:, :d_skip] * (out[:, :d_skip] > 0)), what


def test_the_c_entry_without_activation_writes_no_dskip(dev):
    """relu == 0 (out NULL): dskip is not written (and may be NULL); dx, dgamma, dbeta are mp_bn_train_bwd_f32's"""
    N, d = 777, 8
    x, skip, dy, w, b = (t.to(dev) for t in _inputs(N, d, d, SUM))
    ws, nb = _ws(N, d, dev)
    out, mean, invstd, _ = torch.ops.mp.bn_skip_fwd_raw(x, skip, w, b, EPS, False, SUM)
    dx0, dg0, db0 = torch.ops.mp.bn_bwd_raw(dy, None, x, w, mean, invstd)
    dsb, dsv = out_view(N, d, LAYOUTS[0], dev)
    for ds in (dsv, None):
        dx, dg, db = torch.empty_like(x), torch.empty(d, device=dev), torch.empty(d, device=dev)
        _c_bwd_sum(dy, None, x, w, [mean, invstd], dx, ds, dg, db, ws, nb, "no activation")
        assert torch.equal(dx, dx0) and torch.equal(dg, dg0) and torch.equal(db, db0)
    from _layout import assert_all_sentinel
    assert_all_sentinel(dsb, "dskip without activation")


# ---- every subset of differentiated inputs -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode,d_skip", [(SUM, 12), (CONCAT, 6)], ids=["sum", "cat"])
@pytest.mark.parametrize("relu", [True, False])
def test_every_subset_of_differentiated_inputs(dev, mode, d_skip, relu):
    """gradients of a subset are the all-inputs run's bit for bit, nothing outside the subset receives a .grad; with
    only `skip` in the subset no BatchNorm backward runs, with `skip` outside it no dskip is produced"""
    N, d = 257, 12
    x, skip, dy, w, b = _inputs(N, d_skip, d, mode)
    calls = []

    def op(t):
        return torch.ops.mp.bn_skip_act(t["x"], t["skip"], t["weight"], t["bias"], EPS, relu, mode)[0]

    def oracle(c, t, eng):
        pre = _combine(t["skip"], F.batch_norm(t["x"], None, None, t["weight"], t["bias"], True, MOM, EPS), mode)
        return _gradsub.relu_like(pre, c(eng[0])) if relu else pre
    inputs = {"x": x, "skip": skip, "weight": w, "bias": b}
    from torch.utils._python_dispatch import TorchDispatchMode

    class Spy(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            if str(func).startswith("mp."):
                calls.append((str(func).split(".")[1], args, kwargs or {}))
            return func(*args, **(kwargs or {}))
    full = None
    for s in _gradsub.subsets(list(inputs)):
        del calls[:]
        with Spy():
            res = _gradsub.run(op, inputs, oracle, s, dy, dev, params=("weight", "bias"),
                               what=f"bn_skip_act mode {mode} relu {relu}")
        names = [c[0] for c in calls]
        if s == ("skip",):
            assert "bn_skip_bwd_raw" not in names and "bn_bwd_raw" not in names, names
        else:
            (bwd,) = [c for c in calls if c[0] == "bn_skip_bwd_raw"]
            # want_dskip: the dispatcher drops a trailing argument that has its default value (True)
            want = bwd[1][7] if len(bwd[1]) > 7 else bwd[2].get("want_dskip", True)
            assert want == ("skip" in s), (s, want)
        if full is None:
            full = res
        else:
            _gradsub.hold_bits(full, res, ("y", "x", "skip", "weight", "bias"), f"mode {mode} relu {relu} {s}")


def test_opcheck(dev):
    gen = torch.Generator().manual_seed(0)

    def t(*shape):
        return torch.randn(*shape, generator=gen).to(dev).requires_grad_(True)
    n, d = 300, 32
    for args in [(t(n, d), t(n, d), t(d), t(d), EPS, True, SUM), (t(n, d), t(n, 20), t(d), t(d), EPS, True, CONCAT),
                 (t(n, d), t(n, d), None, None, EPS, False, SUM)]:
        res = torch.library.opcheck(torch.ops.mp.bn_skip_act.default, args, raise_exception=True)
        assert all(v == "SUCCESS" for v in res.values()), res


# ---- rows past 2^32 bytes and 2^31 elements ------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [SUM, CONCAT], ids=["sum", "cat"])
@pytest.mark.parametrize("lay", WIDE, ids=IDS)
def test_wide_buffers(dev, mode, lay):
    """x, skip, out, dy, dx (and dskip) as 8-column slices of [70 000, 32 768 (+3)] buffers"""
    N, d, d_skip = N_WIDE, 8, 8
    width = d if mode == SUM else d_skip + d
    need(6 * N * 32_771 * 4 + (1 << 30), "bn skip, wide")
    what = f"wide bn skip mode {mode} [{lay[0]}]"
    x, skip, dy, w, b = _inputs(N, d_skip, d, mode)
    rows = sample_rows(N, seed=6)
    rd = rows.to(dev)
    gd, bd = w.to(dev), b.to(dev)
    ws, nb = _ws(N, d, dev)
    stats = [torch.empty(d, device=dev) for _ in range(3)]
    xb, xv = wide_of(x, lay, dev)
    sb, sv = wide_of(skip, lay, dev)
    ob, ov = wide_empty(N, width, lay, dev)
    with Kept((xb, xv, lay), (sb, sv, lay)):
        _c_fwd(xv, sv, gd, bd, True, mode, ov, stats, ws, nb, what)
    assert_beside(ob, lay, width, what)
    wide_written(ov, what)
    mask = (ov > 0).cpu()
    _check_pattern(x, skip, w, b, mode, mask)
    r = _oracle(x, skip, dy, w, b, mode, mask)
    take = lambda i: (r[0][i][rows], r[1][i][rows])     # noqa: E731
    got = ov[rd]
    assert bool(torch.isfinite(got).all()), what
    close(got, take(0), what=what + " out")
    del sb, sv
    gb, gv = wide_of(dy, lay, dev)
    dxb, dxv = wide_empty(N, d, lay, dev)
    dgamma, dbeta = torch.empty(d, device=dev), torch.empty(d, device=dev)
    if mode == SUM:
        dsb, dsv = wide_empty(N, d, lay, dev)
        with Kept((gb, gv, lay), (xb, xv, lay), (ob, ov, lay)):
            _c_bwd_sum(gv, ov, xv, gd, stats, dxv, dsv, dgamma, dbeta, ws, nb, what)
        assert_beside(dsb, lay, d, what + " dskip")
        wide_written(dsv, what + " dskip")
        close(dsv[rd], take(2), what=what + " dskip")
    else:
        with Kept((gb, gv, lay), (xb, xv, lay), (ob, ov, lay)):
            _c_bwd_plain(gv[:, d_skip:], ov[:, d_skip:], xv, gd, stats, dxv, dgamma, dbeta, ws, nb, what)
    assert_beside(dxb, lay, d, what + " dx")
    wide_written(dxv, what + " dx")
    got = dxv[rd]
    assert bool(torch.isfinite(got).all()), what
    close(got, take(1), what=what + " dx")
    close_all(dgamma, _pair(r, 3), what=what + " dgamma")
    close_all(dbeta, _pair(r, 4), what=what + " dbeta")
