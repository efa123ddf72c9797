"""Linear (+ ReLU) and BatchNorm1d (+ ReLU) over the node axis on the engine's kernels (csrc/gemm.hip, csrc/bn.hip).

Drop-in for ``torch.nn.BatchNorm1d`` as GraphGym uses it after every conv (graphgym/models/layer.py:26-35)
and as the keras BatchNormalization in the TF path's GIN MLPs (main_zd.py:181-186): same parameter and buffer
names (weight, bias, running_mean, running_var, num_batches_tracked), same momentum / eps semantics.  In
training mode the statistics, the normalisation, the optional ReLU and the whole backward run as four
HBM-bound passes; torch's own kernel needs 0.5 s per backward call on a [10^7, 256] activation.  Any other activation
of GraphGym's act_dict (and SiLU) rides the same passes through bn_act_module / bn_skip_act(act=...): act_spec says which.
gnn.dropout between the BatchNorm and the activation rides them too, as a keyed mask that is recomputed and never stored:
Dropout, dropout_keep_host, bn_act_module / bn_skip_act(drop=...) (csrc/draws.h, csrc/bn_drop.hip).

The 18 BatchNorm ops (torch.ops.mp.bn_*) are six families — bn_act, bn_skip_act, bn_actx, bn_skip_actx, bn_drop_actx,
bn_drop_skip_actx — of a differentiable op over a *_fwd_raw and a *_bwd_raw op.  As the C entries are adapters onto one
forward and one backward runner (csrc/bn_kernels.h), the *_raw ops are adapters onto _bn_fwd and _bn_actx_bwd, their fake
kernels onto _fwd_results and _bwd_results, which also make the real ops' allocations, and the four *actx families share
one autograd formula (_actx_autograd); bn_bwd_raw and bn_skip_bwd_raw, whose entries take the forward's output, keep
bodies of their own.  Every launch goes through _bn_launch, which owns the workspace.
"""
import ctypes as C
from typing import Optional, Tuple

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.library import custom_op, register_autograd

from . import ops, placement
from ._lib import K, check, lib, ptr
from .graph import _require_hip, _stream

Tensor = torch.Tensor


# ---- the BatchNorm ops: the Python half of csrc/bn_kernels.h (see the module docstring) -------------------------------
def _bn_launch(entry, size_fn, x, *args):
    """entry(*args, ws, ws_bytes, stream) on x's device, ws being the workspace that the entry's size function asks for
    at x's [N, d]: mp_bn_ws_bytes, mp_bn_act_ws_bytes or mp_bn_drop_ws_bytes"""
    nb = C.c_size_t(0)
    with torch.cuda.device(x.device):
        check(getattr(lib(), size_fn)(x.size(0), x.size(1), C.byref(nb)))
        ws = torch.empty(nb.value, dtype=torch.uint8, device=x.device)
        check(getattr(lib(), entry)(*args, ptr(ws), nb.value, _stream()), entry)


def _params(weight, bias, slope=None, kind=None):
    """(gamma, beta, PRELU's slope) as the entries read them: detached and contiguous, None where there is none"""
    w = None if weight is None else weight.detach().contiguous()
    b = None if bias is None else bias.detach().contiguous()
    return w, b, _slope32(slope, kind)


def _new32(like, *shape, reads=None):
    """uninitialised fp32 [*shape] on like's device; with reads, an engine output placed against what its launch reads"""
    if reads is None:
        return torch.empty(shape, dtype=torch.float32, device=like.device)
    return placement.empty_or_torch(shape, like.device, reads=reads, streaming=True)


# (forward entry, backward entry, workspace-size function) by (activation kind, skip operand, keyed mask); the entries
# with the run-time relu flag instead of a kind keep the workspace layout of mp_bn_ws_bytes and their own backward ops
_BN_ENTRIES = {
    (False, False, False): ("mp_bn_train_fwd_f32", None, "mp_bn_ws_bytes"),
    (False, True, False): ("mp_bn_train_fwd_skip_f32", None, "mp_bn_ws_bytes"),
    (True, False, False): ("mp_bn_train_fwd_act_f32", "mp_bn_train_bwd_act_f32", "mp_bn_act_ws_bytes"),
    (True, True, False): ("mp_bn_train_fwd_skip_act_f32", "mp_bn_train_bwd_skip_act_f32", "mp_bn_act_ws_bytes"),
    (True, False, True): ("mp_bn_train_fwd_drop_act_f32", "mp_bn_train_bwd_drop_act_f32", "mp_bn_drop_ws_bytes"),
    (True, True, True): ("mp_bn_train_fwd_drop_skip_act_f32", "mp_bn_train_bwd_drop_skip_act_f32", "mp_bn_drop_ws_bytes")}


def _fwd_results(x, skip=None, mode=None, placed=False):
    """(out, mean, invstd, var) of every forward op, uninitialised: out [N, d], or [N, d_skip + d] for SKIP_CONCAT.  As
    it stands the ops' fake kernel; with placed, the real op's allocations (_bn_fwd), so the two cannot disagree"""
    d = x.size(1)
    width = d if (skip is None or mode == SKIP_SUM) else skip.size(1) + d
    reads = None if not placed else (x,) if skip is None else (x, skip)
    out, mean = _new32(x, x.size(0), width, reads=reads), _new32(x, d)
    return out, mean, torch.empty_like(mean), torch.empty_like(mean)


def _bn_fwd(rows, x, weight, bias, eps, relu=None, act=None, skip=None, mode=None, drop=None):
    """(out, mean, invstd, unbiased var): the launch of the six *_fwd_raw ops, with exactly one of relu (a bool: the
    entries with the run-time flag) and act = (kind, param, slope) (the *_act entries), with skip, mode and drop = (T,
    seed, offset) where the op has them, and rows, its rule for its operands, applied after every refusal.  One list:
    x, ldx [, skip, ldskip], N, d [, d_skip, mode], gamma, beta, eps, relu | (kind, param, slope) [, T, seed, offset],
    out, ldo, mean, invstd, var, ws, nb, stream"""
    assert (relu is None) != (act is None)
    has_skip = skip is not None
    kind, param, slope = act or (None, None, None)
    _require_hip(x, "x")
    if has_skip:
        _require_hip(skip, "skip")
        _check_skip_shapes(x, skip, mode)
    if act is not None:
        _check_kind(kind, slope)
    key = () if drop is None else _drop_args(*drop)
    entry, _, size_fn = _BN_ENTRIES[act is not None, has_skip, drop is not None]
    x, skip = rows(x), (rows(skip) if has_skip else None)
    N, d = x.shape
    out, mean, invstd, var_u = _fwd_results(x, skip, mode, placed=True)
    w, b, s = _params(weight, bias, slope, kind)
    operand, dims = ((ptr(skip), skip.stride(0)), (skip.size(1), mode)) if has_skip else ((), ())
    activation = (1 if relu else 0,) if act is None else (kind, float(param), ptr(s))
    _bn_launch(entry, size_fn, x, ptr(x), x.stride(0), *operand, N, d, *dims, ptr(w), ptr(b), float(eps), *activation,
               *key, ptr(out), out.stride(0), ptr(mean), ptr(invstd), ptr(var_u))
    return out, mean, invstd, var_u


def _bn_actx_bwd(rows, dy, x, weight, bias, slope, mean, invstd, kind, param, want_dslope, skip=None, mode=None,
                 want_dskip=False, drop=None):
    """(dx, dgamma, dbeta [, dskip], dslope): the launch of the four *actx_bwd_raw ops; rows, skip, mode, drop as in
    _bn_fwd, whose argument list it follows with dy, lddy in front, mean, invstd for eps, and for the outputs
    dx, lddx [, dskip, lddskip], dgamma, dbeta, dslope"""
    has_skip = skip is not None
    if has_skip:
        _check_skip_shapes(x, skip, mode)
    _check_kind(kind, slope)
    key = () if drop is None else _drop_args(*drop)
    _, entry, size_fn = _BN_ENTRIES[True, has_skip, drop is not None]
    x, skip, dy = rows(x), (rows(skip) if has_skip else None), rows(dy)
    N, d = x.shape
    if has_skip and dy.shape != (N, d if mode == SKIP_SUM else skip.size(1) + d):
        raise ValueError(f"bn_{'' if drop is None else 'drop_'}skip_actx_bwd_raw: dy {tuple(dy.shape)}, x "
                         f"{tuple(x.shape)}, skip {tuple(skip.shape)}, mode {mode} do not fit")
    dx, dgamma, dbeta, *dskip, dslope = results = _bwd_results(dy, x, kind, want_dslope, skip, want_dskip, placed=True)
    operand = dims = dskip_args = ()
    if has_skip:
        operand, dims = (ptr(skip), skip.stride(0)), (skip.size(1), mode)
        dskip_args = (ptr(dskip[0]), dskip[0].stride(0)) if dskip[0].numel() else (None, 0)
    w, b, s = _params(weight, bias, slope, kind)
    _bn_launch(entry, size_fn, x, ptr(dy), dy.stride(0), ptr(x), x.stride(0), *operand, N, d, *dims, ptr(w), ptr(b),
               ptr(mean), ptr(invstd), kind, float(param), ptr(s), *key, ptr(dx), dx.stride(0), *dskip_args,
               ptr(dgamma), ptr(dbeta), ptr(dslope) if dslope.numel() else None)
    return results


def _bwd_results(dy, x, kind=None, want_dslope=False, skip=None, want_dskip=False, placed=False):
    """(dx, dgamma, dbeta [, dskip] [, dslope]), uninitialised, of the four *actx_bwd_raw ops and, without kind, skip and
    dslope, of bn_bwd_raw: the fake kernel as it stands, the real op's allocations with placed (_bn_actx_bwd).  What is
    not written comes back EMPTY (an operator cannot return None or a view of its input): dskip unless asked for and
    there is an activation (without one d(skip) is dy, its left slab, itself: the caller takes it), dslope unless asked
    for and the kind is PRELU"""
    dx = _new32(x, *x.shape, reads=(dy, x) if placed else None)
    dgamma, dskip = _new32(x, x.size(1)), ()
    if skip is not None:
        write = want_dskip and kind != ACT_NONE
        dskip = (_new32(x, *skip.shape, reads=(dy, skip) if placed else None) if write else _new32(x, 0),)
    dslope = () if kind is None else (_new32(x, 1 if (want_dslope and kind == ACT_PRELU) else 0),)
    return (dx, dgamma, torch.empty_like(dgamma)) + dskip + dslope


def _actx_autograd(op, has_skip, has_drop):
    """setup_context and backward of one of the four differentiable *actx ops, whose inputs are
    (x [, skip], weight, bias, slope, eps, kind, param [, mode] [, T, seed, offset]); the backward is <op>_bwd_raw"""
    i = 2 if has_skip else 1                    # inputs[i:] = weight, bias, slope, eps, kind, param [, mode] [, the key]
    n_inputs = i + 6 + (1 if has_skip else 0) + (3 if has_drop else 0)
    bwd_raw = getattr(torch.ops.mp, op._name + "_bwd_raw")

    def setup(ctx, inputs, output):
        weight, bias, slope, _eps, ctx.kind, ctx.param = inputs[i:i + 6]
        _, mean, invstd, _ = output
        ctx.mode, ctx.d_skip = (inputs[i + 6], inputs[1].size(1)) if has_skip else (None, None)
        ctx.drop = tuple(inputs[n_inputs - 3:]) if has_drop else ()
        ctx.has = (weight is not None, bias is not None, slope is not None)
        ctx.slope_shape = None if slope is None else slope.shape
        # x [, skip]: neither the output nor a mask is kept, the backward recomputes the pre-activation from x, the
        # statistics and the key; skip is kept where bn_skip_act keeps out, as an operand of that recomputation
        ctx.save_for_backward(*inputs[:i], weight, bias, slope, mean, invstd)

    def backward(ctx, dy, _dmean, _dinvstd, _dvar):
        x, *skip, w, b, s, mean, invstd = ctx.saved_tensors
        need = ctx.needs_input_grad
        need_x, need_skip, need_w, need_b = need[0], has_skip and need[1], need[i], need[i + 1]
        need_s = need[i + 2] and ctx.kind == ACT_PRELU
        dx = dgamma = dbeta = dskip = dslope = None
        none = ctx.kind == ACT_NONE                 # d(skip) is dy itself: nothing is launched for it
        if need_x or need_w or need_b or need_s or (need_skip and not none):
            if has_skip:
                dx, dgamma, dbeta, dskip, dslope = bwd_raw(dy, x, skip[0], w, b, s, mean, invstd, ctx.mode, ctx.kind,
                                                           ctx.param, *ctx.drop, need_skip, need_s)
            else:
                dx, dgamma, dbeta, dslope = bwd_raw(dy, x, w, b, s, mean, invstd, ctx.kind, ctx.param, *ctx.drop, need_s)
        if need_skip and none:
            dskip = dy if ctx.mode == SKIP_SUM else dy[:, :ctx.d_skip]
        grads = (dx if need_x else None,) + ((dskip if need_skip else None,) if has_skip else ()) + (
            dgamma if (need_w and ctx.has[0]) else None, dbeta if (need_b and ctx.has[1]) else None,
            dslope.reshape(ctx.slope_shape) if need_s else None)
        return grads + (None,) * (n_inputs - len(grads))

    op.register_autograd(backward, setup_context=setup)


def _cols32(t):
    """bn_fwd_raw's and bn_bwd_raw's older rule for x: fp32 with unit column stride, whatever the row stride"""
    return t if (t.dtype == torch.float32 and t.stride(-1) == 1) else t.float().contiguous()


@custom_op("mp::bn_fwd_raw", mutates_args=(), device_types="cuda")
def _op_bn_fwd_raw(x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], eps: float,
                   relu: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(y, mean, invstd, unbiased var) of BatchNorm1d over the node axis with batch statistics [+ ReLU]"""
    return _bn_fwd(_cols32, x, weight, bias, eps, relu=relu)


@custom_op("mp::bn_bwd_raw", mutates_args=(), device_types="cuda")
def _op_bn_bwd_raw(dy: Tensor, y: Optional[Tensor], x: Tensor, weight: Optional[Tensor], mean: Tensor,
                   invstd: Tensor, bias: Optional[Tensor] = None,
                   relu_from_x: bool = False) -> Tuple[Tensor, Tensor, Tensor]:
    """(dx, dgamma, dbeta); y given = the forward's ReLU output (its mask is applied to dy on the fly); relu_from_x:
    the mask is recomputed from x, weight, bias, mean, invstd instead (mp_bn_train_bwd_relu_f32: y is not read)"""
    x = _cols32(x)
    N, d = x.shape
    dy = dy.contiguous()
    dx, dgamma, dbeta = _bwd_results(dy, x, placed=True)
    w, b, _ = _params(weight, bias if relu_from_x else None)
    if relu_from_x:
        _bn_launch("mp_bn_train_bwd_relu_f32", "mp_bn_ws_bytes", x, ptr(dy), dy.stride(0), ptr(x), x.stride(0), N, d,
                   ptr(w), ptr(b), ptr(mean), ptr(invstd), ptr(dx), dx.stride(0), ptr(dgamma), ptr(dbeta))
    else:
        _bn_launch("mp_bn_train_bwd_f32", "mp_bn_ws_bytes", x, ptr(dy), dy.stride(0), ptr(y),
                   y.stride(0) if y is not None else 0, ptr(x), x.stride(0), N, d, ptr(w), ptr(mean), ptr(invstd),
                   ptr(dx), dx.stride(0), ptr(dgamma), ptr(dbeta))
    return dx, dgamma, dbeta


@custom_op("mp::bn_act", mutates_args=(), device_types="cuda")
def _op_bn_act(x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], eps: float,
               relu: bool) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """graphgym/models/layer.py:26-35 (BatchNorm1d, then the activation) in training mode: (y, mean, invstd, var)"""
    return torch.ops.mp.bn_fwd_raw(x, weight, bias, eps, relu)


def _bn_setup(ctx, inputs, output):
    x, weight, bias, eps, relu = inputs
    y, mean, invstd, _ = output
    ctx.relu = relu
    ctx.has_affine = (weight is not None, bias is not None)
    # the ReLU mask of the backward pass is recomputed from x (bit for bit the forward's): y is not kept for it
    ctx.save_for_backward(x, weight, mean, invstd, bias if relu else None)


def _bn_backward(ctx, dy, _dmean, _dinvstd, _dvar):
    x, w, mean, invstd, b = ctx.saved_tensors
    dx, dgamma, dbeta = torch.ops.mp.bn_bwd_raw(dy, None, x, w, mean, invstd, b, ctx.relu)
    return dx, (dgamma if ctx.has_affine[0] else None), (dbeta if ctx.has_affine[1] else None), None, None


register_autograd("mp::bn_act", _bn_backward, setup_context=_bn_setup)


# ---- the skip block of the skipsum / skipconcat stages (graphgym/models/gnn.py:30-60) ---------------------------------
# Behind a last layer built with has_act=False the block computes act(x + BN(h)) or act(cat(x, BN(h))).  As separate
# passes that is BN statistics, BN apply, add / cat, activation: 8 N d elements moved (8 N d + 4 N d_skip for cat); the
# engine's apply pass takes the skip operand and the activation along: 4 N d, or 3 N d + 2 N d_skip.
SKIP_SUM, SKIP_CONCAT = K["MP_BN_SKIP_SUM"], K["MP_BN_SKIP_CONCAT"]
_SKIP_MODES = {"sum": SKIP_SUM, "skipsum": SKIP_SUM, "concat": SKIP_CONCAT, "skipconcat": SKIP_CONCAT,
               SKIP_SUM: SKIP_SUM, SKIP_CONCAT: SKIP_CONCAT}


def _rows32(t):
    """fp32 rows with unit column stride and a row stride that covers them (a column slice stays a view)"""
    ok = t.dtype == torch.float32 and t.stride(-1) == 1 and t.stride(0) >= t.size(1)
    return t if ok else t.float().contiguous()


def _check_skip_shapes(x, skip, mode):
    if mode not in (SKIP_SUM, SKIP_CONCAT):
        raise ValueError(f"mode must be SKIP_SUM ({SKIP_SUM}) or SKIP_CONCAT ({SKIP_CONCAT}), got {mode}")
    if x.dim() != 2 or skip.dim() != 2 or skip.size(0) != x.size(0):
        raise ValueError(f"x and skip must be [N, d] and [N, d_skip], got {tuple(x.shape)} and {tuple(skip.shape)}")
    if mode == SKIP_SUM and skip.size(1) != x.size(1):
        raise ValueError(f"SKIP_SUM needs d_skip == d, got {skip.size(1)} and {x.size(1)}")


@custom_op("mp::bn_skip_fwd_raw", mutates_args=(), device_types="cuda")
def _op_bn_skip_fwd_raw(x: Tensor, skip: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], eps: float,
                        relu: bool, mode: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(out, mean, invstd, unbiased var): out = act(skip + BN(x)) [N, d] (SKIP_SUM) or [act(skip) | act(BN(x))]
    [N, d_skip + d] (SKIP_CONCAT), BN over the node axis with batch statistics; one launch sequence"""
    return _bn_fwd(_rows32, x, weight, bias, eps, relu=relu, skip=skip, mode=mode)


@custom_op("mp::bn_skip_bwd_raw", mutates_args=(), device_types="cuda")
def _op_bn_skip_bwd_raw(dy: Tensor, out: Optional[Tensor], x: Tensor, weight: Optional[Tensor], mean: Tensor,
                        invstd: Tensor, mode: int, want_dskip: bool = True) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(dx, dgamma, dbeta, dskip) of bn_skip_fwd_raw; out = the forward's result when it applied the ReLU, None when not.
    SKIP_SUM: the statistics pass writes dskip = dy * [out > 0] and the apply pass reads it back (7 N d elements moved).
    SKIP_CONCAT: mp_bn_train_bwd_f32 on the right-hand column views of dy and out; the left slab's mask is torch's.
    Without the ReLU d(skip) is dy (its left slab) itself, and without want_dskip nobody asks: dskip then comes back
    EMPTY (an operator cannot return a view of its input) and the caller takes dy."""
    x = _rows32(x)
    dy = _rows32(dy)
    N, d = x.shape
    d_skip = d if mode == SKIP_SUM else dy.size(1) - d
    if mode not in (SKIP_SUM, SKIP_CONCAT) or d_skip <= 0 or dy.size(0) != N or (out is not None and out.shape != dy.shape):
        raise ValueError(f"bn_skip_bwd_raw: dy {tuple(dy.shape)}, x {tuple(x.shape)}, mode {mode} do not fit")
    out = None if out is None else _rows32(out)
    dx, dgamma, dbeta = _bwd_results(dy, x, placed=True)
    dskip = torch.empty(0, dtype=torch.float32, device=x.device)
    w, _, _ = _params(weight, None)
    if mode == SKIP_SUM and out is not None and want_dskip:
        dskip = placement.empty_or_torch((N, d), x.device, reads=(dy, out), streaming=True)
        _bn_launch("mp_bn_train_bwd_skip_f32", "mp_bn_ws_bytes", x, ptr(dy), dy.stride(0), ptr(out), out.stride(0),
                   ptr(x), x.stride(0), N, d, ptr(w), ptr(mean), ptr(invstd), ptr(dx), dx.stride(0), ptr(dskip),
                   dskip.stride(0), ptr(dgamma), ptr(dbeta))
    else:
        dyr = dy if mode == SKIP_SUM else dy[:, d_skip:]
        yr = out if (out is None or mode == SKIP_SUM) else out[:, d_skip:]
        _bn_launch("mp_bn_train_bwd_f32", "mp_bn_ws_bytes", x, ptr(dyr), dyr.stride(0), ptr(yr),
                   yr.stride(0) if yr is not None else 0, ptr(x), x.stride(0), N, d, ptr(w), ptr(mean), ptr(invstd),
                   ptr(dx), dx.stride(0), ptr(dgamma), ptr(dbeta))
        if mode == SKIP_CONCAT and out is not None and want_dskip:
            dskip = _masked(dy[:, :d_skip], out[:, :d_skip])
    return dx, dgamma, dbeta, dskip


@_op_bn_skip_bwd_raw.register_fake
def _(dy, out, x, weight, mean, invstd, mode, want_dskip=True):
    d = x.size(1)
    n_skip = 0 if (out is None or not want_dskip) else (d if mode == SKIP_SUM else dy.size(1) - d)
    return (_new32(x, *x.shape), _new32(x, d), _new32(x, d), _new32(x, x.size(0), n_skip) if n_skip else _new32(x, 0))


def _masked(dy, out):
    """dy * [out > 0] as the kernels write it (a masked element is +0, whatever dy's sign)"""
    return torch.where(out > 0, dy, dy.new_zeros(()))


@custom_op("mp::bn_skip_act", mutates_args=(), device_types="cuda")
def _op_bn_skip_act(x: Tensor, skip: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], eps: float, relu: bool,
                    mode: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """graphgym/models/gnn.py:49-60 behind a last layer without activation, in training mode: act(skip + BN(x)) or
    act(cat(skip, BN(x))): (out, mean, invstd, var)"""
    return torch.ops.mp.bn_skip_fwd_raw(x, skip, weight, bias, eps, relu, mode)


def _bn_skip_setup(ctx, inputs, output):
    x, skip, weight, bias, eps, relu, mode = inputs
    out, mean, invstd, _ = output
    ctx.relu, ctx.mode, ctx.d_skip = relu, mode, skip.size(1)
    ctx.has_affine = (weight is not None, bias is not None)
    # skip is not kept: its gradient is the masked dy, and the mask is out's (kept only when there is one)
    ctx.save_for_backward(x, out if relu else None, weight, mean, invstd)


def _bn_skip_backward(ctx, dy, _dmean, _dinvstd, _dvar):
    x, out, w, mean, invstd = ctx.saved_tensors
    need_x, need_skip, need_w, need_b = ctx.needs_input_grad[:4]
    dx = dgamma = dbeta = dskip = None
    left = (lambda t: t) if ctx.mode == SKIP_SUM else (lambda t: t[:, :ctx.d_skip])
    if need_x or need_w or need_b:
        dx, dgamma, dbeta, g = torch.ops.mp.bn_skip_bwd_raw(dy, out, x, w, mean, invstd, ctx.mode, need_skip)
        if need_skip:
            dskip = left(dy) if out is None else g
    elif need_skip:             # no BatchNorm backward at all
        dskip = left(dy) if out is None else _masked(left(dy), left(out))
    return (dx if need_x else None, dskip, dgamma if (need_w and ctx.has_affine[0]) else None,
            dbeta if (need_b and ctx.has_affine[1]) else None, None, None, None)


register_autograd("mp::bn_skip_act", _bn_skip_backward, setup_context=_bn_skip_setup)


# ---- the same passes with any activation of cfg.gnn.act (graphgym/models/act.py:6-14) --------------------------------
# The unfused composition moves 5 N d elements forward (statistics, BN apply, activation) and 8 N d backward, and keeps
# x AND the BatchNorm's output for the backward; with the activation in the apply pass it is 3 N d and 5 N d, and x
# alone is kept: the backward recomputes the pre-activation from x (csrc/bn.hip, csrc/act.h).
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_PRELU, ACT_ELU, ACT_SELU, ACT_SILU = (
    K["MP_ACT_" + a] for a in "NONE RELU LRELU PRELU ELU SELU SILU".split())


def act_spec(module):
    """(kind, parameter) of an activation module the engine's BatchNorm passes can take along, None for any other:
    nn.ReLU, nn.SELU, nn.SiLU -> (kind, None); nn.LeakyReLU -> (ACT_LRELU, negative_slope); nn.ELU -> (ACT_ELU, alpha);
    nn.PReLU() with ONE slope -> (ACT_PRELU, its weight).  Exact types only: a subclass may compute anything."""
    t = type(module)
    if t is nn.ReLU:
        return ACT_RELU, None
    if t is nn.LeakyReLU:
        return ACT_LRELU, float(module.negative_slope)
    if t is nn.PReLU:
        return (ACT_PRELU, module.weight) if module.num_parameters == 1 else None
    if t is nn.ELU:
        return ACT_ELU, float(module.alpha)
    if t is nn.SELU:
        return ACT_SELU, None
    if t is nn.SiLU:
        return ACT_SILU, None
    return None


def _spec_args(spec):
    """(slope tensor or None, host parameter) of an act_spec result, as the ops take them"""
    kind, p = spec
    return (p if kind == ACT_PRELU else None), (float(p) if kind in (ACT_LRELU, ACT_ELU) else 0.0)


def _check_kind(kind, slope):
    if not ACT_NONE <= kind <= ACT_SILU:
        raise ValueError(f"unknown activation kind {kind}")
    if kind == ACT_PRELU and (slope is None or slope.numel() != 1):
        raise ValueError("ACT_PRELU takes a slope tensor of ONE element (nn.PReLU())")


def _slope32(slope, kind):
    """PRELU's slope as one fp32 element on the device (it is read there, never on the host); None for other kinds"""
    return slope.detach().reshape(1).float().contiguous() if kind == ACT_PRELU else None


@custom_op("mp::bn_actx_fwd_raw", mutates_args=(), device_types="cuda")
def _op_bn_actx_fwd_raw(x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], slope: Optional[Tensor],
                        eps: float, kind: int, param: float) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(y, mean, invstd, unbiased var): y = act(BatchNorm1d(x)) with batch statistics, act = the ACT_* kind"""
    return _bn_fwd(_rows32, x, weight, bias, eps, act=(kind, param, slope))


@custom_op("mp::bn_actx_bwd_raw", mutates_args=(), device_types="cuda")
def _op_bn_actx_bwd_raw(dy: Tensor, x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor],
                        slope: Optional[Tensor], mean: Tensor, invstd: Tensor, kind: int, param: float,
                        want_dslope: bool = True) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(dx, dgamma, dbeta, dslope) of bn_actx_fwd_raw.  The forward's output is not an operand: the pre-activation is
    recomputed from x, weight, bias, mean, invstd.  dslope: [1] for ACT_PRELU with want_dslope, EMPTY otherwise."""
    return _bn_actx_bwd(_rows32, dy, x, weight, bias, slope, mean, invstd, kind, param, want_dslope)


@custom_op("mp::bn_actx", mutates_args=(), device_types="cuda")
def _op_bn_actx(x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], slope: Optional[Tensor], eps: float,
                kind: int, param: float) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """graphgym/models/layer.py:26-35 (BatchNorm1d, then cfg.gnn.act) in training mode: (y, mean, invstd, var)"""
    return torch.ops.mp.bn_actx_fwd_raw(x, weight, bias, slope, eps, kind, param)


@custom_op("mp::bn_skip_actx_fwd_raw", mutates_args=(), device_types="cuda")
def _op_bn_skip_actx_fwd_raw(x: Tensor, skip: Tensor, weight: Optional[Tensor], bias: Optional[Tensor],
                             slope: Optional[Tensor], eps: float, kind: int, param: float,
                             mode: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """bn_skip_fwd_raw with the ACT_* kind in place of the ReLU switch"""
    return _bn_fwd(_rows32, x, weight, bias, eps, act=(kind, param, slope), skip=skip, mode=mode)


@custom_op("mp::bn_skip_actx_bwd_raw", mutates_args=(), device_types="cuda")
def _op_bn_skip_actx_bwd_raw(dy: Tensor, x: Tensor, skip: Tensor, weight: Optional[Tensor], bias: Optional[Tensor],
                             slope: Optional[Tensor], mean: Tensor, invstd: Tensor, mode: int, kind: int, param: float,
                             want_dskip: bool = True,
                             want_dslope: bool = True) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(dx, dgamma, dbeta, dskip, dslope) of bn_skip_actx_fwd_raw from x and skip, without the forward's output.
    SKIP_SUM: the statistics pass writes dskip = dy * act'(skip + BN(x)) and the apply pass reads it back; without
    want_dskip the apply pass recomputes it.  SKIP_CONCAT: dskip = dy[:, :d_skip] * act'(skip).  dskip comes back EMPTY
    without want_dskip and for ACT_NONE (d(skip) is dy itself: the caller takes it); dslope as in bn_actx_bwd_raw."""
    return _bn_actx_bwd(_rows32, dy, x, weight, bias, slope, mean, invstd, kind, param, want_dslope, skip=skip,
                        mode=mode, want_dskip=want_dskip)


@custom_op("mp::bn_skip_actx", mutates_args=(), device_types="cuda")
def _op_bn_skip_actx(x: Tensor, skip: Tensor, weight: Optional[Tensor], bias: Optional[Tensor],
                     slope: Optional[Tensor], eps: float, kind: int, param: float,
                     mode: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """graphgym/models/gnn.py:49-60 behind a last layer without activation, in training mode, with any cfg.gnn.act:
    act(skip + BN(x)) or act(cat(skip, BN(x))): (out, mean, invstd, var)"""
    return torch.ops.mp.bn_skip_actx_fwd_raw(x, skip, weight, bias, slope, eps, kind, param, mode)


# ---- gnn.dropout between the BatchNorm and the activation: a keyed mask (csrc/draws.h, csrc/bn_drop.hip) -------------
# The mask is a pure function of (seed, offset, row, column): nothing is stored, the backward recomputes it.  Its
# definition is the comment in csrc/draws.h; dropout_keep_host restates it in NumPy integers, bit for bit.
_M64 = (1 << 64) - 1
_GOLDEN = 0x9E3779B97F4A7C15
DROP_ONE = 65536                        # a rate is T / 65536


def dropout_threshold(p):
    """T = round(p * 65536) in [0, 65536]: an element is kept iff its 16-bit draw is >= T"""
    p = float(p)
    if not 0.0 <= p <= 1.0:
        raise ValueError(f"dropout probability has to be between 0 and 1, but got {p}")
    return int(p * DROP_ONE + 0.5)


def dropout_scale(p):
    """the fp32 factor of the kept elements, 1 / (1 - T / 65536) rounded once; 0 when everything is dropped"""
    T = dropout_threshold(p)
    return 0.0 if T == DROP_ONE else float(np.float32(65536.0 / (DROP_ONE - T)))


def _mix64(z):
    """draws.h mix64 on a uint64 array (wrapping arithmetic)"""
    with np.errstate(over="ignore"):
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def dropout_keep_host(seed, offset, N, d, p):
    """keep(seed, offset, r, c) of csrc/draws.h over an [N, d] operand on the host: bool tensor [N, d] on the CPU (NumPy
    integers, no device).  One hash per aligned group of four columns; column c takes its 16-bit lane c % 4."""
    T = dropout_threshold(p)
    g = np.uint64(_GOLDEN)
    q = (d + 3) // 4
    with np.errstate(over="ignore"):
        key = _mix64(np.asarray(int(seed) & _M64, dtype=np.uint64) + g)
        key = _mix64((key ^ np.uint64(int(offset) & _M64)) + g)
        group = (np.arange(N, dtype=np.uint64)[:, None] * np.uint64(q) + np.arange(q, dtype=np.uint64)[None, :])
        h = _mix64((key ^ group) + g)                                    # [N, q]
    lanes = (h[:, :, None] >> (np.uint64(16) * np.arange(4, dtype=np.uint64))) & np.uint64(0xFFFF)
    keep = lanes.reshape(N, 4 * q)[:, :d] >= np.uint64(T)
    return torch.from_numpy(np.ascontiguousarray(keep))


def _drop_args(T, seed, offset):
    if not 0 <= T <= DROP_ONE:
        raise ValueError(f"the dropout threshold must lie in [0, {DROP_ONE}], got {T}")
    return int(T), C.c_uint64(int(seed) & _M64), C.c_uint64(int(offset) & _M64)


@custom_op("mp::dropout_keyed", mutates_args=(), device_types="cuda")
def _op_dropout_keyed(x: Tensor, T: int, seed: int, offset: int) -> Tensor:
    """out = keep(seed, offset) * scale * x over an [N, d] fp32 view; kept iff the element's draw is >= T"""
    _require_hip(x, "x")
    if x.dim() != 2:
        raise ValueError(f"dropout_keyed takes [N, d], got {tuple(x.shape)}")
    T, seed_c, off_c = _drop_args(T, seed, offset)
    x = _rows32(x)
    N, d = x.shape
    out = placement.empty_or_torch((N, d), x.device, reads=(x,), streaming=True)
    if N == 0 or d == 0:
        return out
    with torch.cuda.device(x.device):
        check(lib().mp_dropout_keyed_f32(ptr(x), x.stride(0), N, d, T, seed_c, off_c, ptr(out), out.stride(0),
                                         _stream()), "mp_dropout_keyed_f32")
    return out


def _dropout_keyed_setup(ctx, inputs, output):
    _, ctx.T, ctx.seed, ctx.offset = inputs


def _dropout_keyed_backward(ctx, dy):
    # the same launch on dy: the mask is recomputed from the key
    return torch.ops.mp.dropout_keyed(dy, ctx.T, ctx.seed, ctx.offset), None, None, None


register_autograd("mp::dropout_keyed", _dropout_keyed_backward, setup_context=_dropout_keyed_setup)


@custom_op("mp::bn_drop_actx_fwd_raw", mutates_args=(), device_types="cuda")
def _op_bn_drop_actx_fwd_raw(x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], slope: Optional[Tensor],
                             eps: float, kind: int, param: float, T: int, seed: int,
                             offset: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(y, mean, invstd, unbiased var): y = act(keep * scale * BatchNorm1d(x)) with batch statistics"""
    return _bn_fwd(_rows32, x, weight, bias, eps, act=(kind, param, slope), drop=(T, seed, offset))


@custom_op("mp::bn_drop_actx_bwd_raw", mutates_args=(), device_types="cuda")
def _op_bn_drop_actx_bwd_raw(dy: Tensor, x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor],
                             slope: Optional[Tensor], mean: Tensor, invstd: Tensor, kind: int, param: float, T: int,
                             seed: int, offset: int,
                             want_dslope: bool = True) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(dx, dgamma, dbeta, dslope) of bn_drop_actx_fwd_raw.  Neither the forward's output nor a mask is an operand: the
    masked pre-activation is recomputed from x, the statistics and the key.  dslope as in bn_actx_bwd_raw."""
    return _bn_actx_bwd(_rows32, dy, x, weight, bias, slope, mean, invstd, kind, param, want_dslope,
                        drop=(T, seed, offset))


@custom_op("mp::bn_drop_actx", mutates_args=(), device_types="cuda")
def _op_bn_drop_actx(x: Tensor, weight: Optional[Tensor], bias: Optional[Tensor], slope: Optional[Tensor], eps: float,
                     kind: int, param: float, T: int, seed: int,
                     offset: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """graphgym/models/layer.py:26-35 (BatchNorm1d, Dropout, cfg.gnn.act) in training mode with the keyed mask of
    (T, seed, offset): (y, mean, invstd, var)"""
    return torch.ops.mp.bn_drop_actx_fwd_raw(x, weight, bias, slope, eps, kind, param, T, seed, offset)


@custom_op("mp::bn_drop_skip_actx_fwd_raw", mutates_args=(), device_types="cuda")
def _op_bn_drop_skip_actx_fwd_raw(x: Tensor, skip: Tensor, weight: Optional[Tensor], bias: Optional[Tensor],
                                  slope: Optional[Tensor], eps: float, kind: int, param: float, mode: int, T: int,
                                  seed: int, offset: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """bn_skip_actx_fwd_raw with the keyed mask on the BatchNorm term, before the skip operand"""
    return _bn_fwd(_rows32, x, weight, bias, eps, act=(kind, param, slope), skip=skip, mode=mode,
                   drop=(T, seed, offset))


@custom_op("mp::bn_drop_skip_actx_bwd_raw", mutates_args=(), device_types="cuda")
def _op_bn_drop_skip_actx_bwd_raw(dy: Tensor, x: Tensor, skip: Tensor, weight: Optional[Tensor],
                                  bias: Optional[Tensor], slope: Optional[Tensor], mean: Tensor, invstd: Tensor,
                                  mode: int, kind: int, param: float, T: int, seed: int, offset: int,
                                  want_dskip: bool = True,
                                  want_dslope: bool = True) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """(dx, dgamma, dbeta, dskip, dslope) of bn_drop_skip_actx_fwd_raw from x, skip and the key.  dskip = dy * act'(.) is
    NOT masked; the gradient into the BatchNorm is.  dskip and dslope come back EMPTY as in bn_skip_actx_bwd_raw."""
    return _bn_actx_bwd(_rows32, dy, x, weight, bias, slope, mean, invstd, kind, param, want_dslope, skip=skip,
                        mode=mode, want_dskip=want_dskip, drop=(T, seed, offset))


@custom_op("mp::bn_drop_skip_actx", mutates_args=(), device_types="cuda")
def _op_bn_drop_skip_actx(x: Tensor, skip: Tensor, weight: Optional[Tensor], bias: Optional[Tensor],
                          slope: Optional[Tensor], eps: float, kind: int, param: float, mode: int, T: int, seed: int,
                          offset: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """graphgym/models/gnn.py:49-60 behind a last layer [BatchNorm1d, Dropout] in training mode:
    act(skip + drop(BN(x))) or act(cat(skip, drop(BN(x)))): (out, mean, invstd, var)"""
    return torch.ops.mp.bn_drop_skip_actx_fwd_raw(x, skip, weight, bias, slope, eps, kind, param, mode, T, seed, offset)


# the fake kernels, one explicit line per signature (a differentiable op has its forward's), and the shared autograd
for _op in (_op_bn_fwd_raw, _op_bn_act):
    _op.register_fake(lambda x, weight, bias, eps, relu: _fwd_results(x))
for _op in (_op_bn_skip_fwd_raw, _op_bn_skip_act):
    _op.register_fake(lambda x, skip, weight, bias, eps, relu, mode: _fwd_results(x, skip, mode))
for _op in (_op_bn_actx_fwd_raw, _op_bn_actx):
    _op.register_fake(lambda x, weight, bias, slope, eps, kind, param: _fwd_results(x))
for _op in (_op_bn_skip_actx_fwd_raw, _op_bn_skip_actx):
    _op.register_fake(lambda x, skip, weight, bias, slope, eps, kind, param, mode: _fwd_results(x, skip, mode))
for _op in (_op_bn_drop_actx_fwd_raw, _op_bn_drop_actx):
    _op.register_fake(lambda x, weight, bias, slope, eps, kind, param, T, seed, offset: _fwd_results(x))
for _op in (_op_bn_drop_skip_actx_fwd_raw, _op_bn_drop_skip_actx):
    _op.register_fake(lambda x, skip, weight, bias, slope, eps, kind, param, mode, T, seed, offset:
                      _fwd_results(x, skip, mode))
_op_dropout_keyed.register_fake(lambda x, T, seed, offset: _new32(x, *x.shape))
_op_bn_bwd_raw.register_fake(lambda dy, y, x, weight, mean, invstd, bias=None, relu_from_x=False: _bwd_results(dy, x))
_op_bn_actx_bwd_raw.register_fake(lambda dy, x, weight, bias, slope, mean, invstd, kind, param, want_dslope=True:
                                  _bwd_results(dy, x, kind, want_dslope))
_op_bn_drop_actx_bwd_raw.register_fake(
    lambda dy, x, weight, bias, slope, mean, invstd, kind, param, T, seed, offset, want_dslope=True:
    _bwd_results(dy, x, kind, want_dslope))
_op_bn_skip_actx_bwd_raw.register_fake(
    lambda dy, x, skip, weight, bias, slope, mean, invstd, mode, kind, param, want_dskip=True, want_dslope=True:
    _bwd_results(dy, x, kind, want_dslope, skip, want_dskip))
_op_bn_drop_skip_actx_bwd_raw.register_fake(
    lambda dy, x, skip, weight, bias, slope, mean, invstd, mode, kind, param, T, seed, offset, want_dskip=True,
    want_dslope=True: _bwd_results(dy, x, kind, want_dslope, skip, want_dskip))
_actx_autograd(_op_bn_actx, has_skip=False, has_drop=False)
_actx_autograd(_op_bn_skip_actx, has_skip=True, has_drop=False)
_actx_autograd(_op_bn_drop_actx, has_skip=False, has_drop=True)
_actx_autograd(_op_bn_drop_skip_actx, has_skip=True, has_drop=True)


# ---- softmax cross-entropy over the labelled rows (graphgym/loss.py:53-68, 20-37) -------------------------------
def _check_ce_shapes(z, y, idx):
    """host-side shape contract (no device read): one label per selected row.  Label VALUES are checked on the device:
    a label outside [0, C) or an index outside the logit matrix is never dereferenced and turns the loss into NaN."""
    if z.dim() != 2:
        raise ValueError(f"logits must be [n_rows, C], got {tuple(z.shape)}")
    if idx is not None and idx.numel() != y.numel():
        raise ValueError(f"index selects {idx.numel()} rows but there are {y.numel()} labels")
    if idx is None and y.numel() > z.size(0):
        raise ValueError(f"{y.numel()} labels for {z.size(0)} rows of logits")


@custom_op("mp::softmax_ce_rows_raw", mutates_args=(), device_types="cuda")
def _op_ce_rows_raw(logits: Tensor, labels: Tensor, index: Optional[Tensor]) -> Tensor:
    _require_hip(logits, "logits")
    z = logits if (logits.dtype == torch.float32 and logits.stride(-1) == 1) else logits.float().contiguous()
    y = labels.to(torch.int64).contiguous()
    idx = None if index is None else index.to(torch.int64).contiguous()
    n_sel = y.numel()
    _check_ce_shapes(z, y, idx)
    out = torch.empty(n_sel, dtype=torch.float32, device=z.device)
    with torch.cuda.device(z.device):
        check(lib().mp_softmax_ce_rows_f32(ptr(z), z.stride(0), z.size(0), ptr(y), ptr(idx), n_sel, z.size(1), ptr(out),
                                           _stream()), "mp_softmax_ce_rows_f32")
    return out


@_op_ce_rows_raw.register_fake
def _(logits, labels, index):
    return logits.new_empty((labels.numel(),), dtype=torch.float32)


@custom_op("mp::softmax_ce_bwd_raw", mutates_args=(), device_types="cuda")
def _op_ce_bwd_raw(logits: Tensor, labels: Tensor, index: Optional[Tensor], gscale: Tensor, inv_n: float) -> Tensor:
    z = logits if (logits.dtype == torch.float32 and logits.stride(-1) == 1) else logits.float().contiguous()
    y = labels.to(torch.int64).contiguous()
    idx = None if index is None else index.to(torch.int64).contiguous()
    g = gscale.to(torch.float32).reshape(1).contiguous()
    _check_ce_shapes(z, y, idx)
    if idx is not None and ops.deterministic():
        # the per-selected-row gradients [n_sel, C] by the kernel's non-accumulating form on the gathered rows (a row
        # with an invalid label or index stays zero), then summed per logit row over the index's inverted list on the
        # aggregation kernel: no float atomics, a row listed several times gets its terms in list order
        n, n_sel = z.size(0), y.numel()
        ok = (idx >= 0) & (idx < n)
        zs = z.index_select(0, torch.where(ok, idx, torch.zeros_like(idx)))
        ys = torch.where(ok, y, torch.full_like(y, -1))
        ds = torch.zeros((n_sel, z.size(1)), dtype=torch.float32, device=z.device)
        with torch.cuda.device(z.device):
            check(lib().mp_softmax_ce_bwd_f32(ptr(zs), zs.stride(0), n_sel, ptr(ys), None, n_sel, z.size(1), ptr(g),
                                              float(inv_n), ptr(ds), ds.stride(0), _stream()), "mp_softmax_ce_bwd_f32")
        return ops._sum_rows_by_ids(idx, n, ds, clamp=True)
    # with an index the rows accumulate onto zeros (a row listed twice gets both terms); without one every row of the
    # first n_sel is written once and the rest must still be zero
    d = torch.zeros_like(z) if (idx is not None or y.numel() < z.size(0)) else torch.empty_like(z)
    with torch.cuda.device(z.device):
        check(lib().mp_softmax_ce_bwd_f32(ptr(z), z.stride(0), z.size(0), ptr(y), ptr(idx), y.numel(), z.size(1), ptr(g),
                                          float(inv_n), ptr(d), d.stride(0), _stream()), "mp_softmax_ce_bwd_f32")
    return d


@_op_ce_bwd_raw.register_fake
def _(logits, labels, index, gscale, inv_n):
    return logits.new_empty(logits.shape, dtype=torch.float32)


@custom_op("mp::softmax_ce", mutates_args=(), device_types="cuda")
def _op_softmax_ce(logits: Tensor, labels: Tensor, index: Optional[Tensor]) -> Tensor:
    """mean over the labelled rows of softmax cross-entropy(logits[index], labels): one pass forward, one backward"""
    return torch.ops.mp.softmax_ce_rows_raw(logits, labels, index).mean()


@_op_softmax_ce.register_fake
def _(logits, labels, index):
    return logits.new_empty((), dtype=torch.float32)


def _ce_setup(ctx, inputs, output):
    logits, labels, index = inputs
    ctx.save_for_backward(logits, labels, index)


def _ce_backward(ctx, g):
    logits, labels, index = ctx.saved_tensors
    n = max(labels.numel(), 1)
    return torch.ops.mp.softmax_ce_bwd_raw(logits, labels, index, g, 1.0 / n), None, None


register_autograd("mp::softmax_ce", _ce_backward, setup_context=_ce_setup)


def softmax_cross_entropy(logits, labels, index=None):
    """F.cross_entropy(logits[index], labels, reduction='mean') on the engine (no gather copy, one pass each way);
    small problems stay with torch"""
    if (not logits.is_cuda or logits.dim() != 2 or labels.numel() * logits.size(1) < (1 << 20)
            or logits.dtype != torch.float32):
        sel = logits if index is None else logits[index]
        return F.cross_entropy(sel, labels, reduction="mean")
    return torch.ops.mp.softmax_ce(logits, labels, index)


def _update_running_stats(bn, mean, var_u):
    """torch.nn.BatchNorm1d's training-mode bookkeeping from the batch mean and unbiased variance"""
    if bn.training and bn.track_running_stats:
        with torch.no_grad():
            bn.num_batches_tracked += 1
            m = bn.momentum if bn.momentum is not None else 1.0 / float(bn.num_batches_tracked)
            bn.running_mean.mul_(1 - m).add_(mean, alpha=m)
            bn.running_var.mul_(1 - m).add_(var_u, alpha=m)


class BatchNorm1d(nn.BatchNorm1d):
    """``nn.BatchNorm1d`` whose training-mode forward / backward run on the engine; ``relu=True`` fuses the
    activation that follows it in GraphGym's layer wrapper.  Eval mode uses the running statistics (torch)."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, relu=False):
        super().__init__(num_features, eps=eps, momentum=momentum, affine=affine,
                         track_running_stats=track_running_stats)
        self.relu = relu

    def forward(self, x):
        if x.dim() != 2:
            raise ValueError("expected [num_nodes, num_features]")
        if not _batch_stats_on_engine(self, x):
            y = super().forward(x)
            return torch.relu(y) if self.relu else y
        y, mean, _, var_u = torch.ops.mp.bn_act(x, self.weight, self.bias, float(self.eps), bool(self.relu))
        _update_running_stats(self, mean, var_u)
        return y

    def extra_repr(self):
        return super().extra_repr() + f", relu={self.relu}"


def _batch_stats_on_engine(bn, x):
    """the rule of every engine pass: batch statistics over a device tensor [N > 1, d] that is not bf16 (bf16: torch)"""
    return ((bn.training or not bn.track_running_stats) and x.dim() == 2 and x.is_cuda and x.size(0) > 1
            and x.dtype != torch.bfloat16)


def _bn_on_engine(bn, x):
    """BatchNorm1d.forward's rule for the fused passes, and a BatchNorm that carries no fused ReLU of its own"""
    return isinstance(bn, nn.BatchNorm1d) and not getattr(bn, "relu", False) and _batch_stats_on_engine(bn, x)


class Dropout(nn.Dropout):
    """``nn.Dropout`` over [N, d] node features with the KEYED mask of csrc/draws.h: the mask of a training-mode call is a
    pure function of ``(seed, step)`` and the element's row and column, the same on the device (mp::dropout_keyed, or
    fused behind a BatchNorm by bn_act_module / bn_skip_act), on the CPU (dropout_keep_host) and in the backward, which
    recomputes it: no mask is stored.

    ``seed`` is a Python int, drawn at construction from torch's default CPU generator unless given: torch.manual_seed
    fixes a model's masks and every layer has its own.  ``step`` is a host counter that advances by one on every
    training-mode forward; ``set_stream(seed, step)`` sets both.  ``p`` is quantised to T / 65536 (``p_effective``).
    The numbers are not torch's Philox stream.  ``inplace`` is kept for nn.Dropout's signature (cfg.mem.inplace); a
    training-mode call always returns a new tensor.  Limits: a captured HIP graph replays the ONE mask of its capture (seed
    and step are host integers baked into the launch), and a torch.utils.checkpoint recomputation advances the counter,
    so it draws a different mask than the forward it repeats."""

    def __init__(self, p=0.5, inplace=False, seed=None):
        super().__init__(p=p, inplace=inplace)
        self.T = dropout_threshold(p)
        self.seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if seed is None else int(seed)
        self.step = 0

    @property
    def p_effective(self):
        return self.T / DROP_ONE

    def set_stream(self, seed, step=0):
        self.seed, self.step = int(seed), int(step)

    def active(self):
        """a training-mode call draws a mask (and takes a counter value)"""
        return self.training and self.T > 0

    def take_step(self):
        """the counter value of this call; the next call gets the next one"""
        step = self.step
        self.step += 1
        return step

    def forward(self, x):
        if not self.active():
            return x
        step = self.take_step()
        if x.dim() != 2:
            raise ValueError("graphgym_amd.nn.Dropout expects [num_nodes, num_features]")
        if x.is_cuda:
            out = torch.ops.mp.dropout_keyed(x, self.T, self.seed, step)
            return out if x.dtype == torch.float32 else out.to(x.dtype)
        keep = dropout_keep_host(self.seed, step, x.size(0), x.size(1), self.p)
        return x * keep.to(x.dtype) * dropout_scale(self.p)

    def extra_repr(self):
        return super().extra_repr() + f", keyed, p_effective={self.p_effective:.6g}"


def _drop_fused(drop):
    """bn_act_module / bn_skip_act's rule for taking `drop` into the BatchNorm pass: the keyed module, drawing a mask"""
    return isinstance(drop, Dropout) and drop.active()


def bn_act_module(bn, x, act, drop=None):
    """``act(bn(x))`` — GraphGym's post-layer (graphgym/models/layer.py:26-35) — for an activation MODULE `act`, or
    ``act(drop(bn(x)))`` with a dropout module between them (`act` None: no activation, only with `drop`).  When act_spec
    knows the activation and BatchNorm1d.forward's rule holds, this is one engine op: mp::bn_actx — the activation rides
    the BatchNorm's apply pass, the backward recomputes it from x, and a PReLU slope receives its gradient from the same
    passes — or, with a graphgym_amd.nn.Dropout in training mode, mp::bn_drop_actx, which also draws the keyed mask in
    those passes and takes the ONE counter value the module's own forward would have taken.  Everything else — eval
    mode, CPU tensors, bf16, a single row, a subclass, per-channel PReLU, a user module, torch's nn.Dropout — is the
    torch composition.  `bn`'s running statistics are updated as its own forward would."""
    spec = (ACT_NONE, None) if act is None else act_spec(act)
    if spec is None or not _bn_on_engine(bn, x) or (drop is not None and not _drop_fused(drop)) or \
            (drop is None and act is None):
        y = bn(x)
        y = y if drop is None else drop(y)
        return y if act is None else act(y)
    slope, param = _spec_args(spec)
    if drop is None:
        y, mean, _, var_u = torch.ops.mp.bn_actx(x, bn.weight, bn.bias, slope, float(bn.eps), spec[0], param)
    else:
        y, mean, _, var_u = torch.ops.mp.bn_drop_actx(x, bn.weight, bn.bias, slope, float(bn.eps), spec[0], param,
                                                      drop.T, drop.seed, drop.take_step())
    _update_running_stats(bn, mean, var_u)
    return y


def bn_skip_act(bn, x, skip, mode, relu=True, act=None, drop=None):
    """The tail of GraphGym's skip block (graphgym/models/gnn.py:49-60) around its last layer's BatchNorm:
    ``act(skip + bn(x))`` for mode "skipsum" / SKIP_SUM, ``act(cat((skip, bn(x)), 1))`` for "skipconcat" / SKIP_CONCAT,
    with act = ReLU (``relu=True``), nothing (``relu=False``) or an activation module / callable ``act``.

    `bn` is a ``torch.nn.BatchNorm1d`` or this module's BatchNorm1d; its parameters are used and its running statistics
    updated exactly as its own forward would.  With batch statistics on fp32 device tensors this is one engine op:
    mp::bn_skip_act for ReLU or no activation (``act=None``), mp::bn_skip_actx for an ``act`` module that act_spec
    knows (statistics, then one pass that normalises, adds or places the skip operand and activates); everything
    else — eval mode with running statistics, CPU tensors, bf16, a single row, an activation without a spec, a
    BatchNorm that carries its own fused ReLU — is the torch composition, the rule of BatchNorm1d.forward.

    `drop`: the dropout module of the block's last layer, which the reference applies to ``bn(x)`` before the skip
    operand (graphgym/models/layer.py:26-35 inside gnn.py:49-60): ``act(skip + drop(bn(x)))``.  A graphgym_amd.nn.Dropout
    in training mode rides the same pass (mp::bn_drop_skip_actx) and takes one counter value, as in bn_act_module; any
    other dropout module is the composition."""
    mode = _SKIP_MODES[mode]
    _check_skip_shapes(x, skip, mode)
    spec = None if act is None else act_spec(act)
    if not ((act is None or spec is not None) and _bn_on_engine(bn, x) and skip.is_cuda
            and skip.dtype != torch.bfloat16 and (drop is None or _drop_fused(drop))):
        y = bn(x)
        y = y if drop is None else drop(y)
        z = skip + y if mode == SKIP_SUM else torch.cat((skip, y), 1)
        return act(z) if act is not None else (torch.relu(z) if relu else z)
    if drop is not None:
        if spec is None:
            spec = (ACT_RELU if relu else ACT_NONE, None)
        slope, param = _spec_args(spec)
        out, mean, _, var_u = torch.ops.mp.bn_drop_skip_actx(x, skip, bn.weight, bn.bias, slope, float(bn.eps), spec[0],
                                                             param, mode, drop.T, drop.seed, drop.take_step())
    elif spec is None:
        out, mean, _, var_u = torch.ops.mp.bn_skip_act(x, skip, bn.weight, bn.bias, float(bn.eps), bool(relu), mode)
    else:
        slope, param = _spec_args(spec)
        out, mean, _, var_u = torch.ops.mp.bn_skip_actx(x, skip, bn.weight, bn.bias, slope, float(bn.eps), spec[0],
                                                        param, mode)
    _update_running_stats(bn, mean, var_u)
    return out


class _NarrowHead(torch.autograd.Function):
    """y = x W^T + b for a narrow output (a classifier head, <= 16 classes) over many rows: the products with a
    [N, <= 16] side are the library's (they stream at the HBM rate), the weight gradient x^T g is the engine's
    narrow-output kernel (mp_dense_wgrad_f32: 10 GB at the HBM rate; the library's split-K GEMM takes 7.2 ms for it at
    10^7 x 256 x 10) with the bias gradient out of the same pass"""
    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return F.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, g):
        from . import ops
        x, weight = ctx.saved_tensors
        g = g.contiguous()
        dx = torch.mm(g, weight) if ctx.needs_input_grad[0] else None
        dW, db = ops._wgrad_and_bias(x, g, ctx.needs_input_grad[1], ctx.has_bias and ctx.needs_input_grad[2])
        return dx, (None if dW is None else dW.t()), db


def linear(x, weight, bias=None, relu=False):
    """act(x W^T + b) by Linear's dispatch, on any weight [out, in] — a parameter or a view of one (the column halves of
    the edge head's first layer, harness.GNNEdgeHead._concat_pairs)"""
    from . import ops
    out_features, in_features = weight.shape
    # the engine's kernels pay off on wide outputs over many rows (scripts/linear_bench.py: forward + backward
    # 39.8 vs 45.0 ms at 10^7 x 256 -> 256, 18.6 vs 27.8 ms at 1 -> 256; the library wins at 256 -> 10 and on
    # small batches), so narrow heads and small inputs stay on the library
    if (x.dim() == 2 and x.is_cuda and x.dtype == torch.float32 and out_features <= 16 and not relu
            and in_features % 4 == 0 and x.size(0) >= (1 << 17) and x.stride(1) == 1 and x.stride(0) % 4 == 0
            and x.data_ptr() % 16 == 0 and torch.is_grad_enabled()):
        return _NarrowHead.apply(x, weight, bias)
    if (x.dim() != 2 or not x.is_cuda or x.dtype != torch.float32 or out_features < 32
            or x.size(0) * out_features < (1 << 23)):
        y = F.linear(x, weight, bias)
        return torch.relu(y) if relu else y
    return ops.dense_fused(x, weight.t(), bias=bias, relu=relu)


class Linear(nn.Linear):
    """torch.nn.Linear (same parameters, same state dict) whose forward is the engine's transform kernel with bias
    and an optional ReLU fused into the store — the keras Dense(d, relu) / Dense(d) of the TF path's MLPs
    (main_zd.py:181-186,214-225) and GraphGym's Linear -> ReLU -> Linear (idconv.py:432-435).  Backward: the weight
    and bias gradients come from the engine's split-K kernel, g W' from the streaming transform with W^T (the library GEMM
    outside its shapes)."""

    def __init__(self, in_features, out_features, bias=True, relu=False):
        super().__init__(in_features, out_features, bias=bias)
        self.relu = bool(relu)

    def forward(self, x):
        return linear(x, self.weight, self.bias, self.relu)

    def extra_repr(self):
        return super().extra_repr() + (", relu=True" if self.relu else "")
