"""The max backward in pull form over include/mp_maxbwd.h (csrc/spmm.hip: MaxBwdRows): the launchers and
the registered operators `torch.ops.mp.spmm_max_bwd_pull_raw` and `torch.ops.mp.spmm_heads_max_bwd_pull_raw`, which
ops._grad_by_source and ops._heads_grad_by_source select under ops.deterministic().  A module of its own beside ops.py,
as the header is a file of its own beside mp_engine.h."""
import torch
from torch.library import custom_op

from . import _lib, _lib_maxbwd
from ._lib import check, ptr
from .graph import _stream, from_handle
from .ops import HEADS_ONE_LAUNCH, _agg_in, _f32c, _op_rows, _plan_ws

Tensor = torch.Tensor


def _raw_max_bwd_pull(g, dy, argmax, w_t=None, heads=1, out=None):
    """the max backward in pull form (mp_spmm_max_bwd_pull_f32 / _bf16 / mp_spmm_heads_max_bwd_pull_f32): dy, argmax
    [N, d] by destination -> dx [num_cols, d] of dy's dtype, every element written once.  The transposed pattern, its
    pos and its plan come from g._transpose_sorted() — also for a graph flagged symmetric, whose transpose() is the
    graph itself and has no pos — and are cached there, as the permuted values are: a second backward on the batch
    builds nothing.  w_t: the weights in transposed order, [nnz] (default: the transposed graph's own values) or
    [nnz, heads]."""
    gt = g._transpose_sorted()
    d = dy.size(1)
    dx = out if out is not None else torch.empty((gt.num_nodes, d), dtype=dy.dtype, device=dy.device)
    if g.nnz == 0 or gt.num_nodes == 0:      # no entry won anything
        return dx.zero_()
    if w_t is None:
        w_t = gt.val
    plan, counts, ws, ws_bytes = _plan_ws(gt, dy.device, d, _lib.SUM, False)
    head = (ptr(gt.rowptr), ptr(gt.col), ptr(gt.pos), ptr(w_t))
    tail = (gt.num_nodes, gt.nnz, ptr(plan), counts, ptr(argmax), argmax.stride(0), ptr(dy), dy.stride(0), d, ptr(dx),
            dx.stride(0), ptr(ws), ws_bytes, _stream())
    with torch.cuda.device(dy.device):
        if heads > 1:
            st = _lib_maxbwd.lib().mp_spmm_heads_max_bwd_pull_f32(*head, heads, *tail)
            if st == 2:       # a head layout the one launch does not take
                return None
            check(st, "mp_spmm_heads_max_bwd_pull_f32")
            return dx
        name = "mp_spmm_max_bwd_pull_bf16" if dy.dtype == torch.bfloat16 else "mp_spmm_max_bwd_pull_f32"
        check(getattr(_lib_maxbwd.lib(), name)(*head, *tail), name)
    return dx


def _max_bwd_checked(g, dy, argmax):
    dy = _agg_in(dy, "dy")
    if argmax.dtype != torch.int32 or argmax.shape != dy.shape or argmax.stride(1) != 1 or dy.size(0) != g.num_nodes:
        raise ValueError(f"dy {tuple(dy.shape)} and argmax {tuple(argmax.shape)} ({argmax.dtype}) must both be "
                         f"[{g.num_nodes}, d], argmax int32 with unit-stride rows")
    return dy


@custom_op("mp::spmm_max_bwd_pull_raw", mutates_args=(), device_types="cuda")
def _op_spmm_max_bwd_pull_raw(dy: Tensor, argmax: Tensor, graph: int) -> Tensor:
    g = from_handle(graph)
    return _raw_max_bwd_pull(g, _max_bwd_checked(g, dy, argmax), argmax)


def _raw_heads_max_bwd_pull(g, dy, argmax, w, heads):
    """dV[j, slice h] = sum over the entries e of source j that won a column c of head h of w[e, h] dy[row_e, c]: one
    launch for 1, 2, 4 or 8 heads, per head on column slices otherwise (the ladder of _raw_heads_agg)"""
    dy = _f32c(_max_bwd_checked(g, dy, argmax), "dy")
    d = dy.size(1)
    if heads < 1 or d % heads or w.numel() != g.nnz * heads:
        raise ValueError(f"w has {w.numel()} elements and dy {d} columns: not [nnz = {g.nnz}, heads = {heads}]")
    gt = g._transpose_sorted()
    w_t = _f32c(w.reshape(g.nnz, heads), "w")[gt.pos.long()].contiguous()      # the weights in transposed order
    if heads == 1:
        return _raw_max_bwd_pull(g, dy, argmax, w_t.view(-1))
    dV = torch.empty((gt.num_nodes, d), dtype=torch.float32, device=dy.device)
    if g.nnz == 0 or gt.num_nodes == 0:
        return dV.zero_()
    if heads in HEADS_ONE_LAUNCH and _raw_max_bwd_pull(g, dy, argmax, w_t, heads, out=dV) is not None:
        return dV
    dh = d // heads
    for h in range(heads):
        cs = slice(h * dh, (h + 1) * dh)
        _raw_max_bwd_pull(g, dy[:, cs], argmax[:, cs], w_t[:, h].contiguous(), out=dV[:, cs])
    return dV


@custom_op("mp::spmm_heads_max_bwd_pull_raw", mutates_args=(), device_types="cuda")
def _op_spmm_heads_max_bwd_pull_raw(dy: Tensor, argmax: Tensor, w: Tensor, graph: int, heads: int) -> Tensor:
    return _raw_heads_max_bwd_pull(from_handle(graph), dy, argmax, w, heads)


_op_spmm_max_bwd_pull_raw.register_fake(lambda dy, argmax, graph: dy.new_empty((_op_rows(graph, 1), dy.size(1))))
_op_spmm_heads_max_bwd_pull_raw.register_fake(lambda dy, argmax, w, graph, heads:
                                              dy.new_empty((_op_rows(graph, 1), dy.size(1)), dtype=torch.float32))
