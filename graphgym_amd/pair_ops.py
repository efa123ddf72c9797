"""The pair decoders of the link-prediction head (graphgym/models/head.py:62-85) over include/mp_pair.h:
`torch.ops.mp.pair_score` (dot product or cosine similarity of K listed pairs of rows of h) and `torch.ops.mp.pair_sum`
(the first Linear of the concat decoding, distributed over the two halves of the concatenation).  Neither gathers a
[K, d] tensor in either direction: the forward reads 2K rows and writes K scores (or K rows of the MLP's width), the
backward is one aggregation over the inverted index of the pair list (`PairIndex`: row v lists the pairs node v belongs
to) on the plan-based kernel of ops._raw_spmm, hub rows split by the plan.  No float atomics: the same bits every run.
`graphgym_amd.ops` exposes the wrappers as `ops.pair_score` / `ops.pair_sum`; they are registered here, as spline_ops.py
registers its two.  fp32 only; not differentiable in `index`; no double backward."""
import collections
from typing import Optional, Tuple

import torch
from torch.library import custom_op, register_autograd

from . import _lib, _lib_pair
from ._lib import check, ptr
from .graph import CSRGraph, _require_hip, _stream, tensor_stamp
from .ops import _raw_spmm

Tensor = torch.Tensor

_PAIR_KEY = "edge head"
# Two entries: the batch in flight and the one a loader builds ahead.  An entry pins its index, a CSR of 2K entries, the
# plan and (concat) two role operators; with negatives resampled every step older ones are never asked for again.
_CACHE_SIZE = 2
_cache = collections.OrderedDict()      # (tensor_stamp(index), num_nodes) -> PairIndex


def _f32_only(op, **operands):
    for name, t in operands.items():
        if isinstance(t, torch.Tensor) and t.dtype != torch.float32:
            raise TypeError(f"{op} is float32 only: {name} is {t.dtype} (the {_PAIR_KEY} has no bfloat16 or float16 form)")


def _pair_f32(t, name, op):
    """an operand of a pair op: float32 (the head has no bfloat16 or float16 form), on the device, 2-D, rows unit-stride"""
    _f32_only(op, **{name: t})
    _require_hip(t, name)
    if t.dim() != 2:
        raise ValueError(f"{op}: {name} is {tuple(t.shape)}, not [rows, width]")
    return t if t.stride(1) == 1 else t.contiguous()


def _shape_of_pairs(index, op):
    if not isinstance(index, torch.Tensor) or index.dim() != 2 or index.size(0) != 2 or index.dtype != torch.int64:
        raise ValueError(f"{op}: index must be an int64 [2, K] tensor, got "
                         f"{getattr(index, 'dtype', type(index))} {tuple(getattr(index, 'shape', ()))}")
    if index.size(1) > 1 and index.stride(1) != 1:
        raise ValueError(f"{op}: the rows of index must have unit stride, got strides {tuple(index.stride())}")


def _pair_rows(index, op):
    """the two rows of a pair list, checked: [2, K] int64 on the device, each row unit-stride (any slice of a longer
    [2, K'] tensor is); nothing is copied and nothing is read"""
    _shape_of_pairs(index, op)
    _require_hip(index, "index")
    return index[0], index[1]


class PairIndex:
    """The inverted index of a pair list index [2, K] over num_nodes nodes: `graph`, a CSR with num_nodes rows and 2K
    entries (CSRGraph.from_edge_index of cat([index, index.flip(0)], 1)).  Row v holds the other endpoint of every pair v
    belongs to; graph.eid gives the pair (eid mod K) and the role (eid < K: v is index[1, k]; eid >= K: v is
    index[0, k]).  A pair (v, v) has two entries in row v, a duplicated pair stays duplicated.  Built with validation: an
    id outside [0, num_nodes) raises ValueError.  The plan and the longest row are built with it, so a backward pass
    through a prebuilt PairIndex reads nothing on the host.  `index` is held: its address stays its own while the entry
    lives (graph.tensor_stamp)."""

    def __init__(self, index, num_nodes):
        _pair_rows(index, "pair_index")
        self.index = index
        self.stamp = tensor_stamp(index)
        self.num_nodes = int(num_nodes)
        self.K = int(index.size(1))
        self.graph = None
        self._roles = None
        if self.K:
            g = CSRGraph.from_edge_index(torch.cat([index, index.flip(0)], 1), self.num_nodes)
            g.plan()
            g.max_row_entries()
            self.graph = g

    def matches(self, index, num_nodes):
        return self.num_nodes == int(num_nodes) and self.stamp == tensor_stamp(index)

    def role_operators(self):
        """(P_a, P_b): the rectangular operators [num_nodes x K] with one entry (index[0, k], k), (index[1, k], k) per
        pair — rows = nodes, columns = pair ids, as pooling.pool_operator builds its operator; dU = P_a dz, dV = P_b dz"""
        if self._roles is None:
            ids = torch.arange(self.K, device=self.index.device)
            ops_ = []
            for role in (0, 1):
                g = CSRGraph.from_edge_index(torch.stack([ids, self.index[role]]), self.num_nodes, num_cols=self.K)
                g.plan()
                g.max_row_entries()
                ops_.append(g)
            self._roles = tuple(ops_)
        return self._roles


def adopt(pi):
    """make a PairIndex built elsewhere (a loader's side stream: batch.pair_index) the one the ops find for its tensor"""
    key = (pi.stamp, pi.num_nodes)
    _cache[key] = pi
    _cache.move_to_end(key)
    while len(_cache) > _CACHE_SIZE:
        _cache.popitem(last=False)
    return pi


def pair_index(index, num_nodes):
    """the PairIndex of `index`, kept under graph.tensor_stamp(index) (the last _CACHE_SIZE pair lists)"""
    pi = _cache.get((tensor_stamp(index), int(num_nodes)))
    if pi is None:
        pi = PairIndex(index, num_nodes)
    return adopt(pi)


# ---- launchers ------------------------------------------------------------------------------------------------------
def _raw_rnorm(h, eps, want_q=False):
    """r [N] = 1 / max(||h_v||, eps) and, want_q, q [N] = 1 / ||h_v|| (0 for a zero row) (mp_pair_rnorm_f32)"""
    r = torch.empty(h.size(0), dtype=torch.float32, device=h.device)
    q = torch.empty(h.size(0), dtype=torch.float32, device=h.device) if want_q else None
    with torch.cuda.device(h.device):
        check(_lib_pair.lib().mp_pair_rnorm_f32(ptr(h), h.stride(0), h.size(0), h.size(1), float(eps), ptr(r), ptr(q),
                                                _stream()), "mp_pair_rnorm_f32")
    return (r, q) if want_q else r


def _raw_pair_score(h, index, r=None):
    """(score [K], bad [1] int32) of mp_pair_score_f32: the dot products, times r[a] r[b] when r is given; bad counts the
    pairs with an id outside [0, N), whose scores are NaN.  Nothing is read on the host."""
    a, b = index[0], index[1]
    K = a.numel()
    score = torch.empty(K, dtype=torch.float32, device=h.device)
    bad = torch.zeros(1, dtype=torch.int32, device=h.device)
    with torch.cuda.device(h.device):
        check(_lib_pair.lib().mp_pair_score_f32(ptr(h), h.stride(0), h.size(0), h.size(1), ptr(a), ptr(b), K, ptr(r),
                                                ptr(score), ptr(bad), _stream()), "mp_pair_score_f32")
    return score, bad


def _raw_pair_sum(U, V, index, bias=None):
    """(z [K, m], bad [1] int32) of mp_pair_sum_f32: z[k] = U[a_k] + V[b_k] + bias; a bad pair's row is NaN"""
    a, b = index[0], index[1]
    K, m = a.numel(), U.size(1)
    z = torch.empty((K, m), dtype=torch.float32, device=U.device)
    bad = torch.zeros(1, dtype=torch.int32, device=U.device)
    with torch.cuda.device(U.device):
        check(_lib_pair.lib().mp_pair_sum_f32(ptr(U), U.stride(0), ptr(V), V.stride(0), U.size(0), m, ptr(a), ptr(b), K,
                                              ptr(bias), ptr(z), z.stride(0), ptr(bad), _stream()), "mp_pair_sum_f32")
    return z, bad


def _raw_bwd_weights(pi, g, score=None, r=None, q=None):
    """(w [2K], diag [N] or None) of mp_pair_bwd_weights_f32 over pi.graph: the entry values of A_w and, with score, r
    and q (cosine), the diagonal term"""
    a, b = pi.index[0], pi.index[1]
    G = pi.graph
    w = torch.empty(G.nnz, dtype=torch.float32, device=g.device)
    diag = torch.empty(pi.num_nodes, dtype=torch.float32, device=g.device) if r is not None else None
    with torch.cuda.device(g.device):
        check(_lib_pair.lib().mp_pair_bwd_weights_f32(ptr(G.rowptr), ptr(G.eid), pi.num_nodes, pi.K, ptr(g),
                                                      ptr(score if r is not None else None), ptr(r), ptr(q), ptr(a),
                                                      ptr(b), ptr(w), ptr(diag), _stream()), "mp_pair_bwd_weights_f32")
    return w, diag


def _score_operands(h, index, cosine, eps):
    """(h with unit-stride rows, eps) of a pair_score call, checked once, in the op: the types, the index's shape and
    eps before the places, so that a CPU caller hears what is wrong with the call before where it must run"""
    _f32_only("pair_score", h=h)
    _shape_of_pairs(index, "pair_score")
    if cosine and not eps > 0.0:
        raise ValueError(f"pair_score: the cosine similarity clamps each norm at eps > 0, got {eps}")
    _require_hip(index, "index")
    return _pair_f32(h, "h", "pair_score"), float(eps)


def _on_device(*tensors):
    return all(isinstance(t, torch.Tensor) and t.is_cuda for t in tensors if t is not None)


# ---- torch.ops.mp.pair_score ----------------------------------------------------------------------------------------
@custom_op("mp::pair_score", mutates_args=(), device_types="cuda")
def _op_pair_score(h: Tensor, index: Tensor, cosine: bool, eps: float) -> Tensor:
    h, eps = _score_operands(h, index, cosine, eps)
    r = _raw_rnorm(h, eps) if cosine and h.size(0) and index.size(1) else None
    return _raw_pair_score(h, index, r)[0]


@custom_op("mp::pair_score_bwd_raw", mutates_args=(), device_types="cuda")
def _op_pair_score_bwd_raw(g: Tensor, h: Tensor, index: Tensor, score: Optional[Tensor], cosine: bool, eps: float) -> Tensor:
    """dh = A_w h (+ diag (.) h): A_w the PairIndex of `index` with the values of mp_pair_bwd_weights_f32"""
    h, eps = _score_operands(h, index, cosine, eps)
    pi = pair_index(index, h.size(0))          # validates when it has to build: ValueError for an id out of range
    if pi.K == 0 or h.size(0) == 0:
        return h.new_zeros((h.size(0), h.size(1)))
    g = g.contiguous()
    r, q = _raw_rnorm(h, eps, want_q=True) if cosine else (None, None)
    w, diag = _raw_bwd_weights(pi, g, score, r, q)
    dh, _ = _raw_spmm(pi.graph.with_values(w), h, _lib.SUM)
    if diag is not None:
        dh.addcmul_(diag.unsqueeze(1), h)
    return dh


def _pair_score_setup(ctx, inputs, output):
    h, index, cosine, eps = inputs
    ctx.set_materialize_grads(False)
    ctx.cosine, ctx.eps = cosine, eps
    ctx.save_for_backward(h, index, output if cosine else None)


def _pair_score_backward(ctx, g):
    h, index, score = ctx.saved_tensors
    if g is None or not ctx.needs_input_grad[0]:
        return None, None, None, None
    return torch.ops.mp.pair_score_bwd_raw(g, h, index, score, ctx.cosine, ctx.eps), None, None, None


register_autograd("mp::pair_score", _pair_score_backward, setup_context=_pair_score_setup)


# ---- torch.ops.mp.pair_sum ------------------------------------------------------------------------------------------
def _pair_sum_operands(U, V, index, bias):
    """(U, V, bias) of a pair_sum call, checked once, in the op (the types and the index's shape before the places)"""
    _f32_only("pair_sum", U=U, V=V, bias=bias)
    _shape_of_pairs(index, "pair_sum")
    _require_hip(index, "index")
    U, V = _pair_f32(U, "U", "pair_sum"), _pair_f32(V, "V", "pair_sum")
    if U.shape != V.shape or U.size(1) < 1:
        raise ValueError(f"pair_sum: U is {tuple(U.shape)} and V is {tuple(V.shape)}: one row per node, one width")
    if bias is not None:
        _require_hip(bias, "bias")
        if tuple(bias.shape) != (U.size(1),):
            raise ValueError(f"pair_sum: bias is {tuple(bias.shape)}, the rows are {U.size(1)} wide")
        bias = bias.contiguous()
    return U, V, bias


@custom_op("mp::pair_sum", mutates_args=(), device_types="cuda")
def _op_pair_sum(U: Tensor, V: Tensor, index: Tensor, bias: Optional[Tensor]) -> Tensor:
    U, V, bias = _pair_sum_operands(U, V, index, bias)
    return _raw_pair_sum(U, V, index, bias)[0]


@custom_op("mp::pair_sum_bwd_raw", mutates_args=(), device_types="cuda")
def _op_pair_sum_bwd_raw(dz: Tensor, index: Tensor, num_nodes: int, want: int) -> Tuple[Tensor, Tensor]:
    """(dU, dV) = (P_a dz, P_b dz) over the role operators of the PairIndex; bit i of `want` clear: EMPTY"""
    dz = _pair_f32(dz, "dz", "pair_sum")
    pi = pair_index(index, num_nodes)
    out = []
    for role in (0, 1):
        if not want >> role & 1:
            out.append(dz.new_empty((0,)))
        elif pi.K == 0:
            out.append(dz.new_zeros((num_nodes, dz.size(1))))
        else:
            out.append(_raw_spmm(pi.role_operators()[role], dz, _lib.SUM)[0])
    return out[0], out[1]


def _pair_sum_setup(ctx, inputs, output):
    U, V, index, bias = inputs
    ctx.set_materialize_grads(False)
    ctx.num_nodes = U.size(0)
    ctx.save_for_backward(index)


def _pair_sum_backward(ctx, dz):
    (index,) = ctx.saved_tensors
    need_u, need_v, _, need_b = ctx.needs_input_grad
    if dz is None or not (need_u or need_v or need_b):
        return None, None, None, None
    dU = dV = None
    if need_u or need_v:
        want = (1 if need_u else 0) | (2 if need_v else 0)
        dU, dV = torch.ops.mp.pair_sum_bwd_raw(dz, index, ctx.num_nodes, want)
    return (dU if need_u else None), (dV if need_v else None), None, (dz.sum(0) if need_b else None)


register_autograd("mp::pair_sum", _pair_sum_backward, setup_context=_pair_sum_setup)


# ---- the wrappers ---------------------------------------------------------------------------------------------------
def _adopt_if_matching(pi, index, num_nodes):
    if pi is not None and isinstance(pi, PairIndex) and pi.matches(index, num_nodes):
        adopt(pi)


def pair_score(h, index, cosine=False, eps=1e-8, pair_index=None):
    """score[k] = <h[a_k], h[b_k]>, or their cosine similarity under F.cosine_similarity's rule (each norm clamped at eps
    on its own), for the pairs (a_k, b_k) = index[:, k]   ([K]; torch.ops.mp.pair_score)

    h: any 2-D float32 view with unit column stride; index: any int64 [2, K] tensor whose rows have unit stride, read as
    it lies.  The forward reads nothing on the host: a pair with an id outside [0, N) is not dereferenced and scores NaN.
    The gradient flows to h as one aggregation over the PairIndex of `index` (built on the first backward pass and kept
    under graph.tensor_stamp(index), or handed in as `pair_index` and used when its stamp matches); building it raises
    ValueError for an id out of range.  Nothing of size K x d is saved or made."""
    if not _on_device(h, index):              # the op is a device op: say what is wrong before the dispatcher does
        _score_operands(h, index, cosine, eps)
    _adopt_if_matching(pair_index, index, h.size(0))
    return torch.ops.mp.pair_score(h, index, bool(cosine), float(eps))


def pair_sum(U, V, index, bias=None, pair_index=None):
    """z[k] = U[a_k] + V[b_k] + bias   ([K, m]; torch.ops.mp.pair_sum)

    The first Linear of the concat decoding after cat(h[a], h[b]) W^T = (h W[:, :d]^T)[a] + (h W[:, d:]^T)[b].  float32
    only.  The gradients are dU = P_a dz, dV = P_b dz over the role operators of the PairIndex (ops.spmm's kernel) and
    dbias = dz.sum(0)."""
    if not _on_device(U, V, index, bias):
        _pair_sum_operands(U, V, index, bias)
    _adopt_if_matching(pair_index, index, U.size(0))
    return torch.ops.mp.pair_sum(U, V, index, bias)


_op_pair_score.register_fake(lambda h, index, cosine, eps: h.new_empty((index.size(1),)))
_op_pair_score_bwd_raw.register_fake(lambda g, h, index, score, cosine, eps: h.new_empty((h.size(0), h.size(1))))
_op_pair_sum.register_fake(lambda U, V, index, bias: U.new_empty((index.size(1), U.size(1))))
_op_pair_sum_bwd_raw.register_fake(lambda dz, index, num_nodes, want: (
    dz.new_empty((num_nodes, dz.size(1)) if want & 1 else (0,)), dz.new_empty((num_nodes, dz.size(1)) if want & 2 else (0,))))
