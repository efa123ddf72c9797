"""The operators of the B-spline layer (graphgym/models/layer.py:177-186) over include/mp_spline.h: `torch.ops.mp.spline_agg`
and `torch.ops.mp.spline_fold`, each other's adjoint.  `graphgym_amd.ops` exposes them as `ops.spline_agg` /
`ops.spline_fold` beside the other aggregation operators; they are registered here, on that module's shared pieces
(the plan workspace, the placement of outputs, the graph handle and setup_context), as `graphgym_amd.nn` registers the
step operators in a module of its own.  fp32 only; differentiable in the gathered operand, not in the weights."""
import torch
from torch.library import custom_op, register_autograd

from . import _lib, _lib_spline, placement
from ._lib import check, ptr
from .graph import _require_hip, _stream, from_handle, tensor_stamp
from .ops import _agg_of_nothing, _graph_setup, _op_rows, _plan_ws

Tensor = torch.Tensor

_SPLINE_KEY = "key splineconv"


def _spline_variant(g, w, transposed):
    """(operator, its per-entry weights) of a spline op: g and w, or the transposed pattern with w in ITS entry order,
    w[t.pos] — what g.transpose_with does for one value per entry; kept on g for the last w (graph.tensor_stamp)"""
    if not transposed:
        return g, w
    t = g._transpose_sorted()
    stamp = tensor_stamp(w)
    hit = g.__dict__.get("_spline_wt")
    if hit is None or hit[0] != stamp:
        hit = (stamp, w, w.index_select(0, t.pos.long()))      # holding w keeps its address unique
        g.__dict__["_spline_wt"] = hit
    return t, hit[2]


def _spline_f32(t, name, op):
    """an operand of a spline op: on the device, float32 (the layer has no bfloat16 or float16 form), rows unit-stride"""
    _require_hip(t, name)
    if t.dtype != torch.float32:
        raise TypeError(f"{op} is float32 only: {name} is {t.dtype} (the {_SPLINE_KEY} has no bfloat16 or float16 form)")
    return t if t.dim() == 2 and t.stride(1) == 1 else t.contiguous()


def _spline_operands(graph, w, x, op, transposed):
    """(operator, w [nnz, 2] dense in its entry order, x) of a spline op, checked: float32, two weights per entry of the
    graph, x one row per column of the operator (spline_fold: of two halves)"""
    g = from_handle(graph)
    xn = "x" if op == "spline_agg" else "z"
    x, w = _spline_f32(x, xn, op), _spline_f32(w, "w", op)
    if tuple(w.shape) != (g.nnz, 2):
        raise ValueError(f"{op}: w is {tuple(w.shape)}, the operator has {g.nnz} entries with two weights each")
    g, w = _spline_variant(g, w, transposed)
    if x.dim() != 2 or x.size(0) != g.num_cols or x.size(1) < 1 or (op == "spline_fold" and x.size(1) % 2):
        raise ValueError(f"{op}: {xn} is {tuple(x.shape)}: the operator has {g.num_cols} columns"
                         + (" and a row of z holds two halves" if op == "spline_fold" else ""))
    return g, w.contiguous(), x


def _raw_spline(g, w, x, fold, out=None):
    """one launch of mp_spline_agg_f32 (x [n, d] -> [N, 2d]: the halves are the sums under w[:, 0] and w[:, 1]) or, fold,
    of mp_spline_fold_f32 (x [n, 2d] -> [N, d]) (+ the hub launches of the plan); w [nnz, 2] in g's entry order"""
    L = _lib_spline.lib()
    N = g.num_nodes
    d = x.size(1) // 2 if fold else x.size(1)
    width = d if fold else 2 * d
    if g.nnz == 0:          # no entry: col and w have no address; every row is empty
        return _agg_of_nothing(N, width, x, out=out)[0]
    y = out if out is not None else placement.empty_or_torch((N, width), x.device, reads=(x,))
    plan, counts, ws, ws_bytes = _plan_ws(g, x.device, d, _lib.SUM, not fold)
    name = "mp_spline_fold_f32" if fold else "mp_spline_agg_f32"
    with torch.cuda.device(x.device):
        check(getattr(L, name)(ptr(g.rowptr), ptr(g.col), ptr(w), N, ptr(plan), counts, ptr(x), x.stride(0), ptr(y),
                               y.stride(0), d, ptr(ws), ws_bytes, _stream()), name)
    return y


@custom_op("mp::spline_agg", mutates_args=(), device_types="cuda")
def _op_spline_agg(w: Tensor, x: Tensor, graph: int, transposed: bool) -> Tensor:
    g, w, x = _spline_operands(graph, w, x, "spline_agg", transposed)
    return _raw_spline(g, w, x, False)


@custom_op("mp::spline_fold", mutates_args=(), device_types="cuda")
def _op_spline_fold(w: Tensor, z: Tensor, graph: int, transposed: bool) -> Tensor:
    g, w, z = _spline_operands(graph, w, z, "spline_fold", transposed)
    return _raw_spline(g, w, z, True)


def _spline_setup(ctx, inputs, output):
    w, _, graph, transposed = inputs
    _graph_setup(ctx, graph)
    ctx.transposed = transposed
    ctx.save_for_backward(w)


def _spline_backward_of(adjoint):
    def backward(ctx, dy):
        (w,) = ctx.saved_tensors
        if dy is None or not ctx.needs_input_grad[1]:
            return None, None, None, None
        # the adjoint kernel on the other orientation of the same pattern, w in that orientation's entry order
        return None, adjoint(w, dy, ctx.graph, not ctx.transposed), None, None
    return backward


register_autograd("mp::spline_agg", _spline_backward_of(torch.ops.mp.spline_fold), setup_context=_spline_setup)
register_autograd("mp::spline_fold", _spline_backward_of(torch.ops.mp.spline_agg), setup_context=_spline_setup)


def _spline_checked(op, w, x):
    _spline_f32(w, "w", op), _spline_f32(x, "x" if op == "spline_agg" else "z", op)
    if w.requires_grad and torch.is_grad_enabled():
        raise ValueError(f"{op} is not differentiable in w: the spline weights come from edge_feature, which is data in "
                         "the reference (layer.py:183-186); detach it")


def spline_agg(g, w, x):
    """P[i] = [ sum_{e = (i <- j)} w[e, 0] x[j] | sum_e w[e, 1] x[j] ]   ([N, 2d]; torch.ops.mp.spline_agg)

    The aggregation of SplineConv(dim=1, kernel_size=2) in the aggregate-first order (layer.py:177-186): every row of x an
    entry names is gathered ONCE and meets the entry's two weights in registers (mp_spline_agg_f32); P @ [W0; W1] is the
    layer's message sum.  w [nnz, 2] in g's entry order (the entry values of g take no part; fold a mean into w).
    float32 only; the gradient flows to x (spline_fold on the transposed pattern), not to w.  No float atomics."""
    _spline_checked("spline_agg", w, x)
    return torch.ops.mp.spline_agg(w, x, g.handle, False)


def spline_fold(g, w, z):
    """y[i] = sum_{e = (i <- j)} ( w[e, 0] z[j, :d] + w[e, 1] z[j, d:] )   ([N, d]; torch.ops.mp.spline_fold)

    The transform-first order of the same layer with z = x @ [W0 | W1], and the adjoint of spline_agg: two half rows
    gathered from one index, one sum (mp_spline_fold_f32).  float32 only; the gradient flows to z (spline_agg on the
    transposed pattern), not to w.  No float atomics."""
    _spline_checked("spline_fold", w, z)
    return torch.ops.mp.spline_fold(w, z, g.handle, False)


_op_spline_agg.register_fake(lambda w, x, graph, transposed:
                             x.new_empty((_op_rows(graph, 1 if transposed else 0), 2 * x.size(1))))
_op_spline_fold.register_fake(lambda w, z, graph, transposed:
                              z.new_empty((_op_rows(graph, 1 if transposed else 0), z.size(1) // 2)))
