"""GraphGym's B-spline layer on the engine: graphgym/models/layer.py

    SplineConvLayer                         pyg.nn.SplineConv(dim_in, dim_out, dim=1, kernel_size=2, bias=bias), layer.py:180
    SplineConv           'splineconv'       layer.py:177-186

The reference calls the layer as model(node_feature, edge_index, edge_feature): edge_feature [E, 1] holds one
pseudo-coordinate u in [0, 1] per edge.  With those constructor arguments (an open spline of degree 1 over K = 2 kernel
matrices W0, W1, mean aggregation, a root weight and a bias) the layer is

    out_i = mean_{e = (j -> i)} [ b0(u_e) x_j W[k0(u_e)] + b1(u_e) x_j W[k1(u_e)] ] + x_i root + bias
    v = u (kernel_size - degree) = u,  f = v - floor(v),  b0 = 1 - f,  k0 = floor(v) mod 2,  b1 = f,  k1 = (floor(v) + 1) mod 2

over the stored in-edges of i (every copy of a multi-edge counts; a node without in-edges gets x_i root + bias; no self
loops, no normalisation).  A message is therefore c0_e x_j W0 + c1_e x_j W1 with two scalars per edge (c0 collects the b
whose k is 0: (1 - u, u) on [0, 1) and (0, 1) at u = 1), and the layer two weighted neighbour sums of the same rows of x:

    aggregate first   [P0 | P1] = ops.spline_agg(g, w, x) — one gather per entry, two sums per row — then one transform
                      of the message sums, [P0 | P1] weight.view(2 in, out) with weight as it is stored, + x root + bias;
    transform first   z = x [W0 | W1], then ops.spline_fold(g, w, z) — two half rows per entry, one sum — + x root + bias

with w[e] = (c0, c1) / count(row of e) in entry order, cached on the graph per edge_feature.  'auto' gathers the fewer
bytes per entry: in floats against 2 out.

[3P-unverified] Parameter names, shapes and initialisation restate torch_geometric.nn.SplineConv from memory — PyG is
not vendored with the reference, which pins no version: weight [K, in, out], root [in, out], bias [out] are the names
of the PyG releases of the reference's era (so a reference checkpoint's model.weight / model.root / model.bias load);
later releases keep the root weight as lin.weight [out, in], which _load_from_state_dict accepts.  All three are drawn
from U(-b, b) with b = 1 / sqrt(in K), the era's `uniform(size, tensor)` with size = in_channels * K.

Not built: the gradient with respect to edge_feature (data in the reference; a tensor that requires grad is refused),
other dim / kernel_size / degree values, bfloat16.
"""
import math

import torch
import torch.nn as nn
from torch.nn import Parameter

from . import ops
from .graph import tensor_stamp
from .layers import _CachedEdgesMixin

_WHERE = "layer.py:180 builds pyg.nn.SplineConv(dim_in, dim_out, dim=1, kernel_size=2, bias=bias)"


def spline_entry_weights(u):
    """(c0, c1) [E, 2] of the pseudo-coordinates u [E] or [E, 1]: the open degree-1 basis over two kernel matrices,
    b0 = 1 - f at k0 = floor(v) mod 2 and b1 = f at k1 = (floor(v) + 1) mod 2, summed per matrix.  Elementwise, with a
    non-negative mod: whatever u holds, a k is 0 or 1 (or matches neither).  [0, 1] is the contract, as it is PyG's."""
    v = u.reshape(-1)                  # v = u * (kernel_size - degree) = u
    fl = torch.floor(v)
    f = v - fl
    b0, b1 = 1.0 - f, f
    k0, k1 = torch.remainder(fl, 2.0), torch.remainder(fl + 1.0, 2.0)
    zero = torch.zeros_like(v)
    c0 = torch.where(k0 == 0, b0, zero) + torch.where(k1 == 0, b1, zero)
    c1 = torch.where(k0 == 1, b0, zero) + torch.where(k1 == 1, b1, zero)
    return torch.stack([c0, c1], dim=1)


def _entry_weights(g, edge_feature):
    """w [nnz, 2] = spline_entry_weights(u)[eid] / count(row): the mean folded into the entry's two weights, in g's entry
    order; cached on g for the last edge_feature (graph.tensor_stamp)"""
    stamp = tensor_stamp(edge_feature)
    hit = g.__dict__.get("_spline_w")
    if hit is None or hit[0] != stamp:
        with torch.no_grad():
            c = spline_entry_weights(edge_feature.detach())
            w = c[g.eid.long()] / g.entry_counts()[g.row_ids().long()][:, None]
        hit = (stamp, edge_feature, w.contiguous())         # holding edge_feature keeps its address unique
        g.__dict__["_spline_w"] = hit
    return hit[2]


class SplineConvLayer(nn.Module, _CachedEdgesMixin):
    """pyg.nn.SplineConv(in_channels, out_channels, dim=1, kernel_size=2, bias=bias) (layer.py:180)"""

    def __init__(self, in_channels, out_channels, dim=1, kernel_size=2, bias=True, order="auto", **kwargs):
        super().__init__()
        if dim != 1 or kernel_size != 2:
            raise ValueError("SplineConvLayer serves dim=1, kernel_size=2 only ({}), got dim={}, kernel_size={}".format(
                _WHERE, dim, kernel_size))
        if order not in ("auto", "aggregate_first", "transform_first"):
            raise ValueError("order must be 'auto', 'aggregate_first' or 'transform_first', got {!r}".format(order))
        self.in_channels, self.out_channels = in_channels, out_channels
        self.dim, self.kernel_size, self.order = dim, kernel_size, order
        self.cached = False
        self.weight = Parameter(torch.Tensor(kernel_size, in_channels, out_channels))
        self.root = Parameter(torch.Tensor(in_channels, out_channels))
        if bias:
            self.bias = Parameter(torch.Tensor(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        b = 1.0 / math.sqrt(self.in_channels * self.kernel_size)
        for p in (self.weight, self.root, self.bias):
            if p is not None:
                p.data.uniform_(-b, b)
        self.cached_result = None
        self.cached_num_edges = None

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        lin = prefix + "lin.weight"            # later PyG releases: the root weight is a Linear, [out, in]
        if lin in state_dict and prefix + "root" not in state_dict:
            state_dict[prefix + "root"] = state_dict.pop(lin).t()
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)

    def _order(self):
        if self.order != "auto":
            return self.order
        # gathered floats per entry: in (one row of x) against 2 out (two half rows of z)
        return "aggregate_first" if self.in_channels <= 2 * self.out_channels else "transform_first"

    def forward(self, x, edge_index, edge_feature=None, holder=None):
        if edge_feature is None or edge_feature.dim() != 2 or edge_feature.size(1) != 1:
            raise ValueError("SplineConvLayer needs edge_feature [E, 1], one pseudo-coordinate per edge ({}), got {}".format(
                _WHERE, None if edge_feature is None else tuple(edge_feature.shape)))
        if x.dtype != torch.float32 or edge_feature.dtype != torch.float32:
            raise TypeError("the layer splineconv is float32 only (got x {} / edge_feature {}): run it in float32".format(
                x.dtype, edge_feature.dtype))
        if edge_feature.requires_grad and torch.is_grad_enabled():
            raise ValueError("SplineConvLayer has no gradient with respect to edge_feature (data in the reference, "
                             "layer.py:183-186): detach it")
        if edge_feature.size(0) != edge_index.size(1):
            raise ValueError("edge_feature has {} rows, edge_index {} edges".format(edge_feature.size(0),
                                                                                   edge_index.size(1)))
        g = self._graph(holder, edge_index, x.size(0), None, loops="none")
        w = _entry_weights(g, edge_feature)
        if self._order() == "aggregate_first":
            # the two sums are the halves of one row: they meet the kernel matrices stacked as they are stored.  (The
            # root term is a transform of its own: the two products of one mp_dense_fused_f32 share one inner width.)
            msg = ops.dense_fused(ops.spline_agg(g, w, x), self.weight.view(2 * self.in_channels, self.out_channels))
            return msg + ops.dense_fused(x, self.root, bias=self.bias)
        z = ops.dense_fused(x, torch.cat([self.weight[0], self.weight[1]], dim=1))
        return ops.spline_fold(g, w, z) + ops.dense_fused(x, self.root, bias=self.bias)

    def __repr__(self):
        return '{}({}, {}, dim={})'.format(self.__class__.__name__, self.in_channels, self.out_channels, self.dim)


class SplineConv(nn.Module):          # layer.py:177-186
    def __init__(self, dim_in, dim_out, bias=False, **kwargs):
        super().__init__()
        self.model = SplineConvLayer(dim_in, dim_out, dim=1, kernel_size=2, bias=bias)

    def forward(self, batch):
        batch.node_feature = self.model(batch.node_feature, batch.edge_index, batch.edge_feature, holder=batch)
        return batch
