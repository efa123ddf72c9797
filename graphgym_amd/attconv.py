"""GraphGym's attention layers of the design space on the engine: graphgym/contrib/layer/attconv.py

    GeneralAddAttConvLayer   'gaddconv'   attconv.py:14-111    additive attention, cfg.gnn.att_heads heads
    GeneralMulAttConvLayer   'gmulconv'   attconv.py:115-216   dot-product attention, one head

Both are the reference's MessagePassing layers with aggr = cfg.gnn.agg ('add', 'mean' or 'max'): the message of entry
(i <- j) is norm_ij * alpha_ij^h * x_j (attconv.py:93-104, :196-205), x = linear_msg(x).  Here the coefficients come
from the engine's attention kernels (ops.gat_alpha; ops.sddmm_dot + ops.edge_softmax) and the weighted aggregation with
its reduction from ops.spmm_edge_values.  Constructor, parameter names and shapes follow the reference, so state dicts
interchange.  float32 only.
"""
import math

import torch
import torch.nn as nn
from torch.nn import Parameter

from . import nn as mpnn
from . import ops
from .config import cfg
from .layers import _BatchLayer, _CachedEdgesMixin, glorot, zeros

_AGG = {"add": "sum", "sum": "sum", "mean": "mean", "max": "max"}


def _no_bf16(x):
    if x.dtype == torch.bfloat16:
        raise TypeError("the attention layers gaddconv and gmulconv do not support bfloat16: run them in float32")


class _AttConvBase(nn.Module, _CachedEdgesMixin):
    """what the two reference layers share (attconv.py:17-44, :65-89 and :118-189)"""

    def __init__(self, in_channels, out_channels, improved=False, cached=False, bias=True, **kwargs):
        super().__init__()
        self.heads = int(cfg.gnn.att_heads)
        if self.heads < 1 or out_channels % self.heads:
            raise ValueError("{}: dim_out = {} is not a multiple of cfg.gnn.att_heads = {} (the reference's per-head "
                             "view fails there too)".format(type(self).__name__, out_channels, self.heads))
        if cfg.gnn.agg not in _AGG:
            raise ValueError("cfg.gnn.agg must be one of 'add', 'mean', 'max', got {!r}".format(cfg.gnn.agg))
        self.in_channels = int(in_channels // self.heads * self.heads)
        self.out_channels = int(out_channels // self.heads * self.heads)
        self.improved, self.cached = improved, cached
        self.normalize = cfg.gnn.normalize_adj
        self.agg = cfg.gnn.agg
        self.negative_slope = 0.2
        self.head_channels = out_channels // self.heads
        self.linear_msg = mpnn.Linear(in_channels, out_channels, bias=False)

    def _reset_cache(self):
        self.cached_result = None
        self.cached_num_edges = None

    def forward(self, x, edge_index, edge_weight=None, holder=None):
        _no_bf16(x)
        if self.normalize:
            # GCN normalisation with remaining self loops, as GeneralConvLayer builds it (attconv.py:52-64)
            g = self._graph(holder, edge_index, x.size(0), edge_weight, loops="remaining", norm="col",
                            fill=2.0 if self.improved else 1.0)
        else:
            g = self._graph(holder, edge_index, x.size(0), edge_weight, loops="none")
        h = self.linear_msg(x)
        alpha = self._alpha(g, h)                                   # [nnz, H], softmax over each destination's entries
        w = alpha if g.val is None else alpha * g.val[:, None]      # norm * alpha (attconv.py:103-104)
        out = ops.spmm_edge_values(g, w, h, self.heads, _AGG[self.agg])
        return out + self.bias if self.bias is not None else out

    def __repr__(self):
        return '{}({}, {}, {})'.format(self.__class__.__name__, self.in_channels, self.out_channels, self.heads)


class GeneralAddAttConvLayer(_AttConvBase):
    """attconv.py:14-111: alpha_ij^h = softmax_i(leaky_relu(<[x_i^h, x_j^h], att^h>, 0.2)); the concatenated dot is
    split into per-node terms a_dst[i,h] = <x_i^h, att[0,h,:hc]>, a_src[j,h] = <x_j^h, att[0,h,hc:]>"""

    def __init__(self, in_channels, out_channels, improved=False, cached=False, bias=True, **kwargs):
        super().__init__(in_channels, out_channels, improved=improved, cached=cached, bias=bias, **kwargs)
        self.att = Parameter(torch.Tensor(1, self.heads, 2 * self.head_channels))
        if bias:
            self.bias = Parameter(torch.Tensor(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        glorot(self.att)
        zeros(self.bias)
        self._reset_cache()

    def _alpha(self, g, h):
        H, hc = self.heads, self.head_channels
        hv = h.view(-1, H, hc)
        a_dst = (hv * self.att[:, :, :hc]).sum(dim=-1)
        a_src = (hv * self.att[:, :, hc:]).sum(dim=-1)
        return ops.gat_alpha(g, a_dst, a_src, self.negative_slope)


class GeneralMulAttConvLayer(_AttConvBase):
    """attconv.py:115-216: alpha_ij = softmax_i((<x_i, x_j> + sum(bias_att)) / sqrt(out_channels)) — the scaler is
    sqrt(out_channels), not sqrt(head_channels).  Single head: the reference broadcasts bias_att [out_channels] over
    [E, H, out_channels / H], which fails for att_heads > 1."""

    def __init__(self, in_channels, out_channels, improved=False, cached=False, bias=True, **kwargs):
        if int(cfg.gnn.att_heads) != 1:
            raise ValueError("gmulconv supports cfg.gnn.att_heads = 1 only, got {}: the reference adds bias_att "
                             "[dim_out] to the per-head products [E, heads, dim_out / heads], which fails for more "
                             "than one head (attconv.py:196-199)".format(cfg.gnn.att_heads))
        super().__init__(in_channels, out_channels, improved=improved, cached=cached, bias=bias, **kwargs)
        self.bias_att = Parameter(torch.Tensor(out_channels))
        self.scaler = math.sqrt(float(out_channels))
        if bias:
            self.bias = Parameter(torch.Tensor(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        zeros(self.bias)
        zeros(self.bias_att)
        self._reset_cache()

    def _alpha(self, g, h):
        scale = 1.0 / self.scaler
        s = ops.sddmm_dot(g, h, h, 1, scale) + self.bias_att.sum() * scale
        return ops.edge_softmax(g, s)


class GeneralAddAttConv(_BatchLayer):      # attconv.py:219-226
    def __init__(self, dim_in, dim_out, bias=False, **kwargs):
        super().__init__()
        self.model = GeneralAddAttConvLayer(dim_in, dim_out, bias=bias)


class GeneralMulAttConv(_BatchLayer):      # attconv.py:229-236
    def __init__(self, dim_in, dim_out, bias=False, **kwargs):
        super().__init__()
        self.model = GeneralMulAttConvLayer(dim_in, dim_out, bias=bias)
