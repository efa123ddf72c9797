"""GraphGym's edge-feature attention layers on the engine: graphgym/contrib/layer/attconv.py

    GeneralEdgeAttConvv1Layer                             attconv.py:243-375
    GeneralEdgeAttConvv2Layer                             attconv.py:378-517
    GeneralEdgeAttConvv1     'generaledgeattconvv1'       attconv.py:520-528
    GeneralEdgeAttConvv2     'generaledgeattconvv2'       attconv.py:531-539

The message of entry e = (i <- j) with edge feature ef_e is m_e = linear(cat([x_i,] x_j, ef_e)) viewed as [H, hc]
(attconv.py:344-349), its score leaky_relu(<m_e^h, att_msg^h> [+ <task_emb, att_task^h>], 0.2), softmax over the entries
of i, and the layer aggregates norm_e * alpha_e^h * m_e^h with cfg.gnn.agg (attconv.py:352-360).  linear.weight =
[W_i | W_j | W_e] splits by columns (as edgeconv.GeneralEdgeConvLayer._weights splits it), so with

    X = x W_j^T (+ b_v)  [N, d]      M = ef W_e^T  [E, d]      T = x W_i^T  [N, d]  (msg_direction 'both')

m_e = X[j] + M[e] + T[i], the score is additive in per-node and per-edge scalars — a_src = <X^h, att_msg^h>,
a_edge = <M^h, att_msg^h>, a_dst = <T^h, att_msg^h>, the task term a per-head constant folded into a_src — and neither
the concatenated input nor the per-entry message is ever built: ops.edge_att_alpha gives alpha, ops.spmm_edge_heads the
aggregation.  v1 and v2 differ in the message linear alone (linear_msg without bias; linear_value with bias=bias, and a
linear_key that the reference constructs and never uses — kept for the state dict).  Constructor, parameter names and
shapes follow the reference, so state dicts interchange.  float32 only.
"""
import torch
import torch.nn as nn
from torch.nn import Parameter

from . import nn as mpnn
from . import ops
from .config import cfg
from .edgeconv import _aligned_graph
from .layers import _CachedEdgesMixin, glorot, zeros

_AGG = {"add": "sum", "sum": "sum", "mean": "mean", "max": "max"}


class _EdgeAttConvBase(nn.Module, _CachedEdgesMixin):
    """what the two reference layers share: everything but the message linear (attconv.py:246-375, :381-517)"""

    def __init__(self, in_channels, out_channels, task_channels=None, improved=False, cached=False, bias=True,
                 **kwargs):
        super().__init__()
        self.heads = int(cfg.gnn.att_heads)
        if self.heads < 1 or out_channels % self.heads:
            raise ValueError("{}: dim_out = {} is not a multiple of cfg.gnn.att_heads = {} (the reference's per-head "
                             "view fails there too)".format(type(self).__name__, out_channels, self.heads))
        if cfg.gnn.agg not in _AGG:
            raise ValueError("cfg.gnn.agg must be one of 'add', 'mean', 'max', got {!r}".format(cfg.gnn.agg))
        self.in_channels = int(in_channels // self.heads * self.heads)
        self.out_channels = int(out_channels // self.heads * self.heads)
        self.dim_in = int(in_channels)                 # the width the message linear was built for
        self.task_channels = task_channels
        self.improved, self.cached = improved, cached
        self.normalize = cfg.gnn.normalize_adj
        self.agg = cfg.gnn.agg
        self.msg_direction = cfg.gnn.msg_direction
        self.edge_dim = int(cfg.dataset.edge_dim)
        self.negative_slope = 0.2
        self.head_channels = out_channels // self.heads
        self.scaling = self.head_channels ** -0.5
        self.final_linear = bool(getattr(cfg.gnn, "att_final_linear", False))
        self.final_linear_bn = bool(getattr(cfg.gnn, "att_final_linear_bn", False))
        k = in_channels if self.msg_direction == 'single' else 2 * in_channels
        self._build_message_linears(k + self.edge_dim, out_channels, bias)
        self.att_msg = Parameter(torch.Tensor(1, self.heads, self.head_channels))
        if self.task_channels is not None:
            self.att_task = Parameter(torch.Tensor(1, self.heads, self.task_channels))
        if self.final_linear:
            self.linear_final = mpnn.Linear(out_channels, out_channels, bias=False)
        if self.final_linear_bn:
            self.linear_final_bn = mpnn.BatchNorm1d(out_channels, eps=cfg.bn.eps, momentum=cfg.bn.mom)
        if bias:
            self.bias = Parameter(torch.Tensor(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        glorot(self.att_msg)
        if self.task_channels is not None:
            glorot(self.att_task)
        zeros(self.bias)
        self.cached_result = None
        self.cached_num_edges = None

    def _weights(self):
        """(W_i^T or None, W_j^T, W_e^T, b or None): the column blocks of the message linear's weight in the order of the
        reference's concatenation x_i, x_j, edge_feature (attconv.py:345,347), as [in, out] views, and its bias"""
        lin, n = self._message_linear(), self.dim_in
        W = lin.weight
        if self.msg_direction == 'single':
            return None, W[:, :n].t(), W[:, n:].t(), lin.bias
        return W[:, :n].t(), W[:, n:2 * n].t(), W[:, 2 * n:].t(), lin.bias

    def forward(self, x, edge_index, edge_weight=None, edge_feature=None, task_emb=None, holder=None):
        if x.dtype != torch.float32 or (edge_feature is not None and edge_feature.dtype != torch.float32):
            raise TypeError("the edge-feature attention layers generaledgeattconvv1 and generaledgeattconvv2 are float32 "
                            "only (got x {} / edge_feature {}): run them in float32".format(
                                x.dtype, None if edge_feature is None else edge_feature.dtype))
        if edge_feature is None:
            raise ValueError("{} needs edge_feature [E, {}]".format(type(self).__name__, self.edge_dim))
        if self.normalize:
            g = self._graph(holder, edge_index, x.size(0), edge_weight, loops="remaining", norm="col",
                            fill=2.0 if self.improved else 1.0)
        else:
            g = self._graph(holder, edge_index, x.size(0), edge_weight, loops="none")
        ga = _aligned_graph(g, edge_index) if edge_feature.size(0) == g.nnz else None
        if ga is None:
            raise RuntimeError("edge_feature has {} rows, the operator has {} entries (self loops were added or "
                               "removed: the reference fails here too)".format(edge_feature.size(0), g.nnz))
        Wi, Wj, We, b = self._weights()
        H, hc = self.heads, self.head_channels
        X = ops.dense_fused(x, Wj, bias=b)                       # v2's b_v rides here: once per message
        M = ops.dense_fused(edge_feature, We)
        T = None if Wi is None else ops.dense_fused(x, Wi)
        a_src = (X.view(-1, H, hc) * self.att_msg).sum(dim=-1)
        a_edge = (M.view(-1, H, hc) * self.att_msg).sum(dim=-1)
        a_dst = None if T is None else (T.view(-1, H, hc) * self.att_msg).sum(dim=-1)
        if task_emb is not None:                                 # a per-head constant (attconv.py:350-353)
            a_src = a_src + (task_emb.view(1, 1, self.task_channels) * self.att_task).sum(dim=-1)
        alpha = ops.edge_att_alpha(ga, a_dst, a_src, a_edge, self.negative_slope)
        w = alpha if ga.val is None else alpha * ga.val[:, None]      # norm * alpha (attconv.py:358-360)
        out = ops.spmm_edge_heads(ga, w, X, M, t=T, heads=H, reduce=_AGG[self.agg])
        return self.update(out)

    def update(self, aggr_out):
        """attconv.py:362-370: BatchNorm, the final linear, the bias — in that order"""
        if self.final_linear_bn:
            aggr_out = self.linear_final_bn(aggr_out)
        if self.final_linear:
            aggr_out = self.linear_final(aggr_out)
        if self.bias is not None:
            aggr_out = aggr_out + self.bias
        return aggr_out

    def __repr__(self):
        return '{}({}, {}, {})'.format(self.__class__.__name__, self.in_channels, self.out_channels, self.heads)


class GeneralEdgeAttConvv1Layer(_EdgeAttConvBase):
    """attconv.py:243-375: the message is linear_msg(cat([x_i,] x_j, ef)), no bias"""

    def _build_message_linears(self, k, out_channels, bias):
        self.linear_msg = mpnn.Linear(k, out_channels, bias=False)

    def _message_linear(self):
        return self.linear_msg


class GeneralEdgeAttConvv2Layer(_EdgeAttConvBase):
    """attconv.py:378-517: the message is linear_value(cat([x_i,] x_j, ef)) with bias=bias; linear_key is constructed and
    never used (attconv.py:402-408, :484-502) — it is here for the state dict and receives no gradient"""

    def _build_message_linears(self, k, out_channels, bias):
        self.linear_value = mpnn.Linear(k, out_channels, bias=bias)
        self.linear_key = mpnn.Linear(k, out_channels, bias=bias)

    def _message_linear(self):
        return self.linear_value


class _EdgeAttBatchLayer(nn.Module):
    def forward(self, batch):
        batch.node_feature = self.model(batch.node_feature, batch.edge_index, edge_feature=batch.edge_feature,
                                        holder=batch)
        return batch


class GeneralEdgeAttConvv1(_EdgeAttBatchLayer):      # attconv.py:520-528
    def __init__(self, dim_in, dim_out, bias=False, **kwargs):
        super().__init__()
        self.model = GeneralEdgeAttConvv1Layer(dim_in, dim_out, bias=bias)


class GeneralEdgeAttConvv2(_EdgeAttBatchLayer):      # attconv.py:531-539
    def __init__(self, dim_in, dim_out, bias=False, **kwargs):
        super().__init__()
        self.model = GeneralEdgeAttConvv2Layer(dim_in, dim_out, bias=bias)
