"""GraphGym's edge-feature layers on the engine: graphgym/contrib/layer/generalconv.py and graphgym/models/layer.py

    GeneralEdgeConvLayer                            generalconv.py:117-218
    GeneralEdgeConv          'generaledgeconv'        layer.py:199-207
    GeneralSampleEdgeConv    'generalsampleedgeconv'  layer.py:210-221

The message of entry (i <- j) with edge feature e is norm_ij * linear_msg(cat([x_i,] x_j, e)) (generalconv.py:203-209).
linear_msg.weight = [W_i | W_j | W_e] splits by columns, so the message is norm_ij * (W_j x_j + W_e e [+ W_i x_i]) and no
concatenated per-entry tensor is ever built:

    add / mean   linear in the message: (A x) W_j^T + (A_edge EF) W_e^T + (c * x) W_i^T with A_edge the operator over
                 input edges (CSRGraph.input_edge_operator) and c the row sums of norm (over the entry count for mean) —
                 the existing aggregation and transform operators, nothing of size [nnz, dim_out];
    max          ops.spmm_edge: one pass over X = x W_j^T [N, d], M = EF W_e^T [E, d] and T = x W_i^T [N, d].

An entry takes the feature row of ITS input edge.  The reference pairs rows by position after add_remaining_self_loops
has moved the self loops behind the other edges (cfg.gnn.normalize_adj), which is the same thing when the self loops
close edge_index in node order.  Constructor, parameter names and shapes follow the reference, so state dicts
interchange.  float32 only.
"""
import torch
import torch.nn as nn
from torch.nn import Parameter

from . import nn as mpnn
from . import ops
from .config import cfg
from .layers import _CachedEdgesMixin, _pick_order, zeros

_AGG = {"add": "sum", "sum": "sum", "mean": "mean", "max": "max"}


def _aligned_graph(g, edge_index, dst_row=1):
    """g with every entry's eid pointing at an input edge: the self entries that loops="remaining" re-adds (eid < 0)
    take the position of the node's own loop in edge_index.  None if a node had no loop, i.e. an entry was inserted.
    Cached on g (g belongs to this edge_index)."""
    hit = g.__dict__.get("_edge_aligned")
    if hit is None:
        eid = g.eid
        if g.nnz and bool((eid < 0).any()):
            src, dst = edge_index[1 - dst_row], edge_index[dst_row]
            at = torch.nonzero(src == dst).view(-1)
            loop_pos = torch.full((max(g.num_nodes, 1),), -1, dtype=torch.int32, device=eid.device)
            loop_pos[dst[at]] = at.to(torch.int32)
            eid = torch.where(eid < 0, loop_pos[(-1 - eid).clamp(min=0).long()], eid)
        if g.nnz and bool((eid < 0).any()):
            hit = False
        elif eid is g.eid:
            hit = g
        else:
            hit = g.with_values(g.val)
            hit.eid = eid.contiguous()
            hit.symmetric, hit.dinv = g.symmetric, g.dinv
        g.__dict__["_edge_aligned"] = hit
    return hit or None


def _row_weight(g, mean):
    """c[r] = sum of row r's entry values (over its entry count for mean; an empty row gives 0)"""
    key = "_row_weight_mean" if mean else "_row_weight"
    c = g.__dict__.get(key)
    if c is None:
        c = g.entry_counts() if g.val is None else g.degree("row")
        if mean:
            c = c / g.entry_counts().clamp(min=1.0)
        g.__dict__[key] = c
    return c


class GeneralEdgeConvLayer(nn.Module, _CachedEdgesMixin):
    """generalconv.py:117-218"""

    def __init__(self, in_channels, out_channels, improved=False, cached=False, bias=True, **kwargs):
        super().__init__()
        if cfg.gnn.agg not in _AGG:
            raise ValueError("cfg.gnn.agg must be one of 'add', 'mean', 'max', got {!r}".format(cfg.gnn.agg))
        self.in_channels, self.out_channels = in_channels, out_channels
        self.improved, self.cached = improved, cached
        self.normalize = cfg.gnn.normalize_adj
        self.agg = cfg.gnn.agg
        self.self_msg = cfg.gnn.self_msg
        self.msg_direction = cfg.gnn.msg_direction
        self.edge_dim = int(cfg.dataset.edge_dim)
        k = in_channels if self.msg_direction == 'single' else 2 * in_channels
        self.linear_msg = mpnn.Linear(k + self.edge_dim, out_channels, bias=False)
        if self.self_msg == 'concat':
            self.linear_self = mpnn.Linear(in_channels, out_channels, bias=False)
        if bias:
            self.bias = Parameter(torch.Tensor(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        zeros(self.bias)
        self.cached_result = None
        self.cached_num_edges = None

    def _weights(self):
        """(W_i^T or None, W_j^T, W_e^T): the column blocks of linear_msg.weight in the order of the reference's
        concatenation x_i, x_j, edge_feature (generalconv.py:205,207), as [in, out] views"""
        W, n = self.linear_msg.weight, self.in_channels
        if self.msg_direction == 'single':
            return None, W[:, :n].t(), W[:, n:].t()
        return W[:, :n].t(), W[:, n:2 * n].t(), W[:, 2 * n:].t()

    def forward(self, x, edge_index, edge_weight=None, edge_feature=None, holder=None):
        if x.dtype != torch.float32 or (edge_feature is not None and edge_feature.dtype != torch.float32):
            raise TypeError("the edge-feature layers generaledgeconv and generalsampleedgeconv are float32 only "
                            "(got x {} / edge_feature {}): run them in float32".format(
                                x.dtype, None if edge_feature is None else edge_feature.dtype))
        if self.self_msg == 'add' and self.in_channels != self.out_channels:
            raise RuntimeError("self_msg 'add' adds the raw x [{}] to the messages [{}]: dim_in must equal dim_out "
                               "(generalconv.py:199)".format(self.in_channels, self.out_channels))
        if edge_feature is None:
            raise ValueError("GeneralEdgeConvLayer needs edge_feature [E, {}]".format(self.edge_dim))
        if self.normalize:
            g = self._graph(holder, edge_index, x.size(0), edge_weight, loops="remaining", norm="col",
                            fill=2.0 if self.improved else 1.0)
        else:
            g = self._graph(holder, edge_index, x.size(0), edge_weight, loops="none")
        ga = _aligned_graph(g, edge_index) if edge_feature.size(0) == g.nnz else None
        if ga is None:
            raise RuntimeError("edge_feature has {} rows, the operator has {} entries (self loops were added or "
                               "removed: the reference fails here too)".format(edge_feature.size(0), g.nnz))
        Wi, Wj, We = self._weights()
        E = edge_feature.size(0)
        if self.agg == 'max':
            X = ops.dense_fused(x, Wj)
            M = ops.dense_fused(edge_feature, We)
            T = None if Wi is None else ops.dense_fused(x, Wi)
            x_msg = ops.spmm_edge(ga, X, M, "max", t=T, bias=self.bias)
        else:
            mean = _AGG[self.agg] == "mean"
            R = ops.spmm(ga.input_edge_operator(E), edge_feature, self.agg)               # [N, edge_dim]
            cx = None if Wi is None else _row_weight(ga, mean)[:, None] * x
            if _pick_order("auto", self.in_channels, self.out_channels) == "aggregate_first":
                # one transform with linear_msg.weight as it is stored: its column blocks meet [c x | A x | R]
                P = ops.spmm(ga, x, self.agg)
                cat = torch.cat([P, R] if cx is None else [cx, P, R], dim=1)
                x_msg = ops.dense_fused(cat, self.linear_msg.weight.t(), bias=self.bias)
            else:
                x_msg = ops.spmm(ga, ops.dense_fused(x, Wj), self.agg, bias=self.bias)
                rest, Wr = (R, We) if cx is None else (torch.cat([cx, R], dim=1),
                                                       torch.cat([Wi, We], dim=0))
                x_msg = x_msg + ops.dense_fused(rest, Wr)
        if self.self_msg == 'concat':
            return self.linear_self(x) + x_msg
        if self.self_msg == 'add':
            return x + x_msg
        return x_msg

    def __repr__(self):
        return '{}({}, {})'.format(self.__class__.__name__, self.in_channels, self.out_channels)


class GeneralEdgeConv(nn.Module):          # layer.py:199-207
    def __init__(self, dim_in, dim_out, bias=False, **kwargs):
        super().__init__()
        self.model = GeneralEdgeConvLayer(dim_in, dim_out, bias=bias)

    def forward(self, batch):
        batch.node_feature = self.model(batch.node_feature, batch.edge_index, edge_feature=batch.edge_feature,
                                        holder=batch)
        return batch


class GeneralSampleEdgeConv(nn.Module):    # layer.py:210-221
    def __init__(self, dim_in, dim_out, bias=False, **kwargs):
        super().__init__()
        self.model = GeneralEdgeConvLayer(dim_in, dim_out, bias=bias)

    def forward(self, batch):
        # the mask is drawn on the CPU default generator, as layer.py:216 draws it: reproducible from torch.manual_seed
        edge_mask = (torch.rand(batch.edge_index.shape[1]) < cfg.gnn.keep_edge).to(batch.edge_index.device)
        edge_index = batch.edge_index[:, edge_mask]
        edge_feature = batch.edge_feature[edge_mask, :]
        # a fresh edge list every call: nothing to cache on the batch
        batch.node_feature = self.model(batch.node_feature, edge_index, edge_feature=edge_feature)
        return batch
