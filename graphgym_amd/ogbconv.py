"""GraphGym's OGB layers on the engine: graphgym/contrib/layer/generalconv_ogb.py and sageinitconv.py

    GeneralOGBConvLayer / GeneralOGBConv   'generalogbconv'   generalconv_ogb.py:38-141
    SAGEConvLayer / SAGEinitConv           'sageinitconv'     sageinitconv.py:12-115

generalogbconv: the message of entry (i <- j) is norm_ij * (x_j W + b_e) with b_e the sum of three bond-embedding rows
chosen by the edge's integer features (generalconv_ogb.py:30-35,115-118).  The three codes of an edge are packed once
per batch into one combined code q_e < 5 * 6 * 2 = 60 (range-checked there, cached on the batch); the combined table
B[q] = ((0 + T_0[q_0]) + T_1[q_1]) + T_2[q_2] [60, d] is built per call with torch indexing, so autograd carries dB back
to the three tables; ops.spmm_code then runs the two-gather aggregation with B as its edge operand and q as the
entry's row index.  Nothing of size [E, d] exists in the forward or the backward, for add, mean or max.

sageinitconv: the wrapper always builds its layer with concat=True (sageinitconv.py:108): the mean over the neighbours
as edge_index gives them (no self loop added, present ones kept), then cat([x, mean]) @ weight + bias — the two row
blocks of weight [2 in, out] are the two operands of one transform launch, and no concatenation is built.

Constructors and parameter names follow the reference, so state dicts interchange.  float32 only.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn import Parameter

from . import encoders, ops
from .config import cfg
from .edgeconv import _AGG, _aligned_graph
from .encoders import BondEncoder
from .layers import _CachedEdgesMixin, get_graph, glorot, zeros


def pack_bond_codes(codes, dims=None):
    """[E, K] codes (column k in [0, dims[k])) -> [E] combined code, the mixed-radix number with column 0 leading"""
    dims = encoders.full_bond_feature_dims if dims is None else dims
    q = codes[:, 0].clone()
    for k in range(1, len(dims)):
        q = q * int(dims[k]) + codes[:, k]
    return q.contiguous()


def unpack_bond_codes(q, dims=None):
    """the inverse of pack_bond_codes: [E] -> [E, K]"""
    dims = encoders.full_bond_feature_dims if dims is None else dims
    cols = []
    for k in range(len(dims) - 1, -1, -1):
        cols.append(q % int(dims[k]))
        q = torch.div(q, int(dims[k]), rounding_mode="floor")
    return torch.stack(cols[::-1], dim=1)


class GeneralOGBConvLayer(nn.Module, _CachedEdgesMixin):
    """generalconv_ogb.py:38-127"""

    def __init__(self, in_channels, out_channels, improved=False, cached=False, bias=True, **kwargs):
        super().__init__()
        if cfg.gnn.agg not in _AGG:
            raise ValueError("cfg.gnn.agg must be one of 'add', 'mean', 'max', got {!r}".format(cfg.gnn.agg))
        self.in_channels, self.out_channels = in_channels, out_channels
        self.improved, self.cached = improved, cached
        self.normalize = cfg.gnn.normalize_adj
        self.agg = cfg.gnn.agg
        self.weight = Parameter(torch.Tensor(in_channels, out_channels))
        if bias:
            self.bias = Parameter(torch.Tensor(out_channels))
        else:
            self.register_parameter('bias', None)
        self.bond_encoder = BondEncoder(emb_dim=out_channels)
        self.reset_parameters()

    def reset_parameters(self):
        glorot(self.weight)
        zeros(self.bias)
        self.cached_result = None
        self.cached_num_edges = None

    def _dims(self):
        return [emb.weight.size(0) for emb in self.bond_encoder.bond_embedding_list]

    def combined_table(self):
        """B [prod(dims), d]: B[q] = ((0 + T_0[q_0]) + T_1[q_1]) + T_2[q_2], the reference's loop (generalconv_ogb.py:30-35)
        over every combination of codes"""
        dims = self._dims()
        tables = [emb.weight for emb in self.bond_encoder.bond_embedding_list]
        n = 1
        for d in dims:
            n *= d
        idx = unpack_bond_codes(torch.arange(n, device=tables[0].device), dims)
        B = torch.zeros((n, self.out_channels), dtype=tables[0].dtype, device=tables[0].device)
        for k, T in enumerate(tables):
            B = B + T[idx[:, k]]
        return B

    def forward(self, x, edge_index, edge_feature, edge_weight=None, holder=None):
        if x.dtype != torch.float32:
            raise TypeError("the edge-feature layer generalogbconv is float32 only (got x {}): run it in "
                            "float32".format(x.dtype))
        if edge_feature is None:
            raise ValueError("GeneralOGBConvLayer needs edge_feature [E, {}] of integer codes".format(len(self._dims())))
        if self.normalize:
            g = self._graph(holder, edge_index, x.size(0), edge_weight, loops="remaining", norm="col",
                            fill=2.0 if self.improved else 1.0)
        else:
            g = self._graph(holder, edge_index, x.size(0), edge_weight, loops="none")
        ga = _aligned_graph(g, edge_index) if edge_feature.size(0) == g.nnz else None
        if ga is None:
            raise RuntimeError("edge_feature has {} rows, the operator has {} entries (self loops were added or "
                               "removed: the reference fails here too)".format(edge_feature.size(0), g.nnz))
        dims = self._dims()
        codes = encoders.cached_codes(holder, "edge_feature", edge_feature, dims, make=pack_bond_codes)
        h = ops.dense_fused(x, self.weight)
        return ops.spmm_code(ga, h, self.combined_table(), codes, _AGG[self.agg], bias=self.bias)

    def __repr__(self):
        return '{}({}, {})'.format(self.__class__.__name__, self.in_channels, self.out_channels)


class GeneralOGBConv(nn.Module):           # generalconv_ogb.py:130-138
    def __init__(self, dim_in, dim_out, bias=False, **kwargs):
        super().__init__()
        self.model = GeneralOGBConvLayer(dim_in, dim_out, bias=bias)

    def forward(self, batch):
        batch.node_feature = self.model(batch.node_feature, batch.edge_index, batch.edge_feature, holder=batch)
        return batch


class SAGEConvLayer(nn.Module):
    """sageinitconv.py:12-102 for a tensor x (no bipartite DataFlow input)"""

    def __init__(self, in_channels, out_channels, normalize=False, concat=False, bias=True, **kwargs):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.normalize, self.concat = normalize, concat
        self.weight = Parameter(torch.Tensor(2 * in_channels if concat else in_channels, out_channels))
        if bias:
            self.bias = Parameter(torch.Tensor(out_channels))
        else:
            self.register_parameter('bias', None)
        self.reset_parameters()

    def reset_parameters(self):
        glorot(self.weight)
        zeros(self.bias)

    def forward(self, x, edge_index, edge_weight=None, holder=None):
        # concat: the neighbours as they are; otherwise add_remaining_self_loops first (sageinitconv.py:73-75)
        g = get_graph(holder, edge_index, x.size(0), loops="none" if self.concat else "remaining",
                      edge_weight=edge_weight)
        mean = ops.spmm(g, x, "mean")
        if self.concat:       # cat([x, mean]) @ weight: its two row blocks, one launch, no concatenation
            n = self.in_channels
            out = ops.dense_fused(x, self.weight[:n], Q=mean, W_id=self.weight[n:], bias=self.bias)
        else:
            out = ops.dense_fused(mean, self.weight, bias=self.bias)
        if self.normalize:
            out = F.normalize(out, p=2, dim=-1)
        return out

    def __repr__(self):
        return '{}({}, {})'.format(self.__class__.__name__, self.in_channels, self.out_channels)


class SAGEinitConv(nn.Module):             # sageinitconv.py:105-112
    def __init__(self, dim_in, dim_out, bias=False, **kwargs):
        super().__init__()
        self.model = SAGEConvLayer(dim_in, dim_out, bias=bias, concat=True)

    def forward(self, batch):
        batch.node_feature = self.model(batch.node_feature, batch.edge_index, holder=batch)
        return batch
