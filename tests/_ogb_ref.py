"""Plain-torch restatement of GraphGym's OGB pieces, dtype-generic (tests/_tol.both evaluates it in float64 and float32):

    encode              the encoder loop                         graphgym/models/feature_encoder.py:74-81, 96-103
    ogb_conv            GeneralOGBConvLayer                      graphgym/contrib/layer/generalconv_ogb.py:87-123
                          x = x @ weight (:89); edge_feature = bond_encoder(edge_feature) (:90, :30-35)
                          message = norm * (x_j + edge_feature) (:115-118); aggr = cfg.gnn.agg (:44); + bias (:120-123)
    sage_init           SAGEConvLayer with concat=True           graphgym/contrib/layer/sageinitconv.py:63-98
                          mean of x_j over the edges as given (:73-78 adds no loop under concat), cat([x, mean]) (:84-85),
                          @ weight (:90), + bias (:92-93)
    module_tree         the children GNN.__init__ builds         graphgym/models/gnn.py:132-161

Edges are explicit (source, destination) lists; nothing here knows about CSR, plans or the engine.
"""
import torch

from _edgeconv_ref import norm_edges, reduce_rows  # noqa: F401


def encode(codes, tables):
    """feature_encoder.py:75-78: encoded = 0; for i in range(K): encoded += table_i(codes[:, i])"""
    out = 0
    for i in range(codes.shape[1]):
        out = out + tables[i][codes[:, i]]
    return out


def spmm_code(rows, cols, q, val, X, table, bias, n, reduce, win=None):
    """y[r] = reduce_e val_e (X[col_e] + table[q_e]) + bias; q_e < 0: no table term"""
    m = table[q.clamp(min=0)] * (q >= 0).to(X.dtype)[:, None]
    msg = X[cols] + m
    if val is not None:
        msg = val[:, None] * msg
    y = reduce_rows(rows, msg, n, reduce, win)
    return y if bias is None else y + bias


def ogb_conv(x, codes, ei, norm, weight, tables, bias, agg, win=None):
    """generalconv_ogb.py:87-123 on edges ei [2, E] (source, destination) with integer features codes [E, 3]"""
    src, dst = ei[0], ei[1]
    h = x @ weight
    msg = h[src] + encode(codes, tables)
    if norm is not None:
        msg = norm[:, None] * msg
    out = reduce_rows(dst, msg, x.size(0), agg, win)
    return out if bias is None else out + bias


def sage_init(x, ei, weight, bias):
    """sageinitconv.py:63-98 with concat=True"""
    src, dst = ei[0], ei[1]
    mean = reduce_rows(dst, x[src], x.size(0), "mean")
    out = torch.cat([x, mean], dim=-1) @ weight
    return out if bias is None else out + bias


def module_tree(cfg):
    """names of the children GNN.__init__ creates, in order (gnn.py:136-161; `preprocess` holds no parameters and is
    outside the engine's path), with the encoder class key and the stage's layers"""
    ds, gnn = cfg.dataset, cfg.gnn
    tree = []
    if ds.node_encoder:
        tree.append(("node_encoder", ds.node_encoder_name))
        if ds.node_encoder_bn:
            tree.append(("node_encoder_bn", ds.encoder_dim))
    if ds.edge_encoder:
        tree.append(("edge_encoder", ds.edge_encoder_name))
        if ds.edge_encoder_bn:
            tree.append(("edge_encoder_bn", ds.edge_dim))
    if gnn.layers_pre_mp > 0:
        tree.append(("pre_mp", gnn.layers_pre_mp))
    if gnn.layers_mp > 0:
        tree.append(("mp", gnn.layers_mp))
    tree.append(("post_mp", gnn.layers_post_mp))
    return tree
