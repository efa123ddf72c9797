"""torch restatement of GraphGym's edge-feature attention layers (graphgym/contrib/layer/attconv.py:
GeneralEdgeAttConvv1Layer, GeneralEdgeAttConvv2Layer) and of the two operators under them, written for the tests from the
reference's semantics: per edge, the concatenation cat([x_i,] x_j, ef_e), the message linear, the view [E, H, hc], the
score <m^h, att_msg^h> [+ <task_emb, att_task^h>], leaky_relu(0.2), torch_geometric.utils.softmax over each destination's
edges, norm * m * alpha, the reduction of cfg.gnn.agg, then update(): BatchNorm, final linear, bias.  The layer function
builds the concatenated per-edge tensor as the reference does, so the column order [W_i | W_j | W_e] of the linear's
weight is what a comparison pins.  Dtype-generic (tests/_tol.py: both); nothing here knows about CSR or the engine."""
import torch
import torch.nn.functional as F

from _att_ref import att_edges, reduce_rows, segment_softmax  # noqa: F401  (att_edges: re-exported for the tests)


def edge_att_alpha(rows, cols, eids, a_dst, a_src, a_edge, n, slope=0.2):
    """alpha[e, h] = softmax over the entries of row rows[e] of leaky_relu(a_dst[rows] + a_src[cols] + a_edge[eids]);
    a_dst may be None, an entry with eids < 0 has no edge term"""
    s = a_src[cols]
    if a_dst is not None:
        s = a_dst[rows] + s
    if a_edge.size(0):
        s = s + a_edge[eids.clamp(min=0)] * (eids >= 0).to(s.dtype)[:, None]
    return segment_softmax(F.leaky_relu(s, slope), rows, n)


def edge_heads_agg(rows, cols, eids, w, X, M, T, bias, n, heads, reduce, win=None):
    """y[r, slice h] = reduce_e w[e, h] (X[col_e] + M[eid_e] + T[r])[slice h] + bias; eid < 0: no M term; T, bias may be
    None.  The sum is formed in the order (X + M) + T, then scaled."""
    dh = X.size(1) // heads
    m = M[eids.clamp(min=0)] * (eids >= 0).to(X.dtype)[:, None] if M.size(0) else torch.zeros_like(X[cols])
    msg = X[cols] + m
    if T is not None:
        msg = msg + T[rows]
    msg = w.repeat_interleave(dh, dim=1) * msg
    y = reduce_rows(rows, msg, n, reduce, win)
    return y if bias is None else y + bias


def edge_att_conv(x, ef, ei, norm, p, version, heads, agg, msg_direction, task_emb=None, bn=None, win=None,
                  uses=None):
    """one layer's forward on the edges ei [2, E] (source, destination) with features ef [E, k] and weights norm [E] or
    None.  p: the layer's parameters by their state-dict names; version 1 (linear_msg) or 2 (linear_value, with its
    bias); bn = (eps, momentum) when linear_final_bn is present (training-mode statistics).  uses (a dict): the per-edge
    message becomes a leaf of its own, stored there as "msg" — its gradient is the per-edge term of dL/dx, dL/def"""
    n = x.size(0)
    src, dst = ei[0], ei[1]
    parts = [x[dst], x[src], ef] if msg_direction == "both" else [x[src], ef]
    lin = "linear_msg" if version == 1 else "linear_value"
    m = torch.cat(parts, dim=-1) @ p[lin + ".weight"].t()
    if p.get(lin + ".bias") is not None:
        m = m + p[lin + ".bias"]
    if uses is not None:
        m = m.detach().requires_grad_(True)
        uses["msg"] = m
    dout = m.size(1)
    mv = m.view(-1, heads, dout // heads)
    s = (mv * p["att_msg"]).sum(-1)
    if task_emb is not None:
        s = s + (task_emb.view(1, 1, -1) * p["att_task"]).sum(-1)
    alpha = segment_softmax(F.leaky_relu(s, 0.2), dst, n)
    msg = mv * alpha[..., None]
    if norm is not None:
        msg = norm.view(-1, 1, 1) * msg
    out = reduce_rows(dst, msg.reshape(-1, dout), n, agg, win)
    if bn is not None:
        out = F.batch_norm(out, None, None, p["linear_final_bn.weight"], p["linear_final_bn.bias"], True, bn[1], bn[0])
    if p.get("linear_final.weight") is not None:
        out = out @ p["linear_final.weight"].t()
    if p.get("bias") is not None:
        out = out + p["bias"]
    return out


def input_magnitudes(x, ef, ei, norm, p, version, heads, agg, msg_direction, dy, task_emb=None, bn=None, win=None):
    """float64 bounds on |dL/dx| and |dL/def| row by row for L = sum(out * dy): the per-edge gradients of the message,
    as absolute values, through |W_i|, |W_j|, |W_e| and summed over a node's edges (tests/_tol.py rule (d))"""
    uses = {}
    out = edge_att_conv(x, ef, ei, norm, p, version, heads, agg, msg_direction, task_emb, bn, win, uses)
    (out * dy).sum().backward()
    gm = uses["msg"].grad.abs()
    W = p["linear_msg.weight" if version == 1 else "linear_value.weight"].detach().abs()
    k = x.size(1)
    mag_x = torch.zeros_like(x)
    if msg_direction == "both":
        mag_x.index_add_(0, ei[1], gm @ W[:, :k])
        mag_x.index_add_(0, ei[0], gm @ W[:, k:2 * k])
        return mag_x, gm @ W[:, 2 * k:]
    mag_x.index_add_(0, ei[0], gm @ W[:, :k])
    return mag_x, gm @ W[:, k:]
