"""Plain-torch restatement of GraphGym's edge-feature layer (graphgym/contrib/layer/generalconv.py:117-218) and of the
aggregation under it, dtype-generic (tests/_tol.both evaluates it in float64 and float32).  Written from the formulas:

    message_e = n_e * linear_msg(cat([x_i,] x_j, ef_e))                      generalconv.py:203-209
    out_i     = reduce over the edges e into i of message_e + bias           generalconv.py:192, :211-214
                [+ x_i  (self_msg 'add')]  [+ linear_self(x_i)  ('concat')]  generalconv.py:195-201

Edges are explicit (dst, src, feature row, weight) lists; nothing here knows about CSR, plans or the engine.
"""
import torch


def reduce_rows(rows, msg, n, reduce, win=None):
    """[n, d]: sum / mean / max of the per-edge messages msg [m, d] by destination `rows`; a row without edges gives 0.
    max with `win` [n, d] (edge index per output element, -1: none) evaluates the maximum AT those winners, so that
    gradients follow a fixed selection"""
    d = msg.size(1)
    out = torch.zeros(n, d, dtype=msg.dtype)
    if reduce in ("sum", "add", "mean"):
        out = out.index_add(0, rows, msg)
        if reduce == "mean":
            cnt = torch.zeros(n, dtype=msg.dtype).index_add(0, rows, torch.ones(rows.numel(), dtype=msg.dtype))
            out = out / cnt.clamp(min=1)[:, None]
        return out
    if win is not None:
        picked = msg.gather(0, win.clamp(min=0).long())
        return torch.where(win >= 0, picked, torch.zeros_like(picked))
    idx = rows[:, None].expand(-1, d)
    out = torch.full((n, d), float("-inf"), dtype=msg.dtype).scatter_reduce(0, idx, msg, "amax", include_self=True)
    return torch.where(torch.isinf(out), torch.zeros_like(out), out)


def edge_agg(rows, cols, eids, val, X, M, T, bias, n, reduce, win=None):
    """the operator: y[r] = reduce_e val_e (X[col_e] + M[eid_e] + T[r]) + bias; eid < 0: no M term; val, T, bias may be
    None.  The sum is formed in the order (X + M) + T, then scaled."""
    m = M[eids.clamp(min=0)] * (eids >= 0).to(X.dtype)[:, None] if M.size(0) else torch.zeros_like(X[cols])
    msg = X[cols] + m
    if T is not None:
        msg = msg + T[rows]
    if val is not None:
        msg = val[:, None] * msg
    y = reduce_rows(rows, msg, n, reduce, win)
    return y if bias is None else y + bias


def norm_edges(ei, n, dtype):
    """cfg.gnn.normalize_adj for an edge list that already holds one self loop per node (nothing is added): weights
    deg^-1/2[src] * deg^-1/2[dst] with deg the number of edges by SOURCE (generalconv.py:164-169, edge_index[0])"""
    src, dst = ei[0], ei[1]
    deg = torch.zeros(n, dtype=dtype).index_add(0, src, torch.ones(src.numel(), dtype=dtype))
    dis = deg.pow(-0.5)
    dis = torch.where(torch.isinf(dis), torch.zeros_like(dis), dis)
    return dis[src] * dis[dst]


def edge_conv(x, ef, ei, norm, W_msg, W_self, bias, msg_direction, self_msg, agg, win=None):
    """the layer on edges ei [2, E] (source, destination) with features ef [E, k] and weights norm [E] or None"""
    src, dst = ei[0], ei[1]
    parts = [x[dst], x[src], ef] if msg_direction == "both" else [x[src], ef]
    msg = torch.cat(parts, dim=1) @ W_msg.t()
    if norm is not None:
        msg = norm[:, None] * msg
    out = reduce_rows(dst, msg, x.size(0), agg, win)
    if bias is not None:
        out = out + bias
    if self_msg == "concat":
        return x @ W_self.t() + out
    if self_msg == "add":
        return x + out
    return out
