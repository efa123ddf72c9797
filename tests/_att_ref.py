"""torch restatement of GraphGym's attention layers (graphgym/contrib/layer/attconv.py: GeneralAddAttConvLayer,
GeneralMulAttConvLayer) and of their weighted aggregation, written for the tests from the reference's semantics:
MessagePassing with flow source_to_target (messages x_j = x[edge_index[0]] reduced at i = edge_index[1]), aggr
'add' / 'mean' / 'max' as scatter_reduce(..., include_self=False) into zeros (an empty row gives 0),
torch_geometric.utils.softmax over each destination's edges, add_remaining_self_loops + the symmetric GCN norm when
normalize_adj.  Dtype-generic: every float input passes through the cast `c` (tests/_tol.py: both)."""
import math

import torch

_RED = {"sum": "sum", "add": "sum", "mean": "mean", "max": "amax"}


def reduce_rows(rows, msg, n_rows, reduce, win=None):
    """out[i] = reduce over the messages msg[e] with rows[e] == i; win [n_rows, d] (engine argmax, -1 = none): max is
    evaluated at those entries instead, so that gradients follow the engine's winners (near-ties cannot flip one)"""
    d = msg.size(1)
    if reduce == "max" and win is not None:
        w = win.long()
        got = msg.gather(0, w.clamp(min=0))
        return torch.where(w >= 0, got, torch.zeros_like(got))
    out = torch.zeros((n_rows, d), dtype=msg.dtype, device=msg.device)
    return out.scatter_reduce(0, rows[:, None].expand(-1, d), msg, reduce=_RED[reduce], include_self=False)


def edge_values_agg(rows, cols, a, V, n_rows, heads, reduce, win=None):
    """y[i, slice h] = reduce over entries e of row i of a[e, h] V[cols[e], slice h]"""
    dh = V.size(1) // heads
    msg = a.repeat_interleave(dh, dim=1) * V[cols]
    return reduce_rows(rows, msg, n_rows, reduce, win)


def add_remaining_self_loops(ei, w, fill, n):
    """torch_geometric.utils.add_remaining_self_loops: loops of the input keep their weight (one per node), every node
    without one gets a loop of weight `fill`"""
    mask = ei[0] != ei[1]
    loop_w = torch.full((n,), float(fill), dtype=w.dtype)
    inv = ~mask
    loop_w[ei[0][inv]] = w[inv]
    loops = torch.arange(n).repeat(2, 1)
    return torch.cat([ei[:, mask], loops], dim=1), torch.cat([w[mask], loop_w])


def gcn_norm(ei, w, n):
    """attconv.py:52-64: deg over edge_index[0], deg^-1/2 (inf -> 0), norm = dis[row] * w * dis[col]"""
    row, col = ei
    deg = torch.zeros(n, dtype=w.dtype).index_add_(0, row, w)
    dis = deg.pow(-0.5)
    dis[dis == float("inf")] = 0
    return dis[row] * w * dis[col]


def segment_softmax(s, index, n):
    """torch_geometric.utils.softmax over the edges that share index (per column of s)"""
    idx = index[:, None].expand_as(s)
    m = torch.full((n, s.size(1)), -math.inf, dtype=s.dtype).scatter_reduce(0, idx, s, "amax", include_self=True)
    ex = (s - m[index]).exp()
    z = torch.zeros((n, s.size(1)), dtype=s.dtype).index_add_(0, index, ex)
    return ex / (z[index] + 1e-16)


def att_edges(ei, n, normalize, improved=False):
    """the edge list (and per-edge norm or None) the layer propagates over"""
    if not normalize:
        return ei, None
    w = torch.ones(ei.size(1), dtype=torch.float64)
    ei2, w2 = add_remaining_self_loops(ei, w, 2.0 if improved else 1.0, n)
    return ei2, gcn_norm(ei2, w2, n)


def att_conv(kind, x, W, att, bias_att, bias, ei, norm, heads, agg, win=None, uses=None):
    """one layer's forward.  kind 'add' (att [1, H, 2 hc]) or 'mul' (bias_att [dim_out]); W [dim_out, dim_in]
    (linear_msg.weight); ei the propagated edge list, norm its per-edge weights or None.  Returns (out, alpha).
    uses (a dict): the per-edge reads h[dst], h[src] become leaves of their own, stored there as "dst", "src" — their
    gradients are the per-edge terms that sum to dL/dh"""
    n = x.size(0)
    h = x @ W.t()
    dout = h.size(1)
    hc = dout // heads
    src, dst = ei[0], ei[1]
    hv = h.view(-1, heads, hc)
    hd, hs = hv[dst], hv[src]
    if uses is not None:
        hd, hs = hd.detach().requires_grad_(True), hs.detach().requires_grad_(True)
        uses["dst"], uses["src"] = hd, hs
    if kind == "add":
        s = (torch.cat([hd, hs], dim=-1) * att).sum(dim=-1)
        s = torch.nn.functional.leaky_relu(s, 0.2)
    else:
        s = (hd * hs + bias_att).sum(dim=-1) / math.sqrt(dout)
    alpha = segment_softmax(s, dst, n)
    msg = (hs * alpha[..., None])
    if norm is not None:
        msg = norm.view(-1, 1, 1) * msg
    out = reduce_rows(dst, msg.reshape(-1, dout), n, agg, win)
    return (out + bias if bias is not None else out), alpha


def dx_magnitude(kind, x, W, att, bias_att, bias, ei, norm, heads, agg, dy, win=None):
    """a float64 bound on |dL/dx| row by row for L = sum(out * dy): the per-edge terms of dL/dh summed as absolute
    values, times |W| — for rows of x.grad that cancel (tests/_tol.py rule (d))"""
    uses = {}
    out, _ = att_conv(kind, x, W, att, bias_att, bias, ei, norm, heads, agg, win, uses)
    (out * dy).sum().backward()
    n, d = x.size(0), W.size(0)
    mag_h = torch.zeros((n, d), dtype=x.dtype)
    mag_h.index_add_(0, ei[1], uses["dst"].grad.reshape(-1, d).abs())
    mag_h.index_add_(0, ei[0], uses["src"].grad.reshape(-1, d).abs())
    return mag_h @ W.abs()
