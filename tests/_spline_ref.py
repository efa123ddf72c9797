"""The oracle of the splineconv tests: pyg.nn.SplineConv(dim_in, dim_out, dim=1, kernel_size=2) as graphgym/models/layer.py:
177-186 builds and calls it, written the naive way on the CPU and dtype-generic (tests/_tol.py: both).

Per edge and per basis function s of the open degree-1 spline it gathers the kernel matrix W[k_s] of THAT edge, forms
b_s * (x[src] @ W[k_s]), adds the messages by destination with index_add_, divides by the in-edge count, and adds the root
term and the bias.  It knows nothing of coefficients per matrix, of stacked weights or of an aggregation order: no code
and no algebra is shared with graphgym_amd/splineconv.py."""
import torch

KERNEL_SIZE, DEGREE = 2, 1


def basis(u):
    """[(b_s [E], k_s [E] int64) for s = 0, 1] of the pseudo-coordinates u [E] or [E, 1]"""
    v = u.reshape(-1) * (KERNEL_SIZE - DEGREE)
    fl = torch.floor(v)
    f = v - fl
    cell = fl.long()
    return [(1 - f, cell % KERNEL_SIZE), (f, (cell + 1) % KERNEL_SIZE)]


def spline_conv(x, src, dst, u, weight, root, bias=None):
    """x [n, in], edges src -> dst (int64 [E]), u [E, 1], weight [2, in, out], root [in, out], bias [out] or None"""
    n = x.size(0)
    agg = torch.zeros(n, weight.size(2), dtype=x.dtype)
    xs = x[src]
    for b, k in basis(u):
        per_edge = weight[k]                                           # [E, in, out]: the edge's own matrix
        msg = b[:, None] * torch.bmm(xs[:, None, :], per_edge)[:, 0, :]
        agg = agg.index_add(0, dst, msg)
    count = torch.bincount(dst, minlength=n).to(x.dtype)
    out = agg / count.clamp(min=1)[:, None] + x @ root
    return out if bias is None else out + bias


def entry_sums(rows, cols, w, x, n):
    """the two weighted neighbour sums over stored entries (rows, cols int64 [nnz], w [nnz, 2]): [n, 2 d]"""
    xs = x[cols]
    halves = [torch.zeros(n, x.size(1), dtype=x.dtype).index_add(0, rows, w[:, s:s + 1] * xs) for s in (0, 1)]
    return torch.cat(halves, dim=1)


def entry_fold(rows, cols, w, z, n):
    """sum over stored entries of w[e, 0] z[col, :d] + w[e, 1] z[col, d:]: [n, d]"""
    d = z.size(1) // 2
    zs = z[cols]
    return torch.zeros(n, d, dtype=z.dtype).index_add(0, rows, w[:, 0:1] * zs[:, :d] + w[:, 1:2] * zs[:, d:])
