"""The oracle of the pair decoders (graphgym_amd/pair_ops.py): the reference's own composition (head.py:62-85) —
h[index], (a * b).sum(-1), F.cosine_similarity, F.linear(cat) — as dtype-generic closures for tests/_tol.py's `both`, and
the sums of ABSOLUTE terms that rule (d) of that file needs: a width-1 score and a cosine gradient cancel by construction
(at d = 1 the exact cosine gradient is 0), so their own magnitude says nothing about the arithmetic behind them."""
import torch
import torch.nn.functional as F

N = 97
KS = (1, 63, 64, 65, 257, 300)
ZERO_ROW, TINY_ROW, SELF_ROW, OTHER_ROW = 5, 6, 7, 8
EPS = 1e-8


def features(d, n=N, seed=0):
    """[n, d] normal rows; row ZERO_ROW is zero, row TINY_ROW has norm 1e-9 (below eps)"""
    h = torch.randn(n, d, generator=torch.Generator().manual_seed(seed))
    if n > OTHER_ROW:
        h[ZERO_ROW] = 0.0
        h[TINY_ROW] = 0.0
        h[TINY_ROW, 0] = 1e-9
    return h


def pairs(K, n=N, seed=1):
    """[2, K] int64: random pairs in no order, the first min(K, 6) replaced by a pair and its duplicate, a self pair, the
    zero row with itself, the zero row with a normal row, the row of norm 1e-9 with itself"""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, n, (2, K), generator=g)
    special = [(11, 23), (11, 23), (SELF_ROW, SELF_ROW), (ZERO_ROW, ZERO_ROW), (ZERO_ROW, OTHER_ROW), (TINY_ROW, TINY_ROW)]
    for k, (a, b) in enumerate(special[:K]):
        idx[0, k], idx[1, k] = a, b
    return idx


def score(h, index, cosine, eps=EPS):
    """the three lines of the reference's head on h in the dtype it comes in"""
    a, b = h[index[0]], h[index[1]]
    return F.cosine_similarity(a, b, dim=-1, eps=eps) if cosine else (a * b).sum(dim=-1)


def score_and_grad(h, index, g, cosine, eps=EPS):
    """closure for both(): (score [K], dh [N, d]) of the composition under the incoming gradient g"""
    def fn(c):
        x = c(h).detach().clone().requires_grad_(True)
        s = score(x, index, cosine, eps)
        s.backward(c(g))
        return s.detach(), x.grad
    return fn


def pair_sum(c, U, V, index, bias):
    return c(U)[index[0]] + c(V)[index[1]] + (0 if bias is None else c(bias))


def concat_linear(c, h, W, bias, index):
    h = c(h)
    return F.linear(torch.cat((h[index[0]], h[index[1]]), dim=-1), c(W), None if bias is None else c(bias))


def _rnorm(h, cosine, eps):
    H = h.double()
    return 1.0 / H.norm(dim=1).clamp(min=eps) if cosine else torch.ones(H.size(0), dtype=torch.float64)


def score_mag(h, index, cosine, eps=EPS):
    """[K] float64: sum_i |a_i| |b_i|, times r_a r_b for cosine"""
    H, r = h.double().abs(), _rnorm(h, cosine, eps)
    a, b = index[0], index[1]
    return (H[a] * H[b]).sum(-1) * r[a] * r[b]


def grad_mag(h, index, g, s, cosine, eps=EPS):
    """[N, d] float64, row v: sum_{k containing v} |g_k| (|h_o| r_v r_o + |s_k| |h_v| r_v q_v), o the other endpoint; a self
    pair counts once per role.  s: the float64 scores.  dot: r = 1 and no second term.  q_v = 1 / ||h_v|| (0 for a zero
    row): torch differentiates the norm under the clamp, so below eps the second term carries r_v q_v >= r_v^2; on every
    other row q_v = r_v and this is the r_v^2 of the term's usual form."""
    H, r = h.double().abs(), _rnorm(h, cosine, eps)
    nrm = h.double().norm(dim=1)
    q = torch.where(nrm > 0, 1.0 / nrm.clamp(min=1e-300), torch.zeros_like(nrm))
    a, b = index[0], index[1]
    ga = g.double().abs() * r[a] * r[b]
    M = torch.zeros_like(H)
    M.index_add_(0, a, ga[:, None] * H[b])
    M.index_add_(0, b, ga[:, None] * H[a])
    if cosine:
        t = g.double().abs() * s.double().abs()
        M.index_add_(0, a, (t * r[a] * q[a])[:, None] * H[a])
        M.index_add_(0, b, (t * r[b] * q[b])[:, None] * H[b])
    return M
