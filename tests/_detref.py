"""Host side of the deterministic-backward tests (tests/test_deterministic_host.py, tests/test_deterministic_gpu.py): the
NumPy restatement of the pull-form max backward in the engine's own summation order, its float64 evaluation in another
formulation (a scatter over the forward entries), and the graphs both files run on.  No device, no engine call.

The order restated: for source j the fp32 sum starts at +0 and takes the entries t of row j of the
transposed operator in stored order, each as acc = fma(w_t, [argmax[i_t, c] == pos_t] ? dy[i_t, c] : 0, acc).  A row
with more than hub_deg entries is cut into pieces of piece_edges entries; every piece is summed that way from +0 and the
pieces are then added, in piece order, to a second sum that starts at +0."""
import numpy as np


def _fma32(w, x, acc):
    """fma(w, x, acc) in fp32.  w = 1 (an unweighted graph): the plain fp32 add it is, exact.  Otherwise the product is
    formed exactly in float64 (24 + 24 significand bits) and added there, then rounded to fp32: the fused result up to
    a double rounding of the sum in rare cases — which is why only unweighted rows are held to this bit for bit."""
    if w == 1.0:
        return (acc + x).astype(np.float32)
    return (np.float64(w) * x.astype(np.float64) + acc.astype(np.float64)).astype(np.float32)


def max_bwd_pull_host(gt_rowptr, gt_col, gt_pos, val, argmax, dy, hub_deg=None, piece_edges=None, heads=1):
    """dx [n_src, d] fp32 of the pull-form max backward, walked as the kernel walks it.  gt_*: the transposed pattern
    (rowptr by source, col = destination, pos = forward entry); val: the FORWARD weights [nnz] (or [nnz, heads]: column
    c takes val[e, c // (d // heads)]) or None (ones); argmax [N, d] int32; dy [N, d] (taken as fp32).  hub_deg /
    piece_edges: the plan's tunables (None: no row is cut)."""
    gt_rowptr, gt_col, gt_pos = (np.asarray(a, dtype=np.int64) for a in (gt_rowptr, gt_col, gt_pos))
    argmax = np.asarray(argmax)
    dy = np.asarray(dy, dtype=np.float32)
    d = dy.shape[1]
    n_src = gt_rowptr.size - 1
    val = None if val is None else np.asarray(val, dtype=np.float32).reshape(gt_pos.size, -1)
    hw = d // heads
    dx = np.zeros((n_src, d), dtype=np.float32)
    zero = np.zeros(d, dtype=np.float32)

    def run(t0, t1):
        acc = zero.copy()
        for t in range(t0, t1):
            i, e = gt_col[t], gt_pos[t]
            m = np.where(argmax[i] == e, dy[i], zero)
            if val is None:
                acc = _fma32(1.0, m, acc)
            elif val.shape[1] == 1:
                acc = _fma32(float(val[e, 0]), m, acc)
            else:
                for h in range(heads):
                    cs = slice(h * hw, (h + 1) * hw)
                    acc[cs] = _fma32(float(val[e, h]), m[cs], acc[cs])
        return acc

    for j in range(n_src):
        t0, t1 = gt_rowptr[j], gt_rowptr[j + 1]
        if hub_deg is not None and t1 - t0 > hub_deg:
            acc = zero.copy()
            for p0 in range(t0, t1, piece_edges):
                acc = (acc + run(p0, min(p0 + piece_edges, t1))).astype(np.float32)
            dx[j] = acc
        else:
            dx[j] = run(t0, t1)
    return dx


def max_bwd_dense64(rows, cols, val, argmax, dy, n_src, heads=1, absolute=False):
    """the same gradient in float64 as a scatter over the FORWARD entries (rows / cols / val in CSR order): every (i, c)
    with a winner e = argmax[i, c] adds val[e] * dy[i, c] to dx[cols[e], c].  absolute: the sum of |terms| (the
    magnitude a cancelling sum is held to, tests/_tol.py rule (d))"""
    argmax = np.asarray(argmax).astype(np.int64)
    dy = np.asarray(dy, dtype=np.float64)
    N, d = dy.shape
    cols = np.asarray(cols, dtype=np.int64)
    hw = d // heads
    dx = np.zeros((n_src, d), dtype=np.float64)
    ii, cc = np.nonzero(argmax >= 0)
    e = argmax[ii, cc]
    if val is None:
        w = np.ones(e.size)
    else:
        v = np.asarray(val, dtype=np.float64).reshape(cols.size, -1)
        w = v[e, cc // hw] if v.shape[1] > 1 else v[e, 0]
    term = w * dy[ii, cc]
    np.add.at(dx, (cols[e], cc), np.abs(term) if absolute else term)
    return dx


def forward_max_host(rows, cols, val, x, N, heads=1):
    """argmax [N, d] int32 of y[i, c] = max_e val[e] * x[cols[e], c] over the entries of row i in CSR order, the first
    entry among equal candidates, -1 for an empty row (fp32 products, as the kernel forms them)"""
    x = np.asarray(x, dtype=np.float32)
    d = x.shape[1]
    hw = d // heads
    best = np.full((N, d), -np.inf, dtype=np.float32)
    arg = np.full((N, d), -1, dtype=np.int32)
    v = None if val is None else np.asarray(val, dtype=np.float32).reshape(len(cols), -1)
    for e in range(len(cols)):
        if v is None:
            m = x[cols[e]]
        elif v.shape[1] == 1:
            m = v[e, 0] * x[cols[e]]
        else:
            m = np.repeat(v[e], hw) * x[cols[e]]
        i = rows[e]
        win = m > best[i]
        best[i] = np.where(win, m, best[i])
        arg[i] = np.where(win, e, arg[i])
    return arg


def csr_host(dst, src, N):
    """(rows, cols, order) of the CSR of an edge list: entries sorted by (destination, source), input order kept among
    equal pairs; order: the input position of every entry"""
    order = np.lexsort((src, dst))
    return dst[order], src[order], order


def transpose_host(rows, cols, n_src):
    """(gt_rowptr, gt_col, gt_pos): the entries sorted by source, forward order kept within a source"""
    pos = np.argsort(cols, kind="stable")
    rp = np.zeros(n_src + 1, dtype=np.int64)
    np.cumsum(np.bincount(cols, minlength=n_src), out=rp[1:])
    return rp, rows[pos], pos


def reversed_rows(gt_rowptr, gt_col, gt_pos):
    """the transposed entries with every row's entries in the opposite order: another summation order of the same terms"""
    col, pos = np.array(gt_col), np.array(gt_pos)
    for j in range(len(gt_rowptr) - 1):
        a, b = int(gt_rowptr[j]), int(gt_rowptr[j + 1])
        col[a:b], pos[a:b] = col[a:b][::-1].copy(), pos[a:b][::-1].copy()
    return col, pos


# ---- the graphs -------------------------------------------------------------------------------------------------------
GRAPHS = ("multi", "empty_dst", "no_out", "star", "symmetric", "rect")
STAR_PLAN = (64, 1, 64, 64)          # seg_cost, row_cost, hub_deg, piece_edges: the star's centre takes the hub path


def edges(kind, seed=0):
    """(dst, src, N, w): int64 edge lists and one fp32 weight per edge of small graphs that reach every branch.
      multi       a random directed multigraph, one edge in three listed twice or more (equal messages: the first wins)
      empty_dst   destinations 0 mod 5 receive nothing (argmax = -1 rows)
      no_out      sources 0 mod 4 send nothing (empty rows of the transposed operator)
      star        node 0 sends to 300 destinations (more out-entries than STAR_PLAN's hub_deg), each of which also
                  hears two others
      symmetric   an undirected simple graph, both directions stored, weights equal in both (the caller flags it)
      rect        `multi`; the caller takes a row subset of it (num_cols != num_nodes)
    The weights are a function of the unordered pair, so that `symmetric` stays symmetric and duplicates stay equal."""
    g = np.random.default_rng(100 + seed)
    if kind in ("multi", "rect", "empty_dst", "no_out"):
        N, E = 90, 700
        dst, src = g.integers(0, N, E), g.integers(0, N, E)
        if kind == "empty_dst":
            dst = np.where(dst % 5 == 0, dst + 1, dst)
        if kind == "no_out":
            src = np.where(src % 4 == 0, src + 1, src)
        rep = g.integers(0, E, E // 3)
        dst, src = np.concatenate([dst, dst[rep], dst[rep[:40]]]), np.concatenate([src, src[rep], src[rep[:40]]])
    elif kind == "star":
        N = 320
        leaves = np.arange(1, 301)
        dst = np.concatenate([leaves, leaves, leaves, g.integers(0, N, 200)])
        src = np.concatenate([np.zeros(300, dtype=np.int64), g.integers(1, N, 300), g.integers(1, N, 300),
                              g.integers(1, N, 200)])
    elif kind == "symmetric":
        N = 80
        a, b = g.integers(0, N, 400), g.integers(0, N, 400)
        keep = a != b
        key = np.unique(np.minimum(a, b)[keep] * N + np.maximum(a, b)[keep])
        lo, hi = key // N, key % N
        dst, src = np.concatenate([lo, hi]), np.concatenate([hi, lo])
    else:
        raise KeyError(kind)
    lo, hi = np.minimum(dst, src), np.maximum(dst, src)
    w = (0.25 + ((lo * 7919 + hi * 104729) % 1000) / 500.0).astype(np.float32)
    return dst.astype(np.int64), src.astype(np.int64), int(N), w


def spread_dy(shape, seed=0):
    """an incoming gradient with magnitudes spread over 2^20 and both signs: a sum of a few of them in another order
    rounds differently"""
    g = np.random.default_rng(200 + seed)
    mant = 1.0 + g.random(shape)
    return (np.where(g.random(shape) < 0.5, -1.0, 1.0) * mant * np.exp2(g.uniform(-10, 10, shape))).astype(np.float32)


def features(n, d, seed=0, boost=()):
    """x [n, d] fp32 in [-1, 1); the rows in `boost` lifted by 3 so that they win every destination they reach — many
    destinations won by one source, whose gradient row is then a long sum"""
    g = np.random.default_rng(300 + seed)
    x = (g.random((n, d)) * 2 - 1).astype(np.float32)
    for j in boost:
        x[j] += 3.0
    return x
