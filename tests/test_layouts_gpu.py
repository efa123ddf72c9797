"""The fp32 kernels on strided, offset and misaligned operand views.

Every fp32 entry point picks its kernel form on the host from the width, the leading dimensions and the alignment of
the base pointers.  Here each operator runs on column slices of wider buffers (tests/_layout.py: LAYOUTS, plus the mixed
cases where one operand alone is misaligned) and every case asserts
  1. the result against the float64 evaluation of the same formula on the same fp32 inputs (tests/_tol.py);
  2. the result against the same call on contiguous operands — bit for bit where the summation order cannot depend on
     the kernel form (the plan aggregation, max / argmax, row gather and scatter, the identity fix-up), and on the
     layouts with 16-byte aligned rows (the same form as the contiguous call) everywhere else;
  3. that nothing beside an output slice was written (a sentinel bit pattern around it);
  4. that the inputs keep their bits."""
import ctypes as C

import pytest
import torch

import graphgym_amd as ga
from graphgym_amd import _lib, ops
from graphgym_amd._lib import check, ptr
from graphgym_amd.graph import _stream
from _layout import (ALIGNED, CONTIG, LAYOUTS, OFF1, Unchanged, assert_all_sentinel, assert_untouched, assert_written,
                     out_view, same_bits, view_of)
from _tol import both, close, close_all
from oracle import ref_ops as R

pytestmark = pytest.mark.gpu

SUM, MEAN, MAX = _lib.SUM, _lib.MEAN, _lib.MAX
MP_ERR_ALIGNMENT = 5


@pytest.fixture(autouse=True)
def small_graphs_on_the_plan_kernel(monkeypatch):
    monkeypatch.setenv("MP_AGG_TILES", "0")       # the tile tests switch it on themselves
    monkeypatch.setenv("MP_X3", "1")
    monkeypatch.setenv("MP_FUSED", "1")


def assignments(names, layouts=LAYOUTS):
    """(tag, {operand: layout}): every layout on all operands, then each operand alone misaligned — the kernels' width
    choice is an AND over the operands, and a term dropped from it shows in exactly one of the mixed cases"""
    for lay in layouts:
        yield lay[0], {k: lay for k in names}
    if len(names) > 1:
        for k in names:
            yield f"only {k} off", {j: (OFF1 if j == k else CONTIG) for j in names}


def aligned(lay, names=None):
    return all(lay[k][0] in ALIGNED for k in (names or lay))


def graph(dev, n, E, seed, weighted, hubs=True, n_cols=None):
    g = torch.Generator().manual_seed(seed)
    dst = torch.randint(0, n, (E,), generator=g)
    src = torch.randint(0, n, (E,), generator=g)
    if hubs:                                       # rows far beyond hub_deg: cut into pieces
        k = E // 3
        dst[:k] = torch.randint(0, 3, (k,), generator=g) * 7 + 5
    keep = dst % 13 != 4                           # empty rows
    dst, src = dst[keep], src[keep]
    w = (torch.rand(dst.numel(), generator=g) - 0.3) if weighted else None
    G = ga.CSRGraph.from_edge_index(torch.stack([dst, src]).to(dev), n, None if w is None else w.to(dev), dst_row=0)
    return G, dst, src, w


def csr(G):
    """(rows, cols, val or None) of the stored entries in CSR order, on the host"""
    return G.row_ids().cpu().long(), G.col.cpu().long(), None if G.val is None else G.val.cpu()


def vec_of(t, off, dev):
    """a 1-D operand (bias, scale) at element offset `off` of a longer device vector"""
    buf = torch.randn(t.numel() + 4, generator=torch.Generator().manual_seed(t.numel())).to(dev)
    v = buf[off:off + t.numel()]
    v.copy_(t)
    assert v.data_ptr() % 16 == (4 * off) % 16
    return buf, v


def finite(v, what):
    assert bool(torch.isfinite(v).all()), f"{what}: non-finite values in the result"


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------ 1. plan aggregation
def agg_ref(c, dst, src, w, x, S, self_scale, b, relu, red, n, absolute=False):
    a = (lambda t: c(t).abs()) if absolute else c
    r = R.coo_aggregate(dst, src, None if w is None else a(w), a(x), n, red)
    if S is not None:
        r = r + abs(self_scale) * a(S) if absolute else r + self_scale * a(S)
    if b is not None:
        r = r + a(b)
    return torch.relu(r) if (relu and not absolute) else r


AGG_CASES = [   # reduce, weighted, self_scale, bias, relu
    ("sum", True, 1.5, True, True), ("sum", False, 0.0, False, False), ("mean", True, 0.0, False, False),
    ("mean", False, 0.5, True, True), ("max", True, 0.0, False, False), ("max", False, 1.25, True, True)]


@pytest.mark.parametrize("d", [3, 8, 64, 100, 128, 256, 260])
@pytest.mark.parametrize("case", AGG_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_plan_aggregation(dev, monkeypatch, d, case):
    """mp_spmm_csr_f32 through ops._raw_spmm with x, S, out and bias as slices: each column sums its row's entries in
    entry order and hub pieces in piece order whatever the lane width, so every layout gives the contiguous call's bits"""
    reduce, weighted, self_scale, has_bias, relu = case
    monkeypatch.setattr(ga.CSRGraph, "PLAN_CONFIG", (64, 1, 64, 64))
    n = 300
    G, dst, src, w = graph(dev, n, 4000, d * 31 + len(reduce), weighted)
    assert G.plan()[1][1] > 0                                       # hub pieces and the finalize kernel run
    x = rnd(n, d, seed=d)
    s = rnd(n, d, seed=d + 1) if self_scale else None
    b = rnd(d, seed=d + 2) if has_bias else None
    red = _lib.REDUCE[reduce]
    refs = both(lambda c: agg_ref(c, dst, src, w, x, s, self_scale, b, relu, reduce, n))
    mag = both(lambda c: agg_ref(c, dst, src, w, x, s, self_scale, b, relu, reduce, n, absolute=True))[0]
    names = ["x", "out"] + (["s"] if s is not None else []) + (["bias"] if has_bias else [])
    base = None
    for tag, lay in assignments(names):
        what = f"{reduce} d={d} [{tag}]"
        xb, xv = view_of(x, lay["x"], dev)
        sb, sv = view_of(s, lay["s"], dev, 1) if s is not None else (None, None)
        ob, ov = out_view(n, d, lay["out"], dev)
        bb, bv = vec_of(b, 1 if lay["bias"] is OFF1 else 0, dev) if has_bias else (None, None)
        with Unchanged(xb, sb, bb):
            y, arg = ops._raw_spmm(G, xv, red, S=sv, self_scale=self_scale, bias=bv, relu=relu,
                                   want_argmax=reduce == "max", out=ov)
        assert y is ov
        assert_untouched(ob, lay["out"][2], d, what)
        assert_written(ov, what)
        finite(ov, what)
        close(ov, refs, what=what, mag=mag)
        if base is None:
            base = (ov.clone(), arg)
            if reduce == "max":
                rows, cols, val = csr(G)
                assert torch.equal(arg.cpu().long(), R.coo_aggregate_argmax(rows, cols, val, x, n)), what
        else:
            assert same_bits(ov, base[0]), what
            assert arg is None or torch.equal(arg, base[1]), what


@pytest.mark.parametrize("d", [64, 100, 256])
def test_fused_eval_epilogue_on_a_view(dev, monkeypatch, d):
    monkeypatch.setattr(ga.CSRGraph, "PLAN_CONFIG", (64, 1, 64, 64))
    n = 300
    G, dst, src, w = graph(dev, n, 4000, d + 7, True)
    assert G.plan()[1][1] > 0
    x, cs, ct = rnd(n, d, seed=d), torch.rand(d, generator=torch.Generator().manual_seed(d)) + 0.5, rnd(d, seed=d + 3)

    def ref(c, l2, absolute=False):
        a = (lambda t: c(t).abs()) if absolute else c
        r = (R.coo_aggregate(dst, src, a(w), a(x), n, "sum") + 0.5 * a(x)) * a(cs) + a(ct)
        if absolute:
            return r
        r = torch.relu(r)
        return torch.nn.functional.normalize(r, p=2, dim=-1, eps=1e-12) if l2 else r
    for l2 in (False, True):
        refs = both(lambda c: ref(c, l2))
        mag = None if l2 else both(lambda c: ref(c, l2, True))[0]
        base = None
        for lay in LAYOUTS:
            what = f"fused eval d={d} l2={l2} [{lay[0]}]"
            xb, xv = view_of(x, lay, dev)
            with Unchanged(xb):
                y = ops.spmm_fused_eval(G, xv, "sum", self_scale=0.5, col_scale=cs.to(dev), col_shift=ct.to(dev),
                                        relu=True, l2norm=l2)
            finite(y, what)
            close(y, refs, what=what, mag=mag)
            if base is None:
                base = y
            elif not l2:      # (the row norm is a wave reduction or a library pass depending on the width: 1 only)
                assert same_bits(y, base), what


def abi_idgnn(G, ids, xv, Pv, Qv):
    d = xv.size(1)
    plan, counts, ws, nb = ops._plan_ws(G, xv.device, d, SUM, True)
    check(_lib.lib().mp_idgnn_agg_f32(ptr(G.rowptr), ptr(G.mark_ids(ids)), ptr(G.val), G.num_nodes, ptr(plan), counts,
                                      ptr(xv), xv.stride(0), ptr(Pv), Pv.stride(0), ptr(Qv), Qv.stride(0), d, ptr(ws),
                                      nb, _stream()), "mp_idgnn_agg_f32")


@pytest.mark.parametrize("d", [3, 64, 100, 256])
def test_two_branch_aggregation_on_views(dev, monkeypatch, d):
    """ops.idgnn_aggregate on a view of x, and mp_idgnn_agg_f32 itself with P and Q as slices"""
    monkeypatch.setattr(ga.CSRGraph, "PLAN_CONFIG", (64, 1, 64, 64))
    n = 300
    G, dst, src, w = graph(dev, n, 4000, d + 11, True)
    assert G.plan()[1][1] > 0
    x = rnd(n, d, seed=d)
    ids = torch.randperm(n, generator=torch.Generator().manual_seed(d))[: n // 9]
    sel = torch.zeros(n, 1)
    sel[ids] = 1
    refP = both(lambda c: R.coo_aggregate(dst, src, c(w), c(x), n, "sum"))
    refQ = both(lambda c: R.coo_aggregate(dst, src, c(w), c(x * sel), n, "sum"))
    magP = R.coo_aggregate(dst, src, w.double().abs(), x.double().abs(), n, "sum")
    magQ = R.coo_aggregate(dst, src, w.double().abs(), (x * sel).double().abs(), n, "sum")
    idd = ids.to(dev)
    base = None
    for tag, lay in assignments(["x", "P", "Q"]):
        what = f"two-branch d={d} [{tag}]"
        xb, xv = view_of(x, lay["x"], dev)
        Pb, Pv = out_view(n, d, lay["P"], dev)
        Qb, Qv = out_view(n, d, lay["Q"], dev)
        with Unchanged(xb):
            abi_idgnn(G, idd, xv, Pv, Qv)
            P2, Q2 = ops.idgnn_aggregate(G, idd, xv)
        for bf, v, lk, refs, mag in ((Pb, Pv, "P", refP, magP), (Qb, Qv, "Q", refQ, magQ)):
            assert_untouched(bf, lay[lk][2], d, what)
            assert_written(v, what)
            close(v, refs, what=f"{what} {lk}", mag=mag)
        assert same_bits(P2, Pv) and same_bits(Q2, Qv), what
        if base is None:
            base = (Pv.clone(), Qv.clone())
        else:
            assert same_bits(Pv, base[0]) and same_bits(Qv, base[1]), what


def heads_ref(c, a, V, rows, cols, n, dh, reduce, absolute=False):
    f = (lambda t: c(t).abs()) if absolute else c
    msg = f(a).repeat_interleave(dh, dim=1) * f(V)[cols]
    d = msg.size(1)
    if reduce == "max":
        return torch.zeros(n, d, dtype=msg.dtype).scatter_reduce(0, rows[:, None].expand(-1, d), msg, "amax",
                                                                 include_self=False)
    out = torch.zeros(n, d, dtype=msg.dtype).index_add_(0, rows, msg)
    if reduce == "mean":
        out = out / torch.bincount(rows, minlength=n).clamp(min=1).to(msg.dtype)[:, None]
    return out


def heads_argmax(a, V, rows, cols, n, dh):
    """the first entry in CSR order that attains the float32 maximum of a[e, h] * V[col_e, c], -1 for an empty row"""
    msg = a.repeat_interleave(dh, dim=1) * V[cols]
    d = msg.size(1)
    idx = rows[:, None].expand(-1, d)
    best = torch.full((n, d), float("-inf")).scatter_reduce(0, idx, msg, "amax", include_self=True)
    e = torch.arange(rows.numel())[:, None].expand(-1, d)
    cand = torch.where(msg == best[rows], e, torch.full_like(e, 1 << 40))
    arg = torch.full((n, d), 1 << 40, dtype=torch.int64).scatter_reduce(0, idx, cand, "amin", include_self=True)
    return torch.where(arg == (1 << 40), torch.full_like(arg, -1), arg)


HEAD_SHAPES = [(2, 1), (2, 3), (2, 32), (4, 2), (4, 6), (8, 4), (8, 32), (3, 2), (3, 4), (3, 32), (6, 1), (6, 6)]


@pytest.mark.parametrize("heads,dh", HEAD_SHAPES)
def test_multi_head_aggregation_on_views(dev, monkeypatch, heads, dh):
    """_raw_spmm_heads / _raw_spmm_heads_reduce with V a slice: one launch for 2 / 4 / 8 heads (a lane's columns must stay
    inside a head: d / heads bounds the width), per-head column slices — offset views themselves — for 3 / 6"""
    monkeypatch.setattr(ga.CSRGraph, "PLAN_CONFIG", (64, 1, 64, 64))
    n, d = 300, heads * dh
    G, *_ = graph(dev, n, 4000, heads * 100 + dh, False)
    assert G.plan()[1][1] > 0
    rows, cols, _ = csr(G)
    a = torch.rand(G.nnz, heads, generator=torch.Generator().manual_seed(dh)) - 0.3
    V = rnd(n, d, seed=d)
    ad = a.to(dev)
    for reduce in ("sum", "mean", "max"):
        refs = both(lambda c: heads_ref(c, a, V, rows, cols, n, dh, reduce))
        mag = both(lambda c: heads_ref(c, a, V, rows, cols, n, dh, reduce, True))[0]
        base = None
        for lay in LAYOUTS:
            what = f"heads={heads} dh={dh} {reduce} [{lay[0]}]"
            Vb, Vv = view_of(V, lay, dev)
            with Unchanged(Vb):
                if reduce == "sum":
                    y, arg = ops._raw_spmm_heads(G, ad, Vv, heads), None
                else:
                    y, arg = ops._raw_spmm_heads_reduce(G, ad, Vv, heads, _lib.REDUCE[reduce])
            finite(y, what)
            close(y, refs, what=what, mag=mag)
            if base is None:
                base = (y, arg)
                if reduce == "max":
                    assert torch.equal(arg.cpu().long(), heads_argmax(a, V, rows, cols, n, dh)), what
            else:
                assert same_bits(y, base[0]), what
                assert arg is None or torch.equal(arg, base[1]), what


@pytest.mark.parametrize("d,heads", [(3, 1), (64, 1), (100, 1), (6, 2), (64, 4)])
def test_max_backward_scatter_on_views(dev, d, heads):
    """mp_spmm_max_bwd_f32 / mp_spmm_heads_max_bwd_f32 with dY and dX / dV as slices (float atomics: assertion 1 only)"""
    n = 300
    G, *_ = graph(dev, n, 4000, d + heads, heads == 1)
    rows, cols, val = csr(G)
    x, dy = rnd(n, d, seed=d), rnd(n, d, seed=d + 1)
    L = _lib.lib()
    if heads == 1:
        _, arg = ops._raw_spmm(G, x.to(dev), MAX, want_argmax=True)
        wcol = val[:, None].expand(-1, d)
    else:
        a = torch.rand(G.nnz, heads, generator=torch.Generator().manual_seed(d)) + 0.1
        _, arg = ops._raw_spmm_heads_reduce(G, a.to(dev), x.to(dev), heads, MAX)
        wcol = a.repeat_interleave(d // heads, dim=1)
    ar = arg.cpu().long()
    r, c = torch.nonzero(ar >= 0, as_tuple=True)
    e = ar[r, c]
    terms = wcol.double()[e, c] * dy.double()[r, c]
    ref = torch.zeros(n, d, dtype=torch.float64).index_put_((cols[e], c), terms, accumulate=True)
    mag = torch.zeros(n, d, dtype=torch.float64).index_put_((cols[e], c), terms.abs(), accumulate=True)
    for tag, lay in assignments(["dy", "dx"]):
        what = f"max backward d={d} heads={heads} [{tag}]"
        yb, yv = view_of(dy, lay["dy"], dev)
        xb, xv = out_view(n, d, lay["dx"], dev)
        xv.zero_()
        with Unchanged(yb, arg):
            if heads == 1:
                check(L.mp_spmm_max_bwd_f32(ptr(G.col), ptr(G.val), ptr(arg), ptr(yv), yv.stride(0), n, d, ptr(xv),
                                            xv.stride(0), _stream()), what)
            else:
                ad = a.to(dev)
                check(L.mp_spmm_heads_max_bwd_f32(ptr(G.col), ptr(ad), heads, ptr(arg), n, d, ptr(yv), yv.stride(0),
                                                  ptr(xv), xv.stride(0), _stream()), what)
        assert_untouched(xb, lay["dx"][2], d, what)
        finite(xv, what)
        close(xv, ref, what=what, mag=mag)


# ------------------------------------------------------------------------ 2. tile kernels and the one-kernel layer
@pytest.mark.parametrize("d", ops.AGG_TILES_WIDTHS)
@pytest.mark.parametrize("reduce,weighted,self_scale", [("sum", True, 1.5), ("mean", False, 0.0), ("max", True, 0.0)])
def test_tile_aggregation_is_taken_only_on_aligned_rows(dev, monkeypatch, d, reduce, weighted, self_scale):
    """a view with 16-byte aligned rows still takes mp_agg_rows_tiles_f32; any misaligned operand goes to the plan kernel
    (and gives its bits) instead of an MP_ERR_ALIGNMENT"""
    n = 1500
    G, dst, src, w = graph(dev, n, 20000, d + len(reduce), weighted)
    x = rnd(n, d, seed=d)
    s = rnd(n, d, seed=d + 1) if self_scale else None
    red = _lib.REDUCE[reduce]
    refs = both(lambda c: agg_ref(c, dst, src, w, x, s, self_scale, None, False, reduce, n))
    mag = both(lambda c: agg_ref(c, dst, src, w, x, s, self_scale, None, False, reduce, n, absolute=True))[0]
    y_plan, _ = ops._raw_spmm(G, x.to(dev), red, S=None if s is None else s.to(dev), self_scale=self_scale)
    monkeypatch.setenv("MP_AGG_TILES", "1")
    monkeypatch.setattr(ops, "AGG_TILES_MIN_ROWS", 1)
    names = ["x", "out"] + (["s"] if s is not None else [])
    base = None
    for tag, lay in assignments(names):
        what = f"tiles {reduce} d={d} [{tag}]"
        xb, xv = view_of(x, lay["x"], dev)
        sb, sv = view_of(s, lay["s"], dev, 1) if s is not None else (None, None)
        ob, ov = out_view(n, d, lay["out"], dev)
        before = ops.AGG_TILES_CALLS
        with Unchanged(xb, sb):
            ops._raw_spmm(G, xv, red, S=sv, self_scale=self_scale, out=ov)
        tiles = aligned(lay)
        assert ops.AGG_TILES_CALLS == before + (1 if tiles else 0), what
        assert_untouched(ob, lay["out"][2], d, what)
        assert_written(ov, what)
        close(ov, refs, what=what, mag=mag)
        if not tiles or reduce == "max":        # (a maximum is the plan kernel's bit for bit on either structure)
            assert same_bits(ov, y_plan), what
        elif base is None:
            base = ov.clone()
        else:                                   # one tile form, rows cut between waves at the same places
            assert same_bits(ov, base), what


@pytest.mark.parametrize("d", [128, 256])
def test_two_branch_tiles_are_taken_only_on_aligned_rows(dev, monkeypatch, d):
    n = 1500
    G, dst, src, w = graph(dev, n, 20000, d + 3, True)
    x = rnd(n, d, seed=d)
    ids = torch.randperm(n, generator=torch.Generator().manual_seed(d))[:150]
    sel = torch.zeros(n, 1)
    sel[ids] = 1
    idd = ids.to(dev)
    refP = both(lambda c: R.coo_aggregate(dst, src, c(w), c(x), n, "sum"))
    refQ = both(lambda c: R.coo_aggregate(dst, src, c(w), c(x * sel), n, "sum"))
    magQ = R.coo_aggregate(dst, src, w.double().abs(), (x * sel).double().abs(), n, "sum")
    P0, Q0 = ops.idgnn_aggregate(G, idd, x.to(dev))                     # the plan kernel
    monkeypatch.setenv("MP_AGG_TILES", "1")
    monkeypatch.setattr(ops, "AGG_TILES_MIN_ROWS", 1)
    base = None
    for lay in LAYOUTS:
        what = f"two-branch tiles d={d} [{lay[0]}]"
        xb, xv = view_of(x, lay, dev)
        before = ops.AGG_TILES_CALLS
        with Unchanged(xb):
            P, Q = ops.idgnn_aggregate(G, idd, xv)
        tiles = lay[0] in ALIGNED
        assert ops.AGG_TILES_CALLS == before + (1 if tiles else 0), what
        close(P, refP, what=what + " P")
        close(Q, refQ, what=what + " Q", mag=magQ)
        if not tiles:
            assert same_bits(P, P0) and same_bits(Q, Q0), what
        elif base is None:
            base = (P, Q)
        else:
            assert same_bits(P, base[0]) and same_bits(Q, base[1]), what


@pytest.mark.parametrize("F,dout", [(64, 32), (256, 64)])
def test_one_kernel_layer_is_taken_only_on_aligned_rows(dev, F, dout):
    """agg_dense_supported turns a misaligned x down and ops.agg_dense then runs the aggregation and the transform as
    two kernels: the same layer either way"""
    n = 1200
    G, dst, src, w = graph(dev, n, 15000, F, True)
    x, W, b = rnd(n, F, seed=F), rnd(F, dout, seed=F + 1) / F ** 0.5, rnd(dout, seed=F + 2)
    Wd, bd = W.to(dev), b.to(dev)

    def ref(c, absolute=False):
        a = (lambda t: c(t).abs()) if absolute else c
        r = (R.coo_aggregate(dst, src, a(w), a(x), n, "sum") + 0.5 * a(x)) @ a(W) + a(b)
        return r if absolute else torch.relu(r)
    refs, mag = both(ref), both(lambda c: ref(c, True))[0]
    for lay in LAYOUTS:
        what = f"one-kernel layer F={F} [{lay[0]}]"
        xb, xv = view_of(x, lay, dev)
        assert ops.agg_dense_supported(G, xv, Wd) == (lay[0] in ALIGNED), what
        with Unchanged(xb), torch.no_grad():
            out = ops.agg_dense(G, xv, Wd, bias=bd, relu=True, self_scale=0.5)
        finite(out, what)
        close(out, refs, what=what, mag=mag)


DENSE_INTO = [(700, 64, 128), (700, 96, 64), (300, 72, 100), (300, 13, 33)]    # the first two: the streaming kernel's


@pytest.mark.parametrize("M,K,n", DENSE_INTO)
def test_dense_into_a_view(dev, monkeypatch, M, K, n):
    """_dense_into: the streaming kernel when P and the output slice have 16-byte aligned rows, mp_dense_fused_f32 (scalar
    stores: any output alignment) otherwise"""
    monkeypatch.setattr(ops, "X3_MIN_ROWS", 1)
    P, W, b = rnd(M, K, seed=K), rnd(K, n, seed=K + 1) / 8, rnd(n, seed=K + 2)
    Wd = W.to(dev)
    refs = both(lambda c: torch.relu(c(P) @ c(W) + c(b)))
    mag = P.double().abs() @ W.double().abs() + b.double().abs()
    for tag, lay in assignments(["P", "out", "bias"]):
        what = f"dense into M={M} K={K} n={n} [{tag}]"
        Pb, Pv = view_of(P, lay["P"], dev)
        ob, ov = out_view(M, n, lay["out"], dev)
        bb, bv = vec_of(b, 1 if lay["bias"] is OFF1 else 0, dev)
        x3 = ops.dense_x3_supported(Pv, K, n, ov)
        assert x3 == (n in ops.X3_WIDTHS and K % 32 == 0 and aligned(lay, ["P", "out"])), what
        with Unchanged(Pb, bb):
            ops._dense_into(ov, Pv, Wd, bv, True)
        assert_untouched(ob, lay["out"][2], n, what)
        assert_written(ov, what)
        close(ov, refs, what=what, mag=mag)


def test_kernels_that_need_alignment_refuse_misaligned_operands(dev):
    """mp_agg_rows_tiles_f32, mp_idgnn_agg_tiles_f32, mp_agg_dense_f32 and mp_dense_x3_f32 called directly: each
    misaligned operand is MP_ERR_ALIGNMENT and the outputs keep the sentinel; the aligned call is MP_OK"""
    L = _lib.lib()
    n, F, dout = 500, 256, 64
    G, *_ = graph(dev, n, 6000, 17, True)
    x, s = rnd(n, F, seed=1), rnd(n, F, seed=2)
    W = (rnd(F, dout, seed=3) / 16).to(dev)
    Wsp = ops._split_w(W)
    b = rnd(dout, seed=4)
    off = [OFF1, LAYOUTS[7]]                    # a 4-byte aligned base; an aligned base with an odd leading dimension

    def each(names):
        yield "aligned", {k: LAYOUTS[1] for k in names}, 0
        for k in names:
            for bad in off:
                yield f"{k} {bad[0]}", {j: (bad if j == k else CONTIG) for j in names}, MP_ERR_ALIGNMENT

    for tag, lay, want in each(["x", "s", "out"]):
        (_, xv), (_, sv), (ob, ov) = view_of(x, lay["x"], dev), view_of(s, lay["s"], dev), out_view(n, F, lay["out"], dev)
        st = L.mp_agg_rows_tiles_f32(ptr(G.rowptr), ptr(G.col), ptr(G.val), n, SUM, ptr(xv), xv.stride(0), F, ptr(sv),
                                     sv.stride(0), 0.5, ptr(ov), ov.stride(0), _stream())
        torch.cuda.synchronize()
        assert st == want, f"mp_agg_rows_tiles_f32 [{tag}]"
        if want:
            assert_all_sentinel(ob, f"mp_agg_rows_tiles_f32 [{tag}]")
    for tag, lay, want in each(["x", "P", "Q"]):
        (_, xv), (Pb, Pv), (Qb, Qv) = view_of(x, lay["x"], dev), out_view(n, F, lay["P"], dev), out_view(n, F, lay["Q"], dev)
        st = L.mp_idgnn_agg_tiles_f32(ptr(G.rowptr), ptr(G.col), ptr(G.val), n, ptr(xv), xv.stride(0), F, None, None, None,
                                      None, None, 0, None, 0, ptr(Pv), Pv.stride(0), ptr(Qv), Qv.stride(0), _stream())
        torch.cuda.synchronize()
        assert st == want, f"mp_idgnn_agg_tiles_f32 [{tag}]"
        if want:
            assert_all_sentinel(Pb, tag), assert_all_sentinel(Qb, tag)
    for tag, lay, want in each(["x", "s", "P", "out", "bias"]):
        (_, xv), (_, sv) = view_of(x, lay["x"], dev), view_of(s, lay["s"], dev)
        (Pb, Pv), (ob, ov) = out_view(n, F, lay["P"], dev), out_view(n, dout, lay["out"], dev)
        _, bv = vec_of(b, 0 if lay["bias"] in (CONTIG, LAYOUTS[1]) else 1, dev)
        if tag == "out ld+1":                   # (the output needs 8 bytes: an odd leading dimension breaks that too)
            assert ov.stride(0) % 2 == 1
        st = L.mp_agg_dense_f32(ptr(G.rowptr), ptr(G.col), ptr(G.val), n, SUM, ptr(xv), xv.stride(0), F, ptr(sv),
                                sv.stride(0), 0.5, ptr(W), W.stride(0), dout, ptr(bv), _lib.ACT_RELU, None, ptr(Pv),
                                Pv.stride(0), ptr(ov), ov.stride(0), None, _stream())
        torch.cuda.synchronize()
        assert st == want, f"mp_agg_dense_f32 [{tag}]"
        if want:
            assert_all_sentinel(Pb, tag), assert_all_sentinel(ob, tag)
    for tag, lay, want in each(["P", "out"]):
        (_, Pv), (ob, ov) = view_of(x, lay["P"], dev), out_view(n, dout, lay["out"], dev)
        st = L.mp_dense_x3_f32(ptr(Pv), Pv.stride(0), ptr(Wsp), None, _lib.ACT_NONE, ptr(ov), ov.stride(0), n, F, dout,
                               _stream())
        torch.cuda.synchronize()
        assert st == want, f"mp_dense_x3_f32 [{tag}]"
        if want:
            assert_all_sentinel(ob, f"mp_dense_x3_f32 [{tag}]")


# ------------------------------------------------------------------------------------------------------ 3. SDDMM
SDDMM_SHAPES = [(1, 1), (1, 32), (1, 100), (1, 256), (1, 300), (1, 1024),      # heads = 1: any width, several column tiles
                (4, 256), (8, 128), (2, 64), (2, 8),                           # one launch at lane widths 4, 2, 1
                (4, 24), (2, 512)]                                             # head layouts of the row kernel


@pytest.mark.parametrize("heads,d", SDDMM_SHAPES)
def test_sddmm_dot_on_views(dev, heads, d):
    """ops._raw_sddmm_dot with A and B as slices.  A lane's share of a dot product, and so the order of its sum, changes
    with the lane width: bit equality only on the layouts that keep the contiguous call's width"""
    n = 200
    G, *_ = graph(dev, n, 3000, 5, False)
    assert G.nnz % 64 and G.nnz % 256
    rows, cols, _ = csr(G)
    A, B = rnd(n, d, seed=d), rnd(n, d, seed=d + 1)
    dh = d // heads

    def ref(c, absolute=False):
        a = (lambda t: c(t).abs()) if absolute else c
        return (a(A)[rows].view(-1, heads, dh) * a(B)[cols].view(-1, heads, dh)).sum(-1) * 0.5
    refs, mag = both(ref), both(lambda c: ref(c, True))[0]
    base = None
    for tag, lay in assignments(["A", "B"]):
        what = f"sddmm heads={heads} d={d} [{tag}]"
        Ab, Av = view_of(A, lay["A"], dev)
        Bb, Bv = view_of(B, lay["B"], dev, 1)
        with Unchanged(Ab, Bb):
            s = ops._raw_sddmm_dot(G, Av, Bv, heads, 0.5)
        finite(s, what)
        close(s, refs, what=what, mag=mag)
        if base is None:
            base = s
        elif aligned(lay):
            assert same_bits(s, base), what


@pytest.mark.parametrize("heads,d", [(1, 100), (1, 256), (2, 64), (4, 256), (8, 128), (4, 24), (2, 512)])
def test_heads_max_da_on_views(dev, heads, d):
    """ops._raw_heads_max_da with argmax, dy and V as slices, and its per-head slice fallback ((4, 24), (2, 512));
    lanes per head follow the lane width, so bit equality holds on the aligned layouts only"""
    n = 200
    G, *_ = graph(dev, n, 3000, 3, False)
    rows, cols, _ = csr(G)
    dh = d // heads
    a = torch.rand(G.nnz, heads, generator=torch.Generator().manual_seed(d)) + 0.1
    V, dy = rnd(n, d, seed=d), rnd(n, d, seed=d + 1)
    _, arg = ops._raw_spmm_heads_reduce(G, a.to(dev), V.to(dev), heads, MAX)
    arg = arg.cpu()
    won = arg.long()[rows] == torch.arange(G.nnz)[:, None]                   # [nnz, d]: entry e won column c of its row

    def ref(c, absolute=False):
        f = (lambda t: c(t).abs()) if absolute else c
        return (f(dy)[rows] * f(V)[cols] * won.to(c(dy).dtype)).view(-1, heads, dh).sum(-1)
    refs, mag = both(ref), both(lambda c: ref(c, True))[0]
    base = None
    for tag, lay in assignments(["argmax", "dy", "V"]):
        what = f"max da heads={heads} d={d} [{tag}]"
        mb, mv = view_of(arg, lay["argmax"], dev)
        yb, yv = view_of(dy, lay["dy"], dev, 1)
        Vb, Vv = view_of(V, lay["V"], dev, 2)
        with Unchanged(mb, yb, Vb):
            da = ops._raw_heads_max_da(G, mv, yv, Vv, heads)
        finite(da, what)
        close(da, refs, what=what, mag=mag)
        if base is None:
            base = da
        elif aligned(lay):
            assert same_bits(da, base), what


# -------------------------------------------------------------------------- 4. dense transform and its gradients
@pytest.mark.parametrize("M,F,d", [(300, 64, 128), (129, 72, 100), (200, 13, 33)])
@pytest.mark.parametrize("dual", [False, True])
def test_dense_fused_on_views(dev, M, F, d, dual):
    """_raw_dense_fused with P and Q as slices (the 16-byte and the scalar loaders; the same products either way, but
    nothing promises the bits across the two: bit equality on the aligned layouts only)"""
    P, Q = rnd(M, F, seed=F), rnd(M, F, seed=F + 1)
    W, Wi, b = rnd(F, d, seed=F + 2) / F ** 0.5, rnd(F, d, seed=F + 3) / F ** 0.5, rnd(d, seed=F + 4)
    Wd, Wid, bd = W.to(dev), Wi.to(dev), b.to(dev)

    def ref(c, absolute=False):
        a = (lambda t: c(t).abs()) if absolute else c
        r = a(P) @ a(W) + a(b) + (a(Q) @ a(Wi) if dual else 0)
        return r if absolute else torch.relu(r)
    refs, mag = both(ref), both(lambda c: ref(c, True))[0]
    base = None
    for tag, lay in assignments(["P", "Q"] if dual else ["P"]):
        what = f"dense fused {M}x{F}x{d} dual={dual} [{tag}]"
        Pb, Pv = view_of(P, lay["P"], dev)
        Qb, Qv = view_of(Q, lay["Q"], dev, 1) if dual else (None, None)
        with Unchanged(Pb, Qb):
            out = ops._raw_dense_fused(Pv, Wd, Qv, Wid if dual else None, bd, True)
        assert out is not None, what
        finite(out, what)
        close(out, refs, what=what, mag=mag)
        if base is None:
            base = out
        elif aligned(lay):
            assert same_bits(out, base), what


@pytest.mark.parametrize("ku,kn", [(64, 64), (66, 62), (7, 9), (130, 126), (1, 255)])
@pytest.mark.parametrize("relu,bias", [(True, True), (False, False)])
def test_concat_dense_splits(dev, ku, kn, relu, bias):
    """ops.concat_dense forward and backward against float64 autograd: both halves are written through column slices of
    one buffer and the weight gradients read g[:, ku:], out[:, ku:] and write mg[:, ku:]; with ku not a multiple of 4
    every one of those slices (and the bias slice b[ku:]) starts off a 16-byte boundary"""
    M, Fs, Fn = 500, 64, 24
    x, m = rnd(M, Fs, seed=ku), rnd(M, Fn, seed=ku + 1)
    Ws, Wn = rnd(Fs, ku, seed=ku + 2) / 8, rnd(Fn, kn, seed=ku + 3) / 5
    b = rnd(ku + kn, seed=ku + 4) if bias else None
    dy = rnd(M, ku + kn, seed=ku + 5)
    base = None
    for lay in (CONTIG, LAYOUTS[1], OFF1):
        what = f"concat_dense {ku}/{kn} relu={relu} [{lay[0]}]"
        xb, xv = view_of(x, lay, dev)
        mb, mv = view_of(m, lay, dev, 1)
        xg, mg = xv.detach().requires_grad_(True), mv.detach().requires_grad_(True)
        assert xg.stride(0) == xv.stride(0) and xg.data_ptr() == xv.data_ptr()
        par = [t.to(dev).requires_grad_(True) for t in (Ws, Wn)] + ([b.to(dev).requires_grad_(True)] if bias else [None])
        with Unchanged(xb, mb):
            out = ops.concat_dense(xg, mg, par[0], par[1], par[2], relu=relu)
            out.backward(dy.to(dev))
        mask = (out.detach() > 0).cpu() if relu else torch.ones(M, ku + kn, dtype=torch.bool)

        def ref(c):
            ts = [c(t).clone().requires_grad_(True) for t in (x, m, Ws, Wn)] + ([c(b).clone().requires_grad_(True)] if bias else [])
            r = torch.cat([ts[0] @ ts[2], ts[1] @ ts[3]], dim=1)
            if bias:
                r = r + ts[4]
            assert bool(((r.detach() > 0) == mask)[r.detach().abs() > 1e-5 * float(r.detach().abs().max())].all()) or not relu
            o = r * mask.to(r.dtype)
            o.backward(c(dy))
            return [o.detach()] + [t.grad for t in ts]
        r64, r32 = both(ref)
        Wc = torch.zeros(Fs + Fn, ku + kn, dtype=torch.float64)
        Wc[:Fs, :ku], Wc[Fs:, ku:] = Ws.double().abs(), Wn.double().abs()
        xm = torch.cat([x, m], dim=1).double().abs()
        gm = (dy.double() * mask).abs()
        close(out, (r64[0], r32[0]), what=what + " out", mag=xm @ Wc + (b.double().abs() if bias else 0))
        close(xg.grad, (r64[1], r32[1]), what=what + " dx", mag=gm[:, :ku] @ Ws.double().abs().t())
        close(mg.grad, (r64[2], r32[2]), what=what + " dm", mag=gm[:, ku:] @ Wn.double().abs().t())
        close_all(par[0].grad, (r64[3], r32[3]), what=what + " dWs")
        close_all(par[1].grad, (r64[4], r32[4]), what=what + " dWn")
        if bias:
            close_all(par[2].grad, (r64[5], r32[5]), what=what + " db")
        if base is None:
            base = out.detach()
            # the two halves written into a padded buffer: the same bits, nothing beside them touched
            pb, pv = out_view(M, ku + kn, LAYOUTS[5], dev)
            bd = None if not bias else par[2].detach()
            ops._dense_into(pv[:, :ku], xv, par[0].detach(), None if bd is None else bd[:ku], relu)
            ops._dense_into(pv[:, ku:], mv, par[1].detach(), None if bd is None else bd[ku:], relu)
            assert_untouched(pb, LAYOUTS[5][2], ku + kn, what)
            assert same_bits(pv, base), what
        elif lay[0] in ALIGNED:
            assert same_bits(out.detach(), base), what


WGRAD_SHAPES = [(1, 64), (8, 64), (64, 7), (64, 16), (256, 256), (256, 64), (264, 132)]


@pytest.mark.parametrize("F,d", WGRAD_SHAPES)
@pytest.mark.parametrize("relu", [False, True])
def test_weight_gradient_on_views(dev, F, d, relu):
    """_raw_dense_wgrad / _raw_dense_wgrad_relu with P, G, Y and GM as slices, one shape per form of wgrad_common: narrow
    (F <= 8, vector and scalar), narrow output (d <= 16), producer/consumer MFMA, general.  A misaligned operand moves the
    call to another form with another slab order: bit equality on the aligned layouts only"""
    M = 2100 if F <= 8 else 700
    P, G, Y = rnd(M, F, seed=F), rnd(M, d, seed=F + d), rnd(M, d, seed=F + d + 1)
    gm_ref = G * (Y > 0) if relu else G
    refW = both(lambda c: c(P).t() @ c(gm_ref))
    refb = both(lambda c: c(gm_ref).sum(0))
    base = None
    for tag, lay in assignments(["P", "G"] + (["Y", "GM"] if relu else [])):
        what = f"wgrad F={F} d={d} relu={relu} [{tag}]"
        Pb, Pv = view_of(P, lay["P"], dev)
        Gb, Gv = view_of(G, lay["G"], dev, 1)
        if relu:
            Yb, Yv = view_of(Y, lay["Y"], dev, 2)
            mb, mv = out_view(M, d, lay["GM"], dev)
            with Unchanged(Pb, Gb, Yb):
                r = ops._raw_dense_wgrad_relu(Pv, Gv, Yv, want_bias=True, gm_out=mv)
            assert r is not None, what
            dW, db, gm = r
            assert gm is mv
            assert_untouched(mb, lay["GM"][2], d, what)
            assert torch.equal(mv.cpu(), gm_ref), what                    # a masked copy: exact
        else:
            with Unchanged(Pb, Gb):
                dW, db = ops._raw_dense_wgrad(Pv, Gv, want_bias=True)
            assert dW is not None, what
        finite(dW, what)
        close_all(dW, refW, what=what + " dW")
        close_all(db, refb, what=what + " db")
        if base is None:
            base = (dW, db)
        elif aligned(lay):
            assert same_bits(dW, base[0]) and same_bits(db, base[1]), what


# ---------------------------------------------------------------------------------------- 5. the rest of the step
def bn_ws(N, d, dev):
    nb = C.c_size_t(0)
    check(_lib.lib().mp_bn_ws_bytes(N, d, C.byref(nb)))
    return torch.empty(nb.value, dtype=torch.uint8, device=dev), nb.value


@pytest.mark.parametrize("d", [7, 100, 256])
def test_batchnorm_on_views(dev, d):
    """mp_bn_train_fwd_f32, _bwd_f32 and _bwd_relu_f32 on the C ABI with x, y, dy and dx as slices (the Python wrapper
    copies dy).  The vector form gives a thread four columns instead of one; the order of a column's row sum is not
    promised across the two: bit equality on the aligned layouts only"""
    L = _lib.lib()
    N, eps = 500, 1e-5
    x = rnd(N, d, seed=d) * 2 + rnd(d, seed=d + 1)
    dy = rnd(N, d, seed=d + 2)
    gamma = torch.rand(d, generator=torch.Generator().manual_seed(d)) + 0.5
    beta = rnd(d, seed=d + 3) * 0.1
    gd, bd = gamma.to(dev), beta.to(dev)
    ws, nb = bn_ws(N, d, dev)
    stat = lambda: [torch.empty(d, device=dev) for _ in range(3)]

    def fwd(c):
        xc = c(x)
        mean, var = xc.mean(0), xc.var(0, unbiased=False)
        y = torch.relu((xc - mean) / torch.sqrt(var + eps) * c(gamma) + c(beta))
        return y, mean.view(-1, 1), (1 / torch.sqrt(var + eps)).view(-1, 1), (var * N / (N - 1)).view(-1, 1)
    f64, f32 = both(fwd)
    base = None
    for tag, lay in assignments(["x", "y"]):
        what = f"bn forward d={d} [{tag}]"
        xb, xv = view_of(x, lay["x"], dev)
        yb, yv = out_view(N, d, lay["y"], dev)
        mean, invstd, var = stat()
        with Unchanged(xb):
            check(L.mp_bn_train_fwd_f32(ptr(xv), xv.stride(0), N, d, ptr(gd), ptr(bd), eps, 1, ptr(yv), yv.stride(0),
                                        ptr(mean), ptr(invstd), ptr(var), ptr(ws), nb, _stream()), what)
        assert_untouched(yb, lay["y"][2], d, what)
        assert_written(yv, what)
        close(yv, (f64[0], f32[0]), what=what)
        # a column mean is one signed sum that cancels: held against the mean of absolute values (rule d of _tol.py)
        close(mean.view(-1, 1), (f64[1], f32[1]), what=what + " mean", mag=x.double().abs().mean(0).view(-1, 1))
        for got, i in ((invstd, 2), (var, 3)):
            close(got.view(-1, 1), (f64[i], f32[i]), what=f"{what} statistic {i}")
        if base is None:
            base = (yv.clone(), mean, invstd)
        elif aligned(lay):
            assert same_bits(yv, base[0]) and same_bits(mean, base[1]) and same_bits(invstd, base[2]), what
    y0, mean0, invstd0 = base
    mask = (y0 > 0).cpu()

    def bwd(c):
        xc, g = c(x), c(dy) * mask.to(c(dy).dtype)
        mean, var = xc.mean(0), xc.var(0, unbiased=False)
        istd = 1 / torch.sqrt(var + eps)
        xh = (xc - mean) * istd
        dbeta, dgamma = g.sum(0), (g * xh).sum(0)
        dx = c(gamma) * istd * (g - dbeta / N - xh * dgamma / N)
        return dx, dgamma, dbeta
    b64, b32 = both(bwd)
    for from_x in (False, True):
        base = None
        for tag, lay in assignments(["dy", "x", "dx"] + ([] if from_x else ["y"])):
            what = f"bn backward d={d} mask from x={from_x} [{tag}]"
            gb, gv = view_of(dy, lay["dy"], dev)
            xb, xv = view_of(x, lay["x"], dev, 1)
            ob, ov = out_view(N, d, lay["dx"], dev)
            dgamma, dbeta, _ = stat()
            if from_x:
                with Unchanged(gb, xb):
                    check(L.mp_bn_train_bwd_relu_f32(ptr(gv), gv.stride(0), ptr(xv), xv.stride(0), N, d, ptr(gd), ptr(bd),
                                                     ptr(mean0), ptr(invstd0), ptr(ov), ov.stride(0), ptr(dgamma),
                                                     ptr(dbeta), ptr(ws), nb, _stream()), what)
            else:
                yb, yv = view_of(y0, lay["y"], dev, 2)
                with Unchanged(gb, xb, yb):
                    check(L.mp_bn_train_bwd_f32(ptr(gv), gv.stride(0), ptr(yv), yv.stride(0), ptr(xv), xv.stride(0), N, d,
                                                ptr(gd), ptr(mean0), ptr(invstd0), ptr(ov), ov.stride(0), ptr(dgamma),
                                                ptr(dbeta), ptr(ws), nb, _stream()), what)
            assert_untouched(ob, lay["dx"][2], d, what)
            assert_written(ov, what)
            close(ov, (b64[0], b32[0]), what=what + " dx")
            close_all(dgamma, (b64[1], b32[1]), what=what + " dgamma")
            close_all(dbeta, (b64[2], b32[2]), what=what + " dbeta")
            if base is None:
                base = (ov.clone(), dgamma, dbeta)
            elif aligned(lay):
                assert same_bits(ov, base[0]) and same_bits(dgamma, base[1]) and same_bits(dbeta, base[2]), what


@pytest.mark.parametrize("Cn", [3, 10, 41])
@pytest.mark.parametrize("indexed", [False, True])
def test_softmax_cross_entropy_on_views(dev, Cn, indexed):
    """mp_softmax_ce_rows_f32 / _bwd_f32 with the logits and dlogits as slices; one form of each kernel, a row's sums
    in one order: the contiguous call's bits on every layout"""
    L = _lib.lib()
    n = 400
    g = torch.Generator().manual_seed(Cn)
    z = torch.randn(n, Cn, generator=g) * 3
    n_sel = 250 if indexed else n
    idx = torch.randint(0, n, (n_sel,), generator=g) if indexed else None       # rows may repeat: they accumulate
    lab = torch.randint(0, Cn, (n_sel,), generator=g)
    gs, inv_n = torch.tensor([0.75]), 1.0 / n_sel
    sel = idx if indexed else torch.arange(n)

    def ref(c):
        zc = c(z)
        ls = torch.log_softmax(zc[sel], dim=1)
        loss = -ls.gather(1, lab[:, None])
        grad = (ls.exp() - torch.nn.functional.one_hot(lab, Cn).to(zc.dtype)) * (0.75 * inv_n)
        return loss, torch.zeros_like(zc).index_add_(0, sel, grad)
    r64, r32 = both(ref)
    zs = z.double()[sel]
    mag_loss = torch.logsumexp(zs.abs(), dim=1, keepdim=True) + zs.abs().gather(1, lab[:, None])
    mag_grad = torch.zeros(n, Cn, dtype=torch.float64).index_add_(
        0, sel, (torch.softmax(zs, 1) + torch.nn.functional.one_hot(lab, Cn)) * (0.75 * inv_n))
    labd, idxd, gsd = lab.to(dev), None if idx is None else idx.to(dev), gs.to(dev)
    base = None
    for tag, lay in assignments(["z", "dz"]):
        what = f"softmax CE C={Cn} indexed={indexed} [{tag}]"
        zb, zv = view_of(z, lay["z"], dev)
        db, dv = out_view(n, Cn, lay["dz"], dev)
        dv.zero_()
        loss = torch.empty(n_sel, device=dev)
        with Unchanged(zb):
            check(L.mp_softmax_ce_rows_f32(ptr(zv), zv.stride(0), n, ptr(labd), ptr(idxd), n_sel, Cn, ptr(loss),
                                           _stream()), what)
            check(L.mp_softmax_ce_bwd_f32(ptr(zv), zv.stride(0), n, ptr(labd), ptr(idxd), n_sel, Cn, ptr(gsd), inv_n,
                                          ptr(dv), dv.stride(0), _stream()), what)
        assert_untouched(db, lay["dz"][2], Cn, what)
        close(loss[:, None], (r64[0], r32[0]), what=what + " loss", mag=mag_loss)
        close(dv, (r64[1], r32[1]), what=what + " dlogits", mag=mag_grad)
        if base is None:
            base = (loss, dv.clone())
        else:
            assert same_bits(loss, base[0]), what
            if not indexed:                     # (repeated rows accumulate with float atomics)
                assert same_bits(dv, base[1]), what


@pytest.mark.parametrize("d", [1, 7, 20, 64, 100])
def test_row_gather_and_scatter_on_views(dev, d):
    """gather_rows / index_add_rows with X, H and U as slices (the wrappers keep such views), and the two entry points
    themselves with `out` and H as slices: copies and single adds, exact"""
    L = _lib.lib()
    n, k = 120, 37
    x, u = rnd(n, d, seed=d), rnd(k, d, seed=d + 1)
    ids = torch.randperm(n, generator=torch.Generator().manual_seed(d))[:k]
    idd = ids.to(dev)
    want_g, want_s = x[ids], x.index_add(0, ids, u)
    for tag, lay in assignments(["x", "u", "out"]):
        what = f"rows d={d} [{tag}]"
        xb, xv = view_of(x, lay["x"], dev)
        ub, uv = view_of(u, lay["u"], dev, 1)
        with Unchanged(xb, ub):
            assert torch.equal(ops.gather_rows(xv, idd).cpu(), want_g), what
            assert torch.equal(ops.index_add_rows(xv, idd, uv).cpu(), want_s), what
            ob, ov = out_view(k, d, lay["out"], dev)
            check(L.mp_rows_gather_f32(ptr(xv), xv.stride(0), ptr(idd), k, d, ptr(ov), ov.stride(0), _stream()), what)
        assert_untouched(ob, lay["out"][2], d, what)
        assert torch.equal(ov.cpu(), want_g), what
        hb, hv = out_view(n, d, lay["out"], dev)
        hv.copy_(x)
        with Unchanged(ub):
            check(L.mp_rows_scatter_add_f32(ptr(hv), hv.stride(0), ptr(idd), k, d, ptr(uv), uv.stride(0), _stream()), what)
        assert_untouched(hb, lay["out"][2], d, what)
        assert torch.equal(hv.cpu(), want_s), what


@pytest.mark.parametrize("d", [7, 64, 100, 256])
def test_identity_rows_on_views(dev, d):
    """mp_id_fixup_f32 / mp_id_rows_f32 with Z and out as slices: a column's terms are added in entry order in the 16-byte
    and the scalar form alike, so every layout gives the contiguous call's bits"""
    L = _lib.lib()
    n, n_id, n_rows = 90, 11, 40
    g = torch.Generator().manual_seed(d)
    rows = torch.sort(torch.randperm(n, generator=g)[:n_rows]).values
    cnt = torch.randint(1, 5, (n_rows,), generator=g)
    crp = torch.cat([torch.zeros(1, dtype=torch.int64), cnt.cumsum(0)])
    slot = torch.randint(0, n_id, (int(crp[-1]),), generator=g)
    val = torch.rand(int(crp[-1]), generator=g) - 0.3
    Z, out0 = rnd(n_id, d, seed=d), rnd(n, d, seed=d + 1)
    owner = torch.repeat_interleave(torch.arange(n_rows), cnt)

    def ref(c, fix, absolute=False):
        a = (lambda t: c(t).abs()) if absolute else c
        add = torch.zeros(n, d, dtype=c(Z).dtype).index_add_(0, rows[owner], a(val)[:, None] * a(Z)[slot])
        if not fix:
            return add[rows]
        r = a(out0) + add
        if not absolute:
            r[rows] = torch.relu(r[rows])
        return r
    i32 = lambda t: t.to(torch.int32).to(dev)
    rd, cd, sd, vd = i32(rows), i32(crp), i32(slot), val.to(dev)
    for fix in (True, False):
        refs, mag = both(lambda c: ref(c, fix)), both(lambda c: ref(c, fix, True))[0]
        base = None
        for tag, lay in assignments(["Z", "out"]):
            what = f"identity rows d={d} fixup={fix} [{tag}]"
            Zb, Zv = view_of(Z, lay["Z"], dev)
            ob, ov = out_view(n, d, lay["out"], dev)
            with Unchanged(Zb):
                if fix:
                    ov.copy_(out0)
                    check(L.mp_id_fixup_f32(ptr(rd), ptr(cd), ptr(sd), ptr(vd), n_rows, ptr(Zv), Zv.stride(0), ptr(ov),
                                            ov.stride(0), d, _lib.ACT_RELU, _stream()), what)
                    got = ov
                else:
                    check(L.mp_id_rows_f32(ptr(rd), ptr(cd), ptr(sd), ptr(vd), n_rows, ptr(Zv), Zv.stride(0), ptr(ov),
                                           ov.stride(0), d, _stream()), what)
                    got = ov[rd.long()]
                    rest = torch.ones(n, dtype=torch.bool, device=dev)
                    rest[rd.long()] = False
                    assert_all_sentinel(ov[rest], what)                      # rows that are not listed are not written
            assert_untouched(ob, lay["out"][2], d, what)
            assert_written(got, what)
            close(got, refs, what=what, mag=mag)
            if base is None:
                base = got.clone()
            else:
                assert same_bits(got, base), what
