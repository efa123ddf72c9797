"""Every kernel beyond 2^31 elements and 2^32 bytes of offset.

Group A runs each operator on column slices of [70 000, 32 768] device buffers (tests/_bigview.py): a row's offset
row * ld passes 2^32 bytes at row 32 768 (fp32) and 2^31 elements at row 65 536, so one 32-bit product in an address reads
or writes the wrong row.  Group B runs the kernels that index flat (N * d, argmax[r * d + c]) on contiguous operands of
2^23 + 4096 rows x 256 columns, just over 2^31 elements.  The cases assert
  1. sampled rows (both sides of both thresholds, the last row, the hub rows, an empty row) against the float64
     evaluation of the same formula on the same inputs (tests/_tol.py);
  2. on the aligned layout, the full result bit for bit against the same call on contiguous copies of the operands,
     under the rule of tests/test_layouts_gpu.py (the plan aggregation, max / argmax, gather and scatter: always; the
     others: the aligned layout takes the contiguous call's kernel form);
  3. that the sentinel beside every output slice is intact (checked in row chunks) — wherever the entry point takes an
     output leading dimension; where the Python wrapper allocates the output itself, the entry point is also called
     directly with a wide output slice;
  4. that every input buffer keeps its bits."""
import ctypes as C

import pytest
import torch

import graphgym_amd as ga
from graphgym_amd import _lib, graphgen, ops
from graphgym_amd._lib import check, ptr
from graphgym_amd.graph import _stream
from _layout import SENTINEL
from _bigview import (IDS, N_WIDE, ROW_BYTES32, ROW_ELEMS31, WIDE, Kept, assert_beside, assert_written, need, same_bits,
                      sample_rows, wide_empty, wide_of)
from _tol import both, close, close_all
from oracle import ref_ops as R

pytestmark = pytest.mark.gpu

SUM, MEAN, MAX = _lib.SUM, _lib.MEAN, _lib.MAX
BF = torch.bfloat16
HUB_A, HUB_B = 66_000, 69_000          # >= 3 000 and >= 40 000 entries, both past 2^31 elements
EMPTY = [4, 32_777, 65_537]            # rows left without entries (r % 13 == 4): below, between and past the thresholds
N_BIG = (1 << 23) + 4096               # x 256 columns: just over 2^31 elements


@pytest.fixture(autouse=True)
def plan_kernel_unless_asked(monkeypatch):
    monkeypatch.setenv("MP_AGG_TILES", "0")       # the tile test switches it on itself
    monkeypatch.setenv("MP_X3", "1")
    monkeypatch.setenv("MP_FUSED", "1")
    yield
    torch.cuda.empty_cache()


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def wide_bytes(k, lay=WIDE[1], elem=4):
    return k * N_WIDE * lay[1] * elem + (1 << 30)


class Sub:
    """the stored entries (CSR order) whose `key` is one of the sorted rows `sample`: e their positions, seg the
    position of their key in `sample`, other / val their other index and value"""
    def __init__(self, key, other, val, sample):
        m = torch.isin(key, sample)
        self.e = torch.nonzero(m)[:, 0]
        self.seg = torch.searchsorted(sample, key[m])
        self.other = other[m]
        self.val = None if val is None else val[m]
        self.rows, self.k = sample, sample.numel()


class WideGraph:
    def __init__(self, dev):
        n, g = N_WIDE, torch.Generator().manual_seed(5)
        dst, src = torch.randint(0, n, (600_000,), generator=g), torch.randint(0, n, (600_000,), generator=g)
        keep = dst % 13 != 4
        hubs = torch.cat([torch.full((3_500,), HUB_A), torch.full((41_000,), HUB_B)])
        dst = torch.cat([dst[keep], hubs])
        src = torch.cat([src[keep], torch.randint(0, n, (hubs.numel(),), generator=g)])
        w = torch.rand(dst.numel(), generator=g) - 0.3
        self.G = ga.CSRGraph.from_edge_index(torch.stack([dst, src]).to(dev), n, w.to(dev), dst_row=0)
        G = self.G
        self.rows, self.cols, self.val = G.row_ids().cpu().long()[:G.nnz], G.col.cpu().long(), G.val.cpu()
        cnt = torch.bincount(self.rows, minlength=n)
        assert int(cnt[HUB_A]) >= 3_000 and int(cnt[HUB_B]) >= 40_000 and all(int(cnt[r]) == 0 for r in EMPTY)
        assert int(cnt[n - 1]) > 0 and int(self.cols.max()) >= ROW_ELEMS31 and int(self.cols.min()) < ROW_BYTES32
        self.sample = sample_rows(n, extra=[HUB_A, HUB_B] + EMPTY)
        self.sd = self.sample.to(dev)
        self.sub = Sub(self.rows, self.cols, self.val, self.sample)          # the sampled rows' entries
        self.subT = Sub(self.cols, self.rows, self.val, self.sample)         # the sampled columns' entries


@pytest.fixture(scope="module")
def wg(dev):
    w = WideGraph(dev)
    yield w
    del w
    torch.cuda.empty_cache()


def take(t, rows_dev):
    return t[rows_dev].cpu()


def finite(v, what):
    assert bool(torch.isfinite(v).all()), f"{what}: non-finite values in the sampled rows (a stray read?)"


def agg_ref(c, sub, w, x, S, self_scale, b, relu, red, absolute=False):
    """the aggregation of the sampled rows: oracle/ref_ops.coo_aggregate on their entries, the gathered rows of x"""
    a = (lambda t: c(t).abs()) if absolute else c
    r = R.coo_aggregate(sub.seg, sub.other, None if w is None else a(w), a(x), sub.k, red)
    if S is not None:
        r = r + abs(self_scale) * a(S[sub.rows]) if absolute else r + self_scale * a(S[sub.rows])
    if b is not None:
        r = r + a(b)
    return torch.relu(r) if (relu and not absolute) else r


def argmax_ref(sub, wcol, x, cols=None):
    """the first entry in CSR order that attains the float32 maximum of wcol[e, c] * x[col_e, c]; -1 for an empty row"""
    msg = x[sub.other] * wcol
    d, big = msg.size(1), 1 << 40
    idx = sub.seg[:, None].expand(-1, d)
    best = torch.full((sub.k, d), float("-inf")).scatter_reduce(0, idx, msg, "amax", include_self=True)
    cand = torch.where(msg == best[sub.seg], sub.e[:, None].expand(-1, d), torch.full_like(idx, big))
    arg = torch.full((sub.k, d), big, dtype=torch.int64).scatter_reduce(0, idx, cand, "amin", include_self=True)
    return torch.where(arg == big, torch.full_like(arg, -1), arg)


def bf16_close(got, r64, mag, what):
    """the bound of tests/test_spmm_bf16_gpu.py: one bf16 rounding of the result (2^-8 relative, elementwise) plus the
    fp32 accumulation (1e-5 of the row's largest sum of absolute terms)"""
    err = (got.double() - r64).abs()
    tol = 2.0 ** -8 * r64.abs() + 1e-5 * mag.abs().amax(dim=1, keepdim=True)
    assert bool((err <= tol).all()), f"{what}: {int((err > tol).sum())} elements outside the bound, worst {float((err - tol).max())}"


def max_bwd_ref(argc, cols, rows, w_of, dy):
    """float64 rows `rows` (sorted) of dX[col[e], c] += w_of(e, c) * dy[r, c] for e = argc[r, c] >= 0, from every row of
    argc: (the sums, the sums of the absolute terms)"""
    r, c = torch.nonzero(argc >= 0, as_tuple=True)
    e = argc[r, c]
    hit = torch.isin(cols[e], rows)
    r, c, e = r[hit], c[hit], e[hit]
    pos = torch.searchsorted(rows, cols[e])
    terms = w_of(e, c) * dy.double()[r, c]
    return [torch.zeros(rows.numel(), argc.size(1), dtype=torch.float64).index_put_((pos, c), t, accumulate=True)
            for t in (terms, terms.abs())]


def heads_ref(c, a, V, sub, dh, reduce, absolute=False):
    f = (lambda t: c(t).abs()) if absolute else c
    msg = f(a).repeat_interleave(dh, dim=1) * f(V)[sub.other]
    d = msg.size(1)
    if reduce == "max":
        return torch.zeros(sub.k, d, dtype=msg.dtype).scatter_reduce(0, sub.seg[:, None].expand(-1, d), msg, "amax",
                                                                     include_self=False)
    out = torch.zeros(sub.k, d, dtype=msg.dtype).index_add_(0, sub.seg, msg)
    if reduce == "mean":
        out = out / torch.bincount(sub.seg, minlength=sub.k).clamp(min=1).to(msg.dtype)[:, None]
    return out


# =========================================================================================== A. wide leading dimension
PLAN_CASES = [("sum", 1.5, True, True), ("sum", 0.0, False, False), ("mean", 0.0, False, False), ("max", 0.0, True, True)]


@pytest.mark.parametrize("lay", WIDE, ids=IDS)
@pytest.mark.parametrize("case", PLAN_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_plan_aggregation(dev, wg, lay, case):
    """mp_spmm_csr_f32 with x, S and out as wide slices: sum / mean / max, with S and self_scale, bias and ReLU, argmax.
    A column sums its row's entries in entry order whatever the lane width: the contiguous call's bits on both layouts"""
    reduce, self_scale, has_bias, relu = case
    n, d, G, sub = N_WIDE, 128, wg.G, wg.sub
    need(wide_bytes(3), "plan aggregation")
    what = f"wide {reduce} s={self_scale} [{lay[0]}]"
    x = rnd(n, d, seed=1)
    s = rnd(n, d, seed=2) if self_scale else None
    b = rnd(d, seed=3) if has_bias else None
    red = _lib.REDUCE[reduce]
    refs = both(lambda c: agg_ref(c, sub, sub.val, x, s, self_scale, b, relu, reduce))
    mag = both(lambda c: agg_ref(c, sub, sub.val, x, s, self_scale, b, relu, reduce, absolute=True))[0]
    xb, xv = wide_of(x, lay, dev)
    sb, sv = wide_of(s, lay, dev) if s is not None else (None, None)
    ob, ov = wide_empty(n, d, lay, dev)
    bd = None if b is None else b.to(dev)
    with Kept((xb, xv, lay), (sb, sv, lay)):
        y, arg = ops._raw_spmm(G, xv, red, S=sv, self_scale=self_scale, bias=bd, relu=relu,
                               want_argmax=reduce == "max", out=ov)
    assert y is ov
    assert_beside(ob, lay, d, what)
    assert_written(ov, what)
    got = take(ov, wg.sd)
    finite(got, what)
    close(got, refs, what=what, mag=mag)
    if reduce == "max":
        assert torch.equal(take(arg, wg.sd).long(), argmax_ref(sub, sub.val[:, None], x)), what
    y0, a0 = ops._raw_spmm(G, x.to(dev), red, S=None if s is None else s.to(dev), self_scale=self_scale, bias=bd,
                           relu=relu, want_argmax=reduce == "max")
    assert same_bits(ov, y0), what
    assert arg is None or torch.equal(arg, a0), what


@pytest.mark.parametrize("lay", WIDE, ids=IDS)
def test_fused_eval_epilogue(dev, wg, lay):
    n, d, G, sub = N_WIDE, 128, wg.G, wg.sub
    need(wide_bytes(1), "fused eval")
    x = rnd(n, d, seed=4)
    cs, ct = torch.rand(d, generator=torch.Generator().manual_seed(d)) + 0.5, rnd(d, seed=5)

    def ref(c, l2, absolute=False):
        a = (lambda t: c(t).abs()) if absolute else c
        r = agg_ref(c, sub, sub.val, x, x, 0.5, None, False, "sum", absolute) * a(cs) + a(ct)
        if absolute:
            return r
        r = torch.relu(r)
        return torch.nn.functional.normalize(r, p=2, dim=-1, eps=1e-12) if l2 else r
    xb, xv = wide_of(x, lay, dev)
    for l2 in (False, True):
        what = f"wide fused eval l2={l2} [{lay[0]}]"
        refs = both(lambda c: ref(c, l2))
        mag = None if l2 else both(lambda c: ref(c, l2, True))[0]
        with Kept((xb, xv, lay)):
            y = ops.spmm_fused_eval(G, xv, "sum", self_scale=0.5, col_scale=cs.to(dev), col_shift=ct.to(dev), relu=True,
                                    l2norm=l2)
        got = take(y, wg.sd)
        finite(got, what)
        close(got, refs, what=what, mag=mag)
        if lay is WIDE[0] or not l2:
            y0 = ops.spmm_fused_eval(G, x.to(dev), "sum", self_scale=0.5, col_scale=cs.to(dev), col_shift=ct.to(dev),
                                     relu=True, l2norm=l2)
            assert same_bits(y, y0), what
        # the entry point itself, y a wide slice (st 2 with l2norm: the row is wider than one wave, nothing is written)
        ob, ov = wide_empty(n, d, lay, dev)
        plan, counts, ws, nb = ops._plan_ws(G, dev, d, SUM, False)
        csd, ctd = cs.to(dev), ct.to(dev)
        with Kept((xb, xv, lay)):
            st = _lib.lib().mp_spmm_csr_epilogue_f32(ptr(G.rowptr), ptr(G.col), ptr(G.val), n, ptr(plan), counts, ptr(xv),
                                                     xv.stride(0), ptr(ov), ov.stride(0), d, SUM, ptr(xv), xv.stride(0),
                                                     0.5, ptr(csd), ptr(ctd), _lib.ACT_RELU, 1 if l2 else 0, 1e-12, ptr(ws),
                                                     nb, _stream())
        assert st == 0 or (l2 and st == 2), what
        assert_beside(ob, lay, d, what)
        if st == 0:
            assert same_bits(ov, y), what
        del ob, ov


@pytest.mark.parametrize("lay", WIDE, ids=IDS)
def test_two_branch_aggregation(dev, wg, lay):
    """mp_idgnn_agg_f32 with x, P and Q as wide slices, and ops.idgnn_aggregate on the view of x"""
    n, d, G, sub = N_WIDE, 128, wg.G, wg.sub
    need(wide_bytes(3), "two-branch")
    what = f"wide two-branch [{lay[0]}]"
    x = rnd(n, d, seed=6)
    ids = torch.unique(torch.cat([torch.randperm(n, generator=torch.Generator().manual_seed(6))[: n // 9],
                                  torch.arange(ROW_ELEMS31, ROW_ELEMS31 + 300)]))
    sel = torch.zeros(n, 1)
    sel[ids] = 1
    xs = x * sel
    refP = both(lambda c: agg_ref(c, sub, sub.val, x, None, 0.0, None, False, "sum"))
    refQ = both(lambda c: agg_ref(c, sub, sub.val, xs, None, 0.0, None, False, "sum"))
    magP = both(lambda c: agg_ref(c, sub, sub.val, x, None, 0.0, None, False, "sum", True))[0]
    magQ = both(lambda c: agg_ref(c, sub, sub.val, xs, None, 0.0, None, False, "sum", True))[0]
    idd = ids.to(dev)
    xb, xv = wide_of(x, lay, dev)
    Pb, Pv = wide_empty(n, d, lay, dev)
    Qb, Qv = wide_empty(n, d, lay, dev)
    with Kept((xb, xv, lay)):
        plan, counts, ws, nb = ops._plan_ws(G, dev, d, SUM, True)
        check(_lib.lib().mp_idgnn_agg_f32(ptr(G.rowptr), ptr(G.mark_ids(idd)), ptr(G.val), n, ptr(plan), counts, ptr(xv),
                                          xv.stride(0), ptr(Pv), Pv.stride(0), ptr(Qv), Qv.stride(0), d, ptr(ws), nb,
                                          _stream()), what)
        P2, Q2 = ops.idgnn_aggregate(G, idd, xv)
    for bf, v, refs, mag, k in ((Pb, Pv, refP, magP, "P"), (Qb, Qv, refQ, magQ, "Q")):
        assert_beside(bf, lay, d, what)
        assert_written(v, what)
        got = take(v, wg.sd)
        finite(got, what)
        close(got, refs, what=f"{what} {k}", mag=mag)
    P0, Q0 = ops.idgnn_aggregate(G, idd, x.to(dev))
    for got, want in ((Pv, P0), (Qv, Q0), (P2, P0), (Q2, Q0)):
        assert same_bits(got, want), what


@pytest.mark.parametrize("lay", WIDE, ids=IDS)
@pytest.mark.parametrize("hot", [False, True], ids=["tiles", "hot-columns"])
def test_tile_aggregation(dev, wg, monkeypatch, lay, hot):
    """mp_agg_rows_tiles_f32 and its hot-column form (taken on 16-byte aligned rows; the plan kernel and its bits
    otherwise), and the two-branch tile kernel through ops.idgnn_aggregate"""
    n, d, G, sub = N_WIDE, 256, wg.G, wg.sub
    need(wide_bytes(3), "tiles")
    x, s = rnd(n, d, seed=7), rnd(n, d, seed=8)
    refs = both(lambda c: agg_ref(c, sub, sub.val, x, s, 1.5, None, False, "sum"))
    mag = both(lambda c: agg_ref(c, sub, sub.val, x, s, 1.5, None, False, "sum", True))[0]
    refm = both(lambda c: agg_ref(c, sub, sub.val, x, None, 0.0, None, False, "max"))
    xd, sdv = x.to(dev), s.to(dev)
    y_plan, _ = ops._raw_spmm(G, xd, SUM, S=sdv, self_scale=1.5)
    m_plan, _ = ops._raw_spmm(G, xd, MAX)
    monkeypatch.setenv("MP_AGG_TILES", "1")
    monkeypatch.setattr(ops, "AGG_TILES_MIN_ROWS", 1)
    monkeypatch.setattr(ops, "AGG_HOT_MIN_BYTES", 1 if hot else 1 << 62)
    monkeypatch.setenv("MP_AGG_HOT_MB", "16")
    tiles = lay is WIDE[0]
    xb, xv = wide_of(x, lay, dev)
    sb, sv = wide_of(s, lay, dev)
    for red, S, scale, ref, mg, plan_y in ((SUM, sv, 1.5, refs, mag, y_plan), (MAX, None, 0.0, refm, None, m_plan)):
        what = f"wide tiles red={red} hot={hot} [{lay[0]}]"
        ob, ov = wide_empty(n, d, lay, dev)
        t0, h0 = ops.AGG_TILES_CALLS, ops.AGG_HOT_CALLS
        with Kept((xb, xv, lay), (sb, sv, lay)):
            ops._raw_spmm(G, xv, red, S=S, self_scale=scale, out=ov)
        assert ops.AGG_TILES_CALLS == t0 + (1 if tiles else 0), what
        assert ops.AGG_HOT_CALLS == h0 + (1 if tiles and hot else 0), what
        assert_beside(ob, lay, d, what)
        assert_written(ov, what)
        got = take(ov, wg.sd)
        finite(got, what)
        close(got, ref, what=what, mag=mg)
        if not tiles or red == MAX:             # (a maximum is the plan kernel's bit for bit on either structure)
            assert same_bits(ov, plan_y), what
        else:                                   # the same tile form on contiguous operands
            t0 = ops.AGG_TILES_CALLS
            y0, _ = ops._raw_spmm(G, xd, red, S=sdv, self_scale=scale)
            assert ops.AGG_TILES_CALLS == t0 + 1 and same_bits(ov, y0), what
        del ob, ov
    if not hot:
        ids = torch.randperm(n, generator=torch.Generator().manual_seed(9))[: n // 50].to(dev)
        selx = torch.zeros(n, 1)
        selx[ids.cpu()] = 1
        xs = x * selx
        t0 = ops.AGG_TILES_CALLS
        with Kept((xb, xv, lay)):
            P, Q = ops.idgnn_aggregate(G, ids, xv)
        assert ops.AGG_TILES_CALLS == t0 + (1 if tiles else 0)
        close(take(P, wg.sd), both(lambda c: agg_ref(c, sub, sub.val, x, None, 0.0, None, False, "sum")),
              what="wide two-branch tiles P", mag=both(lambda c: agg_ref(c, sub, sub.val, x, None, 0, None, False, "sum", True))[0])
        close(take(Q, wg.sd), both(lambda c: agg_ref(c, sub, sub.val, xs, None, 0.0, None, False, "sum")),
              what="wide two-branch tiles Q", mag=both(lambda c: agg_ref(c, sub, sub.val, xs, None, 0, None, False, "sum", True))[0])
        if tiles:                               # the same tile form on the contiguous x
            P0, Q0 = ops.idgnn_aggregate(G, ids, xd)
            assert same_bits(P, P0) and same_bits(Q, Q0)
            # the entry point itself with P, Q and Z = x[ids] as wide slices
            br = G.id_branch(ids)
            Zb, Zv = wide_of(x[ids.cpu()], lay, dev)
            Pb, Pv = wide_empty(n, d, lay, dev)
            Qb, Qv = wide_empty(n, d, lay, dev)
            with Kept((xb, xv, lay), (Zb, Zv, lay)):
                check(_lib.lib().mp_idgnn_agg_tiles_f32(ptr(G.rowptr), ptr(G.col), ptr(G.val), n, ptr(xv), xv.stride(0), d,
                                                        ptr(br.defer), ptr(br.rows), ptr(br.crp), ptr(br.slot), ptr(br.val),
                                                        br.n_rows, ptr(Zv), Zv.stride(0), ptr(Pv), Pv.stride(0), ptr(Qv),
                                                        Qv.stride(0), _stream()), "mp_idgnn_agg_tiles_f32")
            assert_beside(Pb, lay, d, "two-branch tiles P"), assert_beside(Qb, lay, d, "two-branch tiles Q")
            assert same_bits(Pv, P) and same_bits(Qv, Q)


@pytest.mark.parametrize("lay", WIDE, ids=IDS)
def test_one_kernel_layer(dev, wg, lay):
    """mp_agg_dense_f32 with x, S, P and out as wide slices (want_P), and mp::agg_dense_id on the view of x; a misaligned
    x is turned down by agg_dense_supported and the layer runs as two kernels"""
    n, F, dout, G, sub = N_WIDE, 128, 64, wg.G, wg.sub
    need(wide_bytes(4), "one-kernel layer")
    x, W, Wi, b = rnd(n, F, seed=10), rnd(F, dout, seed=11) / F ** 0.5, rnd(F, dout, seed=12) / F ** 0.5, rnd(dout, seed=13)
    Wd, Wid, bd = W.to(dev), Wi.to(dev), b.to(dev)
    ids = torch.unique(torch.cat([torch.randperm(n, generator=torch.Generator().manual_seed(10))[: n // 50],
                                  torch.arange(ROW_ELEMS31 + 5, ROW_ELEMS31 + 200)]))
    sel = torch.zeros(n, 1)
    sel[ids] = 1

    def ref(c, absolute=False, with_id=False):
        a = (lambda t: c(t).abs()) if absolute else c
        P = agg_ref(c, sub, sub.val, x, x, 0.5, None, False, "sum", absolute)
        r = P @ a(W) + a(b)
        if with_id:
            r = r + agg_ref(c, sub, sub.val, x * sel, None, 0.0, None, False, "sum", absolute) @ a(Wi)
        return (r if absolute else torch.relu(r)), P
    refs, mag = both(ref), both(lambda c: ref(c, True))[0]
    what = f"wide one-kernel layer [{lay[0]}]"
    xb, xv = wide_of(x, lay, dev)
    ok = ops.agg_dense_supported(G, xv, Wd)
    assert ok == (lay is WIDE[0]), what
    with Kept((xb, xv, lay)), torch.no_grad():
        out, P = torch.ops.mp.agg_dense_raw(xv, Wd, bd, G.handle, 0, SUM, xv, 0.5, True, True)
    for got, i, k in ((out, 0, "out"), (P, 1, "P")):
        g = take(got, wg.sd)
        finite(g, what)
        close(g, (refs[0][i], refs[1][i]), what=f"{what} {k}", mag=mag[i])
    if ok:
        out0, P0 = torch.ops.mp.agg_dense_raw(x.to(dev), Wd, bd, G.handle, 0, SUM, x.to(dev), 0.5, True, True)
        assert same_bits(out, out0) and same_bits(P, P0), what
        # the entry point itself, P and out as wide slices too
        Pb, Pv = wide_empty(n, F, lay, dev)
        ob, ov = wide_empty(n, dout, lay, dev)
        with Kept((xb, xv, lay)):
            ops._raw_agg_dense(G, xv, Wd, bd, True, S=xv, self_scale=0.5, want_P=False, out=ov)
            assert_beside(ob, lay, dout, what)
            assert same_bits(ov, out0), what
            ov.view(torch.int32).fill_(SENTINEL)
            L = _lib.lib()
            Wsp = ops._split_w(Wd)
            check(L.mp_agg_dense_f32(ptr(G.rowptr), ptr(G.col), ptr(G.val), n, SUM, ptr(xv), xv.stride(0), F, ptr(xv),
                                     xv.stride(0), 0.5, ptr(Wd), Wd.stride(0), dout, ptr(bd), _lib.ACT_RELU, None, ptr(Pv),
                                     Pv.stride(0), ptr(ov), ov.stride(0), ptr(Wsp), _stream()), what)
        assert_beside(Pb, lay, F, what), assert_beside(ob, lay, dout, what)
        assert same_bits(ov, out0) and same_bits(Pv, P0), what
        # mp_agg_dense_add_f32: act(... + R) with the residual R a wide slice as well
        Rm = rnd(n, dout, seed=14)
        Rb, Rv = wide_of(Rm, lay, dev)
        ov.view(torch.int32).fill_(SENTINEL)

        def ref_add(c, absolute=False):
            a = (lambda t: c(t).abs()) if absolute else c
            r = agg_ref(c, sub, sub.val, x, x, 0.5, None, False, "sum", absolute) @ a(W) + a(b) + a(Rm[sub.rows])
            return r if absolute else torch.relu(r)
        with Kept((xb, xv, lay), (Rb, Rv, lay)):
            check(L.mp_agg_dense_add_f32(ptr(G.rowptr), ptr(G.col), ptr(G.val), n, SUM, ptr(xv), xv.stride(0), F, ptr(xv),
                                         xv.stride(0), 0.5, ptr(Wd), Wd.stride(0), dout, ptr(bd), _lib.ACT_RELU, None, None,
                                         0, ptr(ov), ov.stride(0), ptr(Wsp), ptr(Rv), Rv.stride(0), _stream()), what)
        assert_beside(ob, lay, dout, what)
        got = take(ov, wg.sd)
        finite(got, what)
        close(got, both(ref_add), what=what + " with residual", mag=both(lambda c: ref_add(c, True))[0])
        xd_ = x.to(dev)
        o1, _ = ops._raw_agg_dense(G, xd_, Wd, bd, True, S=xd_, self_scale=0.5, residual=Rm.to(dev))
        assert same_bits(ov, o1), what
        del Pb, Pv, ob, ov, Rb, Rv
    del out, P
    refi, magi = both(lambda c: ref(c, with_id=True)), both(lambda c: ref(c, True, True))[0]
    with Kept((xb, xv, lay)), torch.no_grad():
        out, P, x_id = torch.ops.mp.agg_dense_id_raw(xv, Wd, Wid, bd, G.handle, ids.to(dev), 0.5, True, True)
    assert torch.equal(x_id.cpu(), x[ids]), what
    close(take(out, wg.sd), (refi[0][0], refi[1][0]), what=what + " id out", mag=magi[0])
    close(take(P, wg.sd), (refi[0][1], refi[1][1]), what=what + " id P", mag=magi[1])
    if ok:
        out0, P0, _ = torch.ops.mp.agg_dense_id_raw(x.to(dev), Wd, Wid, bd, G.handle, ids.to(dev), 0.5, True, True)
        assert same_bits(out, out0) and same_bits(P, P0), what


@pytest.mark.parametrize("lay", WIDE, ids=IDS)
def test_multi_head_aggregation(dev, wg, lay):
    """_raw_spmm_heads, _raw_spmm_heads_reduce (mean, max with argmax), _raw_heads_max_da and the max backward into V,
    node operands as wide slices, the per-entry weights natural"""
    n, heads, dh, G, sub = N_WIDE, 4, 32, wg.G, wg.sub
    d = heads * dh
    need(wide_bytes(4), "multi-head")
    a = torch.rand(G.nnz, heads, generator=torch.Generator().manual_seed(14)) - 0.3
    V, dy = rnd(n, d, seed=15), rnd(n, d, seed=16)
    ad, Vd = a.to(dev), V.to(dev)
    Vb, Vv = wide_of(V, lay, dev)
    asub = a[sub.e]
    arg = None
    for reduce in ("sum", "mean", "max"):
        what = f"wide heads {reduce} [{lay[0]}]"
        refs = both(lambda c: heads_ref(c, asub, V, sub, dh, reduce))
        mag = both(lambda c: heads_ref(c, asub, V, sub, dh, reduce, True))[0]
        with Kept((Vb, Vv, lay)):
            if reduce == "sum":
                y, am = ops._raw_spmm_heads(G, ad, Vv, heads), None
                y0, a0 = ops._raw_spmm_heads(G, ad, Vd, heads), None
            else:
                y, am = ops._raw_spmm_heads_reduce(G, ad, Vv, heads, _lib.REDUCE[reduce])
                y0, a0 = ops._raw_spmm_heads_reduce(G, ad, Vd, heads, _lib.REDUCE[reduce])
        got = take(y, wg.sd)
        finite(got, what)
        close(got, refs, what=what, mag=mag)
        assert same_bits(y, y0), what                      # entry order per column, whatever the lane width
        if reduce == "max":
            assert torch.equal(take(am, wg.sd).long(), argmax_ref(sub, asub.repeat_interleave(dh, dim=1), V)), what
            assert torch.equal(am, a0), what
            arg = am
        # the entry points themselves, y a wide slice
        red = _lib.REDUCE[reduce]
        ob, ov = wide_empty(n, d, lay, dev)
        plan, counts, ws, nb = ops._plan_ws(G, dev, d, red, False)
        am2 = torch.empty((n, d), dtype=torch.int32, device=dev) if reduce == "max" else None
        L = _lib.lib()
        with Kept((Vb, Vv, lay)):
            check(L.mp_spmm_csr_heads_reduce_f32(ptr(G.rowptr), ptr(G.col), ptr(ad), n, ptr(plan), counts, heads, red,
                                                 ptr(Vv), Vv.stride(0), ptr(ov), ov.stride(0), d, ptr(am2), ptr(ws), nb,
                                                 _stream()), what)
        assert_beside(ob, lay, d, what)
        assert same_bits(ov, y), what
        assert am2 is None or torch.equal(am2, am), what
        del ob, ov
    # da[e, h] over the sampled rows' entries
    argc = arg.cpu().long()
    won = argc[wg.rows[sub.e]] == sub.e[:, None]
    rows_g = sub.rows[sub.seg]

    def ref_da(c, absolute=False):
        f = (lambda t: c(t).abs()) if absolute else c
        return (f(dy)[rows_g] * f(V)[sub.other] * won.to(c(dy).dtype)).view(-1, heads, dh).sum(-1)
    mb, mv = wide_of(arg, lay, dev)
    yb, yv = wide_of(dy, lay, dev)
    what = f"wide heads max da [{lay[0]}]"
    with Kept((mb, mv, lay), (yb, yv, lay), (Vb, Vv, lay)):
        da = ops._raw_heads_max_da(G, mv, yv, Vv, heads)
    got = da[sub.e.to(dev)].cpu()
    finite(got, what)
    close(got, both(ref_da), what=what, mag=both(lambda c: ref_da(c, True))[0])
    if lay is WIDE[0]:
        assert same_bits(da, ops._raw_heads_max_da(G, arg, dy.to(dev), Vd, heads)), what
    del mb, mv
    # dV[col_e, c] += a[e, h] dY[r, c] for e = argmax[r, c]: the sampled rows of dV, from every row of argmax
    what = f"wide heads max backward [{lay[0]}]"
    ref, mag = max_bwd_ref(argc, wg.cols, sub.rows, lambda e, c: a.double()[e, c // dh], dy)
    xb, xv = wide_empty(n, d, lay, dev)
    xv.zero_()
    with Kept((yb, yv, lay)):
        check(_lib.lib().mp_spmm_heads_max_bwd_f32(ptr(G.col), ptr(ad), heads, ptr(arg), n, d, ptr(yv), yv.stride(0),
                                                   ptr(xv), xv.stride(0), _stream()), what)
    assert_beside(xb, lay, d, what)
    got = take(xv, wg.sd)
    finite(got, what)
    close(got, ref, what=what, mag=mag)


@pytest.mark.parametrize("lay", WIDE, ids=IDS)
def test_max_backward(dev, wg, lay):
    """mp_spmm_max_bwd_f32 with dY and dX as wide slices (float atomics: assertion 1 only)"""
    n, d, G, sub = N_WIDE, 64, wg.G, wg.sub
    need(wide_bytes(2), "max backward")
    what = f"wide max backward [{lay[0]}]"
    x, dy = rnd(n, d, seed=17), rnd(n, d, seed=18)
    _, arg = ops._raw_spmm(G, x.to(dev), MAX, want_argmax=True)
    argc = arg.cpu().long()
    ref, mag = max_bwd_ref(argc, wg.cols, sub.rows, lambda e, c: wg.val.double()[e], dy)
    yb, yv = wide_of(dy, lay, dev)
    xb, xv = wide_empty(n, d, lay, dev)
    xv.zero_()
    with Kept((yb, yv, lay)):
        check(_lib.lib().mp_spmm_max_bwd_f32(ptr(G.col), ptr(G.val), ptr(arg), ptr(yv), yv.stride(0), n, d, ptr(xv),
                                             xv.stride(0), _stream()), what)
    assert_beside(xb, lay, d, what)
    got = take(xv, wg.sd)
    finite(got, what)
    close(got, ref, what=what, mag=mag)


@pytest.mark.parametrize("lay", WIDE, ids=IDS)
@pytest.mark.parametrize("heads,d", [(1, 128), (4, 128), (4, 24)], ids=["stream-1x128", "stream-4x32", "rows-4x6"])
def test_sddmm(dev, wg, lay, heads, d):
    """sddmm_dot (the entry-balanced kernel; the row kernel for the head layout 4 x 6), mp_sddmm_dot_f32 at scale 1, and the
    gradients of sddmm_dot into Q and K; node operands as wide slices, the per-entry arrays natural"""
    n, G, sub, subT = N_WIDE, wg.G, wg.sub, wg.subT
    dh = d // heads
    need(wide_bytes(2), "sddmm")
    what = f"wide sddmm heads={heads} d={d} [{lay[0]}]"
    A, B = rnd(n, d, seed=19), rnd(n, d, seed=20)
    ds = rnd(G.nnz, heads, seed=21)
    rows_g = sub.rows[sub.seg]

    def ref(c, scale, absolute=False):
        a = (lambda t: c(t).abs()) if absolute else c
        return (a(A)[rows_g].view(-1, heads, dh) * a(B)[sub.other].view(-1, heads, dh)).sum(-1) * scale
    Ab, Av = wide_of(A, lay, dev)
    Bb, Bv = wide_of(B, lay, dev)
    ed = sub.e.to(dev)
    Ag, Bg = Av.detach().requires_grad_(True), Bv.detach().requires_grad_(True)
    assert Ag.data_ptr() == Av.data_ptr() and Ag.stride(0) == lay[1]
    with Kept((Ab, Av, lay), (Bb, Bv, lay)):
        s = ops.sddmm_dot(G, Ag, Bg, heads, 0.5)
        s.backward(ds.to(dev))
        g = torch.empty(G.nnz * heads, device=dev)
        check(_lib.lib().mp_sddmm_dot_f32(ptr(G.rowptr), ptr(G.col), n, G.nnz, ptr(Av), Av.stride(0), ptr(Bv),
                                          Bv.stride(0), d, heads, 1.0, ptr(g), _stream()), what)
    got = s.detach()[ed].cpu()
    finite(got, what)
    close(got, both(lambda c: ref(c, 0.5)), what=what, mag=both(lambda c: ref(c, 0.5, True))[0])
    close(g.view(-1, heads)[ed].cpu(), both(lambda c: ref(c, 1.0)), what=what + " grad kernel",
          mag=both(lambda c: ref(c, 1.0, True))[0])
    # dQ[i] = scale * sum_e ds[e, h] K[col_e]; dK[j] = scale * sum_{e: col_e = j} ds[e, h] Q[row_e]
    for grad, sb_, src, k in ((Ag.grad, sub, B, "dQ"), (Bg.grad, subT, A, "dK")):
        w = ds[sb_.e] * 0.5
        gq = take(grad, wg.sd)
        finite(gq, what)
        close(gq, both(lambda c: heads_ref(c, w, src, sb_, dh, "sum")), what=f"{what} {k}",
              mag=both(lambda c: heads_ref(c, w, src, sb_, dh, "sum", True))[0])
    if lay is WIDE[0]:
        A0, B0 = A.to(dev).requires_grad_(True), B.to(dev).requires_grad_(True)
        s0 = ops.sddmm_dot(G, A0, B0, heads, 0.5)
        s0.backward(ds.to(dev))
        assert same_bits(s.detach(), s0.detach()), what
        assert same_bits(Ag.grad, A0.grad) and same_bits(Bg.grad, B0.grad), what      # aggregations in entry order
        g0 = torch.empty_like(g)
        check(_lib.lib().mp_sddmm_dot_f32(ptr(G.rowptr), ptr(G.col), n, G.nnz, ptr(A0), d, ptr(B0), d, d, heads, 1.0,
                                          ptr(g0), _stream()), what)
        assert same_bits(g, g0), what


@pytest.mark.parametrize("lay", WIDE, ids=IDS)
def test_additive_attention(dev, wg, lay):
    """sddmm_add, gat_alpha and edge_softmax with the per-node terms taken from wide buffers.  mp_sddmm_add_f32,
    mp_gat_alpha_f32 and the row softmax and its backward take packed arrays and no leading dimension (the wrappers call
    .contiguous()): what crosses the thresholds here is the rows the entries name, so only the forward is run, on the
    sampled rows' entries; their backwards at small sizes are tests/test_parity_gpu.py's"""
    n, H, G, sub = N_WIDE, 4, wg.G, wg.sub
    need(wide_bytes(2), "additive attention")
    what = f"wide additive attention [{lay[0]}]"
    a_dst, a_src = rnd(n, H, seed=22), rnd(n, H, seed=23)
    db, dv = wide_of(a_dst, lay, dev)
    sb, sv = wide_of(a_src, lay, dev)
    rows_g, ed = sub.rows[sub.seg], sub.e.to(dev)

    def pre(c):
        return torch.nn.functional.leaky_relu(c(a_dst)[rows_g] + c(a_src)[sub.other], 0.2)
    with Kept((db, dv, lay), (sb, sv, lay)):
        sa = ops.sddmm_add(G, dv[:, 1], sv[:, 1], 0.2)
        alpha = ops.gat_alpha(G, dv, sv, 0.2)
        sc = ops._raw_sddmm_dot(G, dv, sv, 1, 1.0)
        p = ops.edge_softmax(G, sc)
    close(sa[ed].cpu(), both(lambda c: pre(c)[:, 1:2]), what=what + " sddmm_add")
    close(alpha[ed].cpu(), both(lambda c: R.softmax(pre(c), sub.seg, sub.k)), what=what + " gat_alpha")
    close(p[ed].cpu(), both(lambda c: R.softmax((c(a_dst)[rows_g] * c(a_src)[sub.other]).sum(-1, keepdim=True), sub.seg,
                                                sub.k)), what=what + " edge_softmax")


@pytest.mark.parametrize("lay", WIDE, ids=IDS)
def test_dense_transforms(dev, lay, monkeypatch):
    """dense_fused (single and dual), _raw_dense_x3 (d = 64 / 128 / 256, trans both ways; aligned rows only: the
    misaligned layout asserts that it is turned down) and concat_dense, P / Q / x / m and the outputs as wide slices"""
    monkeypatch.setattr(ops, "X3_MIN_ROWS", 1)
    M, F = N_WIDE, 72
    need(wide_bytes(4), "dense")
    rows = sample_rows(M, seed=3)
    rd = rows.to(dev)
    P, Q = rnd(M, F, seed=24), rnd(M, F, seed=25)
    Pb, Pv = wide_of(P, lay, dev)
    Qb, Qv = wide_of(Q, lay, dev)
    for d, dual in ((100, False), (100, True), (33, True)):
        what = f"wide dense fused d={d} dual={dual} [{lay[0]}]"
        W, Wi, b = rnd(F, d, seed=26) / F ** 0.5, rnd(F, d, seed=27) / F ** 0.5, rnd(d, seed=28)

        def ref(c, absolute=False):
            a = (lambda t: c(t).abs()) if absolute else c
            r = a(P[rows]) @ a(W) + a(b) + (a(Q[rows]) @ a(Wi) if dual else 0)
            return r if absolute else torch.relu(r)
        with Kept((Pb, Pv, lay), (Qb, Qv, lay)):
            out = ops._raw_dense_fused(Pv, W.to(dev), Qv if dual else None, Wi.to(dev) if dual else None, b.to(dev), True)
        assert out is not None, what
        got = take(out, rd)
        finite(got, what)
        close(got, both(ref), what=what, mag=both(lambda c: ref(c, True))[0])
        if lay is WIDE[0]:
            out0 = ops._raw_dense_fused(P.to(dev), W.to(dev), Q.to(dev) if dual else None, Wi.to(dev) if dual else None,
                                        b.to(dev), True)
            assert same_bits(out, out0), what
        # into a wide output slice (mp_dense_fused_f32: scalar stores, any alignment)
        ob, ov = wide_empty(M, d, lay, dev)
        if not dual:
            ops._dense_into(ov, Pv, W.to(dev), b.to(dev), True)
        else:
            Wd_, Wid_, bd_ = W.to(dev), Wi.to(dev), b.to(dev)
            with Kept((Pb, Pv, lay), (Qb, Qv, lay)):
                check(_lib.lib().mp_dense_fused_f32(ptr(Pv), Pv.stride(0), ptr(Wd_), ptr(Qv), Qv.stride(0), ptr(Wid_),
                                                    ptr(bd_), _lib.ACT_RELU, ptr(ov), ov.stride(0), M, F, d, _stream()), what)
        assert_beside(ob, lay, d, what)
        assert same_bits(ov, out), what
        del ob, ov
    del Qb, Qv, Pb, Pv
    # the streaming kernel
    K = 64
    P = rnd(M, K, seed=29)
    Pb, Pv = wide_of(P, lay, dev)
    for d in (64, 128, 256):
        for trans in (False, True):
            what = f"wide dense x3 d={d} trans={trans} [{lay[0]}]"
            W, b = rnd(K, d, seed=30 + d) / 8, rnd(d, seed=31)
            Wd = (W.t().contiguous() if trans else W).to(dev)
            ob, ov = wide_empty(M, d, lay, dev)
            ok = ops.dense_x3_supported(Pv, K, d, ov)
            assert ok == (lay is WIDE[0]), what
            if not ok:
                continue
            with Kept((Pb, Pv, lay)):
                ops._raw_dense_x3(Pv, Wd, b.to(dev), True, trans=trans, out=ov)
            assert_beside(ob, lay, d, what)
            assert_written(ov, what)
            got = take(ov, rd)
            finite(got, what)
            close(got, both(lambda c: torch.relu(c(P[rows]) @ c(W) + c(b))), what=what,
                  mag=P[rows].double().abs() @ W.double().abs() + b.double().abs())
            assert same_bits(ov, ops._raw_dense_x3(P.to(dev), Wd, b.to(dev), True, trans=trans)), what
            del ob, ov
    del Pb, Pv
    # concat_dense, forward and backward
    Fs, Fn, ku, kn = 64, 24, 66, 62
    x, m = rnd(M, Fs, seed=32), rnd(M, Fn, seed=33)
    Ws, Wn, b = rnd(Fs, ku, seed=34) / 8, rnd(Fn, kn, seed=35) / 5, rnd(ku + kn, seed=36)
    dy = torch.zeros(M, ku + kn)
    dy[rows] = rnd(rows.numel(), ku + kn, seed=37)       # the weight gradients then depend on the sampled rows only
    what = f"wide concat_dense [{lay[0]}]"
    xb, xv = wide_of(x, lay, dev)
    mb, mv = wide_of(m, lay, dev)
    xg, mg = xv.detach().requires_grad_(True), mv.detach().requires_grad_(True)
    par = [t.to(dev).requires_grad_(True) for t in (Ws, Wn, b)]
    with Kept((xb, xv, lay), (mb, mv, lay)):
        out = ops.concat_dense(xg, mg, par[0], par[1], par[2], relu=True)
        out.backward(dy.to(dev))
    mask = (take(out.detach(), rd) > 0)

    def ref(c):
        ts = [c(t).clone().requires_grad_(True) for t in (x[rows], m[rows], Ws, Wn, b)]
        r = torch.cat([ts[0] @ ts[2], ts[1] @ ts[3]], dim=1) + ts[4]
        o = r * mask.to(r.dtype)
        o.backward(c(dy[rows]))
        return [o.detach()] + [t.grad for t in ts]
    r64, r32 = both(ref)
    Wc = torch.zeros(Fs + Fn, ku + kn, dtype=torch.float64)
    Wc[:Fs, :ku], Wc[Fs:, ku:] = Ws.double().abs(), Wn.double().abs()
    gm = (dy[rows].double() * mask).abs()
    close(take(out.detach(), rd), (r64[0], r32[0]), what=what + " out",
          mag=torch.cat([x[rows], m[rows]], dim=1).double().abs() @ Wc + b.double().abs())
    close(take(xg.grad, rd), (r64[1], r32[1]), what=what + " dx", mag=gm[:, :ku] @ Ws.double().abs().t())
    close(take(mg.grad, rd), (r64[2], r32[2]), what=what + " dm", mag=gm[:, ku:] @ Wn.double().abs().t())
    for i, k in ((0, "dWs"), (1, "dWn"), (2, "db")):
        close_all(par[i].grad, (r64[3 + i], r32[3 + i]), what=f"{what} {k}")
    if lay is WIDE[0]:
        with torch.no_grad():
            out0 = ops.concat_dense(x.to(dev), m.to(dev), par[0].detach(), par[1].detach(), par[2].detach(), relu=True)
        assert same_bits(out.detach(), out0), what
    zero = torch.ones(M, dtype=torch.bool, device=dev)
    zero[rd] = False
    assert not bool(xg.grad[zero].any()) and not bool(mg.grad[zero].any()), what     # rows without a gradient stay zero


WGRAD_SHAPES = [(64, 64), (64, 7), (4, 64), (256, 64)]


@pytest.mark.parametrize("lay", WIDE, ids=IDS)
@pytest.mark.parametrize("F,d", WGRAD_SHAPES)
def test_weight_gradient(dev, lay, F, d):
    """_raw_dense_wgrad and _raw_dense_wgrad_relu with P, G, Y and GM as wide slices: the MFMA form, the narrow-output
    (d = 7) and narrow-input (F = 4) forms; a reduction over all 70 000 rows, float64 on the host"""
    M = N_WIDE
    need(wide_bytes(4), "wgrad")
    P, G, Y = rnd(M, F, seed=F), rnd(M, d, seed=F + d), rnd(M, d, seed=F + d + 1)
    Pb, Pv = wide_of(P, lay, dev)
    Gb, Gv = wide_of(G, lay, dev)
    Yb, Yv = wide_of(Y, lay, dev)
    for relu in (False, True):
        what = f"wide wgrad F={F} d={d} relu={relu} [{lay[0]}]"
        gm_ref = G * (Y > 0) if relu else G
        refW = both(lambda c: c(P).t() @ c(gm_ref))
        refb = both(lambda c: c(gm_ref).sum(0))
        if relu:
            mb, mv = wide_empty(M, d, lay, dev)
            with Kept((Pb, Pv, lay), (Gb, Gv, lay), (Yb, Yv, lay)):
                r = ops._raw_dense_wgrad_relu(Pv, Gv, Yv, want_bias=True, gm_out=mv)
            assert r is not None, what
            dW, db, gm = r
            assert_beside(mb, lay, d, what)
            assert torch.equal(mv.cpu(), gm_ref), what                        # a masked copy: exact
            del mb, mv
        else:
            with Kept((Pb, Pv, lay), (Gb, Gv, lay)):
                dW, db = ops._raw_dense_wgrad(Pv, Gv, want_bias=True)
            assert dW is not None, what
        finite(dW, what)
        close_all(dW, refW, what=what + " dW")
        close_all(db, refb, what=what + " db")
        if lay is WIDE[0]:
            if relu:
                dW0, db0, _ = ops._raw_dense_wgrad_relu(P.to(dev), G.to(dev), Y.to(dev), want_bias=True)
            else:
                dW0, db0 = ops._raw_dense_wgrad(P.to(dev), G.to(dev), want_bias=True)
            assert same_bits(dW, dW0) and same_bits(db, db0), what


def bn_ws(N, d, dev):
    nb = C.c_size_t(0)
    check(_lib.lib().mp_bn_ws_bytes(N, d, C.byref(nb)))
    return torch.empty(nb.value, dtype=torch.uint8, device=dev), nb.value


@pytest.mark.parametrize("lay", WIDE, ids=IDS)
def test_batchnorm(dev, lay):
    """mp_bn_train_fwd_f32, _bwd_f32 and _bwd_relu_f32 with x, y, dy and dx as wide slices"""
    L = _lib.lib()
    N, d, eps = N_WIDE, 64, 1e-5
    need(wide_bytes(5), "batchnorm")
    rows = sample_rows(N, seed=4)
    rd = rows.to(dev)
    x = rnd(N, d, seed=40) * 2 + rnd(d, seed=41)
    dy = rnd(N, d, seed=42)
    gamma = torch.rand(d, generator=torch.Generator().manual_seed(d)) + 0.5
    beta = rnd(d, seed=43) * 0.1
    gd, bd = gamma.to(dev), beta.to(dev)
    ws, nb = bn_ws(N, d, dev)
    stat = lambda: [torch.empty(d, device=dev) for _ in range(3)]

    def fwd(c):
        xc = c(x)
        mean, var = xc.mean(0), xc.var(0, unbiased=False)
        y = torch.relu((xc[rows] - mean) / torch.sqrt(var + eps) * c(gamma) + c(beta))
        return y, mean.view(-1, 1), (1 / torch.sqrt(var + eps)).view(-1, 1), (var * N / (N - 1)).view(-1, 1)
    f64, f32 = both(fwd)
    what = f"wide bn forward [{lay[0]}]"
    xb, xv = wide_of(x, lay, dev)
    yb, yv = wide_empty(N, d, lay, dev)
    mean, invstd, var = stat()
    with Kept((xb, xv, lay)):
        check(L.mp_bn_train_fwd_f32(ptr(xv), xv.stride(0), N, d, ptr(gd), ptr(bd), eps, 1, ptr(yv), yv.stride(0),
                                    ptr(mean), ptr(invstd), ptr(var), ptr(ws), nb, _stream()), what)
    assert_beside(yb, lay, d, what)
    assert_written(yv, what)
    got = take(yv, rd)
    finite(got, what)
    close(got, (f64[0], f32[0]), what=what)
    close(mean.view(-1, 1), (f64[1], f32[1]), what=what + " mean", mag=x.double().abs().mean(0).view(-1, 1))
    for g_, i in ((invstd, 2), (var, 3)):
        close(g_.view(-1, 1), (f64[i], f32[i]), what=f"{what} statistic {i}")
    if lay is WIDE[0]:
        y0 = torch.empty(N, d, device=dev)
        m0, i0, v0 = stat()
        xd = x.to(dev)
        check(L.mp_bn_train_fwd_f32(ptr(xd), d, N, d, ptr(gd), ptr(bd), eps, 1, ptr(y0), d, ptr(m0), ptr(i0), ptr(v0),
                                    ptr(ws), nb, _stream()), what)
        assert same_bits(yv, y0) and same_bits(mean, m0) and same_bits(invstd, i0), what
    mask_all = (yv > 0).cpu()

    def bwd(c):
        xc, g = c(x), c(dy) * mask_all.to(c(dy).dtype)
        mean_, var_ = xc.mean(0), xc.var(0, unbiased=False)
        istd = 1 / torch.sqrt(var_ + eps)
        xh = (xc - mean_) * istd
        dbeta, dgamma = g.sum(0), (g * xh).sum(0)
        dx = c(gamma) * istd * (g - dbeta / N - xh * dgamma / N)
        return dx[rows], dgamma, dbeta
    b64, b32 = both(bwd)
    gb, gv = wide_of(dy, lay, dev)
    for from_x in (False, True):
        what = f"wide bn backward mask from x={from_x} [{lay[0]}]"
        ob, ov = wide_empty(N, d, lay, dev)
        dgamma, dbeta, _ = stat()
        with Kept((gb, gv, lay), (xb, xv, lay), (yb, yv, lay)):
            if from_x:
                check(L.mp_bn_train_bwd_relu_f32(ptr(gv), gv.stride(0), ptr(xv), xv.stride(0), N, d, ptr(gd), ptr(bd),
                                                 ptr(mean), ptr(invstd), ptr(ov), ov.stride(0), ptr(dgamma), ptr(dbeta),
                                                 ptr(ws), nb, _stream()), what)
            else:
                check(L.mp_bn_train_bwd_f32(ptr(gv), gv.stride(0), ptr(yv), yv.stride(0), ptr(xv), xv.stride(0), N, d,
                                            ptr(gd), ptr(mean), ptr(invstd), ptr(ov), ov.stride(0), ptr(dgamma),
                                            ptr(dbeta), ptr(ws), nb, _stream()), what)
        assert_beside(ob, lay, d, what)
        assert_written(ov, what)
        got = take(ov, rd)
        finite(got, what)
        close(got, (b64[0], b32[0]), what=what + " dx")
        close_all(dgamma, (b64[1], b32[1]), what=what + " dgamma")
        close_all(dbeta, (b64[2], b32[2]), what=what + " dbeta")
        if lay is WIDE[0]:
            o0, dyd = torch.empty(N, d, device=dev), dy.to(dev)
            dg0, db0, _ = stat()
            if from_x:
                check(L.mp_bn_train_bwd_relu_f32(ptr(dyd), d, ptr(xd), d, N, d, ptr(gd), ptr(bd), ptr(mean), ptr(invstd),
                                                 ptr(o0), d, ptr(dg0), ptr(db0), ptr(ws), nb, _stream()), what)
            else:
                check(L.mp_bn_train_bwd_f32(ptr(dyd), d, ptr(y0), d, ptr(xd), d, N, d, ptr(gd), ptr(mean), ptr(invstd),
                                            ptr(o0), d, ptr(dg0), ptr(db0), ptr(ws), nb, _stream()), what)
            assert same_bits(ov, o0) and same_bits(dgamma, dg0) and same_bits(dbeta, db0), what
        del ob, ov


@pytest.mark.parametrize("lay", WIDE, ids=IDS)
@pytest.mark.parametrize("form", ["all-rows", "unique-index", "repeating-index"])
def test_softmax_cross_entropy(dev, lay, form):
    """mp_softmax_ce_rows_f32 / _bwd_f32, logits and dlogits wide slices with C = 7: every row, a unique index, and an
    index that lists some rows past 2^31 elements twice (the accumulating form)"""
    L = _lib.lib()
    n, Cn = N_WIDE, 7
    need(wide_bytes(2), "softmax CE")
    what = f"wide softmax CE {form} [{lay[0]}]"
    g = torch.Generator().manual_seed(50)
    z = torch.randn(n, Cn, generator=g) * 3
    if form == "all-rows":
        idx, sel = None, torch.arange(n)
    else:
        idx = torch.unique(torch.cat([sample_rows(n, seed=5), torch.arange(ROW_ELEMS31 - 50, n, 7)]))
        if form == "repeating-index":
            idx = torch.cat([idx, idx[idx >= ROW_ELEMS31][::3], torch.tensor([n - 1, n - 1])])
        idx = idx[torch.randperm(idx.numel(), generator=g)]
        sel = idx
    n_sel = sel.numel()
    lab = torch.randint(0, Cn, (n_sel,), generator=g)
    gs, inv_n = torch.tensor([0.75]), 1.0 / n_sel

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
    zb, zv = wide_of(z, lay, dev)
    db, dv = wide_empty(n, Cn, lay, dev)
    dv.zero_()
    loss = torch.empty(n_sel, device=dev)
    with Kept((zb, zv, lay)):
        check(L.mp_softmax_ce_rows_f32(ptr(zv), zv.stride(0), n, ptr(labd), ptr(idxd), n_sel, Cn, ptr(loss), _stream()),
              what)
        check(L.mp_softmax_ce_bwd_f32(ptr(zv), zv.stride(0), n, ptr(labd), ptr(idxd), n_sel, Cn, ptr(gsd), inv_n, ptr(dv),
                                      dv.stride(0), _stream()), what)
    assert_beside(db, lay, Cn, what)
    finite(loss, what), finite(dv, what)
    close(loss[:, None], (r64[0], r32[0]), what=what + " loss", mag=mag_loss)
    close(dv, (r64[1], r32[1]), what=what + " dlogits", mag=mag_grad)        # every row: the untouched ones are zero
    zd, d0, l0 = z.to(dev), torch.zeros(n, Cn, device=dev), torch.empty(n_sel, device=dev)
    check(L.mp_softmax_ce_rows_f32(ptr(zd), Cn, n, ptr(labd), ptr(idxd), n_sel, Cn, ptr(l0), _stream()), what)
    check(L.mp_softmax_ce_bwd_f32(ptr(zd), Cn, n, ptr(labd), ptr(idxd), n_sel, Cn, ptr(gsd), inv_n, ptr(d0), Cn,
                                  _stream()), what)
    assert same_bits(loss, l0), what
    if form != "repeating-index":               # (repeated rows accumulate with float atomics)
        assert same_bits(dv, d0), what


@pytest.mark.parametrize("lay", WIDE, ids=IDS)
def test_row_gather_scatter_and_identity_rows(dev, lay):
    """gather_rows / index_add_rows and the two entry points with X, H, U and out as wide slices, the indices
    concentrated past the thresholds; mp_id_fixup_f32 / mp_id_rows_f32 with Z and out as wide slices.  Copies and adds
    in entry order: exact, and the contiguous call's bits"""
    L = _lib.lib()
    n, d = N_WIDE, 20
    need(wide_bytes(4), "rows")
    what = f"wide rows [{lay[0]}]"
    g = torch.Generator().manual_seed(60)
    x, u = rnd(n, d, seed=61), rnd(n, d, seed=62)          # u is [n, d] too: its own rows k.. cross the thresholds
    ids = torch.cat([torch.randperm(n - ROW_ELEMS31, generator=g)[:4000] + ROW_ELEMS31,
                     torch.randperm(ROW_ELEMS31 - ROW_BYTES32, generator=g)[:1500] + ROW_BYTES32,
                     torch.randperm(ROW_BYTES32, generator=g)[:499], torch.tensor([n - 1])])
    ids = torch.unique(ids)
    ids = ids[torch.randperm(ids.numel(), generator=g)]
    k = ids.numel()
    idd = ids.to(dev)
    # U's rows: the last k rows of a wide buffer, so they lie past the thresholds too
    xb, xv = wide_of(x, lay, dev)
    ub, uv_all = wide_of(u, lay, dev)
    uv = uv_all[n - k:]
    uk = u[n - k:]
    want_g, want_s = x[ids], x.index_add(0, ids, uk)
    with Kept((xb, xv, lay), (ub, uv_all, lay)):
        assert torch.equal(ops.gather_rows(xv, idd).cpu(), want_g), what
        assert torch.equal(ops.index_add_rows(xv, idd, uv).cpu(), want_s), what
        ob, ov_all = wide_empty(n, d, lay, dev)
        ov = ov_all[n - k:]                                 # the gathered rows land past the thresholds
        check(L.mp_rows_gather_f32(ptr(xv), xv.stride(0), ptr(idd), k, d, ptr(ov), ov.stride(0), _stream()), what)
    assert torch.equal(ov.cpu(), want_g), what
    ov.view(torch.int32).fill_(SENTINEL)
    assert_beside(ob, lay, 0, what)                         # nothing else of the buffer was written
    hb, hv = ob, ov_all
    hv.copy_(x)
    with Kept((ub, uv_all, lay)):
        check(L.mp_rows_scatter_add_f32(ptr(hv), hv.stride(0), ptr(idd), k, d, ptr(uv), uv.stride(0), _stream()), what)
    assert_beside(hb, lay, d, what)
    assert torch.equal(hv.cpu(), want_s), what
    del xb, xv, ub, uv_all, uv
    # identity rows: rows past the thresholds own entries; Z is a wide slice whose slots cross them too
    n_id, n_rows = n, 3000
    rows = torch.sort(torch.cat([torch.randperm(n - ROW_ELEMS31, generator=g)[:n_rows - 500] + ROW_ELEMS31,
                                 torch.randperm(ROW_ELEMS31, generator=g)[:500]])).values
    cnt = torch.randint(1, 5, (n_rows,), generator=g)
    crp = torch.cat([torch.zeros(1, dtype=torch.int64), cnt.cumsum(0)])
    slot = torch.randint(0, n_id, (int(crp[-1]),), generator=g)
    val = torch.rand(int(crp[-1]), generator=g) - 0.3
    Z, out0 = rnd(n_id, d, seed=63), rnd(n, d, seed=64)
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
    rdv, cd, sd, vd = i32(rows), i32(crp), i32(slot), val.to(dev)
    Zb, Zv = wide_of(Z, lay, dev)
    for fix in (True, False):
        what = f"wide identity rows fixup={fix} [{lay[0]}]"
        refs, mag = both(lambda c: ref(c, fix)), both(lambda c: ref(c, fix, True))[0]
        hv.view(torch.int32).fill_(SENTINEL)
        c0 = torch.full((n, d), SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
        Zd = Z.to(dev)
        with Kept((Zb, Zv, lay)):
            if fix:
                hv.copy_(out0), c0.copy_(out0)
                check(L.mp_id_fixup_f32(ptr(rdv), ptr(cd), ptr(sd), ptr(vd), n_rows, ptr(Zv), Zv.stride(0), ptr(hv),
                                        hv.stride(0), d, _lib.ACT_RELU, _stream()), what)
                check(L.mp_id_fixup_f32(ptr(rdv), ptr(cd), ptr(sd), ptr(vd), n_rows, ptr(Zd), d, ptr(c0), d, d,
                                        _lib.ACT_RELU, _stream()), what)
                got = hv
            else:
                check(L.mp_id_rows_f32(ptr(rdv), ptr(cd), ptr(sd), ptr(vd), n_rows, ptr(Zv), Zv.stride(0), ptr(hv),
                                       hv.stride(0), d, _stream()), what)
                check(L.mp_id_rows_f32(ptr(rdv), ptr(cd), ptr(sd), ptr(vd), n_rows, ptr(Zd), d, ptr(c0), d, d, _stream()),
                      what)
                got = hv[rdv.long()]
        assert_beside(hb, lay, d, what)
        assert same_bits(hv, c0), what                       # rows that are not listed keep the sentinel in both
        finite(got, what)
        close(got, refs, what=what, mag=mag)


BF_CASES = [("sum", True, False), ("mean", False, False), ("max", True, True)]


@pytest.mark.parametrize("lay", WIDE, ids=IDS)
@pytest.mark.parametrize("case", BF_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_bf16_aggregation(dev, wg, lay, case):
    """mp_spmm_csr_bf16 with x, S and out as wide bf16 slices (both thresholds at row 65 536): bit for bit the fp32
    plan kernel on x.float() rounded once — the contract of tests/test_spmm_bf16_gpu.py —, and float64 on sampled rows"""
    reduce, has_bias, want_arg = case
    n, d, G, sub = N_WIDE, 128, wg.G, wg.sub
    need(wide_bytes(3, elem=2) + wide_bytes(0), "bf16 aggregation")
    what = f"wide bf16 {reduce} [{lay[0]}]"
    x = rnd(n, d, seed=70).to(BF)
    b = rnd(d, seed=71) if has_bias else None
    red = _lib.REDUCE[reduce]
    scale = 0.5 if reduce == "sum" else 0.0
    xb, xv = wide_of(x, lay, dev)
    ob, ov = wide_empty(n, d, lay, dev, BF)
    bd = None if b is None else b.to(dev)
    with Kept((xb, xv, lay)):
        y, arg = ops._raw_spmm(G, xv, red, S=xv if scale else None, self_scale=scale, bias=bd, want_argmax=want_arg,
                               out=ov)
    assert_beside(ob, lay, d, what)
    assert_written(ov, what)
    xf = x.float()
    y32, a32 = ops._raw_spmm(G, xf.to(dev), red, S=xf.to(dev) if scale else None, self_scale=scale, bias=bd,
                             want_argmax=want_arg)
    assert same_bits(ov, y32.to(BF)), what
    if want_arg:
        assert torch.equal(arg, a32), what
        assert torch.equal(take(arg, wg.sd).long(), argmax_ref(sub, sub.val[:, None], xf)), what
    # float64: one bf16 rounding of the result (2^-8 relative) on top of the fp32 bar, against the sum of absolute terms
    r64 = agg_ref(lambda t: t.double(), sub, sub.val, xf, xf if scale else None, scale, b, False, reduce)
    mag = agg_ref(lambda t: t.double(), sub, sub.val, xf, xf if scale else None, scale, b, False,
                  "sum" if reduce == "max" else reduce, absolute=True)
    got = take(ov, wg.sd)
    finite(got, what)
    bf16_close(got, r64, mag, what)


@pytest.mark.parametrize("lay", WIDE, ids=IDS)
def test_bf16_two_branch_and_max_backward(dev, wg, lay):
    n, d, G, sub = N_WIDE, 128, wg.G, wg.sub
    need(wide_bytes(3, elem=2) + wide_bytes(0), "bf16 two-branch")
    what = f"wide bf16 two-branch [{lay[0]}]"
    x = rnd(n, d, seed=72).to(BF)
    ids = torch.unique(torch.cat([torch.randperm(n, generator=torch.Generator().manual_seed(7))[: n // 9],
                                  torch.arange(ROW_ELEMS31, ROW_ELEMS31 + 300)])).to(dev)
    xb, xv = wide_of(x, lay, dev)
    Pb, Pv = wide_empty(n, d, lay, dev, BF)
    Qb, Qv = wide_empty(n, d, lay, dev, BF)
    with Kept((xb, xv, lay)):
        plan, counts, ws, nb = ops._plan_ws(G, dev, d, SUM, True)
        check(_lib.lib().mp_idgnn_agg_bf16(ptr(G.rowptr), ptr(G.mark_ids(ids)), ptr(G.val), n, ptr(plan), counts, ptr(xv),
                                           xv.stride(0), ptr(Pv), Pv.stride(0), ptr(Qv), Qv.stride(0), d, ptr(ws), nb,
                                           _stream()), what)
        P2, Q2 = ops.idgnn_aggregate(G, ids, xv)
    assert_beside(Pb, lay, d, what), assert_beside(Qb, lay, d, what)
    P32, Q32 = ops.idgnn_aggregate(G, ids, x.float().to(dev))
    for got in ((Pv, Qv), (P2, Q2)):
        assert same_bits(got[0], P32.to(BF)) and same_bits(got[1], Q32.to(BF)), what
    xf = x.float()
    sel = torch.zeros(n, 1)
    sel[ids.cpu()] = 1
    for got, src, k in ((Pv, xf, "P"), (Qv, xf * sel, "Q")):
        r64 = agg_ref(lambda t: t.double(), sub, sub.val, src, None, 0.0, None, False, "sum")
        mag = agg_ref(lambda t: t.double(), sub, sub.val, xf, None, 0.0, None, False, "sum", absolute=True)
        bf16_close(take(got, wg.sd), r64, mag, f"{what} {k}")
    del Pb, Pv, Qb, Qv, P2, Q2, P32, Q32
    # the bf16 max backward: dY a wide bf16 slice, dX (fp32, accumulated) a wide fp32 slice
    what = f"wide bf16 max backward [{lay[0]}]"
    _, arg = ops._raw_spmm(G, xv, MAX, want_argmax=True)
    dy = rnd(n, d, seed=73).to(BF)
    argc = arg.cpu().long()
    ref, mag = max_bwd_ref(argc, wg.cols, sub.rows, lambda e, c: wg.val.double()[e], dy)
    yb, yv = wide_of(dy, lay, dev)
    gb, gv = wide_empty(n, d, lay, dev)
    gv.zero_()
    with Kept((yb, yv, lay)):
        check(_lib.lib().mp_spmm_max_bwd_bf16(ptr(G.col), ptr(G.val), ptr(arg), ptr(yv), yv.stride(0), n, d, ptr(gv),
                                              gv.stride(0), _stream()), what)
    assert_beside(gb, lay, d, what)
    got = take(gv, wg.sd)
    finite(got, what)
    close(got, ref, what=what, mag=mag)


# ======================================================================================================= B. natural size
def big_rows(n, seed):
    """sampled rows of a natural-size operand: always some of the last 4096 (past 2^31 elements at d = 256)"""
    g = torch.Generator().manual_seed(seed)
    return torch.unique(torch.cat([torch.tensor([0, 1, (1 << 22) - 1, 1 << 22, (1 << 23) - 1, 1 << 23, n - 2, n - 1]),
                                   torch.randint(0, n, (200,), generator=g),
                                   torch.randint(n - 4096, n, (200,), generator=g)]))


@pytest.fixture(scope="module")
def ba_big(dev):
    need(8 << 30, "BA graph")
    G = ga.CSRGraph.from_edge_index(graphgen.ba_edge_index(N_BIG, 5, seed=3, device=dev), N_BIG).gcn_norm("row")
    yield G
    del G
    torch.cuda.empty_cache()


def big_sub(G, rows):
    """the entries of the sampled rows of a device graph, as a Sub on the host"""
    rp = G.rowptr.long()
    rd = rows.to(G.rowptr.device)
    start, deg = rp[rd], rp[rd + 1] - rp[rd]
    seg = torch.repeat_interleave(torch.arange(rows.numel(), device=rd.device), deg)
    e = torch.arange(int(deg.sum()), device=rd.device) - (torch.cumsum(deg, 0) - deg)[seg] + start[seg]
    s = Sub.__new__(Sub)
    s.e, s.seg, s.other, s.val = e.cpu(), seg.cpu(), G.col[e].cpu().long(), G.val[e].cpu()
    s.rows, s.k = rows, rows.numel()
    return s


def test_max_with_argmax_and_both_backwards_at_natural_size(dev, ba_big):
    """mp_spmm_csr_f32 max with argmax ([N, d] int32, indexed r * d + c), then mp_spmm_max_bwd_f32 and its bf16 form
    (total = N * d > 2^31): sampled rows against float64"""
    G, n, d = ba_big, N_BIG, 256
    assert n * d > 1 << 31
    need(5 * n * d * 4 + (2 << 30), "max at natural size")
    gen = torch.Generator(device=dev).manual_seed(80)
    x = torch.rand(n, d, device=dev, generator=gen) * 2 - 1
    rows = big_rows(n, 80)
    rd = rows.to(dev)
    sub = big_sub(G, rows)
    # x on the host only where the sampled rows' entries read it
    cols_u, inv = torch.unique(sub.other, return_inverse=True)
    xg = x[cols_u.to(dev)].cpu()
    loc = Sub.__new__(Sub)
    loc.e, loc.seg, loc.other, loc.val, loc.rows, loc.k = sub.e, sub.seg, inv, sub.val, torch.arange(sub.k), sub.k
    y, arg = ops._raw_spmm(G, x, MAX, want_argmax=True)
    got = take(y, rd)
    finite(got, "max at natural size")
    close(got, both(lambda c: agg_ref(c, loc, loc.val, xg, None, 0.0, None, False, "max")), what="max at natural size")
    assert torch.equal(take(arg, rd).long(), argmax_ref(loc, loc.val[:, None], xg)), "argmax at natural size"
    assert int(arg.max()) < G.nnz and int(arg.min()) >= -1
    del y, x
    torch.cuda.empty_cache()
    # backward: dX[col[e], c] += val[e] * dY[r, c]; check the rows of dX that the LAST 4096 rows of dY feed (and all
    # other contributions to those rows), found on the device
    dy = torch.rand(n, d, device=dev, generator=gen) * 2 - 1
    tail = arg[n - 4096:].long()
    tgt = torch.unique(G.col[tail[tail >= 0]].long())[:256]          # rows of dX fed from past 2^31 elements
    tgt = torch.unique(torch.cat([tgt, rd]))
    cidx = torch.arange(d, device=dev)

    def ref_of(g):
        """(float64 rows tgt of dX for the gradient g, the sums of the absolute terms), in row chunks on the device:
        nothing of size [N, d] int64"""
        ref = torch.zeros(tgt.numel(), d, dtype=torch.float64, device=dev)
        mag = torch.zeros_like(ref)
        for r0 in range(0, n, 1 << 20):
            a = arg[r0:r0 + (1 << 20)].long()
            colof = torch.where(a >= 0, G.col[a.clamp(min=0)].long(), torch.full_like(a, -1))
            pos = torch.searchsorted(tgt, colof.clamp(min=0))
            hit = (a >= 0) & (tgt[pos.clamp(max=tgt.numel() - 1)] == colof)
            rr, cc = torch.nonzero(hit, as_tuple=True)
            t = G.val[a[rr, cc]].double() * g[r0 + rr, cc].double()
            ref.index_put_((pos[rr, cc], cidx[cc]), t, accumulate=True)
            mag.index_put_((pos[rr, cc], cidx[cc]), t.abs(), accumulate=True)
            del a, colof, pos, hit
        return ref, mag
    ref, mag = ref_of(dy)
    assert bool((mag.sum(1) > 0).any())
    L = _lib.lib()
    dx = torch.zeros(n, d, device=dev)
    check(L.mp_spmm_max_bwd_f32(ptr(G.col), ptr(G.val), ptr(arg), ptr(dy), d, n, d, ptr(dx), d, _stream()))
    close(dx[tgt].cpu(), ref.cpu(), what="max backward at natural size", mag=mag.cpu())
    # the bf16 form on the bf16 rounding of dy: the same reference with the rounded gradient
    dyb = dy.to(BF)
    del dy
    dx.zero_()
    check(L.mp_spmm_max_bwd_bf16(ptr(G.col), ptr(G.val), ptr(arg), ptr(dyb), d, n, d, ptr(dx), d, _stream()))
    refb, magb = ref_of(dyb)
    close(dx[tgt].cpu(), refb.cpu(), what="bf16 max backward at natural size", mag=magb.cpu())


def colsum64(t, fn, chunk=1 << 19):
    """float64 column sums of fn(rows r0 .. r1 of t as float64) on the device, in row chunks"""
    acc = None
    for r0 in range(0, t.size(0), chunk):
        s = fn(t[r0:r0 + chunk].double(), r0).sum(0)
        acc = s if acc is None else acc + s
    return acc


def test_batchnorm_at_natural_size(dev):
    """BatchNorm forward and both backwards on [2^23 + 4096, 256]: column statistics against a float64 reduction on the
    device in chunks, sampled rows against the formula in float64"""
    L = _lib.lib()
    N, d, eps = N_BIG, 256, 1e-5
    need(4 * N * d * 4 + (3 << 30), "batchnorm at natural size")
    gen = torch.Generator(device=dev).manual_seed(81)
    x = torch.randn(N, d, device=dev, generator=gen)
    x[N - 4096:] += 3.0                                  # the rows past 2^31 elements weigh on every statistic
    gamma = torch.rand(d, device=dev, generator=gen) + 0.5
    beta = torch.randn(d, device=dev, generator=gen) * 0.1
    rows = big_rows(N, 81)
    rd = rows.to(dev)
    ws, nb = bn_ws(N, d, dev)
    y = torch.empty(N, d, device=dev)
    mean, invstd, var = (torch.empty(d, device=dev) for _ in range(3))
    check(L.mp_bn_train_fwd_f32(ptr(x), d, N, d, ptr(gamma), ptr(beta), eps, 1, ptr(y), d, ptr(mean), ptr(invstd),
                                ptr(var), ptr(ws), nb, _stream()))
    m64 = colsum64(x, lambda c, r0: c) / N
    v64 = colsum64(x, lambda c, r0: (c - m64) ** 2) / N
    i64 = 1 / torch.sqrt(v64 + eps)
    mabs = colsum64(x, lambda c, r0: c.abs()) / N
    close(mean.view(-1, 1), m64.view(-1, 1).cpu(), what="big bn mean", mag=mabs.view(-1, 1).cpu())
    close(invstd.view(-1, 1), i64.view(-1, 1).cpu(), what="big bn invstd")
    close(var.view(-1, 1), (v64 * N / (N - 1)).view(-1, 1).cpu(), what="big bn var")
    g64, b64 = gamma.double(), beta.double()
    yref = torch.relu((x[rd].double() - m64) * i64 * g64 + b64)
    y32 = torch.relu((x[rd] - m64.float()) * i64.float() * gamma + beta)
    close(y[rd].cpu(), (yref.cpu(), y32.cpu()), what="big bn forward")
    dy = torch.randn(N, d, device=dev, generator=gen)
    dbeta64 = colsum64(dy, lambda c, r0: c * (y[r0:r0 + c.size(0)] > 0))
    dgamma64 = colsum64(dy, lambda c, r0: c * (y[r0:r0 + c.size(0)] > 0) * (x[r0:r0 + c.size(0)].double() - m64) * i64)
    gs = dy[rd].double() * (y[rd] > 0)
    xh = (x[rd].double() - m64) * i64
    dxref = g64 * i64 * (gs - dbeta64 / N - xh * dgamma64 / N)
    dx = torch.empty(N, d, device=dev)
    for from_x in (False, True):
        what = f"big bn backward mask from x={from_x}"
        dgamma, dbeta = torch.empty(d, device=dev), torch.empty(d, device=dev)
        dx.view(torch.int32).fill_(SENTINEL)
        if from_x:
            check(L.mp_bn_train_bwd_relu_f32(ptr(dy), d, ptr(x), d, N, d, ptr(gamma), ptr(beta), ptr(mean), ptr(invstd),
                                             ptr(dx), d, ptr(dgamma), ptr(dbeta), ptr(ws), nb, _stream()), what)
        else:
            check(L.mp_bn_train_bwd_f32(ptr(dy), d, ptr(y), d, ptr(x), d, N, d, ptr(gamma), ptr(mean), ptr(invstd),
                                        ptr(dx), d, ptr(dgamma), ptr(dbeta), ptr(ws), nb, _stream()), what)
        close_all(dgamma, dgamma64.cpu(), what=what + " dgamma")
        close_all(dbeta, dbeta64.cpu(), what=what + " dbeta")
        mag = (g64 * i64 * (gs.abs() + dbeta64.abs() / N + xh.abs() * dgamma64.abs() / N)).cpu()
        close(dx[rd].cpu(), dxref.cpu(), what=what + " dx", mag=mag)
        assert_written(dx[N - 4096:], what)


def test_gather_and_scatter_add_at_natural_size(dev):
    """gather_rows with n x d > 2^31 output elements from a small X, and the scatter-add back (total = n * d).  X holds
    small integers, so every sum is exact in fp32 whatever the order of the atomics: both are compared exactly"""
    L = _lib.lib()
    n, d, nx = N_BIG, 256, 5000
    need(2 * n * d * 4 + (4 << 30), "gather at natural size")
    gen = torch.Generator(device=dev).manual_seed(82)
    X = torch.randint(-64, 65, (nx, d), device=dev, generator=gen).float()
    idx = torch.randint(0, nx, (n,), device=dev, generator=gen)
    idx[n - 4096:] = torch.arange(4096, device=dev) % 7           # the rows past 2^31 elements feed rows 0 .. 6 of H
    out = ops.gather_rows(X, idx)
    assert out.numel() > 1 << 31
    for r0 in range(0, n, 1 << 20):                               # every row, in chunks
        assert torch.equal(out[r0:r0 + (1 << 20)], X[idx[r0:r0 + (1 << 20)]]), r0
    cnt = torch.bincount(idx, minlength=nx)
    assert int(cnt.max()) * 64 < 1 << 24                          # every partial sum is an integer below 2^24
    H = torch.zeros(nx, d, device=dev)
    check(L.mp_rows_scatter_add_f32(ptr(H), d, ptr(idx), n, d, ptr(out), d, _stream()))
    assert torch.equal(H.double(), cnt.double()[:, None] * X.double())


def test_weight_gradient_relu_at_natural_size(dev):
    """_raw_dense_wgrad_relu at M = 2^23 + 4096, d = 256 (G, Y and GM just over 2^31 elements): a reduction over all
    rows, so one scale for the tensor (close_all); the last 4096 rows carry a large share of it.  The float32 evaluation
    beside the float64 one is the same product accumulated in fp32 over the same row chunks, on the device"""
    M, F, d = N_BIG, 64, 256
    need(3 * M * d * 4 + M * F * 4 + (3 << 30), "wgrad at natural size")
    gen = torch.Generator(device=dev).manual_seed(83)
    P = torch.randn(M, F, device=dev, generator=gen)
    G = torch.randn(M, d, device=dev, generator=gen)
    Y = torch.randn(M, d, device=dev, generator=gen)
    G[M - 4096:] *= 30.0                                  # a fault in the rows past 2^31 elements moves the result
    r = ops._raw_dense_wgrad_relu(P, G, Y, want_bias=True)
    assert r is not None
    dW, db, gm = r
    W64 = torch.zeros(F, d, dtype=torch.float64, device=dev)
    b64 = torch.zeros(d, dtype=torch.float64, device=dev)
    W32 = torch.zeros(F, d, device=dev)
    for r0 in range(0, M, 1 << 19):
        s = slice(r0, r0 + (1 << 19))
        g = G[s] * (Y[s] > 0)
        assert torch.equal(gm[s], g), r0                  # the masked copy: exact, every row
        W64 += P[s].double().t() @ g.double()
        W32 += P[s].t() @ g
        b64 += g.double().sum(0)
    close_all(dW, (W64.cpu(), W32.cpu()), what="wgrad relu at natural size dW")
    close_all(db, b64.cpu(), what="wgrad relu at natural size db")
    tailW = P[M - 4096:].double().t() @ (G[M - 4096:] * (Y[M - 4096:] > 0)).double()
    assert float(tailW.abs().max()) > 1e-3 * float(W64.abs().max())


def test_bf16_sum_with_bias_at_natural_size(dev, ba_big):
    """mp_spmm_csr_bf16, sum with bias, x and y of 2^31 + 2^20 bf16 elements: the fp32 plan kernel's bits rounded once
    in row chunks, and sampled rows against float64"""
    G, n, d = ba_big, N_BIG, 256
    need(2 * n * d * 2 + 2 * n * d * 4 + (2 << 30), "bf16 at natural size")
    gen = torch.Generator(device=dev).manual_seed(84)
    x = (torch.rand(n, d, device=dev, generator=gen) * 2 - 1).to(BF)
    b = torch.randn(d, device=dev, generator=gen)
    y, _ = ops._raw_spmm(G, x, SUM, bias=b)
    assert y.dtype == BF and y.numel() > 1 << 31
    xf = x.float()
    y32, _ = ops._raw_spmm(G, xf, SUM, bias=b)
    for r0 in range(0, n, 1 << 20):
        assert same_bits(y[r0:r0 + (1 << 20)], y32[r0:r0 + (1 << 20)].to(BF)), r0
    del y32
    rows = big_rows(n, 84)
    sub = big_sub(G, rows)
    cols_u, inv = torch.unique(sub.other, return_inverse=True)
    xg = xf[cols_u.to(dev)].cpu()
    sub.other, sub.rows = inv, torch.arange(sub.k)
    r64 = agg_ref(lambda t: t.double(), sub, sub.val, xg, None, 0.0, b.cpu(), False, "sum")
    mag = agg_ref(lambda t: t.double(), sub, sub.val, xg, None, 0.0, b.cpu(), False, "sum", absolute=True)
    bf16_close(y[rows.to(dev)].cpu(), r64, mag, "bf16 at natural size")
