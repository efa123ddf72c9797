"""The bf16 aggregation (mp_spmm_csr_bf16, mp_idgnn_agg_bf16, mp_spmm_max_bwd_bf16): bf16 storage, fp32 accumulation.

Every output is, bit for bit, the fp32 plan-based kernel (mp_spmm_csr_f32) run on the widened input with the same plan,
rounded once to bf16; argmax is bit for bit its argmax.  The float64 oracle checks the same outputs within one bf16
rounding (2^-8 relative) plus the fp32 accumulation (1e-5 of the row's magnitude)."""
import pytest
import torch

import graphgym_amd as ga
from graphgym_amd import _lib, graphgen, ops
from oracle import ref_ops as R

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


@pytest.fixture(autouse=True)
def plan_kernel(monkeypatch):
    monkeypatch.setenv("MP_AGG_TILES", "0")      # the fp32 side runs the plan-based kernel at every size


def graph(dev, n, E, seed, weighted, hubs=False):
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


def bits_equal(a, b):
    return a.dtype == b.dtype == BF and torch.equal(a.view(torch.int16), b.view(torch.int16))


def oracle_close(y, y64, mag, what):
    """|y - y64| <= 2^-8 |y64| elementwise + 1e-5 * (the row's largest magnitude)"""
    err = (y.double().cpu() - y64).abs()
    tol = 2.0 ** -8 * y64.abs() + 1e-5 * mag.abs().amax(dim=1, keepdim=True)
    bad = err > tol
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} elements outside the bound, worst {float((err - tol).max())}"


def bf16_input(n, d, seed, ld=None, off=0, dev=None):
    """bf16 x [n, d]; with ld: a column slice at element offset `off` of an [n, ld] buffer (ldx > d, 2- or 4-byte
    aligned base pointers)"""
    g = torch.Generator().manual_seed(seed)
    if ld is None:
        return torch.randn(n, d, generator=g).to(BF).to(dev)
    buf = torch.randn(n, ld, generator=g).to(BF).to(dev)
    return buf[:, off:off + d]


CASES = [   # reduce, weighted, self_scale, bias, relu
    ("sum", True, 0.0, None, False), ("sum", False, 0.0, None, False), ("sum", True, 1.5, "f32", True),
    ("sum", False, 0.7, "bf16", False), ("mean", True, 0.0, None, False), ("mean", False, 0.5, "f32", True),
    ("max", True, 0.0, None, False), ("max", False, 0.0, "f32", True), ("max", True, 1.25, None, False)]


@pytest.mark.parametrize("d", [1, 3, 8, 64, 96, 128, 200, 256, 512])
@pytest.mark.parametrize("case", CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_bits_equal_the_fp32_plan_kernel(dev, monkeypatch, d, case):
    reduce, weighted, self_scale, bias_kind, relu = case
    monkeypatch.setattr(ga.CSRGraph, "PLAN_CONFIG", (64, 1, 64, 64))     # many hubs: rows of > 64 entries in pieces
    n = 700
    G, *_ = graph(dev, n, 9000, d * 31 + len(reduce), weighted, hubs=True)
    assert G.plan()[1][1] > 0                                           # the hub path runs
    x = bf16_input(n, d, d, dev=dev)
    gen = torch.Generator().manual_seed(7)
    b32 = (torch.randn(d, generator=gen)).to(dev) if bias_kind else None
    b = b32.to(BF) if bias_kind == "bf16" else b32
    red = _lib.REDUCE[reduce]
    want_arg = reduce == "max"
    S = x if self_scale else None
    yb, ab = ops._raw_spmm(G, x, red, S=S, self_scale=self_scale, bias=b, relu=relu, want_argmax=want_arg)
    xf = x.float()
    y32, a32 = ops._raw_spmm(G, xf, red, S=xf if self_scale else None, self_scale=self_scale,
                             bias=None if b is None else b.float(), relu=relu, want_argmax=want_arg)
    assert bits_equal(yb, y32.to(BF))
    if want_arg:
        assert torch.equal(ab, a32)
    # the public operator: the same launch
    out = ops.spmm(G, x, reduce, self_scale=self_scale, bias=b, relu=relu)
    assert bits_equal(out, yb)


@pytest.mark.parametrize("ld,off", [(260, 1), (260, 2), (264, 8), (515, 3)])
@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
def test_column_slices_and_narrow_alignment(dev, ld, off, reduce):
    n, d = 900, 256 if ld < 500 else 500
    G, *_ = graph(dev, n, 12000, ld + off, True)
    x = bf16_input(n, d, ld, ld=ld, off=off, dev=dev)
    assert x.stride(0) == ld and x.data_ptr() % 4 == (2 if off % 2 else 0)
    red = _lib.REDUCE[reduce]
    yb, ab = ops._raw_spmm(G, x, red, S=x if reduce == "sum" else None, self_scale=0.5 if reduce == "sum" else 0.0,
                           want_argmax=reduce == "max")
    xf = x.float()
    y32, a32 = ops._raw_spmm(G, xf, red, S=xf if reduce == "sum" else None,
                             self_scale=0.5 if reduce == "sum" else 0.0, want_argmax=reduce == "max")
    assert bits_equal(yb, y32.to(BF))
    if reduce == "max":
        assert torch.equal(ab, a32)


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
def test_against_the_float64_oracle(dev, monkeypatch, reduce):
    monkeypatch.setattr(ga.CSRGraph, "PLAN_CONFIG", (64, 1, 64, 64))
    n, d = 600, 96
    G, dst, src, w = graph(dev, n, 8000, 11, True, hubs=True)
    x = bf16_input(n, d, 12, dev=dev)
    gen = torch.Generator().manual_seed(13)
    bias = torch.randn(d, generator=gen).to(dev)
    y = ops.spmm(G, x, reduce, bias=bias)
    x64, w64 = x.double().cpu(), w.double()
    y64 = R.coo_aggregate(dst, src, w64, x64, n, reduce) + bias.double().cpu()
    mag = R.coo_aggregate(dst, src, w64.abs(), x64.abs(), n, reduce if reduce != "max" else "sum")
    oracle_close(y, y64, mag + bias.double().cpu().abs(), f"bf16 {reduce}")


def test_two_branch_form_bits_and_oracle(dev, monkeypatch):
    monkeypatch.setattr(ga.CSRGraph, "PLAN_CONFIG", (64, 1, 64, 64))
    for d in (3, 64, 128, 256):
        n = 800
        G, dst, src, w = graph(dev, n, 10000, 40 + d, True, hubs=True)
        ids = torch.randperm(n, generator=torch.Generator().manual_seed(d))[: n // 9].to(dev)
        x = bf16_input(n, d, d + 1, dev=dev)
        P, Q = ops.idgnn_aggregate(G, ids, x)
        P32, Q32 = ops.idgnn_aggregate(G, ids, x.float())
        assert bits_equal(P, P32.to(BF)) and bits_equal(Q, Q32.to(BF)), d
        sel = torch.zeros(n, 1, dtype=torch.float64)
        sel[ids.cpu()] = 1
        x64 = x.double().cpu()
        oracle_close(Q, R.coo_aggregate(dst, src, w.double(), x64 * sel, n, "sum"),
                     R.coo_aggregate(dst, src, w.double().abs(), x64.abs(), n, "sum"), f"Q d={d}")


def test_ba_graph_of_two_million_nodes(dev):
    n, d = 2_000_000, 256
    G = ga.CSRGraph.from_edge_index(graphgen.ba_edge_index(n, 5, seed=3, device=dev), n).gcn_norm("row")
    x = torch.randn(n, d, device=dev).to(BF)
    for reduce in ("sum", "mean", "max"):
        red = _lib.REDUCE[reduce]
        yb, _ = ops._raw_spmm(G, x, red)
        y32, _ = ops._raw_spmm(G, x.float(), red)
        assert bits_equal(yb, y32.to(BF)), reduce


@pytest.mark.parametrize("reduce", ["sum", "mean"])
@pytest.mark.parametrize("self_scale", [0.0, 1.5])
def test_input_gradient_bits_equal_the_fp32_path(dev, monkeypatch, reduce, self_scale):
    monkeypatch.setattr(ga.CSRGraph, "PLAN_CONFIG", (64, 1, 64, 64))
    n, d = 700, 128
    G, *_ = graph(dev, n, 9000, 5, True, hubs=True)
    x0 = bf16_input(n, d, 6, dev=dev)
    dy = torch.randn(n, d, generator=torch.Generator().manual_seed(8)).to(BF).to(dev)
    xb = x0.clone().requires_grad_(True)
    ops.spmm(G, xb, reduce, self_scale=self_scale).backward(dy)
    x32 = x0.float().requires_grad_(True)
    ops.spmm(G, x32, reduce, self_scale=self_scale).backward(dy.float())
    assert xb.grad.dtype == BF and bits_equal(xb.grad, x32.grad.to(BF))


@pytest.mark.parametrize("bias_dtype", [torch.float32, BF])
def test_max_and_bias_gradients_against_the_oracle(dev, bias_dtype):
    n, d = 500, 64
    G, dst, src, w = graph(dev, n, 6000, 9, True)
    x0 = bf16_input(n, d, 10, dev=dev)
    dy = torch.randn(n, d, generator=torch.Generator().manual_seed(12)).to(BF).to(dev)
    xb = x0.clone().requires_grad_(True)
    bias = torch.randn(d, generator=torch.Generator().manual_seed(14)).to(bias_dtype).to(dev).requires_grad_(True)
    ops.spmm(G, xb, "max", bias=bias).backward(dy)
    assert xb.grad.dtype == BF and bias.grad.dtype == bias_dtype
    # oracle: the gradient flows to the winning entry of every (row, column), ties to the first entry
    _, arg = ops._raw_spmm(G, x0, _lib.MAX, want_argmax=True)
    arg = arg.long().cpu()
    dy64 = dy.double().cpu()
    col, val = G.col.long().cpu(), G.val.double().cpu()
    dx64 = torch.zeros(n, d, dtype=torch.float64)
    r, c = torch.nonzero(arg >= 0, as_tuple=True)
    e = arg[r, c]
    dx64.index_put_((col[e], c), val[e] * dy64[r, c], accumulate=True)
    mag = torch.zeros(n, d, dtype=torch.float64).index_put_((col[e], c), (val[e] * dy64[r, c]).abs(), accumulate=True)
    oracle_close(xb.grad, dx64, mag, "max dx")
    db64 = dy64.sum(0, keepdim=True)
    oracle_close(bias.grad.view(1, -1), db64, dy64.abs().sum(0, keepdim=True), "bias grad")


def test_custom_ops_opcheck(dev):
    n, d = 300, 64
    G, *_ = graph(dev, n, 4000, 21, True)
    gen = torch.Generator().manual_seed(0)

    def t(*shape, dtype=BF):
        return torch.randn(*shape, generator=gen).to(dtype).to(dev).requires_grad_(True)
    ids = torch.arange(0, n, 11, device=dev)
    cases = [
        (torch.ops.mp.spmm.default, (t(n, d), G.handle, 0, 0.5, t(d, dtype=torch.float32), True)),
        (torch.ops.mp.spmm.default, (t(n, d), G.handle, 1, 0.0, t(d), False)),
        (torch.ops.mp.spmm.default, (t(n, d), G.handle, 2, 0.0, None, False)),
        (torch.ops.mp.idgnn_agg.default, (t(n, d), G.handle, ids)),
    ]
    for op, args in cases:
        res = torch.library.opcheck(op, args, raise_exception=True)
        assert all(v == "SUCCESS" for v in res.values()), (op, res)


def test_other_dtypes_still_raise(dev):
    G, *_ = graph(dev, 100, 500, 1, False)
    with pytest.raises(TypeError):
        ops.spmm(G, torch.randn(100, 8, device=dev).half(), "sum")
    with pytest.raises(TypeError):
        ops.idgnn_aggregate(G, torch.arange(3, device=dev), torch.randn(100, 8, device=dev).half())
    with pytest.raises(TypeError):
        ops.spmm(G, torch.randn(100, 8, device=dev).double(), "mean")


def test_bf16_never_takes_the_tile_kernels(dev, monkeypatch):
    monkeypatch.setenv("MP_AGG_TILES", "1")
    monkeypatch.setattr(ops, "AGG_TILES_MIN_ROWS", 1)
    G, *_ = graph(dev, 3000, 30000, 2, True)
    x = bf16_input(3000, 256, 3, dev=dev)
    t0, h0 = ops.AGG_TILES_CALLS, ops.AGG_HOT_CALLS
    ops.spmm(G, x, "sum")
    ops.idgnn_aggregate(G, torch.arange(0, 3000, 7, device=dev), x)
    assert (ops.AGG_TILES_CALLS, ops.AGG_HOT_CALLS) == (t0, h0)
    ops.spmm(G, x.float(), "sum")
    assert ops.AGG_TILES_CALLS == t0 + 1
