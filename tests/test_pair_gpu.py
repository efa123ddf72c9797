"""The pair decoders on the device (graphgym_amd/pair_ops.py over include/mp_pair.h): ops.pair_score (dot, cosine) and
ops.pair_sum against the reference's composition of tests/_pair_ref.py in float64 / float32 (tests/_tol.py), operand
layouts, degenerate inputs, out-of-range indices, host reads and determinism, the op checks, the memory bound, the head's
route and a three-step training run on each route."""
import contextlib
import copy

import pytest
import torch
from torch.utils._python_dispatch import TorchDispatchMode

import _gradsub
import _pair_ref as R
from _bigview import N_WIDE, WIDE, Kept, need, sample_rows, wide_of
from _tol import both, close, close_all

pytestmark = pytest.mark.gpu

DS = (1, 3, 4, 20, 64, 100, 256, 260, 516)
MS = (1, 3, 16, 128, 260)
_REF = {}


def _score_ref(K, d, cosine):
    """(h, index, g, (r64, r32), score mag, gradient mag) of one shape, computed once and shared"""
    key = (K, d, cosine)
    if key not in _REF:
        h, idx = R.features(d), R.pairs(K)
        g = torch.randn(K, generator=torch.Generator().manual_seed(2))
        refs = both(R.score_and_grad(h, idx, g, cosine))
        _REF[key] = (h, idx, g, refs, R.score_mag(h, idx, cosine), R.grad_mag(h, idx, g, refs[0][0], cosine))
    return _REF[key]


def _check_score(s, dh, K, d, cosine, what):
    h, idx, g, (r64, r32), smag, gmag = _score_ref(K, d, cosine)
    close(s[:, None], (r64[0][:, None], r32[0][:, None]), mag=smag[:, None], what=f"{what} score")
    close(dh, (r64[1], r32[1]), mag=gmag, what=f"{what} dh")


# ---- parity ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("K", R.KS)
def test_pair_score_parity(dev, K, d):
    from graphgym_amd import ops
    for cosine in (False, True):
        h, idx, g, *_ = _score_ref(K, d, cosine)
        hd = h.to(dev).requires_grad_(True)
        s = ops.pair_score(hd, idx.to(dev), cosine=cosine, eps=R.EPS)
        assert s.shape == (K,) and s.dtype == torch.float32
        s.backward(g.to(dev))
        _check_score(s.detach(), hd.grad, K, d, cosine, f"K={K} d={d} cosine={cosine}")


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("K", R.KS)
def test_pair_sum_parity(dev, K, m):
    from graphgym_amd import ops
    gen = torch.Generator().manual_seed(3)
    U, V, b = torch.randn(R.N, m, generator=gen), torch.randn(R.N, m, generator=gen), torch.randn(m, generator=gen)
    dz, idx = torch.randn(K, m, generator=gen), R.pairs(K)
    for bias in (b, None):
        def ref(c):
            t = [None if v is None else c(v).clone().requires_grad_(True) for v in (U, V, bias)]
            z = R.pair_sum(lambda v: v, t[0], t[1], idx, t[2])
            z.backward(c(dz))
            return [z.detach()] + [v.grad for v in t if v is not None]
        r64, r32 = both(ref)
        Ud, Vd = U.to(dev).requires_grad_(True), V.to(dev).requires_grad_(True)
        bd = None if bias is None else bias.to(dev).requires_grad_(True)
        z = ops.pair_sum(Ud, Vd, idx.to(dev), bd)
        z.backward(dz.to(dev))
        what = f"pair_sum K={K} m={m} bias={bias is not None}"
        close(z.detach(), (r64[0], r32[0]), what=what)
        close(Ud.grad, (r64[1], r32[1]), what=what + " dU")
        close(Vd.grad, (r64[2], r32[2]), what=what + " dV")
        if bias is not None:
            close_all(bd.grad, (r64[3], r32[3]), what=what + " dbias")


def test_concat_is_the_sum_of_two_products(dev):
    """the algebra of the head: F.linear(cat(h[a], h[b]), W, bias) = pair_sum(h W[:, :d]^T, h W[:, d:]^T, index, bias)"""
    from graphgym_amd import ops
    d, m, K = 20, 16, 300
    gen = torch.Generator().manual_seed(4)
    h, W, b, idx = R.features(d), torch.randn(m, 2 * d, generator=gen) / 6, torch.randn(m, generator=gen), R.pairs(K)
    Wd, hd = W.to(dev), h.to(dev)
    z = ops.pair_sum(torch.nn.functional.linear(hd, Wd[:, :d]), torch.nn.functional.linear(hd, Wd[:, d:]), idx.to(dev),
                     b.to(dev))
    mag = both(lambda c: R.concat_linear(c, h.abs(), W.abs(), b.abs(), idx))[0]
    close(z, both(lambda c: R.concat_linear(c, h, W, b, idx)), mag=mag, what="concat as a pair sum")


# ---- operand layouts ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("layout", ["column slice", "row offset", "index slice"])
@pytest.mark.parametrize("d", [20, 64])
def test_operand_layouts(dev, layout, d):
    from graphgym_amd import ops
    K = 257
    for cosine in (False, True):
        h, idx, g, *_ = _score_ref(K, d, cosine)
        hd, id_ = h.to(dev), idx.to(dev)
        if layout == "column slice":        # row stride != d, base misaligned by 4 bytes
            wide = torch.full((R.N, d + 7), float("nan"), device=dev)
            hv = wide[:, 1:1 + d]
            hv.copy_(hd)
            assert hv.stride(0) == d + 7 and hv.data_ptr() % 16 == 4
        elif layout == "row offset":
            tall = torch.full((R.N + 5, d), float("nan"), device=dev)
            hv = tall[3:3 + R.N]
            hv.copy_(hd)
        else:
            hv = hd
            longer = torch.full((2, K + 9), -7, dtype=torch.int64, device=dev)
            longer[:, 4:4 + K] = id_
            id_ = longer[:, 4:4 + K]
            assert id_.stride() == (K + 9, 1) and not id_.is_contiguous()
        leaf = hv.detach().requires_grad_(True)
        s = ops.pair_score(leaf, id_, cosine=cosine)
        s.backward(g.to(dev))
        assert leaf.grad.shape == (R.N, d)
        _check_score(s.detach(), leaf.grad, K, d, cosine, f"{layout} d={d} cosine={cosine}")
    # pair_sum on the same kind of views
    m = d
    gen = torch.Generator().manual_seed(6)
    U, V = torch.randn(R.N, m, generator=gen), torch.randn(R.N, m, generator=gen)
    wide = torch.full((R.N, 2 * m + 3), float("nan"), device=dev)
    Uv, Vv = wide[:, 1:1 + m], wide[:, 1 + m:1 + 2 * m]
    Uv.copy_(U)
    Vv.copy_(V)
    z = ops.pair_sum(Uv, Vv, R.pairs(K).to(dev))
    close(z, both(lambda c: R.pair_sum(c, U, V, R.pairs(K), None)), what="pair_sum on column slices")


def test_offset_beyond_4_gib(dev):
    """h as a column slice of a [70 000, 32 768] buffer: rows past 2^32 bytes and 2^31 elements, forward and backward"""
    from graphgym_amd import ops
    lay, d = WIDE[0], 8
    need(N_WIDE * lay[1] * 4 + (1 << 30), "pair_score on a wide view")
    h = torch.randn(N_WIDE, d, generator=torch.Generator().manual_seed(7))
    rows = sample_rows(N_WIDE)
    idx = torch.stack([rows, rows.flip(0)])
    g = torch.randn(idx.size(1), generator=torch.Generator().manual_seed(8))
    hb, hv = wide_of(h, lay, dev)
    for cosine in (False, True):
        r64, r32 = both(R.score_and_grad(h, idx, g, cosine))
        leaf = hv.detach().requires_grad_(True)
        with Kept((hb, hv, lay)):
            s = ops.pair_score(leaf, idx.to(dev), cosine=cosine)
            s.backward(g.to(dev))
        close(s.detach()[:, None], (r64[0][:, None], r32[0][:, None]), mag=R.score_mag(h, idx, cosine)[:, None],
              what=f"wide score cosine={cosine}")
        close(leaf.grad, (r64[1], r32[1]), mag=R.grad_mag(h, idx, g, r64[0], cosine), what=f"wide dh cosine={cosine}")


# ---- degenerate inputs ------------------------------------------------------------------------------------------------------

def test_no_pairs(dev):
    from graphgym_amd import ops
    h = R.features(12).to(dev).requires_grad_(True)
    idx = torch.zeros((2, 0), dtype=torch.int64, device=dev)
    for cosine in (False, True):
        s = ops.pair_score(h, idx, cosine=cosine)
        assert s.shape == (0,)
        h.grad = None
        s.sum().backward()
        assert h.grad.shape == h.shape and not bool(h.grad.any())
    z = ops.pair_sum(h, h, idx)
    assert z.shape == (0, 12)


@pytest.mark.parametrize("cosine", [False, True])
def test_one_node_and_width_one(dev, cosine):
    from graphgym_amd import ops
    g = torch.tensor([0.5, -2.0, 1.5])
    for h, idx in ((torch.tensor([[1.5, -2.0, 0.25]]), torch.zeros((2, 3), dtype=torch.int64)),       # N = 1
                   (R.features(1), R.pairs(3))):                                                      # d = 1
        r64, r32 = both(R.score_and_grad(h, idx, g, cosine))
        leaf = h.to(dev).requires_grad_(True)
        s = ops.pair_score(leaf, idx.to(dev), cosine=cosine)
        s.backward(g.to(dev))
        close(s.detach()[:, None], (r64[0][:, None], r32[0][:, None]), mag=R.score_mag(h, idx, cosine)[:, None],
              what="tiny score")
        close(leaf.grad, (r64[1], r32[1]), mag=R.grad_mag(h, idx, g, r64[0], cosine), what="tiny dh")


@pytest.mark.parametrize("cosine", [False, True])
def test_all_pairs_on_one_node(dev, cosine):
    """a single hub row of 2K entries at K = 5000: the plan splits it into pieces; a node in no pair gets exactly 0"""
    from graphgym_amd import ops
    K, d = 5000, 20
    h = R.features(d)
    idx = torch.full((2, K), 11, dtype=torch.int64)
    g = torch.randn(K, generator=torch.Generator().manual_seed(9))
    r64, r32 = both(R.score_and_grad(h, idx, g, cosine))
    leaf = h.to(dev).requires_grad_(True)
    s = ops.pair_score(leaf, idx.to(dev), cosine=cosine)
    s.backward(g.to(dev))
    pi = ops.pair_index(idx.to(dev), R.N)
    assert pi.graph.nnz == 2 * K and pi.graph.plan()[1][1] > 0, "the long-row split must be live"
    close(s.detach()[:, None], (r64[0][:, None], r32[0][:, None]), mag=R.score_mag(h, idx, cosine)[:, None], what="hub score")
    close(leaf.grad, (r64[1], r32[1]), mag=R.grad_mag(h, idx, g, r64[0], cosine), what="hub dh")
    others = torch.arange(R.N) != 11
    assert not bool(leaf.grad[others.to(dev)].any()), "a node in no pair has a zero gradient row"


# ---- out-of-range indices -----------------------------------------------------------------------------------------------

def test_out_of_range_index(dev):
    from graphgym_amd import ops, pair_ops
    K, d = 300, 20
    for cosine in (False, True):
        h, idx, *_ = _score_ref(K, d, cosine)
        hd = h.to(dev)
        good = ops.pair_score(hd, idx.to(dev), cosine=cosine)
        off = idx.clone()
        off[0, 17], off[1, 200] = -1, R.N
        offd = off.to(dev)
        r = pair_ops._raw_rnorm(hd, R.EPS) if cosine else None
        s, bad = pair_ops._raw_pair_score(hd, offd, r)
        assert int(bad) == 2
        nan = torch.isnan(s)
        assert nan.nonzero().flatten().tolist() == [17, 200]
        assert torch.equal(s[~nan], good[~nan]), "every other score is unchanged to the bit"
        leaf = hd.clone().requires_grad_(True)
        s = ops.pair_score(leaf, offd, cosine=cosine)
        assert torch.equal(torch.isnan(s), nan)
        with pytest.raises(ValueError, match="outside"):
            s.sum().backward()
    U = torch.randn(R.N, 16, device=dev)
    z, bad = pair_ops._raw_pair_sum(U, U, offd, None)
    assert int(bad) == 2
    rows = torch.isnan(z).all(1)
    assert rows.nonzero().flatten().tolist() == [17, 200] and not bool(torch.isnan(z[~rows]).any())
    assert torch.equal(z[~rows], ops.pair_sum(U, U, idx.to(dev))[~rows])


# ---- host reads and determinism -------------------------------------------------------------------------------------------

@contextlib.contextmanager
def _no_host_reads():
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_no_host_read_and_the_same_bits(dev):
    from graphgym_amd import ops
    K, d = 300, 64
    for cosine in (False, True):
        h, idx, g, *_ = _score_ref(K, d, cosine)
        hd, id_, gd = h.to(dev), idx.to(dev), g.to(dev)
        U, bias = torch.randn(R.N, 16, device=dev), torch.randn(16, device=dev)
        with _no_host_reads():                    # the forward alone, no index anywhere
            s0 = ops.pair_score(hd, id_, cosine=cosine)
            z0 = ops.pair_sum(U, U, id_, bias)
        pi = ops.pair_index(id_, R.N)             # built ahead (host reads), as a loader's side stream would
        pi.role_operators()
        runs = []
        for _ in range(2):
            leaf, Ul = hd.clone().requires_grad_(True), U.clone().requires_grad_(True)
            with _no_host_reads():
                s = ops.pair_score(leaf, id_, cosine=cosine, pair_index=pi)
                s.backward(gd)
                z = ops.pair_sum(Ul, Ul, id_, bias, pair_index=pi)
                z.backward(torch.ones_like(z))
            runs.append((s.detach(), leaf.grad, z.detach(), Ul.grad))
        for x, y in zip(*runs):
            assert torch.equal(x, y), "two runs give equal bits"
        assert torch.equal(runs[0][0], s0) and torch.equal(runs[0][2], z0)


# ---- op checks ----------------------------------------------------------------------------------------------------------

def test_opcheck(dev):
    from graphgym_amd import ops  # noqa: F401
    idx = R.pairs(65).to(dev)
    t = lambda *shape: torch.rand(*shape, device=dev).requires_grad_(True)        # noqa: E731
    cases = [(torch.ops.mp.pair_score.default, (t(R.N, 6), idx, False, 1e-8)),
             (torch.ops.mp.pair_score.default, (t(R.N, 8), idx, True, 1e-8)),
             (torch.ops.mp.pair_sum.default, (t(R.N, 6), t(R.N, 6), idx, t(6))),
             (torch.ops.mp.pair_sum.default, (t(R.N, 8), t(R.N, 8), idx, None))]
    for op, args in cases:
        res = torch.library.opcheck(op, args, raise_exception=True)
        assert all(v == "SUCCESS" for v in res.values()), (op, res)


def test_every_subset_of_differentiated_inputs(dev):
    from graphgym_amd import ops
    K, m = 257, 20
    gen = torch.Generator().manual_seed(10)
    idx = R.pairs(K)
    inputs = {"U": torch.randn(R.N, m, generator=gen), "V": torch.randn(R.N, m, generator=gen),
              "bias": torch.randn(m, generator=gen)}
    _gradsub.sweep(lambda t: ops.pair_sum(t["U"], t["V"], idx.to(dev), t["bias"]), inputs,
                   lambda c, t, eng: R.pair_sum(lambda v: v, t["U"], t["V"], idx, t["bias"]),
                   torch.randn(K, m, generator=gen), dev, params=("bias",), bits=("y", "U", "V", "bias"), what="pair_sum")
    for cosine in (False, True):
        h, _, g, refs, smag, gmag = _score_ref(K, m, cosine)
        _gradsub.sweep(lambda t: ops.pair_score(t["h"], idx.to(dev), cosine=cosine), {"h": h},
                       lambda c, t, eng: R.score(t["h"], idx, cosine), g, dev, mags={"y": smag, "h": gmag},
                       what=f"pair_score cosine={cosine}")


# ---- memory -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("cosine", [False, True])
def test_peak_memory_stays_below_one_gathered_operand(dev, cosine):
    """derived, not measured: the composition's two gathered operands alone take 2 K d 4 bytes; forward + backward on
    the engine route, index build included, stay below K d 4 bytes above the inputs"""
    from graphgym_amd import ops
    N, K, d = 1024, 65536, 256
    gen = torch.Generator(device=dev).manual_seed(11)
    h = torch.randn(N, d, device=dev, generator=gen).requires_grad_(True)
    idx = torch.randint(0, N, (2, K), device=dev, generator=gen)
    g = torch.randn(K, device=dev, generator=gen)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    s = ops.pair_score(h, idx, cosine=cosine)
    s.backward(g)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    print(f"peak above the inputs: {peak} bytes; one gathered operand: {K * d * 4}")
    assert peak < K * d * 4
    assert bool(torch.isfinite(h.grad).all())


# ---- the head -----------------------------------------------------------------------------------------------------------

class Spy(TorchDispatchMode):
    def __init__(self):
        super().__init__()
        self.seen = []

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        self.seen.append((str(func), tuple(out.shape) if isinstance(out, torch.Tensor) else None))
        return out

    def mp(self):
        return {s.split(".")[1] for s, _ in self.seen if s.startswith("mp.")}

    def gathers(self, K):
        return [(s, shape) for s, shape in self.seen if s.startswith("aten.index") and shape is not None
                and len(shape) == 3 and shape[:2] == (2, K)]


@contextlib.contextmanager
def _cfg(**kw):
    import graphgym_amd.graphgym_plugin  # noqa: F401
    from graphgym_amd.config import cfg
    old = {}
    for key, v in kw.items():
        sect, name = key.split("__")
        node = getattr(cfg, sect)
        old[key] = getattr(node, name, None)
        setattr(node, name, v)
    try:
        yield cfg
    finally:
        for key, v in old.items():
            sect, name = key.split("__")
            if v is None:
                delattr(getattr(cfg, sect), name)
            else:
                setattr(getattr(cfg, sect), name, v)


def _head_run(head, h, idx, up, dev):
    """(pred, dh, parameter gradients by name) of one forward + backward of a copy of `head` on `dev`"""
    from graphgym_amd import harness as H
    m = copy.deepcopy(head).to(device=dev, dtype=h.dtype)
    m.train()
    leaf = h.detach().clone().to(dev).requires_grad_(True)
    pred, label = m(H.Batch(node_feature=leaf, edge_label_index=idx.to(dev), edge_label=torch.ones(idx.size(1), device=dev)))
    (pred * up.to(device=dev, dtype=h.dtype)).sum().backward()
    return pred.detach(), leaf.grad, {n: p.grad for n, p in m.named_parameters()}


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("decoding", ["concat", "dot", "cosine_similarity"])
def test_head_routes(dev, monkeypatch, decoding, layers):
    """GNNEdgeHead with the threshold lowered equals the composition of the same module (evaluated on the CPU in float64
    and float32: CPU tensors never take the route); at the default threshold the same small shapes keep the composition"""
    from graphgym_amd import harness as H
    monkeypatch.delenv("MP_PAIR_DECODE", raising=False)
    d, K = 20, 300
    dim_out = 3 if decoding == "concat" else 1
    gen = torch.Generator().manual_seed(12)
    h = torch.randn(R.N, d, generator=gen)
    idx = R.pairs(K)
    up = torch.randn((K, dim_out) if decoding == "concat" else (K,), generator=gen)
    with _cfg(model__edge_decoding=decoding, gnn__layers_post_mp=layers, gnn__batchnorm=True, gnn__act="relu",
              gnn__dropout=0.0):
        torch.manual_seed(3)
        head = H.GNNEdgeHead(d, dim_out)
        r64, r32 = both(lambda c: _head_run(head, c(h), idx, up, "cpu"))
        monkeypatch.setattr(H, "PAIR_DECODE_MIN", 1)
        with Spy() as spy:
            pred, dh, grads = _head_run(head, h, idx, up, dev)
        assert ("pair_sum" if decoding == "concat" else "pair_score") in spy.mp(), spy.mp()
        assert not spy.gathers(K), "no index op may produce a [2, K, d] tensor"
        what = f"head {decoding} layers={layers}"
        if decoding == "concat":
            close(pred, (r64[0], r32[0]), what=what)
        else:
            # the width-1 score cancels: its sum of absolute terms, from the float64 features the pairs are taken from
            m64 = copy.deepcopy(head).double()
            z = m64.layer_post_mp(H.Batch(node_feature=h.double())).node_feature.detach()
            close(pred[:, None], (r64[0][:, None], r32[0][:, None]), mag=R.score_mag(z, idx, decoding != "dot")[:, None],
                  what=what)
        close(dh, (r64[1], r32[1]), what=what + " dh")
        assert set(grads) == set(r64[2])
        for n in grads:
            close_all(grads[n], (r64[2][n], r32[2][n]), what=f"{what} d{n}")
        # the default threshold: these shapes stay on the composition, bit for bit
        monkeypatch.undo()
        monkeypatch.delenv("MP_PAIR_DECODE", raising=False)
        assert K * d < H.PAIR_DECODE_MIN and not H.pair_decode_route(True, torch.float32, K, d, decoding == "concat")
        with Spy() as spy:
            kept = _head_run(head, h, idx, up, dev)
        assert not spy.mp() & {"pair_score", "pair_sum"}
        monkeypatch.setattr(H, "PAIR_DECODE_MIN", None)
        comp = _head_run(head, h, idx, up, dev)
        assert torch.equal(kept[0], comp[0]) and torch.equal(kept[1], comp[1])
        assert all(torch.equal(kept[2][n], comp[2][n]) for n in comp[2])


def test_head_uses_a_prebuilt_pair_index(dev, monkeypatch):
    from graphgym_amd import graph, ops
    from graphgym_amd import harness as H
    monkeypatch.delenv("MP_PAIR_DECODE", raising=False)
    monkeypatch.setattr(H, "PAIR_DECODE_MIN", 1)
    d, K = 20, 300
    idx = R.pairs(K).to(dev)
    with _cfg(model__edge_decoding="dot", gnn__layers_post_mp=1):
        torch.manual_seed(3)
        head = H.GNNEdgeHead(d, 1).to(dev)
        pi = ops.pair_index(idx, R.N)
        built = graph.BUILDS["csr"]
        leaf = R.features(d).to(dev).requires_grad_(True)
        pred, _ = head(H.Batch(node_feature=leaf, edge_label_index=idx, edge_label=torch.ones(K, device=dev), pair_index=pi))
        pred.sum().backward()
        assert graph.BUILDS["csr"] == built, "the batch's PairIndex was used: nothing was built"
        other = ops.PairIndex(R.pairs(K, seed=5).to(dev), R.N)      # a stamp that does not match is not used
        built = graph.BUILDS["csr"]
        idx2 = idx.clone()
        pred, _ = head(H.Batch(node_feature=leaf, edge_label_index=idx2, edge_label=torch.ones(K, device=dev),
                               pair_index=other))
        pred.sum().backward()
        assert graph.BUILDS["csr"] == built + 1


# ---- end to end -----------------------------------------------------------------------------------------------------------

def test_three_adam_steps_on_each_route(dev, monkeypatch):
    """the model of tests/test_link_pred_gpu.py::test_edge_head_without_the_transform (8 BA(64, 2) graphs, generalconv,
    d = 32, edge_decoding dot), three Adam steps on each route from the same seed.  Both runs are float32 evaluations of
    one model; the losses are held to 1e-5 of the largest, the bar of the whole-model comparisons of two float32 routes
    (tests/test_graph_loader_gpu.py)."""
    import graphgym_amd as ga
    from graphgym_amd import graphgen
    from graphgym_amd import harness as H
    from graphgym_amd.link_pred import link_batch, link_split
    monkeypatch.delenv("MP_PAIR_DECODE", raising=False)
    n, k = 64, 8
    parts = [graphgen.ba_edge_index(n, 2, seed=s) + s * n for s in range(k)]
    base = ga.CSRGraph.from_edge_index(torch.cat(parts, 1).to(dev), n * k)
    gp = torch.arange(0, n * k + 1, n)
    x = torch.rand(base.num_nodes, 10, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    kw = dict(gnn__layers_mp=2, gnn__dim_inner=32, gnn__layers_pre_mp=1, gnn__layers_post_mp=1, gnn__batchnorm=True,
              gnn__l2norm=True, gnn__act="relu", gnn__dropout=0.0, gnn__agg="add", gnn__normalize_adj=False,
              gnn__stage_type="stack", gnn__layer_type="generalconv", dataset__task="link_pred",
              dataset__transform="none", model__edge_decoding="dot")
    results = {}
    with _cfg(**kw):
        for route, threshold in (("engine", 1), ("composition", None)):
            monkeypatch.setattr(H, "PAIR_DECODE_MIN", threshold)
            splits = link_split(base, gp, (0.8, 0.2), generator=torch.Generator().manual_seed(0))
            torch.manual_seed(0)
            model = H.GNN(10, 1).to(dev)
            opt = torch.optim.Adam(model.parameters(), lr=0.01)
            losses = []
            with Spy() as spy:
                for step in range(3):
                    def forward_loss():
                        batch = link_batch(splits["train"], x, ratio=1.0, seed=1, offset=step)
                        pred, y = model(batch)
                        return torch.nn.functional.binary_cross_entropy_with_logits(pred, y)
                    losses.append(float(H.train_step(model, opt, forward_loss)))
                with torch.no_grad():
                    model.eval()
                    pred, y = model(link_batch(splits["val"], x, ratio=1.0, seed=1, offset=9))
            assert ("pair_score" in spy.mp()) == (route == "engine")
            assert bool(torch.isfinite(pred).all()) and pred.numel() == y.numel() > 0
            results[route] = torch.tensor(losses, dtype=torch.float64)
    print("losses", [[f"{float(v):.9f}" for v in r] for r in results.values()])
    assert bool(torch.isfinite(results["engine"]).all())
    close_all(results["engine"], results["composition"], tol=1e-5, what="three Adam steps, engine against composition")
