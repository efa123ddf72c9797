"""Every autograd formula of graphgym_amd/ops.py and graphgym_amd/nn.py under every non-empty subset of its differentiable
inputs (a frozen weight, a first layer whose x is a leaf without gradient, bias-only training, affine=False, one output
of two unused), against a float64 evaluation of the same formula with torch autograd on the CPU — tests/_gradsub.py.

Each formula picks its launches from `needs_input_grad`, from which output gradients are None and from what the forward
kept; a swapped index, a dropped term or a stale saved tensor trains without an error.  Tolerances: the defaults of
tests/_tol.py; a `mag=` only where the operator's own test has one (results that cancel by construction).  Results whose
launches do not depend on the subset and use no float atomics are held bit for bit against the all-inputs run; the
forward result is, for every operator whose forward launch does not depend on gradient state."""
import pytest
import torch
import torch.nn.functional as F

import _att_ref as A
import _edgeconv_ref as E
from _gradsub import abs_mags, hold_bits, hub_graph, relu_like, run, subsets, sweep
from oracle import ref_ops as R

pytestmark = pytest.mark.gpu

LAYOUTS = ("expand", "slice", "transposed")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _act(pre, eng, relu):
    return relu_like(pre, eng[0]) if relu else pre


# ---- ops.spmm -----------------------------------------------------------------------------------------------------------
def _spmm_case(dev, reduce, relu, ss, seed=1):
    from graphgym_amd import ops
    G, rows, cols, val, _ = hub_graph(dev)
    N, d = G.num_nodes, 96
    g = _gen(seed)
    inputs = {"x": torch.randn(N, d, generator=g), "bias": torch.randn(d, generator=g)}
    dy = torch.randn(N, d, generator=g)

    def op(t):
        return ops.spmm(G, t["x"], reduce, self_scale=ss, bias=t["bias"], relu=relu)

    # max, as test_backward_matches_oracle_autograd has it: the oracle's entries in CSR order.  Its autograd would share
    # the gradient of a tied maximum evenly where the kernel gives it to the first winner in CSR order; the weights and x
    # are continuous draws, so a row has one winner per column (an exact tie is a null event) and the two rules agree.
    def oracle(c, t, eng):
        pre = R.coo_aggregate(rows, cols, c(val), t["x"], N, reduce) + ss * t["x"] + t["bias"]
        return _act(pre, eng, relu)
    return op, inputs, oracle, dy


@pytest.mark.parametrize("ss", [0.0, 0.5])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
def test_spmm(dev, reduce, relu, ss):
    op, inputs, oracle, dy = _spmm_case(dev, reduce, relu, ss)
    # max: the forward writes its argmax (another launch than inference) and dx is an atomic scatter: float64 only
    bits = () if reduce == "max" else ("y", "x")
    sweep(op, inputs, oracle, dy, dev, params=("bias",), bits=bits, what=f"spmm {reduce} relu={relu} s={ss}")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_spmm_dy_layouts(dev, layout):
    for reduce in ("mean", "max"):
        op, inputs, oracle, dy = _spmm_case(dev, reduce, True, 0.5)
        run(op, inputs, oracle, ("x", "bias"), dy, dev, params=("bias",), layout=layout, what=f"spmm {reduce} dy {layout}")


@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_spmm_bf16(dev, reduce):
    """bf16 x and bias: the output and every requested gradient are the fp32 kernel's on the widened inputs, rounded once"""
    from graphgym_amd import ops
    BF = torch.bfloat16
    G, *_ = hub_graph(dev)
    N, d = G.num_nodes, 96
    g = _gen(2)
    x, b, dy = (torch.randn(s, generator=g).to(BF).to(dev) for s in ((N, d), (d,), (N, d)))
    ys = []
    for s in subsets(("x", "bias")):
        xb, bb = x.clone().requires_grad_("x" in s), b.clone().requires_grad_("bias" in s)
        yb = ops.spmm(G, xb, reduce, self_scale=0.5, bias=bb)
        yb.backward(dy)
        xf, bf = x.float().requires_grad_("x" in s), b.float().requires_grad_("bias" in s)
        yf = ops.spmm(G, xf, reduce, self_scale=0.5, bias=bf)
        yf.backward(dy.float())
        assert yb.dtype == BF and torch.equal(yb.detach(), yf.detach().to(BF)), s
        for lo, hi, name in ((xb, xf, "x"), (bb, bf, "bias")):
            if name in s:
                assert lo.grad.dtype == BF and torch.equal(lo.grad, hi.grad.to(BF)), (s, name)
            else:
                assert lo.grad is None and hi.grad is None, (s, name)
        assert torch.equal(xb.detach(), x) and torch.equal(bb.detach(), b)
        ys.append(yb.detach())
    assert all(torch.equal(ys[0], y) for y in ys[1:])


# ---- ops.spmm_edge ------------------------------------------------------------------------------------------------------
def _spmm_edge_case(dev, reduce, has_t, has_b, loops=False, seed=3):
    from graphgym_amd import ops
    build = dict(add_self_loops=True, fill=0.75) if loops else {}
    G, rows, cols, val, ei = hub_graph(dev, **build)
    eids = G.eid.cpu().long()
    assert bool((eids < 0).any()) == loops
    N, d = G.num_nodes, 96
    g = _gen(seed)
    inputs = {"x": torch.randn(N, d, generator=g), "m": torch.randn(ei.size(1) + 3, d, generator=g),
              "t": torch.randn(N, d, generator=g) if has_t else None,
              "bias": torch.randn(d, generator=g) if has_b else None}
    dy = torch.randn(N, d, generator=g)
    win = None
    # max: the oracle is evaluated AT the engine's winners (a near-tie cannot flip one between the float64 and float32
    # evaluations), its forward value included, so this file's reference is not independent of the kernel's choice of
    # winner; that choice is checked on its own in tests/test_edgeconv_gpu.py (and tests/test_attconv_gpu.py for
    # spmm_edge_values below, which does the same)
    if reduce == "max":
        dv = [None if v is None else v.to(dev) for v in inputs.values()]
        win = ops._raw_spmm_edge(G, *dv, ops._lib.MAX, True)[1].cpu()

    def op(t):
        return ops.spmm_edge(G, t["x"], t["m"], reduce, t=t["t"], bias=t["bias"])

    def oracle(c, t, eng):
        return E.edge_agg(rows, cols, eids, c(val), t["x"], t["m"], t["t"], t["bias"], N, reduce, win)
    return op, inputs, oracle, dy


def _spmm_edge_bits(reduce):
    # dm and dt are plain stores; dx of max is the atomic scatter
    return ("y", "m", "t") + (() if reduce == "max" else ("x",))


@pytest.mark.parametrize("has_b", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("has_t", [False, True], ids=["not", "t"])
@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
def test_spmm_edge(dev, reduce, has_t, has_b):
    op, inputs, oracle, dy = _spmm_edge_case(dev, reduce, has_t, has_b)
    sweep(op, inputs, oracle, dy, dev, params=("bias",), mags=abs_mags(oracle, inputs, dy),
          bits=_spmm_edge_bits(reduce), what=f"spmm_edge {reduce} t={has_t} b={has_b}")


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
def test_spmm_edge_with_inserted_loops(dev, reduce):
    op, inputs, oracle, dy = _spmm_edge_case(dev, reduce, True, True, loops=True)
    sweep(op, inputs, oracle, dy, dev, params=("bias",), mags=abs_mags(oracle, inputs, dy),
          bits=_spmm_edge_bits(reduce), what=f"spmm_edge {reduce} loops")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_spmm_edge_dy_layouts(dev, layout):
    for reduce in ("mean", "max"):
        op, inputs, oracle, dy = _spmm_edge_case(dev, reduce, True, True)
        # (an expanded all-ones gradient is its own absolute value)
        run(op, inputs, oracle, ("x", "m", "t", "bias"), dy, dev, params=("bias",),
            mags=abs_mags(oracle, inputs, torch.ones_like(dy) if layout == "expand" else dy), layout=layout,
            what=f"spmm_edge {reduce} dy {layout}")


# ---- ops.idgnn_aggregate ------------------------------------------------------------------------------------------------
def test_idgnn_aggregate_output_subsets(dev):
    """the loss uses P only, Q only, both: the three dP / dQ None branches of _idgnn_backward"""
    from graphgym_amd import ops
    G, rows, cols, val, _ = hub_graph(dev)
    N, d = G.num_nodes, 96
    g = _gen(4)
    inputs = {"x": torch.randn(N, d, generator=g)}
    ids = torch.randperm(N, generator=g)[:37]
    ids[0] = 3                                        # the hub row's own node among the identity nodes
    ids = ids.unique()
    dP, dQ = torch.randn(N, d, generator=g), torch.randn(N, d, generator=g)
    sel = torch.zeros(N, 1)
    sel[ids] = 1

    def op(t):
        return ops.idgnn_aggregate(G, ids.to(dev), t["x"])

    def oracle(c, t, eng):
        return (R.coo_aggregate(rows, cols, c(val), t["x"], N, "sum"),
                R.coo_aggregate(rows, cols, c(val), t["x"] * c(sel), N, "sum"))
    res = [run(op, inputs, oracle, ("x",), dys, dev, what=f"idgnn_aggregate {name}")
           for name, dys in (("both", (dP, dQ)), ("P", (dP, None)), ("Q", (None, dQ)))]
    for r in res[1:]:
        hold_bits(res[0], r, ("y0", "y1"), "idgnn_aggregate")


# ---- ops.dense_fused ----------------------------------------------------------------------------------------------------
def _dense_case(M, Fi, d, pair, relu, seed=5):
    from graphgym_amd import ops
    g = _gen(seed + M)
    inputs = {"P": torch.randn(M, Fi, generator=g), "W": torch.randn(Fi, d, generator=g) / Fi ** 0.5,
              "Q": torch.randn(M, Fi, generator=g) if pair else None,
              "W_id": torch.randn(Fi, d, generator=g) / Fi ** 0.5 if pair else None, "bias": torch.randn(d, generator=g)}
    dy = torch.randn(M, d, generator=g)

    def op(t):
        return ops.dense_fused(t["P"], t["W"], t["Q"], t["W_id"], t["bias"], relu=relu)

    def oracle(c, t, eng):
        pre = t["P"] @ t["W"] + t["bias"]
        if pair:
            pre = pre + t["Q"] @ t["W_id"]
        return _act(pre, eng, relu)

    def mags(eng):      # F = 1: dP, dQ are width-1 results, a signed sum per row: held to their sums of absolute terms
        if Fi != 1:
            return {}
        gm = (dy * (eng[0] > 0) if relu else dy).abs().double()
        return {"P": gm @ inputs["W"].abs().double().t(), "Q": gm @ inputs["W_id"].abs().double().t() if pair else None}
    return op, inputs, oracle, dy, mags


@pytest.mark.parametrize("M,Fi,d", [(1000, 256, 256), (333, 1, 7)])
@pytest.mark.parametrize("pair", [False, True], ids=["P", "PQ"])
@pytest.mark.parametrize("relu", [False, True])
def test_dense_fused(dev, relu, pair, M, Fi, d):
    op, inputs, oracle, dy, mags = _dense_case(M, Fi, d, pair, relu)
    sweep(op, inputs, oracle, dy, dev, params=("W", "W_id", "bias"), mags=mags, bits=("y",),
          what=f"dense_fused relu={relu} pair={pair} M={M}")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_dense_fused_dy_layouts(dev, layout):
    op, inputs, oracle, dy, mags = _dense_case(1000, 256, 256, True, True)
    run(op, inputs, oracle, tuple(inputs), dy, dev, params=("W", "W_id", "bias"), layout=layout,
        what=f"dense_fused dy {layout}")


@pytest.mark.parametrize("subset,wants", [(("W", "bias"), False), (("W",), False), (("W", "W_id"), True),
                                          (("P", "W"), True), (("Q", "W", "bias"), True)],
                         ids=lambda v: "_".join(v) if isinstance(v, tuple) else ("written" if v else "absent"))
def test_no_masked_gradient_without_an_input_gradient(dev, monkeypatch, subset, wants):
    """with ReLU and dW wanted, the mask rides in the weight-gradient kernel; its [M, d] masked-gradient output is
    allocated and written only when dP, dQ or dW_id will read it (a first layer, or a frozen input, has no reader).
    No result depends on that buffer, so only the kernel's own return shows it."""
    from graphgym_amd import ops
    op, inputs, oracle, dy, mags = _dense_case(1000, 256, 256, True, True)
    seen, orig = [], ops._raw_dense_wgrad_relu

    def spy(*a, **k):
        r = orig(*a, **k)
        seen.append((bool(k.get("want_gm", True)), r is not None and r[2] is not None))
        return r
    monkeypatch.setattr(ops, "_raw_dense_wgrad_relu", spy)
    run(op, inputs, oracle, subset, dy, dev, params=("W", "W_id", "bias"), what="dense_fused masked gradient")
    assert seen == [(wants, wants)], seen


# ---- ops.agg_dense, ops.agg_dense_id ------------------------------------------------------------------------------------
def _spy(monkeypatch, name):
    """the keyword arguments of every call of graphgym_amd.ops.<name> from here on"""
    from graphgym_amd import ops
    calls, orig = [], getattr(ops, name)

    def spy(*a, **k):
        calls.append(k)
        return orig(*a, **k)
    monkeypatch.setattr(ops, name, spy)
    return calls


def _agg_dense_case(dev, reduce, relu, ss, Fi, want_P=None, seed=6, *, calls):
    """calls: a _spy on _raw_agg_dense; the forward must enter the one-kernel layer exactly at a shape it covers (F = 64)
    unless the reduction is a mean with a self term, which mp_agg_dense_f32 does not have"""
    from graphgym_amd import _lib, ops
    n, d = 900, 64
    G, rows, cols, val, _ = hub_graph(dev, N=n, E=9000, hub=0, seed=seed)
    g = _gen(seed)
    inputs = {"x": torch.randn(n, Fi, generator=g), "W": torch.randn(Fi, d, generator=g) / Fi ** 0.5,
              "bias": torch.randn(d, generator=g)}
    dy = torch.randn(n, d, generator=g)
    assert ops.agg_dense_supported(G, inputs["x"].to(dev), inputs["W"].to(dev)) == (Fi == 64)

    def fwd(t):
        if want_P is None:
            return ops.agg_dense(G, t["x"], t["W"], bias=t["bias"], relu=relu, self_scale=ss, reduce=reduce)
        return torch.ops.mp.agg_dense(t["x"], t["W"], t["bias"], G.handle, _lib.REDUCE[reduce], float(ss), relu, want_P)[0]

    def op(t):
        before = len(calls)
        y = fwd(t)
        one_kernel = Fi == 64 and not (reduce == "mean" and ss != 0.0)
        assert len(calls) - before == int(one_kernel), (reduce, ss, Fi)
        if one_kernel:      # the aggregated rows are written exactly when they were asked for
            assert bool(calls[-1]["want_P"]) == (t["W"].requires_grad if want_P is None else want_P)
        return y

    def oracle(c, t, eng):
        pre = (R.coo_aggregate(rows, cols, c(val), t["x"], n, reduce) + ss * t["x"]) @ t["W"] + t["bias"]
        return _act(pre, eng, relu)
    return op, inputs, oracle, dy


@pytest.mark.parametrize("Fi", [64, 96], ids=["one_kernel", "fallback"])
@pytest.mark.parametrize("ss", [0.0, 0.5])
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("reduce", ["sum", "mean"])
def test_agg_dense(dev, monkeypatch, reduce, relu, ss, Fi):
    """F = 64 is a one-kernel shape; a mean with a self term is outside mp_agg_dense_f32 at every shape and takes the
    aggregation kernel followed by the fused transform, as F = 96 does"""
    op, inputs, oracle, dy = _agg_dense_case(dev, reduce, relu, ss, Fi, calls=_spy(monkeypatch, "_raw_agg_dense"))
    sweep(op, inputs, oracle, dy, dev, params=("W", "bias"), what=f"agg_dense {reduce} relu={relu} s={ss} F={Fi}")


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("reduce,ss", [("sum", 0.5), ("mean", 0.0), ("mean", 0.5)])
def test_agg_dense_recomputes_the_aggregated_rows(dev, monkeypatch, reduce, ss, relu):
    """the registered operator called with want_P=False while W requires a gradient: the backward aggregates again, with
    the forward's reduction and self term (sum with a self term and a plain mean: one-kernel forward; mean with a self
    term: the two-kernel forward)"""
    op, inputs, oracle, dy = _agg_dense_case(dev, reduce, relu, ss, 64, want_P=False,
                                             calls=_spy(monkeypatch, "_raw_agg_dense"))
    sweep(op, inputs, oracle, dy, dev, params=("W", "bias"), what=f"agg_dense {reduce} s={ss} relu={relu} want_P=False")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_agg_dense_dy_layouts(dev, monkeypatch, layout):
    calls = _spy(monkeypatch, "_raw_agg_dense")
    for reduce, ss in (("sum", 0.5), ("mean", 0.0), ("mean", 0.5)):      # one kernel, one kernel, two kernels
        op, inputs, oracle, dy = _agg_dense_case(dev, reduce, True, ss, 64, calls=calls)
        run(op, inputs, oracle, ("x", "W", "bias"), dy, dev, params=("W", "bias"), layout=layout,
            what=f"agg_dense {reduce} s={ss} dy {layout}")


def _agg_dense_id_case(dev, relu, ss, want_P=None, seed=7):
    from graphgym_amd import ops
    n, Fi, d = 900, 64, 64
    G, rows, cols, val, _ = hub_graph(dev, N=n, E=9000, hub=0, seed=seed)
    g = _gen(seed)
    inputs = {"x": torch.randn(n, Fi, generator=g), "W": torch.randn(Fi, d, generator=g) / Fi ** 0.5,
              "W_id": torch.randn(Fi, d, generator=g) / Fi ** 0.5, "bias": torch.randn(d, generator=g)}
    ids = torch.randperm(n, generator=g)[:37]
    dy = torch.randn(n, d, generator=g)

    def op(t):
        if want_P is None:
            out = ops.agg_dense_id(G, t["x"], t["W"], t["W_id"], ids.to(dev), bias=t["bias"], relu=relu, self_scale=ss)
            assert out is not None
            return out
        return torch.ops.mp.agg_dense_id(t["x"], t["W"], t["W_id"], t["bias"], G.handle, ids.to(dev), float(ss), relu,
                                         want_P)[0]

    def oracle(c, t, eng):
        h = t["x"] @ t["W"]
        h = h.index_add(0, ids, t["x"][ids] @ t["W_id"])
        pre = R.coo_aggregate(rows, cols, c(val), h, n, "sum") + ss * (t["x"] @ t["W"]) + t["bias"]
        return _act(pre, eng, relu)
    return op, inputs, oracle, dy


@pytest.mark.parametrize("ss", [0.0, 0.5])
@pytest.mark.parametrize("relu", [False, True])
def test_agg_dense_id(dev, relu, ss):
    op, inputs, oracle, dy = _agg_dense_id_case(dev, relu, ss)
    sweep(op, inputs, oracle, dy, dev, params=("W", "W_id", "bias"), what=f"agg_dense_id relu={relu} s={ss}")


@pytest.mark.parametrize("relu", [False, True])
def test_agg_dense_id_recomputes_the_aggregated_rows(dev, relu):
    op, inputs, oracle, dy = _agg_dense_id_case(dev, relu, 0.5, want_P=False)
    sweep(op, inputs, oracle, dy, dev, params=("W", "W_id", "bias"), what=f"agg_dense_id relu={relu} want_P=False")


# ---- ops.concat_dense, ops.sage_concat ----------------------------------------------------------------------------------
def _concat_case(M, ku, kn, relu, seed=8):
    from graphgym_amd import ops
    Fi = 64
    g = _gen(seed)
    inputs = {"x": torch.randn(M, Fi, generator=g), "m": torch.randn(M, Fi, generator=g),
              "Ws": torch.randn(Fi, ku, generator=g) / Fi ** 0.5, "Wn": torch.randn(Fi, kn, generator=g) / Fi ** 0.5,
              "bias": torch.randn(ku + kn, generator=g)}
    dy = torch.randn(M, ku + kn, generator=g)

    def op(t):
        return ops.concat_dense(t["x"], t["m"], t["Ws"], t["Wn"], t["bias"], relu=relu)

    def oracle(c, t, eng):
        return _act(torch.cat([t["x"] @ t["Ws"], t["m"] @ t["Wn"]], dim=1) + t["bias"], eng, relu)
    return op, inputs, oracle, dy


@pytest.mark.parametrize("ku,kn", [(64, 64), (66, 62)])
@pytest.mark.parametrize("relu", [False, True])
def test_concat_dense(dev, relu, ku, kn):
    op, inputs, oracle, dy = _concat_case(700, ku, kn, relu)
    sweep(op, inputs, oracle, dy, dev, params=("Ws", "Wn", "bias"), bits=("y",),
          what=f"concat_dense relu={relu} {ku}/{kn}")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_concat_dense_dy_layouts(dev, layout):
    op, inputs, oracle, dy = _concat_case(700, 66, 62, True)
    run(op, inputs, oracle, tuple(inputs), dy, dev, params=("Ws", "Wn", "bias"), layout=layout,
        what=f"concat_dense dy {layout}")


def _sage_case(dev, n, E, Fi, relu, k=32, seed=9):
    from graphgym_amd import ops
    G, rows, cols, val, _ = hub_graph(dev, N=n, E=E, hub=0, seed=seed)
    g = _gen(seed)
    inputs = {"x": torch.randn(n, Fi, generator=g), "Ws": torch.randn(Fi, k, generator=g) / Fi ** 0.5,
              "Wn": torch.randn(Fi, k, generator=g) / Fi ** 0.5, "bias": torch.randn(2 * k, generator=g)}
    dy = torch.randn(n, 2 * k, generator=g)
    assert ops.agg_dense_supported(G, inputs["x"].to(dev), inputs["Wn"].to(dev)) == (Fi == 64)

    def op(t):
        return ops.sage_concat(G, t["x"], t["Ws"], t["Wn"], t["bias"], relu=relu)

    def oracle(c, t, eng):
        mean = R.coo_aggregate(rows, cols, c(val), t["x"], n, "mean")
        return _act(torch.cat([t["x"] @ t["Ws"], mean @ t["Wn"]], dim=1) + t["bias"], eng, relu)
    return op, inputs, oracle, dy


@pytest.mark.parametrize("Fi", [64, 96], ids=["fused", "fallback"])
@pytest.mark.parametrize("relu", [False, True])
def test_sage_concat(dev, relu, Fi):
    op, inputs, oracle, dy = _sage_case(dev, 900, 9000, Fi, relu)
    sweep(op, inputs, oracle, dy, dev, params=("Ws", "Wn", "bias"), what=f"sage_concat relu={relu} F={Fi}")


@pytest.mark.parametrize("subset", [("x", "Ws", "Wn"), ("Ws", "Wn")], ids=["x_Ws_Wn", "Ws_Wn"])
@pytest.mark.parametrize("which", ["concat_dense", "sage_concat"])
def test_input_gradients_through_the_streaming_transform(dev, monkeypatch, which, subset):
    """the input-gradient launches read halves of one masked-gradient buffer through mp_dense_x3_f32 (from X3_MIN_ROWS
    rows, lowered here as tests/test_dense_x3_gpu.py does); without x in the subset no masked gradient is written"""
    from graphgym_amd import ops
    M = 2500                                          # ten 256-row blocks, the last one ragged
    monkeypatch.setattr(ops, "X3_MIN_ROWS", 1)
    calls = []
    orig = ops._raw_dense_x3

    def spy(*a, **k):
        calls.append(bool(k.get("trans", a[4] if len(a) > 4 else False)))
        return orig(*a, **k)
    monkeypatch.setattr(ops, "_raw_dense_x3", spy)
    if which == "concat_dense":
        op, inputs, oracle, dy = _concat_case(M, 64, 64, True)
        params = ("Ws", "Wn", "bias")
    else:
        op, inputs, oracle, dy = _sage_case(dev, M, 25000, 64, True, k=64)
        params = ("Ws", "Wn", "bias")
    run(op, inputs, oracle, subset, dy, dev, params=params, what=f"{which} x3")
    assert calls, "the streaming transform was not entered"
    assert any(calls) == ("x" in subset), calls      # its transposed form: the input-gradient launch


# ---- attention pieces ---------------------------------------------------------------------------------------------------
def _att_graph(dev):
    return hub_graph(dev, weighted=False)


@pytest.mark.parametrize("heads", [1, 4])
def test_sddmm_dot(dev, heads):
    from graphgym_amd import ops
    G, rows, cols, _, _ = _att_graph(dev)
    N, d = G.num_nodes, 32
    g = _gen(10 + heads)
    inputs = {"Q": torch.randn(N, d, generator=g), "K": torch.randn(N, d, generator=g)}
    dy = torch.randn(G.nnz, heads, generator=g)

    def oracle(c, t, eng):
        return (t["Q"][rows].view(-1, heads, d // heads) * t["K"][cols].view(-1, heads, d // heads)).sum(-1) * 0.5
    # one head: a score is a width-1 result, one signed dot product per entry, held to its sum of absolute terms
    mags = {"y": abs_mags(oracle, inputs, dy)["y"]} if heads == 1 else None
    sweep(lambda t: ops.sddmm_dot(G, t["Q"], t["K"], heads, 0.5), inputs, oracle, dy, dev, bits=("y", "Q", "K"),
          mags=mags, what=f"sddmm_dot H={heads}")


def test_sddmm_add(dev):
    from graphgym_amd import ops
    G, rows, cols, _, _ = _att_graph(dev)
    N = G.num_nodes
    g = _gen(12)
    inputs = {"ai": torch.randn(N, generator=g), "aj": torch.randn(N, generator=g)}
    dy = torch.randn(G.nnz, 1, generator=g)

    def oracle(c, t, eng):
        return F.leaky_relu(t["ai"][rows] + t["aj"][cols], 0.2).view(-1, 1)
    # one number per node, a signed sum of per-entry terms ds_e * lrelu'(z_e): held against the same sum with |ds|
    ai, aj = (inputs[k].double().requires_grad_(True) for k in ("ai", "aj"))
    F.leaky_relu(ai[rows] + aj[cols], 0.2).view(-1, 1).backward(dy.double().abs())
    sweep(lambda t: ops.sddmm_add(G, t["ai"], t["aj"], 0.2), inputs, oracle, dy, dev, bits=("y",),
          mags={"ai": ai.grad, "aj": aj.grad}, what="sddmm_add")


def _softmax_terms(alpha64, dl64, rows, N):
    """|alpha_e| (|dalpha_e| + sum_row |alpha dalpha|): the absolute terms of a softmax row's gradient"""
    rowdot = torch.zeros(N, alpha64.size(1), dtype=torch.float64).index_add_(0, rows, (alpha64 * dl64).abs())
    return alpha64.abs() * (dl64.abs() + rowdot[rows])


@pytest.mark.parametrize("heads", [1, 4])
def test_gat_alpha(dev, heads):
    from graphgym_amd import ops
    G, rows, cols, _, _ = _att_graph(dev)
    N = G.num_nodes
    g = _gen(13 + heads)
    inputs = {"a_dst": torch.randn(N, heads, generator=g), "a_src": torch.randn(N, heads, generator=g)}
    dy = torch.randn(G.nnz, heads, generator=g)

    def oracle(c, t, eng):
        return R.softmax(F.leaky_relu(t["a_dst"][rows] + t["a_src"][cols], 0.2), rows, N)
    al = oracle(None, {k: v.double() for k, v in inputs.items()}, None)
    terms = _softmax_terms(al, dy.double(), rows, N)
    zero = torch.zeros(N, heads, dtype=torch.float64)
    # (the sums of absolute terms with lrelu' <= 1; never below the reference itself)
    mags = {"a_dst": zero.index_add(0, rows, terms), "a_src": zero.index_add(0, cols, terms)}
    sweep(lambda t: ops.gat_alpha(G, t["a_dst"], t["a_src"], 0.2), inputs, oracle, dy, dev, bits=("y",), mags=mags,
          what=f"gat_alpha H={heads}")


@pytest.mark.parametrize("heads", [1, 4])
def test_edge_softmax(dev, heads):
    from graphgym_amd import ops
    G, rows, cols, _, _ = _att_graph(dev)
    N = G.num_nodes
    g = _gen(15 + heads)
    inputs = {"s": torch.randn(G.nnz, heads, generator=g) * 3}
    dy = torch.randn(G.nnz, heads, generator=g)

    def oracle(c, t, eng):
        return R.softmax(t["s"], rows, N)
    al = R.softmax(inputs["s"].double(), rows, N)
    mags = {"s": _softmax_terms(al, dy.double(), rows, N)}
    op = lambda t: ops.edge_softmax(G, t["s"])      # noqa: E731
    a = run(op, inputs, oracle, ("s",), dy, dev, mags=mags, what=f"edge_softmax H={heads}")
    b = run(op, inputs, oracle, ("s",), dy, dev, mags=mags, what=f"edge_softmax H={heads}")
    hold_bits(a, b, ("y", "s"), "edge_softmax")


@pytest.mark.parametrize("heads", [1, 4, 3], ids=["H1", "H4", "H3_per_head"])
@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
def test_spmm_edge_values(dev, reduce, heads):
    from graphgym_amd import ops
    G, rows, cols, _, _ = _att_graph(dev)
    N, d = G.num_nodes, 48 if heads == 3 else 64
    g = _gen(17 + heads)
    signed = reduce != "sum"      # the operator's own tests: attention weights for sum, signed weights for mean / max
    inputs = {"a": torch.rand(G.nnz, heads, generator=g) * (2 if signed else 1) - (0.5 if signed else 0),
              "V": torch.randn(N, d, generator=g)}
    dy = torch.randn(N, d, generator=g)
    win = None
    if reduce == "max":
        win = ops._raw_spmm_heads_reduce(G, inputs["a"].to(dev), inputs["V"].to(dev), heads, ops._lib.MAX)[1].cpu()

    def oracle(c, t, eng):
        return A.edge_values_agg(rows, cols, t["a"], t["V"], N, heads, reduce, win)
    mags = None
    if signed:                    # da, dV: sums of products of either sign, held to their sums of absolute terms
        mags = {k: v for k, v in abs_mags(oracle, inputs, dy).items() if k != "y"}
    elif heads == 1:              # da [nnz, 1]: a width-1 result, one signed dot product per entry
        mags = {"a": abs_mags(oracle, inputs, dy)["a"]}
    # dV of max is a scatter through the argmax with float atomics
    sweep(lambda t: ops.spmm_edge_values(G, t["a"], t["V"], heads, reduce=reduce), inputs, oracle, dy, dev, mags=mags,
          bits=("y", "a") + (() if reduce == "max" else ("V",)), what=f"spmm_edge_values {reduce} H={heads}")


# ---- row gather / scatter -----------------------------------------------------------------------------------------------
def test_gather_rows_and_index_add_rows(dev):
    from graphgym_amd import ops
    g = _gen(19)
    n, d, k = 300, 40, 500
    ids = torch.randint(0, 60, (k,), generator=g)                 # every listed row about eight times
    x = {"x": torch.randn(n, d, generator=g)}
    sweep(lambda t: ops.gather_rows(t["x"], ids.to(dev)), x, lambda c, t, eng: t["x"][ids],
          torch.randn(k, d, generator=g), dev, bits=("y",), what="gather_rows")
    hu = {"h": torch.randn(n, d, generator=g), "u": torch.randn(k, d, generator=g)}
    # the forward adds repeated rows with float atomics (no bit equality); dh is dy itself and du a gather of it
    sweep(lambda t: ops.index_add_rows(t["h"], ids.to(dev), t["u"]), hu, lambda c, t, eng: t["h"].index_add(0, ids, t["u"]),
          torch.randn(n, d, generator=g), dev, bits=("h", "u"), what="index_add_rows")


# ---- nn.BatchNorm1d, nn.softmax_cross_entropy, nn.Linear ---------------------------------------------------------------
def _bn_case(dev, relu, affine, seed=20):
    from graphgym_amd.nn import BatchNorm1d
    N, d = 1000, 96
    g = _gen(seed)
    inputs = {"x": torch.randn(N, d, generator=g) * (torch.rand(d, generator=g) * 3 + 0.1) + torch.randn(d, generator=g),
              "weight": torch.rand(d, generator=g) + 0.5 if affine else None,
              "bias": torch.randn(d, generator=g) if affine else None}
    dy = torch.randn(N, d, generator=g)

    def op(t):
        bn = BatchNorm1d(d, eps=1e-5, momentum=0.1, affine=affine, relu=relu).to(dev)
        if affine:            # the module's parameters ARE the harness' leaves (or plain tensors outside the subset)
            del bn.weight, bn.bias
            bn.weight, bn.bias = t["weight"], t["bias"]
        bn.train()
        return bn(t["x"])

    def oracle(c, t, eng):
        return _act(F.batch_norm(t["x"], None, None, t["weight"], t["bias"], True, 0.1, 1e-5), eng, relu)
    return op, inputs, oracle, dy


@pytest.mark.parametrize("affine", [True, False], ids=["affine", "plain"])
@pytest.mark.parametrize("relu", [False, True])
def test_batchnorm(dev, relu, affine):
    """with `x` outside the subset this is a first layer; _bn_backward computes all three results whatever is asked"""
    op, inputs, oracle, dy = _bn_case(dev, relu, affine)
    sweep(op, inputs, oracle, dy, dev, params=("weight", "bias"), bits=("y", "x", "weight", "bias"),
          what=f"BatchNorm1d relu={relu} affine={affine}")


@pytest.mark.parametrize("layout", LAYOUTS)
def test_batchnorm_dy_layouts(dev, layout):
    op, inputs, oracle, dy = _bn_case(dev, True, True)
    run(op, inputs, oracle, ("x", "weight", "bias"), dy, dev, params=("weight", "bias"), layout=layout,
        what=f"BatchNorm1d dy {layout}")


@pytest.mark.parametrize("indexed", [False, True])
def test_softmax_ce(dev, indexed):
    g = _gen(22)
    N, Cn = 4096, 16
    inputs = {"logits": torch.randn(N, Cn, generator=g) * 3}
    idx = torch.randperm(N, generator=g)[: N // 3] if indexed else None
    y = torch.randint(0, Cn, (idx.numel() if indexed else N,), generator=g)
    dy = torch.randn((), generator=g)

    def op(t):
        return torch.ops.mp.softmax_ce(t["logits"], y.to(dev), None if idx is None else idx.to(dev))

    def oracle(c, t, eng):
        return F.cross_entropy(t["logits"] if idx is None else t["logits"][idx], y, reduction="mean")
    # a softmax gradient: the row g / n (p - onehot) cancels at the label of a confidently right row (p -> 1), so it is
    # held to its absolute terms |g| / n (p + onehot) (the operator's own test: one scale for the whole tensor)
    z = inputs["logits"].double()
    sel = torch.arange(N) if idx is None else idx
    terms = (torch.softmax(z[sel], dim=1) + F.one_hot(y, Cn)) * (float(dy.abs()) / y.numel())
    mags = {"logits": torch.zeros(N, Cn, dtype=torch.float64).index_add_(0, sel, terms)}
    res = run(op, inputs, oracle, ("logits",), dy, dev, scalar_loss=True, mags=mags, what=f"softmax_ce indexed={indexed}")
    if indexed:       # rows outside the index: exact zeros
        out = torch.ones(N, dtype=torch.bool)
        out[idx] = False
        assert float(res["logits"].cpu()[out].abs().max()) == 0.0


@pytest.mark.parametrize("has_bias", [True, False], ids=["bias", "nobias"])
def test_narrow_head_linear(dev, has_bias):
    """nn.Linear through _NarrowHead at the smallest shape its dispatch accepts: 2^17 x 8 -> 10"""
    from graphgym_amd import nn as mpnn
    g = _gen(23)
    N, fi, fo = 1 << 17, 8, 10
    inputs = {"x": torch.randn(N, fi, generator=g), "weight": torch.randn(fo, fi, generator=g) / fi ** 0.5,
              "bias": torch.randn(fo, generator=g) if has_bias else None}
    dy = torch.randn(N, fo, generator=g)

    def op(t):
        lin = mpnn.Linear(fi, fo, bias=has_bias).to(dev)
        del lin.weight
        lin.weight = t["weight"]
        if has_bias:
            del lin.bias
            lin.bias = t["bias"]
        out = lin(t["x"])
        assert "_NarrowHead" in type(out.grad_fn).__name__
        return out

    def oracle(c, t, eng):
        return F.linear(t["x"], t["weight"], t["bias"])
    sweep(op, inputs, oracle, dy, dev, params=("weight", "bias"), bits=("y",), what=f"Linear narrow bias={has_bias}")
