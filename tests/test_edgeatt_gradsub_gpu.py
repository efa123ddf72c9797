"""ops.edge_att_alpha and ops.spmm_edge_heads under every non-empty subset of their differentiable inputs, with the harness
of tests/_gradsub.py (as tests/test_grad_subsets_gpu.py runs the other formulas): a gradient that is not asked for must
not disturb one that is, and no subset may crash.  Results whose launches do not depend on the subset and use no float
atomics are held bit for bit against the all-inputs run."""
import pytest
import torch

import _edgeatt_ref as E
from _gradsub import abs_mags, hub_graph, sweep

pytestmark = pytest.mark.gpu


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _softmax_terms(alpha64, dl64, rows, N):
    """|alpha_e| (|dalpha_e| + sum_row |alpha dalpha|): the absolute terms of a softmax row's gradient"""
    rowdot = torch.zeros(N, alpha64.size(1), dtype=torch.float64).index_add_(0, rows, (alpha64 * dl64).abs())
    return alpha64.abs() * (dl64.abs() + rowdot[rows])


@pytest.mark.parametrize("loops", [False, True], ids=["edges", "inserted_loops"])
@pytest.mark.parametrize("has_dst", [True, False], ids=["dst", "nodst"])
@pytest.mark.parametrize("heads", [1, 4])
def test_edge_att_alpha(dev, heads, has_dst, loops):
    from graphgym_amd import ops
    build = dict(add_self_loops=True) if loops else {}
    G, rows, cols, _, ei = hub_graph(dev, weighted=False, **build)
    eids = G.eid.cpu().long()
    assert bool((eids < 0).any()) == loops
    N, Ein = G.num_nodes, ei.size(1) + 3
    g = _gen(30 + heads)
    inputs = {"a_dst": torch.randn(N, heads, generator=g) if has_dst else None,
              "a_src": torch.randn(N, heads, generator=g), "a_edge": torch.randn(Ein, heads, generator=g)}
    dy = torch.randn(G.nnz, heads, generator=g)

    def oracle(c, t, eng):
        return E.edge_att_alpha(rows, cols, eids, t["a_dst"], t["a_src"], t["a_edge"], N, 0.2)
    al = oracle(None, {k: (None if v is None else v.double()) for k, v in inputs.items()}, None)
    terms = _softmax_terms(al, dy.double(), rows, N)
    zero = torch.zeros(N, heads, dtype=torch.float64)
    has = eids >= 0
    mag_e = torch.zeros(Ein, heads, dtype=torch.float64)
    mag_e[eids[has]] = terms[has]
    # (the sums of absolute terms with lrelu' <= 1; never below the reference itself)
    mags = {"a_dst": zero.index_add(0, rows, terms), "a_src": zero.index_add(0, cols, terms), "a_edge": mag_e}
    # d_edge is an indexed store; d_dst and d_src are index_add_ sums (float atomics)
    sweep(lambda t: ops.edge_att_alpha(G, t["a_dst"], t["a_src"], t["a_edge"], 0.2), inputs, oracle, dy, dev,
          bits=("y", "a_edge"), mags=mags, what=f"edge_att_alpha H={heads} dst={has_dst} loops={loops}")


def _heads_case(dev, reduce, heads, d, has_t, has_b, loops=False, seed=40):
    from graphgym_amd import ops
    build = dict(add_self_loops=True) if loops else {}
    G, rows, cols, _, ei = hub_graph(dev, weighted=False, **build)
    eids = G.eid.cpu().long()
    assert bool((eids < 0).any()) == loops
    N = G.num_nodes
    g = _gen(seed + heads)
    inputs = {"w": torch.rand(G.nnz, heads, generator=g) * 2 - 0.5, "x": torch.randn(N, d, generator=g),
              "m": torch.randn(ei.size(1) + 3, d, generator=g),
              "t": torch.randn(N, d, generator=g) if has_t else None,
              "bias": torch.randn(d, generator=g) if has_b else None}
    dy = torch.randn(N, d, generator=g)
    win = None
    # max: the oracle is evaluated AT the engine's winners (tests/test_edgeattconv_gpu.py checks the choice of winner)
    if reduce == "max":
        dv = {k: (None if v is None else v.to(dev)) for k, v in inputs.items()}
        win = ops._raw_spmm_edge_heads(G, dv["w"], dv["x"], dv["m"], dv["t"], dv["bias"], heads, ops._lib.MAX, True)[1].cpu()

    def op(t):
        return ops.spmm_edge_heads(G, t["w"], t["x"], t["m"], t=t["t"], heads=heads, reduce=reduce, bias=t["bias"])

    def oracle(c, t, eng):
        return E.edge_heads_agg(rows, cols, eids, t["w"], t["x"], t["m"], t["t"], t["bias"], N, heads, reduce, win)
    return op, inputs, oracle, dy


def _bits(reduce):
    # dw, dm and dt are plain stores and ordered sums; dx of max is the atomic scatter
    return ("y", "w", "m", "t") + (() if reduce == "max" else ("x",))


@pytest.mark.parametrize("heads,d", [(1, 48), (4, 64), (3, 48)], ids=["H1", "H4", "H3_per_head"])
@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
def test_spmm_edge_heads(dev, reduce, heads, d):
    op, inputs, oracle, dy = _heads_case(dev, reduce, heads, d, True, True)
    sweep(op, inputs, oracle, dy, dev, params=("bias",), mags=abs_mags(oracle, inputs, dy), bits=_bits(reduce),
          what=f"spmm_edge_heads {reduce} H={heads}")


@pytest.mark.parametrize("reduce", ["sum", "max"])
def test_spmm_edge_heads_without_t_and_bias(dev, reduce):
    op, inputs, oracle, dy = _heads_case(dev, reduce, 4, 64, False, False)
    sweep(op, inputs, oracle, dy, dev, mags=abs_mags(oracle, inputs, dy), bits=_bits(reduce),
          what=f"spmm_edge_heads {reduce} plain")


@pytest.mark.parametrize("reduce", ["sum", "mean", "max"])
def test_spmm_edge_heads_with_inserted_loops(dev, reduce):
    op, inputs, oracle, dy = _heads_case(dev, reduce, 4, 64, True, True, loops=True)
    sweep(op, inputs, oracle, dy, dev, params=("bias",), mags=abs_mags(oracle, inputs, dy), bits=_bits(reduce),
          what=f"spmm_edge_heads {reduce} loops")
