"""No mp_pair_* entry may depend on the contents of its fresh allocations: the cases of tests/test_poison_gpu.py for
include/mp_pair.h, under the same harness (tests/_poison.py through that file's `differential`: the three fills in their
order, the recorder, the guards) and the same checks 1-5 of its docstring.

The pair list puts 1 500 of its 2 000 pairs on node 3: a row of the inverted index above the default hub_deg, so the
backward's pieces live in a poisoned workspace and the finalize kernel reads them; nodes 7, 27, ... are in no pair.
Forward and backward run, and the PairIndex (CSR, plan, role operators) is built inside the poisoned context.  Every sum
has a fixed order: the results under the three fills are equal bit for bit."""
import pytest
import torch

import _pair_ref as R
from _tol import both, close
from test_poison_gpu import Case, N_NODES, differential, gen, leaf, rnd

D, K, HUB, M = 12, 2000, 1500, 20


def _pairs():
    idx = torch.randint(0, N_NODES, (2, K), generator=gen(11))
    idx[idx % 20 == 7] += 1
    idx[1, :HUB] = 3
    return idx


def _run_score(dev, cosine):
    from graphgym_amd import ops
    idx = _pairs().to(dev)
    h = leaf(rnd(N_NODES, D, seed=12), dev)
    s = ops.pair_score(h, idx, cosine=cosine)
    s.backward(rnd(K, seed=13).to(dev))
    pi = ops.pair_index(idx, N_NODES)
    assert pi.graph.plan()[1][1] > 0, "the hub pieces and the finalize kernel must be live"
    return s, h.grad


def run_dot(dev):
    return _run_score(dev, False)


def run_cosine(dev):
    return _run_score(dev, True)


def run_sum(dev):
    from graphgym_amd import ops
    idx = _pairs().to(dev)
    U, V, b = leaf(rnd(N_NODES, M, seed=14), dev), leaf(rnd(N_NODES, M, seed=15), dev), leaf(rnd(M, seed=16), dev)
    z = ops.pair_sum(U, V, idx, b)
    z.backward(rnd(K, M, seed=17).to(dev))
    return z, U.grad, V.grad, b.grad


def _oracle_score(cosine):
    def check(outs):
        s, dh = (t.cpu() for t in outs)
        idx, h, g = _pairs(), rnd(N_NODES, D, seed=12), rnd(K, seed=13)
        r64, r32 = both(R.score_and_grad(h, idx, g, cosine))
        close(s[:, None], (r64[0][:, None], r32[0][:, None]), mag=R.score_mag(h, idx, cosine)[:, None], what="pair score")
        close(dh, (r64[1], r32[1]), mag=R.grad_mag(h, idx, g, r64[0], cosine), what="pair score input gradient")
    return check


def _oracle_sum(outs):
    z = outs[0].cpu()
    idx = _pairs()
    U, V, b = rnd(N_NODES, M, seed=14), rnd(N_NODES, M, seed=15), rnd(M, seed=16)
    close(z, both(lambda c: R.pair_sum(c, U, V, idx, b)), what="pair sum")


CASES = [
    Case("pair_score_dot", ("mp_pair_score_f32", "mp_pair_bwd_weights_f32"), run_dot, oracle=_oracle_score(False)),
    Case("pair_score_cosine", ("mp_pair_rnorm_f32", "mp_pair_score_f32", "mp_pair_bwd_weights_f32"), run_cosine,
         oracle=_oracle_score(True)),
    Case("pair_sum", ("mp_pair_sum_f32",), run_sum, oracle=_oracle_sum),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_no_pair_entry_depends_on_fresh_allocations(dev, monkeypatch, case):
    from graphgym_amd import _lib_pair
    _lib_pair.lib()                   # bound before the recorder stands in: binding fetches every entry by name
    seen = differential(case.run, dev, monkeypatch, case.entries, case.oracle, what=case.name)
    print(f"{case.name}: {seen} bytes through the shim")
