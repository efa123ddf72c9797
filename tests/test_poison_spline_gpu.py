"""Neither mp_spline_* entry may depend on the contents of its fresh allocations: the cases of tests/test_poison_gpu.py
for include/mp_spline.h, under the same harness (tests/_poison.py through that file's `differential`: the three fills in
their order, the recorder, the guards) and the same checks 1-5 of its docstring.

The graph is that file's hub graph: one row of 1 300 entries above the default hub_deg, so the pieces' partial sums —
both slabs of the two-sum form — live in a poisoned workspace and the finalize kernel reads them; one row in twenty is
empty.  Forward and backward run, so each case reaches both entries: the other one on the transposed pattern, with the
weights permuted into its entry order.  Every sum has a fixed order: the results under the three fills are equal bit for
bit."""
import pytest
import torch

import _spline_ref as R
from _tol import both, close
from test_poison_gpu import Case, N_NODES, differential, hub_graph, leaf, rnd

D = 12


def _weights(g, seed):
    return torch.rand(g.nnz, 2, generator=torch.Generator().manual_seed(seed)).to(g.device)


def run_spline_agg(dev):
    from graphgym_amd import ops
    g = hub_graph(dev, weighted=False)
    w, x = _weights(g, 3), leaf(rnd(N_NODES, D, seed=4), dev)
    y = ops.spline_agg(g, w, x)
    y.backward(rnd(N_NODES, 2 * D, seed=5).to(dev))
    return y, x.grad, w, g.row_ids(), g.col


def run_spline_fold(dev):
    from graphgym_amd import ops
    g = hub_graph(dev, weighted=False)
    w, z = _weights(g, 6), leaf(rnd(N_NODES, 2 * D, seed=7), dev)
    y = ops.spline_fold(g, w, z)
    y.backward(rnd(N_NODES, D, seed=8).to(dev))
    return y, z.grad, w, g.row_ids(), g.col


def _oracle(fold):
    def check(outs):
        y, dx, w, rows, cols = (t.cpu() for t in outs)
        rows, cols = rows.long(), cols.long()
        x = rnd(N_NODES, 2 * D if fold else D, seed=7 if fold else 4)
        dy = rnd(N_NODES, D if fold else 2 * D, seed=8 if fold else 5)
        fwd, bwd = (R.entry_fold, R.entry_sums) if fold else (R.entry_sums, R.entry_fold)
        close(y, both(lambda c: fwd(rows, cols, c(w), c(x), N_NODES)), what="spline forward")
        close(dx, both(lambda c: bwd(cols, rows, c(w), c(dy), N_NODES)), what="spline input gradient")
    return check


CASES = [
    Case("spline_agg", ("mp_spline_agg_f32", "mp_spline_fold_f32"), run_spline_agg, oracle=_oracle(False)),
    Case("spline_fold", ("mp_spline_fold_f32", "mp_spline_agg_f32"), run_spline_fold, oracle=_oracle(True)),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_no_spline_entry_depends_on_fresh_allocations(dev, monkeypatch, case):
    from graphgym_amd import _lib_spline
    _lib_spline.lib()                 # bound before the recorder stands in: binding fetches every entry by name
    seen = differential(case.run, dev, monkeypatch, case.entries, case.oracle, what=case.name)
    print(f"{case.name}: {seen} bytes through the shim")
