"""No mp_eval_* entry may depend on the contents of its fresh allocations: the cases of tests/test_poison_gpu.py for the
loss and evaluation layer (include/mp_eval.h), under the same harness (tests/_poison.py through that file's
`differential`: the three fills in their order, the recorder, the guards) and the same checks 1-4 of its docstring.

The state tensor is a `torch.zeros` the caller owns (never poisoned: its zero IS the contract); the per-workgroup partial
sums, the kept scores and labels, the scores, losses and gradients are `torch.empty` (mp_eval_multi_scores_f32 takes no
buffer of its own: its case allocates the score matrix it reads).  Every case builds everything inside
the poisoned context and returns the state itself, so a partial sum read before it was written shows in the double words.
All cases have at least 4 rows and 4 classes (the integer-1 fill stays in range)."""
import re

import pytest
import torch

from test_poison_gpu import Case, differential, gen, ints, rnd

N = 700          # three workgroups, the last one partly filled
C = 7


def _logits(dev):
    wide = ints(N, C + 3, seed=1).to(dev)
    return wide[:, 1:C + 1]                       # ld > C


def _labels(dev, hi, seed):
    return torch.randint(0, hi, (N,), generator=gen(seed)).to(dev)


def run_losses(dev):
    from graphgym_amd import metrics
    out = []
    y = torch.rand(N, generator=gen(3)).to(dev)
    for op in (metrics.bce_logits, metrics.mse):
        for size_average in ("mean", "sum"):
            z = rnd(N, seed=2).mul(4).to(dev).requires_grad_(True)
            loss, score = op(z, y, size_average)
            (loss * 1.5).backward()
            out += [loss.detach(), score, z.grad]
    return tuple(out)


def run_multi_logits(dev):
    from graphgym_amd import metrics
    m = metrics.Meter("classification_multi")
    z, y = _logits(dev), _labels(dev, C, 4)
    idx = torch.randint(0, N, (N + 5,), generator=gen(5)).to(dev)
    m.update_logits(z, y)
    m.update_logits(z, y[idx], idx)
    return (m.state,)


def run_multi_scores(dev):
    from graphgym_amd import metrics
    m = metrics.Meter("classification_multi")
    y = _labels(dev, C, 6)
    z = torch.empty((N, C), device=dev).copy_(_logits(dev))     # the scores of a step are a fresh allocation themselves
    m.update(y, z, torch.tensor(0.75, device=dev))
    m.update(y[:300], z[:300], 0.5)
    return (m.state,)


def run_binary(dev):
    from graphgym_amd import metrics
    m = metrics.Meter("classification_binary")
    s = (torch.rand(N, generator=gen(7)) * 16).floor().div(16).to(dev)          # tie groups
    y = _labels(dev, 2, 8)
    m.update(y, s, torch.tensor(0.75, device=dev))
    m.update(y[:300].float()[:, None], s[:300, None], 0.5)
    counts = m.counts()                                                         # sort, prefix count, pair-count kernel
    assert counts["p"] + counts["n"] == N + 300 and counts["two_u"] > 0
    return (m.state, m._scores[0], m._labels[0])


def run_regression(dev):
    from graphgym_amd import metrics
    m = metrics.Meter("regression")
    p, t = rnd(N, seed=9).to(dev), rnd(N, seed=10).to(dev)
    m.update(t, p, torch.tensor(0.75, device=dev))
    m.update(t[:300, None], p[:300], 0.5)
    return (m.state,)


CASES = [
    Case("eval_losses", ("mp_eval_loss_fwd_f32", "mp_eval_loss_bwd_f32"), run_losses),
    Case("eval_multi_logits", ("mp_eval_multi_logits_f32",), run_multi_logits),
    Case("eval_multi_scores", ("mp_eval_multi_scores_f32",), run_multi_scores),
    Case("eval_binary", ("mp_eval_binary_f32", "mp_eval_auc_pairs"), run_binary),
    Case("eval_regression", ("mp_eval_regression_f32",), run_regression),
]

HOST_ONLY = "host-only: no device memory is touched"
EXCLUDED = {"mp_eval_state_words": HOST_ONLY, "mp_eval_ws_bytes": HOST_ONLY}
_ADMISSIBLE = re.compile(r"^(mp_eval_.*_bytes|mp_eval_state_words)$")


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_no_eval_entry_depends_on_fresh_allocations(dev, monkeypatch, case):
    from graphgym_amd import _lib_eval
    _lib_eval.lib()                      # bound before the recorder stands in: binding fetches every entry by name
    seen = differential(case.run, dev, monkeypatch, case.entries, what=case.name)
    print(f"{case.name}: {seen} bytes through the shim")


def test_every_eval_entry_has_a_case_or_a_reason():
    """a new mp_eval_* entry fails here until someone gives it a case above"""
    from graphgym_amd import _lib_eval
    covered = set()
    for case in CASES:
        assert case.entries and case.exact and callable(case.run), case.name
        covered |= set(case.entries)
    names = [c.name for c in CASES]
    assert len(names) == len(set(names))
    every = set(_lib_eval.PROTOTYPES_EVAL)
    assert covered <= every, f"cases name entries that do not exist: {sorted(covered - every)}"
    assert not (covered & set(EXCLUDED)), f"both covered and excluded: {sorted(covered & set(EXCLUDED))}"
    assert set(EXCLUDED) <= every, f"excluded names that do not exist: {sorted(set(EXCLUDED) - every)}"
    for name, reason in EXCLUDED.items():
        assert _ADMISSIBLE.match(name) and reason == HOST_ONLY, f"{name}: not an admissible exclusion"
    missing = every - covered - set(EXCLUDED)
    assert not missing, f"C entries without a case: {sorted(missing)}"
