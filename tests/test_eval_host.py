"""Loss and evaluation, host side (no device): the NumPy restatement of the metric formulas (tests/_eval_ref.py) against
scikit-learn, the closure of include/mp_eval.h over the library's exports and graphgym_amd._lib_eval.PROTOTYPES_EVAL, the
argument validation of every mp_eval_* entry, and metrics.compute_loss on CPU tensors against the reference's formulas
(graphgym/loss.py:11-50)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _eval_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mp_eval.h")
M = 5000
EPS = 4 * 2.0 ** -53


def _scores(levels, seed):
    """continuous scores (levels None) or scores quantised to `levels` values"""
    rng = np.random.default_rng(seed)
    s = rng.random(M).astype(np.float32)
    if levels is not None:
        s = (np.floor(s * levels) / max(levels, 1)).astype(np.float32)
    return s


def _labels(frac, score, seed):
    """positives with probability frac, pushed towards the high scores so that the AUC is not 0.5"""
    rng = np.random.default_rng(seed + 100)
    y = (rng.random(M) < frac).astype(np.int64)
    flip = rng.random(M) < 0.3
    lean = (score > np.quantile(score, 1 - frac)).astype(np.int64)
    y = np.where(flip, lean, y)
    if y.min() == y.max():
        y[0], y[1] = 0, 1
    return y


@pytest.mark.parametrize("frac", [0.02, 0.5, 0.98])
@pytest.mark.parametrize("levels", [None, 1, 2, 3, 7, 1000])
def test_restatement_matches_scikit_learn(levels, frac):
    sk = pytest.importorskip("sklearn.metrics")
    s = _scores(levels, 1)
    y = _labels(frac, s, 2)
    got = R.binary_metrics(y, s)
    pred = (s > 0.5).astype(np.int64)
    tp, fp, tn, fn, invalid = R.binary_counts(y, s)
    assert invalid == 0
    assert (tp, fp, tn, fn) == (int(((y == 1) & (pred == 1)).sum()), int(((y == 0) & (pred == 1)).sum()),
                                int(((y == 0) & (pred == 0)).sum()), int(((y == 1) & (pred == 0)).sum()))
    ref = {"accuracy": sk.accuracy_score(y, pred), "precision": sk.precision_score(y, pred, zero_division=0.0),
           "recall": sk.recall_score(y, pred, zero_division=0.0), "f1": sk.f1_score(y, pred, zero_division=0.0)}
    for k, v in ref.items():
        print(k, got[k], v, abs(got[k] - v))
        assert abs(got[k] - v) <= EPS, k
    auc = sk.roc_auc_score(y, s)
    print("auc", got["auc"], auc, abs(got["auc"] - auc))
    assert abs(got["auc"] - auc) <= (M + 1) * 2.0 ** -50
    # the engine's own host formulas are the restatement's, bit for bit
    from graphgym_amd import metrics
    two_u, p, n, nan = R.auc_counts(y, s)
    assert metrics.binary_stats(tp, fp, tn, fn, two_u, p, n) == got


def test_restatement_special_cases():
    sk = pytest.importorskip("sklearn.metrics")
    s = _scores(None, 3)
    with pytest.warns(Warning):
        one_class = sk.roc_auc_score(np.ones(M, dtype=np.int64), s)
    assert math.isnan(one_class) and math.isnan(R.binary_metrics(np.ones(M, dtype=np.int64), s)["auc"])
    assert math.isnan(R.binary_metrics(np.zeros(M, dtype=np.int64), s)["auc"])
    y = _labels(0.5, s, 4)
    bad = s.copy()
    bad[17] = np.nan
    with pytest.raises(ValueError):
        sk.roc_auc_score(y, bad)
    with pytest.raises(ValueError, match="NaN"):
        R.binary_metrics(y, bad)
    assert R.auc_counts(y, bad)[3] == 1
    low = s * np.float32(0.25)                                   # no predicted positives
    got = R.binary_metrics(y, low)
    assert got["precision"] == 0.0 == sk.precision_score(y, np.zeros(M, dtype=np.int64), zero_division=0.0)
    assert got["recall"] == 0.0 and got["f1"] == 0.0
    # -0.0 and 0.0 are one tie group
    z = np.array([-0.0, 0.0, -0.0, 0.0], dtype=np.float32)
    assert R.auc_counts([1, 0, 0, 1], z)[:3] == (4, 2, 2) and R.binary_metrics([1, 0, 0, 1], z)["auc"] == 0.5
    # multi-class and regression
    g = np.random.default_rng(5)
    sc = np.round(g.standard_normal((M, 7)), 1).astype(np.float32)        # rounded: ties between columns occur
    yt = g.integers(0, 7, M)
    best = R.first_argmax(sc)
    loop = np.zeros(M, dtype=np.int64)
    for c in range(1, 7):
        loop = np.where(sc[:, c] > sc[np.arange(M), loop], c, loop)
    assert (best == loop).all() and bool((np.sort(sc, 1)[:, -1] == np.sort(sc, 1)[:, -2]).any())
    assert abs(R.multi_metrics(yt, sc)["accuracy"] - sk.accuracy_score(yt, best)) <= EPS
    p, t = g.standard_normal(M), g.standard_normal(M)
    reg = R.regression_metrics(t, p)
    assert abs(reg["mae"] - sk.mean_absolute_error(t, p)) <= EPS * max(1.0, reg["mae"])
    assert abs(reg["mse"] - sk.mean_squared_error(t, p)) <= EPS * max(1.0, reg["mse"])
    assert reg["rmse"] == math.sqrt(reg["mse"])


# ---- the header's closure -------------------------------------------------------------------------------------------------
def declared_symbols(path=HEADER):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mp_eval_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound_and_the_reverse():
    from graphgym_amd import _lib, _lib_eval
    from graphgym_amd import build as mpbuild
    lib = _lib_eval.lib()
    names = declared_symbols()
    assert len(names) >= 8
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mp_eval.h but not exported"
        assert n in _lib_eval.PROTOTYPES_EVAL, f"{n} has no ctypes prototype"
    for n in _lib_eval.PROTOTYPES_EVAL:
        assert n.startswith("mp_eval_") and n in names, f"ctypes binds {n} which mp_eval.h does not declare"
        assert getattr(lib, n).argtypes == _lib_eval.PROTOTYPES_EVAL[n][1]
    # nothing of it in the engine's header or table
    engine = open(os.path.join(ROOT, "include", "mp_engine.h")).read()
    assert "mp_eval_" not in engine
    assert not [n for n in _lib.PROTOTYPES if n.startswith("mp_eval_")]
    assert HEADER in mpbuild.HEADERS and "evalmetrics.hip" in mpbuild.SOURCES
    assert lib.mp_eval_state_words() == _lib_eval.STATE_WORDS
    # the state words of the header's enum are the table's
    text = open(HEADER).read()
    for name, value in (("COUNT", _lib_eval.COUNT), ("HITS", _lib_eval.HITS), ("INVALID", _lib_eval.INVALID),
                        ("TP", _lib_eval.TP), ("FP", _lib_eval.FP), ("TN", _lib_eval.TN), ("FN", _lib_eval.FN),
                        ("NAN", _lib_eval.NAN), ("TWO_U", _lib_eval.TWO_U), ("P", _lib_eval.P), ("N", _lib_eval.N),
                        ("SIZE", _lib_eval.SIZE), ("LOSS", _lib_eval.LOSS), ("ABS", _lib_eval.ABS), ("SQ", _lib_eval.SQ),
                        ("STATE_WORDS", _lib_eval.STATE_WORDS)):
        assert re.search(rf"\bMP_EVAL_{name} = {value}\b", text), name


def test_argument_validation_without_device():
    """null pointers, negative sizes, ld < C and C <= 0 are MP_ERR_INVALID_ARG before any launch"""
    from graphgym_amd import _lib_eval
    lib = _lib_eval.lib()
    INVALID = 1
    buf = (C.c_double * 64)()                      # a host buffer stands in for every pointer: nothing is launched
    p = C.cast(buf, C.c_void_p)
    nb = C.c_size_t(0)
    assert lib.mp_eval_ws_bytes(-1, C.byref(nb)) == INVALID
    assert lib.mp_eval_ws_bytes(10, None) == INVALID
    assert lib.mp_eval_ws_bytes(0, C.byref(nb)) == 0 and nb.value >= 16
    assert lib.mp_eval_ws_bytes(10 ** 7, C.byref(nb)) == 0 and nb.value >= 2048 * 16
    ws = nb.value
    # mp_eval_loss_fwd_f32(kind, z, y, n, scale, score, loss, ws, ws_bytes, stream)
    for kind in (0, 1):
        assert lib.mp_eval_loss_fwd_f32(kind, None, p, 4, 1.0, p, p, p, ws, None) == INVALID
        assert lib.mp_eval_loss_fwd_f32(kind, p, None, 4, 1.0, p, p, p, ws, None) == INVALID
        assert lib.mp_eval_loss_fwd_f32(kind, p, p, 4, 1.0, None, p, p, ws, None) == INVALID
        assert lib.mp_eval_loss_fwd_f32(kind, p, p, 4, 1.0, p, None, p, ws, None) == INVALID
        assert lib.mp_eval_loss_fwd_f32(kind, p, p, 4, 1.0, p, p, None, ws, None) == INVALID
        assert lib.mp_eval_loss_fwd_f32(kind, p, p, -1, 1.0, p, p, p, ws, None) == INVALID
        assert lib.mp_eval_loss_fwd_f32(kind, p, p, 4, 1.0, p, p, p, 0, None) == 3          # workspace too small
        # mp_eval_loss_bwd_f32(kind, z, y, n, g, scale, dz, stream)
        assert lib.mp_eval_loss_bwd_f32(kind, None, p, 4, p, 1.0, p, None) == INVALID
        assert lib.mp_eval_loss_bwd_f32(kind, p, None, 4, p, 1.0, p, None) == INVALID
        assert lib.mp_eval_loss_bwd_f32(kind, p, p, 4, None, 1.0, p, None) == INVALID
        assert lib.mp_eval_loss_bwd_f32(kind, p, p, 4, p, 1.0, None, None) == INVALID
        assert lib.mp_eval_loss_bwd_f32(kind, p, p, -1, p, 1.0, p, None) == INVALID
        assert lib.mp_eval_loss_bwd_f32(kind, p, p, 0, p, 1.0, p, None) == 0                # nothing to do
    assert lib.mp_eval_loss_fwd_f32(2, p, p, 4, 1.0, p, p, p, ws, None) == INVALID          # unknown kind
    assert lib.mp_eval_loss_bwd_f32(-1, p, p, 4, p, 1.0, p, None) == INVALID
    # mp_eval_multi_logits_f32(logits, ld, n_rows, labels, index, n_sel, C, state, ws, ws_bytes, stream)
    assert lib.mp_eval_multi_logits_f32(None, 7, 4, p, None, 4, 7, p, p, ws, None) == INVALID
    assert lib.mp_eval_multi_logits_f32(p, 7, 4, None, None, 4, 7, p, p, ws, None) == INVALID
    assert lib.mp_eval_multi_logits_f32(p, 7, 4, p, None, 4, 7, None, p, ws, None) == INVALID
    assert lib.mp_eval_multi_logits_f32(p, 7, 4, p, None, 4, 7, p, None, ws, None) == INVALID
    assert lib.mp_eval_multi_logits_f32(p, 7, 4, p, None, -1, 7, p, p, ws, None) == INVALID
    assert lib.mp_eval_multi_logits_f32(p, 7, -1, p, None, 4, 7, p, p, ws, None) == INVALID
    assert lib.mp_eval_multi_logits_f32(p, 6, 4, p, None, 4, 7, p, p, ws, None) == INVALID      # ld < C
    assert lib.mp_eval_multi_logits_f32(p, 7, 4, p, None, 4, 0, p, p, ws, None) == INVALID      # C <= 0
    assert lib.mp_eval_multi_logits_f32(p, 7, 4, p, None, 4, -3, p, p, ws, None) == INVALID
    assert lib.mp_eval_multi_logits_f32(p, 7, 4, p, None, 5, 7, p, p, ws, None) == INVALID      # more labels than rows
    assert lib.mp_eval_multi_logits_f32(p, 2000, 4, p, None, 4, 1025, p, p, ws, None) == 2      # unsupported
    assert lib.mp_eval_multi_logits_f32(p, 7, 4, p, None, 4, 7, p, p, 0, None) == 3
    assert lib.mp_eval_multi_logits_f32(p, 7, 4, p, None, 0, 7, p, p, ws, None) == 0
    # mp_eval_multi_scores_f32(scores, ld, n, labels, C, loss_dev, loss_host, state, stream)
    assert lib.mp_eval_multi_scores_f32(None, 7, 4, p, 7, None, 0.0, p, None) == INVALID
    assert lib.mp_eval_multi_scores_f32(p, 7, 4, None, 7, None, 0.0, p, None) == INVALID
    assert lib.mp_eval_multi_scores_f32(p, 7, 4, p, 7, None, 0.0, None, None) == INVALID
    assert lib.mp_eval_multi_scores_f32(p, 7, -1, p, 7, None, 0.0, p, None) == INVALID
    assert lib.mp_eval_multi_scores_f32(p, 6, 4, p, 7, None, 0.0, p, None) == INVALID
    assert lib.mp_eval_multi_scores_f32(p, 7, 4, p, 0, None, 0.0, p, None) == INVALID
    assert lib.mp_eval_multi_scores_f32(p, 2000, 4, p, 1025, None, 0.0, p, None) == 2
    assert lib.mp_eval_multi_scores_f32(p, 7, 0, p, 7, None, 0.0, p, None) == 0
    # mp_eval_binary_f32(score, labels, labels_f32, n, thresh, loss_dev, loss_host, score_keep, label_keep, state, stream)
    for li, lf in ((p, None), (None, p)):
        assert lib.mp_eval_binary_f32(None, li, lf, 4, 0.5, None, 0.0, None, None, p, None) == INVALID
        assert lib.mp_eval_binary_f32(p, li, lf, 4, 0.5, None, 0.0, None, None, None, None) == INVALID
        assert lib.mp_eval_binary_f32(p, li, lf, -1, 0.5, None, 0.0, None, None, p, None) == INVALID
        assert lib.mp_eval_binary_f32(p, li, lf, 4, 0.5, None, 0.0, p, None, p, None) == INVALID    # one keep buffer only
        assert lib.mp_eval_binary_f32(p, li, lf, 4, 0.5, None, 0.0, None, p, p, None) == INVALID
        assert lib.mp_eval_binary_f32(p, li, lf, 0, 0.5, None, 0.0, None, None, p, None) == 0
    assert lib.mp_eval_binary_f32(p, None, None, 4, 0.5, None, 0.0, None, None, p, None) == INVALID  # no labels
    assert lib.mp_eval_binary_f32(p, p, p, 4, 0.5, None, 0.0, None, None, p, None) == INVALID        # both forms
    # mp_eval_regression_f32(pred, truth, n, loss_dev, loss_host, state, ws, ws_bytes, stream)
    assert lib.mp_eval_regression_f32(None, p, 4, None, 0.0, p, p, ws, None) == INVALID
    assert lib.mp_eval_regression_f32(p, None, 4, None, 0.0, p, p, ws, None) == INVALID
    assert lib.mp_eval_regression_f32(p, p, 4, None, 0.0, None, p, ws, None) == INVALID
    assert lib.mp_eval_regression_f32(p, p, 4, None, 0.0, p, None, ws, None) == INVALID
    assert lib.mp_eval_regression_f32(p, p, -1, None, 0.0, p, p, ws, None) == INVALID
    assert lib.mp_eval_regression_f32(p, p, 4, None, 0.0, p, p, 0, None) == 3
    assert lib.mp_eval_regression_f32(p, p, 0, None, 0.0, p, p, ws, None) == 0
    # mp_eval_auc_pairs(sorted_score, sorted_label, cn, n, state, stream)
    assert lib.mp_eval_auc_pairs(None, p, p, 4, p, None) == INVALID
    assert lib.mp_eval_auc_pairs(p, None, p, 4, p, None) == INVALID
    assert lib.mp_eval_auc_pairs(p, p, None, 4, p, None) == INVALID
    assert lib.mp_eval_auc_pairs(p, p, p, 4, None, None) == INVALID
    assert lib.mp_eval_auc_pairs(p, p, p, -1, p, None) == INVALID
    assert lib.mp_eval_auc_pairs(p, p, p, 0, p, None) == 0


# ---- compute_loss on CPU tensors ------------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("size_average", ["mean", "sum"])
def test_compute_loss_cpu_is_the_reference_formulas(size_average):
    from graphgym_amd import metrics
    n = 65
    # multi-class
    z = torch.randn(n, 7, generator=_gen(0))
    y = torch.randint(0, 7, (n,), generator=_gen(1))
    loss, score = metrics.compute_loss(z, y, "cross_entropy", size_average)
    assert torch.equal(score, F.log_softmax(z, dim=-1)) and torch.equal(loss, F.nll_loss(score, y))
    # binary, [M] and [M, 1]
    b = torch.randn(n, generator=_gen(2)) * 6
    t = torch.randint(0, 2, (n,), generator=_gen(3))
    ref = F.binary_cross_entropy_with_logits(b, t.float(), reduction=size_average)
    for pred, true in ((b, t), (b[:, None], t), (b[:, None], t[:, None]), (b, t.float())):
        loss, score = metrics.compute_loss(pred, true, "cross_entropy", size_average)
        assert torch.equal(loss, ref) and torch.equal(score, torch.sigmoid(b)) and score.shape == (n,)
    # multi-task binary [M, T]: flattened
    bt = torch.randn(n, 3, generator=_gen(4))
    tt = torch.randint(0, 2, (n, 3), generator=_gen(5))
    loss, score = metrics.compute_loss(bt, tt, "cross_entropy", size_average)
    assert score.shape == (3 * n,) and torch.equal(score, torch.sigmoid(bt.flatten()))
    assert torch.equal(loss, F.binary_cross_entropy_with_logits(bt.flatten(), tt.flatten().float(), reduction=size_average))
    # mse: [M, T] is not flattened, [M, 1] is squeezed, the score is pred itself
    r = torch.randn(n, 1, generator=_gen(6))
    loss, score = metrics.compute_loss(b[:, None], r, "mse", size_average)
    assert torch.equal(loss, F.mse_loss(b, r[:, 0], reduction=size_average)) and torch.equal(score, b)
    loss, score = metrics.compute_loss(bt, tt, "mse", size_average)
    assert torch.equal(loss, F.mse_loss(bt, tt.float(), reduction=size_average)) and score.shape == (n, 3)
    with pytest.raises(ValueError, match="Loss func hinge not supported"):
        metrics.compute_loss(b, t, "hinge", size_average)


def test_defaults_come_from_cfg(monkeypatch):
    from graphgym_amd import metrics
    from graphgym_amd.config import _defaults, cfg
    d = _defaults()
    assert (d.model.size_average, d.model.thresh, d.round, d.metric_best) == ("mean", 0.5, 4, "auto")
    assert (d.model.loss_fun, d.model.graph_pooling) == ("cross_entropy", "add")           # existing keys unchanged
    b = torch.randn(33, generator=_gen(7))
    t = torch.randint(0, 2, (33,), generator=_gen(8))
    monkeypatch.setattr(cfg.model, "loss_fun", "cross_entropy", raising=False)
    monkeypatch.setattr(cfg.model, "size_average", "sum", raising=False)
    assert torch.equal(metrics.compute_loss(b, t)[0], F.binary_cross_entropy_with_logits(b, t.float(), reduction="sum"))
    monkeypatch.setattr(cfg.model, "loss_fun", "mse", raising=False)
    assert torch.equal(metrics.compute_loss(b, t)[0], F.mse_loss(b, t.float(), reduction="sum"))
    monkeypatch.setattr(cfg.model, "loss_fun", "nope", raising=False)
    with pytest.raises(ValueError, match="Loss func nope not supported"):
        metrics.compute_loss(b, t)
    monkeypatch.setattr(cfg.model, "thresh", 0.25, raising=False)
    assert metrics.Meter("classification_binary").thresh == 0.25
    assert metrics.Meter("classification_binary", thresh=0.75).thresh == 0.75
    with pytest.raises(ValueError, match="Task has to be regression or classification"):
        metrics.Meter("classification")


def test_engine_ops_refuse_what_they_do_not_serve():
    from graphgym_amd import EngineError, metrics
    b = torch.randn(8)
    with pytest.raises(TypeError):
        metrics.bce_logits(b.double(), b.double())
    with pytest.raises(TypeError):
        metrics.mse(b, b.half())
    with pytest.raises(EngineError):
        metrics.Meter("regression").update(b, b, 0.0)          # CPU tensors: the meter has no CPU path
    with pytest.raises(ValueError, match="reduction"):
        metrics._scale(4, "none")
    m = metrics.Meter("classification_multi")
    assert m.counts()["count"] == 0 and math.isnan(m.raw()["loss"])      # an epoch without updates
