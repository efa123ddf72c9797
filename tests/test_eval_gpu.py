"""Loss and evaluation on the device (graphgym_amd.metrics, csrc/evalmetrics.hip) against tests/_eval_ref.py and torch on
the CPU: integer statistics exactly (hence every ratio bit for bit), float results under tests/_tol.py.

Sizes: 1, 63, 64, 65, 257 (a lane, a wave and a workgroup, and one past each) and BIG = 524 288 + 257, one past a single
pass of flat_grid's 2 048 workgroups of 256 threads; C in {1, 2, 7, 47}; logits as column slices of a wider matrix
(ld > C); an index with repeats."""
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

import _eval_ref as R
from _tol import both, close, close_all

pytestmark = pytest.mark.gpu

ONE_PASS = 256 * 8 * 256
BIG = ONE_PASS + 257
SIZES = [1, 63, 64, 65, 257, BIG]
INT_WORDS = 12                      # words 0 .. 11 of the state are the int64 counters


def gen(seed):
    return torch.Generator().manual_seed(seed)


def f64(v):
    return torch.tensor(v, dtype=torch.float64)


def logits_like(n, seed, *cols):
    """N(0, 6^2) with a few entries set to +-100 by hand; no infinities"""
    z = torch.randn(n, *cols, generator=gen(seed)) * 6
    flat = z.view(-1)
    for k, v in ((0, 100.0), (flat.numel() // 3, -100.0), (flat.numel() // 2, 100.0), (flat.numel() - 1, -100.0)):
        flat[k] = v
    return z


def chunks(n, parts=3):
    """an epoch of `parts` uneven updates (empty ones dropped)"""
    cuts = sorted({0, n // 5, (2 * n) // 3, n})
    return [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]


def binary_meter(dev, score, label, thresh=0.5, order=None):
    from graphgym_amd import metrics
    m = metrics.Meter("classification_binary", thresh=thresh)
    parts = chunks(score.numel())
    for a, b in (parts if order is None else [parts[i] for i in order]):
        m.update(label[a:b].to(dev), score[a:b].to(dev), 0.25)
    return m


def check_binary(dev, score, label, thresh=0.5):
    """the engine's counters equal the restatement's exactly, its ratios bit for bit"""
    m = binary_meter(dev, score, label, thresh)
    c = m.counts()
    tp, fp, tn, fn, invalid = R.binary_counts(label.numpy(), score.numpy(), thresh)
    two_u, p, n, nan = R.auc_counts(label.numpy(), score.numpy())
    got = (c["tp"], c["fp"], c["tn"], c["fn"], c["invalid"], c["two_u"], c["p"], c["n"], c["nan"], c["count"])
    print("binary", score.numel(), got)
    assert got == (tp, fp, tn, fn, invalid, two_u, p, n, nan, tp + fp + tn + fn)
    want = R.binary_metrics(label.numpy(), score.numpy(), thresh)
    raw = m.raw()
    for k, v in want.items():
        assert raw[k] == v or (math.isnan(raw[k]) and math.isnan(v)), (k, raw[k], v)
    assert set(m.compute()) == {"loss", "accuracy", "precision", "recall", "f1", "auc"}
    assert m.counts() == c, "compute() twice gives the same state"
    return m


# ---- integer statistics are exact ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_binary_statistics_and_auc_are_exact(dev, n):
    g = gen(n)
    score = torch.rand(n, generator=g)
    tied = torch.rand(n, generator=g) < 0.5
    score = torch.where(tied, torch.floor(score * 7) / 7, score)        # half of the scores in 7 tie groups
    label = (torch.rand(n, generator=g) < 0.2 + 0.6 * score).long()
    check_binary(dev, score, label)
    check_binary(dev, score, label.float(), thresh=0.3)                 # link_pred's float labels (transform.py:93-98)


def _two_values(n, boundary):
    score = torch.full((n,), 0.75)
    score[:boundary] = 0.25
    label = (torch.arange(n) % 3 == 0).long()
    perm = torch.randperm(n, generator=gen(boundary))
    return score[perm], label[perm]


AUC_INPUTS = {
    "all_equal": lambda: (torch.full((300,), 0.5), (torch.arange(300) % 2).long()),
    "saturated": lambda: ((torch.arange(400) % 5 < 2).float(), (torch.arange(400) % 3 == 0).long()),
    "one_positive": lambda: (torch.rand(300, generator=gen(1)), (torch.arange(300) == 17).long()),
    "one_negative": lambda: (torch.rand(300, generator=gen(2)), (torch.arange(300) != 17).long()),
    "one_class": lambda: (torch.rand(300, generator=gen(3)), torch.ones(300, dtype=torch.int64)),
    "signed_zero": lambda: (torch.where(torch.arange(300) % 2 == 0, torch.tensor(-0.0), torch.tensor(0.0)),
                            (torch.arange(300) % 3 == 0).long()),
    "denormal": lambda: (torch.randint(-40, 41, (300,), generator=gen(4)).float() * 1.4e-45,
                         (torch.arange(300) % 2).long()),
}
for _b in (255, 256, 257):
    AUC_INPUTS[f"two_values_{_b}"] = (lambda b: (lambda: _two_values(600, b)))(_b)
for _b in (ONE_PASS - 1, ONE_PASS):
    AUC_INPUTS[f"two_values_{_b}"] = (lambda b: (lambda: _two_values(BIG, b)))(_b)


@pytest.mark.parametrize("name", sorted(AUC_INPUTS))
def test_auc_inputs(dev, name):
    score, label = AUC_INPUTS[name]()
    if name == "denormal":
        assert bool(((score != 0) & (score.abs() < 1.2e-38)).any())
    m = check_binary(dev, score, label, thresh=0.5)
    if name == "one_class":
        assert math.isnan(m.compute()["auc"])
    if name in ("all_equal", "signed_zero"):
        assert m.raw()["auc"] == 0.5


def multi_case(n, C, seed):
    """logits as a column slice of a wider matrix (ld > C), labels, an index with repeats"""
    wide = logits_like(n, seed, C + 3)
    wide = (wide * 2).round() / 2                                       # halves: maxima tie between columns
    z = wide[:, 1:C + 1]
    y = torch.randint(0, C, (n,), generator=gen(seed + 1))
    y = torch.where(torch.rand(n, generator=gen(seed + 2)) < 0.5, z.argmax(1), y)
    idx = torch.randint(0, n, (n + 3,), generator=gen(seed + 3))
    idx[:2] = idx[2]
    return wide, z, y, idx


@pytest.mark.parametrize("n,C", [(n, C) for n in SIZES[:-1] for C in (1, 2, 7, 47)] + [(BIG, 7)])
def test_multi_class_statistics_are_exact(dev, n, C):
    from graphgym_amd import metrics
    wide, z, y, idx = multi_case(n, C, 10 * n + C)
    zd = wide.to(dev)[:, 1:C + 1]
    assert zd.stride(0) == C + 3
    # the score form, in uneven updates
    m = metrics.Meter("classification_multi")
    for a, b in chunks(n):
        m.update(y[a:b].to(dev), zd[a:b], torch.tensor(0.5, device=dev))
    c = m.counts()
    assert (c["count"], c["hits"], c["invalid"]) == R.multi_counts(y.numpy(), z.numpy()) and c["size"] == n
    assert m.raw()["accuracy"] == R.multi_metrics(y.numpy(), z.numpy())["accuracy"] and m.raw()["loss"] == 0.5
    # the logit form through an index with repeats, and its loss against nn.softmax_cross_entropy's op on the same rows
    m2 = metrics.Meter("classification_multi")
    yi = y[idx]
    m2.update_logits(zd, yi.to(dev), idx.to(dev))
    c2 = m2.counts()
    assert (c2["count"], c2["hits"], c2["invalid"]) == R.multi_counts(yi.numpy(), z[idx].numpy())
    assert c2["size"] == idx.numel() and set(m2.compute()) == {"loss", "accuracy"}
    ce = torch.ops.mp.softmax_ce(zd, yi.to(dev), idx.to(dev))
    refs = both(lambda c: F.cross_entropy(c(z)[idx], yi))
    print("multi", n, C, m2.raw()["loss"], float(ce), float(refs[0]))
    close_all(f64(m2.raw()["loss"]), ce.double().cpu(), what="update_logits loss vs softmax_ce")
    close_all(f64(m2.raw()["loss"]), refs, what="update_logits loss vs torch")


def test_more_than_1024_classes_run_on_torch_and_say_so(dev):
    """C = 1030: the same statistics and loss, no synchronisation either, and a warning"""
    from graphgym_amd import metrics
    n, C = 65, 1030
    wide, z, y, idx = multi_case(n, C, 77)
    zd = wide.to(dev)[:, 1:C + 1]
    y[3] = -100
    yi = y[idx]
    m, m2 = metrics.Meter("classification_multi"), metrics.Meter("classification_multi")
    old = torch.cuda.get_sync_debug_mode()
    with pytest.warns(UserWarning, match="1030 classes"):
        m.update(y.to(dev), zd, 0.5)                            # (warmed outside the mode)
    yd, yid, idxd, half = y.to(dev), yi.to(dev), idx.to(dev), torch.tensor(0.5, device=dev)
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.warns(UserWarning, match="runs on torch"):
            m.update(yd, zd, half)
            m2.update_logits(zd, yid, idxd)
    finally:
        torch.cuda.set_sync_debug_mode(old)
    c, c2 = m.counts(), m2.counts()
    count, hits, invalid = R.multi_counts(y.numpy(), z.numpy())
    assert (c["count"], c["hits"], c["invalid"], c["size"]) == (2 * count, 2 * hits, 2 * invalid, 2 * n) and invalid == 1
    assert c["loss"] == 0.5 * 2 * n
    assert (c2["count"], c2["hits"], c2["invalid"]) == R.multi_counts(yi.numpy(), z[idx].numpy())
    ok = yi >= 0
    refs = both(lambda f: F.cross_entropy(f(z)[idx][ok], yi[ok], reduction="sum"))
    close_all(f64(c2["loss"]), refs, what="torch fallback loss")


def test_counters_are_64_bit(dev):
    """a counter pre-loaded with 2^31 - 3, one update of 10 rows: 2^31 + 7"""
    from graphgym_amd import _lib_eval as E
    from graphgym_amd import metrics
    start = 2 ** 31 - 3
    z = torch.eye(10, 7)[:, :7].contiguous()
    z[7:, 0] = 1.0
    y = z.argmax(1)
    m = metrics.Meter("classification_multi")
    st = m._state_on(dev)
    st[E.COUNT], st[E.HITS], st[E.SIZE] = start, start, start
    m.update(y.to(dev), z.to(dev), 0.0)
    c = m.counts()
    assert (c["count"], c["hits"], c["size"]) == (2 ** 31 + 7,) * 3
    b = metrics.Meter("classification_binary")
    st = b._state_on(dev)
    st[E.TP], st[E.TN] = start, start
    b.update(torch.ones(10, dtype=torch.int64, device=dev), torch.ones(10, device=dev), 0.0)
    b.update(torch.zeros(10, dtype=torch.int64, device=dev), torch.zeros(10, device=dev), 0.0)
    c = b.counts()
    assert (c["tp"], c["tn"], c["fp"], c["fn"]) == (2 ** 31 + 7, 2 ** 31 + 7, 0, 0) and c["two_u"] == 2 * 10 * 10


# ---- float parity ---------------------------------------------------------------------------------------------------------
def soft_targets(n, seed):
    y = torch.rand(n, generator=gen(seed))
    hard = torch.rand(n, generator=gen(seed + 1)) < 0.5
    return torch.where(hard, (y > 0.5).float(), y)                      # BCEWithLogitsLoss allows soft targets


@pytest.mark.parametrize("size_average", ["mean", "sum"])
@pytest.mark.parametrize("n", SIZES)
def test_bce_and_mse_match_torch(dev, n, size_average):
    from graphgym_amd import metrics
    z, y = logits_like(n, n), soft_targets(n, n + 7)
    gout = 1.75
    for name, fn, op, score_of in (("bce", F.binary_cross_entropy_with_logits, metrics.bce_logits, torch.sigmoid),
                                   ("mse", F.mse_loss, metrics.mse, lambda t: t)):
        def ref(c):
            a = c(z).clone().requires_grad_(True)
            loss = fn(a, c(y), reduction=size_average)
            (g,) = torch.autograd.grad(loss * gout, a)
            return loss.detach(), score_of(a.detach()), g
        r64, r32 = both(ref)
        zd = z.to(dev).requires_grad_(True)
        loss, score = op(zd, y.to(dev), size_average)
        assert loss.shape == () and loss.dtype == torch.float32 and score.shape == (n,) and not score.requires_grad
        (loss * gout).backward()
        print(name, n, size_average, float(loss.detach()), float(r64[0]))
        close_all(loss, (r64[0], r32[0]), what=f"{name} loss")
        close(score[:, None], (r64[1][:, None], r32[1][:, None]), what=f"{name} score")
        # the gradient is a difference of two fp32 values (sigmoid(z) - y, z - y) that cancels where the prediction is
        # right: held to the terms' absolute values (rule (d) of _tol.py)
        scale = gout / n if size_average == "mean" else gout
        mag = ((torch.sigmoid(z.double()) + y.double()) if name == "bce" else 2 * (z.double().abs() + y.double())) * scale
        close(zd.grad[:, None], (r64[2][:, None], r32[2][:, None]), mag=mag[:, None] * (1 + 1e-6), what=f"{name} grad")


@pytest.mark.parametrize("n", SIZES)
def test_regression_statistics_match_float64(dev, n):
    from graphgym_amd import metrics
    p, t = torch.randn(n, generator=gen(n)) * 3, torch.randn(n, generator=gen(n + 1)) * 3
    m = metrics.Meter("regression")
    for a, b in chunks(n):
        m.update(t[a:b, None].to(dev), p[a:b].to(dev), torch.tensor(2.0, device=dev))
    c, raw = m.counts(), m.raw()
    want = R.regression_metrics(t.numpy(), p.numpy())
    d32 = (p - t)
    ref32 = {"mae": float(d32.abs().mean()), "mse": float((d32 * d32).mean())}
    assert c["count"] == n == c["size"] and raw["loss"] == 2.0 and set(m.compute()) == {"loss", "mae", "mse", "rmse"}
    for k in ("mae", "mse"):
        print("regression", n, k, raw[k], want[k])
        close_all(f64(raw[k]), (f64(want[k]), f64(ref32[k])), what=f"regression {k}")
    assert raw["rmse"] == math.sqrt(raw["mse"])
    # the loss the meter reports for compute_loss's value: sum(loss * batch) / size
    m.reset()
    loss, score = metrics.compute_loss(p.to(dev), t.to(dev), "mse", "mean")
    m.update(t.to(dev), score, loss)
    close_all(f64(m.raw()["loss"]), f64(want["mse"]), what="meter loss")
    assert m.raw()["loss"] == float(loss)


# ---- determinism ----------------------------------------------------------------------------------------------------------
def test_epochs_are_reproducible(dev):
    from graphgym_amd import metrics
    n = 40000
    score = torch.rand(n, generator=gen(1)).round(decimals=2)
    label = (torch.rand(n, generator=gen(2)) < score).long()
    parts = list(range(len(chunks(n))))
    states = []
    for order in (parts, parts, parts[::-1]):
        m = binary_meter(dev, score, label, order=order)
        m.counts()
        states.append(m.state.clone())
    assert torch.equal(states[0], states[1])
    assert torch.equal(states[0][:INT_WORDS], states[2][:INT_WORDS])
    wide, z, y, idx = multi_case(n, 7, 5)
    zd, yd, p = wide.to(dev)[:, 1:8], y.to(dev), torch.randn(n, generator=gen(3)).to(dev)
    states = []
    for order in (parts, parts, parts[::-1]):
        m, r = metrics.Meter("classification_multi"), metrics.Meter("regression")
        for i in order:
            a, b = chunks(n)[i]
            m.update_logits(zd[a:b], yd[a:b])
            r.update(zd[a:b, 0], p[a:b], 0.125)
        states.append((m.state.clone(), r.state.clone()))
    assert torch.equal(states[0][0], states[1][0]) and torch.equal(states[0][1], states[1][1])
    assert torch.equal(states[0][0][:INT_WORDS], states[2][0][:INT_WORDS])
    assert torch.equal(states[0][1][:INT_WORDS], states[2][1][:INT_WORDS])


# ---- no synchronisation -----------------------------------------------------------------------------------------------------
def test_updates_do_not_synchronise(dev):
    from graphgym_amd import metrics
    n = 1000
    z = logits_like(n, 1, 7).to(dev)
    y = torch.randint(0, 7, (n,), generator=gen(2)).to(dev)
    b = logits_like(n, 3).to(dev)
    t = (torch.rand(n, generator=gen(4)) < 0.5).float().to(dev)
    idx = torch.randint(0, n, (n,), generator=gen(5)).to(dev)
    loss = torch.tensor(0.5, device=dev)
    meters = [metrics.Meter(k) for k in metrics.TASK_TYPES]

    def epoch():
        bm, mm, rm = meters
        bm.update(t, torch.sigmoid(b), loss)
        bm.update(t.long()[:, None], torch.sigmoid(b)[:, None], 0.5)
        bm.update_logits(b, t)
        mm.update(y, F.log_softmax(z, dim=-1), loss)
        mm.update_logits(z, y)
        mm.update_logits(z, y, idx)
        rm.update(t, b, loss)
        rm.update_logits(b[:, None], t[:, None])

    epoch()                                                     # warmed: code loaded, the states allocated
    for m in meters:
        m.reset()
    probe = torch.ones(1, device=dev)
    torch.cuda.synchronize()
    old = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):
            probe.item()                                        # the control: the mode does raise in this build
        epoch()
    finally:
        torch.cuda.set_sync_debug_mode(old)
    out = [m.compute() for m in meters]                         # outside the mode: the one copy per meter
    assert out[0]["accuracy"] > 0 and out[1]["loss"] > 0 and out[2]["mse"] > 0


# ---- bad input is counted, not dereferenced -------------------------------------------------------------------------------
def test_bad_labels_and_indices_are_counted(dev):
    from graphgym_amd import metrics
    n, C = 65, 7
    wide, z, y, _ = multi_case(n, C, 3)
    zd = wide.to(dev)[:, 1:C + 1]
    bad_rows = [3, 17, 64]
    ybad = y.clone()
    ybad[bad_rows] = torch.tensor([-100, C, 2 ** 40])
    keep = torch.ones(n, dtype=torch.bool)
    keep[bad_rows] = False
    for form in ("scores", "logits"):
        m = metrics.Meter("classification_multi")
        if form == "scores":
            m.update(ybad.to(dev), zd, 0.0)
        else:
            m.update_logits(zd, ybad.to(dev))
        c = m.counts()
        assert c["invalid"] == 3 and (c["count"], c["hits"]) == R.multi_counts(y[keep].numpy(), z[keep].numpy())[:2]
        with pytest.raises(ValueError, match="3 examples"):
            m.compute()
    # index values -1 and n_rows
    idx = torch.arange(n)
    idx[[5, 9]] = torch.tensor([-1, n])
    ok = torch.ones(n, dtype=torch.bool)
    ok[[5, 9]] = False
    m = metrics.Meter("classification_multi")
    m.update_logits(zd, y.to(dev), idx.to(dev))
    c = m.counts()
    assert c["invalid"] == 2 and (c["count"], c["hits"]) == R.multi_counts(y[ok].numpy(), z[ok].numpy())[:2]
    good = metrics.Meter("classification_multi")
    good.update_logits(zd, y[ok].to(dev), idx[ok].to(dev))
    # (the same rows in other lanes: the double sum groups them differently, so equal to rounding, not to the bit)
    assert abs(good.counts()["loss"] - c["loss"]) <= 1e-12 * abs(c["loss"]), "the valid rows' loss is unchanged"
    with pytest.raises(ValueError, match="2 examples"):
        m.compute()
    # binary: labels outside {0, 1}
    score = torch.rand(n, generator=gen(9))
    lab = (torch.rand(n, generator=gen(10)) < 0.5).long()
    labbad = lab.clone()
    labbad[bad_rows] = torch.tensor([-100, 2, 2 ** 40])
    m = binary_meter(dev, score, labbad)
    c = m.counts()
    tp, fp, tn, fn, _ = R.binary_counts(lab[keep].numpy(), score[keep].numpy())
    two_u, p, nn_, _ = R.auc_counts(lab[keep].numpy(), score[keep].numpy())
    assert (c["invalid"], c["tp"], c["fp"], c["tn"], c["fn"], c["two_u"], c["p"], c["n"]) == (3, tp, fp, tn, fn, two_u, p, nn_)
    with pytest.raises(ValueError, match="3 examples"):
        m.compute()
    half = binary_meter(dev, score, torch.where(torch.arange(n) == 4, torch.tensor(0.5), lab.float()))
    assert half.counts()["invalid"] == 1                       # a float label that is no integer
    # a NaN score
    snan = score.clone()
    snan[11] = float("nan")
    m = binary_meter(dev, snan, lab)
    assert m.counts()["nan"] == 1
    with pytest.raises(ValueError, match="NaN"):
        m.compute()


# ---- custom ops -----------------------------------------------------------------------------------------------------------
def test_opcheck(dev):
    from graphgym_amd import metrics  # noqa: F401
    z, y = logits_like(257, 1).to(dev), soft_targets(257, 2).to(dev)
    for op in (torch.ops.mp.bce_logits.default, torch.ops.mp.mse.default):
        for args in ((z.clone().requires_grad_(True), y, "mean"), (z.clone().requires_grad_(True), y, "sum"),
                     (z[:64].reshape(8, 8).clone().requires_grad_(True), y[:64].reshape(8, 8), "mean")):
            res = torch.library.opcheck(op, args, raise_exception=True)
            assert all(v == "SUCCESS" for v in res.values()), (op, res)
    for kind in (0, 1):
        res = torch.library.opcheck(torch.ops.mp.eltwise_loss_fwd_raw.default, (z, y, kind, 0.5), raise_exception=True)
        assert all(v == "SUCCESS" for v in res.values()), res
        res = torch.library.opcheck(torch.ops.mp.eltwise_loss_bwd_raw.default,
                                    (z, y, torch.tensor(2.0, device=dev), kind, 0.5), raise_exception=True)
        assert all(v == "SUCCESS" for v in res.values()), res


@pytest.mark.parametrize("name", ["bce", "mse"])
def test_gradients_under_every_subset(dev, name):
    """every subset of {pred, true} that requires grad: pred gets the formula's gradient, true gets none"""
    from graphgym_amd import metrics
    op = metrics.bce_logits if name == "bce" else metrics.mse
    fn = F.binary_cross_entropy_with_logits if name == "bce" else F.mse_loss
    z, y = logits_like(65, 1), soft_targets(65, 2)
    a = z.double().requires_grad_(True)
    (want,) = torch.autograd.grad(fn(a, y.double()), a)
    for subset in itertools.chain.from_iterable(itertools.combinations(("pred", "true"), k) for k in range(3)):
        zd = z.to(dev).requires_grad_("pred" in subset)
        yd = y.to(dev).requires_grad_("true" in subset)
        loss, score = op(zd, yd)
        assert loss.requires_grad == bool(subset) and not score.requires_grad
        if subset:
            loss.backward()
        assert yd.grad is None
        if "pred" in subset:
            close_all(zd.grad, want, what=f"{name} grad {subset}")
        else:
            assert zd.grad is None
    with pytest.raises(TypeError):
        op(z.to(dev).double(), y.to(dev).double())
    with pytest.raises(TypeError):
        torch.ops.mp.eltwise_loss_fwd_raw(z.to(dev).half(), y.to(dev).half(), 0, 1.0)


def test_compute_loss_routes_on_the_device(dev):
    from graphgym_amd import metrics
    n = 257
    z, t = logits_like(n, 1), (torch.rand(n, generator=gen(2)) < 0.5).long()
    for pred, true in ((z, t), (z[:, None], t[:, None]), (z.reshape(-1, 1), t.float())):
        loss, score = metrics.compute_loss(pred.to(dev), true.to(dev), "cross_entropy", "mean")
        refs = both(lambda c: F.binary_cross_entropy_with_logits(c(z), c(t.float())))
        close_all(loss, refs, what="compute_loss bce")
        assert score.shape == (n,)
    zt, tt = logits_like(n, 3, 3), (torch.rand(n, 3, generator=gen(4)) < 0.5).long()
    loss, score = metrics.compute_loss(zt.to(dev), tt.to(dev), "cross_entropy", "sum")
    close_all(loss, both(lambda c: F.binary_cross_entropy_with_logits(c(zt), c(tt.float()), reduction="sum")), what="[M, T]")
    assert score.shape == (3 * n,)
    zm, ym = logits_like(n, 5, 7), torch.randint(0, 7, (n,), generator=gen(6))
    loss, score = metrics.compute_loss(zm.to(dev), ym.to(dev), "cross_entropy")
    close_all(loss, both(lambda c: F.cross_entropy(c(zm), ym)), what="multi-class")
    assert torch.equal(score, F.log_softmax(zm.to(dev), dim=-1))
    loss, score = metrics.compute_loss(z[:, None].to(dev), t.to(dev), "mse", "mean")
    close_all(loss, both(lambda c: F.mse_loss(c(z), c(t.float()))), what="mse")
    assert score.shape == (n,) and torch.equal(score.cpu(), z)
    with pytest.raises(ValueError, match="Loss func l1 not supported"):
        metrics.compute_loss(z.to(dev), t.to(dev), "l1")


# ---- end to end -------------------------------------------------------------------------------------------------------------
def test_link_prediction_end_to_end(dev):
    """harness.GNN with the link_pred head on a link_pred.py batch of a 300-node BA graph: compute_loss -> backward ->
    Meter.update, then compute(); eval_epoch on the validation batch"""
    import graphgym_amd as ga
    import graphgym_amd.graphgym_plugin  # noqa: F401
    from graphgym_amd import graphgen, metrics
    from graphgym_amd import harness as H
    from graphgym_amd.config import cfg
    from graphgym_amd.link_pred import link_batch, link_split
    N = 300
    base = ga.CSRGraph.from_edge_index(graphgen.ba_edge_index(N, 3, seed=4).to(dev), N)
    splits = link_split(base, torch.tensor([0, N]), (0.8, 0.2), generator=gen(0))
    x = torch.rand(N, 10, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    want = dict(layers_mp=2, dim_inner=32, layers_pre_mp=1, layers_post_mp=1, batchnorm=True, l2norm=True, act="relu",
                dropout=0.0, agg="add", normalize_adj=False, stage_type="stack", layer_type="generalconv")
    old = {k: getattr(cfg.gnn, k) for k in want}
    old_task, old_dec = cfg.dataset.task, getattr(cfg.model, "edge_decoding", None)
    try:
        for k, v in want.items():
            setattr(cfg.gnn, k, v)
        cfg.dataset.task, cfg.model.edge_decoding = "link_pred", "dot"
        torch.manual_seed(0)
        model = H.GNN(10, 1).to(dev)
        opt = torch.optim.Adam(model.parameters(), lr=0.01)
        meter = metrics.Meter("classification_binary")
        kept = []

        def forward_loss():
            batch = link_batch(splits["train"], x, ratio=1.0, seed=1, offset=len(kept))
            pred, true = model(batch)
            loss, score = metrics.compute_loss(pred, true, "cross_entropy", "mean")
            kept.append((true.detach(), score.detach(), loss.detach()))
            return loss
        for _ in range(2):
            H.train_step(model, opt, forward_loss)
            true, score, loss = kept[-1]
            meter.update(true, score, loss, lr=0.01, params=7)
        out = meter.compute()
        assert list(out) == ["loss", "accuracy", "precision", "recall", "f1", "auc"]
        true = torch.cat([k[0] for k in kept]).cpu().numpy()
        score = torch.cat([k[1] for k in kept]).cpu().numpy()
        ref = R.binary_metrics(true, score)
        for k, v in ref.items():
            assert out[k] == round(v, 4) and meter.raw()[k] == v, k
        sizes = [k[0].numel() for k in kept]
        mean_loss = sum(float(k[2].double()) * s for k, s in zip(kept, sizes)) / sum(sizes)
        assert abs(meter.raw()["loss"] - mean_loss) <= 1e-12 * abs(mean_loss) and meter.lr == 0.01 and meter.params == 7
        # evaluation: the raw logits of the validation batch through eval_epoch
        val = metrics.Meter("classification_binary")
        vb = link_batch(splits["val"], x, ratio=1.0, seed=1, offset=9)
        H.eval_epoch(model, [vb], val)
        assert not model.training
        with torch.no_grad():
            pred, true = model(link_batch(splits["val"], x, ratio=1.0, seed=1, offset=9))
        ref = R.binary_metrics(true.cpu().numpy(), torch.sigmoid(pred).cpu().numpy())
        got = val.raw()
        assert got["accuracy"] == ref["accuracy"] and abs(got["auc"] - ref["auc"]) < 0.02 and 0.0 <= got["auc"] <= 1.0
    finally:
        for k, v in old.items():
            setattr(cfg.gnn, k, v)
        cfg.dataset.task = old_task
        if old_dec is None:
            if hasattr(cfg.model, "edge_decoding"):
                delattr(cfg.model, "edge_decoding")
        else:
            cfg.model.edge_decoding = old_dec
