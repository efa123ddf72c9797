"""NumPy restatement of the epoch statistics of graphgym/logger.py:85-113 (scikit-learn's accuracy / precision / recall /
f1 / roc_auc_score and the regression errors), as integer counts first and float64 ratios second.
tests/test_eval_host.py holds it to scikit-learn; tests/test_eval_gpu.py holds the engine to it."""
import math

import numpy as np


def _div(num, den):
    """scikit-learn's zero_division default"""
    return int(num) / int(den) if den else 0.0


def binary_counts(true, score, thresh=0.5):
    """(tp, fp, tn, fn, invalid): pred_int = score > thresh (logger.py:85-89); labels outside {0, 1} are invalid"""
    true = np.asarray(true).astype(np.int64)
    pred = np.asarray(score) > thresh
    pos, neg = true == 1, true == 0
    return (int((pos & pred).sum()), int((neg & pred).sum()), int((neg & ~pred).sum()), int((pos & ~pred).sum()),
            int((~pos & ~neg).sum()))


def auc_counts(true, score):
    """(2U, P, N, number of NaN scores) with 2U = sum over positives of 2 #(negatives below) + #(negatives equal), by the
    definition: the scores' distinct values, counted per class.  -0.0 and 0.0 are one value (np.unique compares with ==).
    Examples with a NaN score are counted and left out."""
    true = np.asarray(true).astype(np.int64)
    score = np.asarray(score, dtype=np.float32)
    nan = np.isnan(score)
    true, score = true[~nan], score[~nan] + np.float32(0.0)        # (-0.0 + 0.0 = 0.0: one tie group)
    values, inv = np.unique(score, return_inverse=True)
    negs = np.bincount(inv[true == 0], minlength=values.size).astype(np.int64)
    poss = np.bincount(inv[true == 1], minlength=values.size).astype(np.int64)
    below = np.cumsum(negs) - negs
    two_u = sum(int(p) * (2 * int(b) + int(e)) for p, b, e in zip(poss, below, negs) if p)
    return two_u, int(poss.sum()), int(negs.sum()), int(nan.sum())


def auc_from_counts(two_u, p, n):
    return two_u / (2 * p * n) if (p and n) else float("nan")


def binary_metrics(true, score, thresh=0.5):
    """Logger.classification_binary before rounding; raises on a NaN score as scikit-learn does"""
    tp, fp, tn, fn, invalid = binary_counts(true, score, thresh)
    two_u, p, n, nan = auc_counts(true, score)
    if nan:
        raise ValueError("Input contains NaN.")
    if invalid:
        raise ValueError(f"{invalid} labels are not in {{0, 1}}")
    return {"accuracy": _div(tp + tn, tp + fp + tn + fn), "precision": _div(tp, tp + fp), "recall": _div(tp, tp + fn),
            "f1": _div(2 * tp, 2 * tp + fp + fn), "auc": auc_from_counts(two_u, p, n)}


def first_argmax(scores):
    """best = 0; for c in 1 .. C: if z[c] > z[best]: best = c — the lowest index among the maxima"""
    return np.argmax(np.asarray(scores), axis=1)        # numpy's argmax returns the first occurrence


def multi_counts(true, scores):
    """(count, hits, invalid)"""
    true = np.asarray(true).astype(np.int64)
    scores = np.asarray(scores)
    ok = (true >= 0) & (true < scores.shape[1])
    best = first_argmax(scores)
    return int(ok.sum()), int((ok & (best == true)).sum()), int((~ok).sum())


def multi_metrics(true, scores):
    count, hits, invalid = multi_counts(true, scores)
    if invalid:
        raise ValueError(f"{invalid} labels are out of range")
    return {"accuracy": _div(hits, count)}


def regression_metrics(true, pred):
    d = np.asarray(pred, dtype=np.float64).reshape(-1) - np.asarray(true, dtype=np.float64).reshape(-1)
    mse = float(np.mean(d * d))
    return {"mae": float(np.mean(np.abs(d))), "mse": mse, "rmse": math.sqrt(mse)}
