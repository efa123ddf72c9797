"""Loss and evaluation on the device (csrc/evalmetrics.hip, include/mp_eval.h).

    compute_loss(pred, true)        graphgym/loss.py:11-50, line for line: (loss, pred_score)
    Meter(task_type)                what Logger accumulates and write_epoch reports (graphgym/logger.py:85-113,123-139)
    torch.ops.mp.bce_logits / mse   the two element-wise losses, one forward pass (loss and score) and one backward pass

The reference copies `true` and `pred_score` to the host and calls `loss.item()` on every step (train.py:26-28,74-76),
then runs scikit-learn on the concatenation.  Here every update is a device pass into a 16-word state tensor and returns
nothing to the host; `Meter.compute()` is one copy of that tensor.  The AUC is exact: an integer pair count over the
sorted scores, not a trapezoid sum.
"""
import ctypes as C
import math
import warnings
from typing import Tuple

import torch
import torch.nn.functional as F
from torch import Tensor
from torch.library import custom_op, register_autograd

from . import _lib_eval as E
from . import nn as mpnn
from ._lib import check, ptr
from .config import cfg
from .graph import _require_hip, _stream

TASK_TYPES = ("classification_binary", "classification_multi", "regression")


def _ws(n, device):
    nb = C.c_size_t(0)
    check(E.lib().mp_eval_ws_bytes(n, C.byref(nb)), "mp_eval_ws_bytes")
    return torch.empty(nb.value, dtype=torch.uint8, device=device)


def _scale(n, size_average):
    """the factor on the summed terms: nn.BCEWithLogitsLoss / nn.MSELoss(reduction=cfg.model.size_average)"""
    if size_average == "mean":
        return 1.0 / n if n else float("nan")       # torch: the mean of no terms is NaN
    if size_average == "sum":
        return 1.0
    raise ValueError(f"{size_average} is not a valid value for reduction (the engine has 'mean' and 'sum')")


def _check_f32(pred, true):
    if pred.dtype != torch.float32 or true.dtype != torch.float32:
        raise TypeError(f"the engine's element-wise losses are fp32 only, got {pred.dtype} and {true.dtype}")
    if pred.shape != true.shape:
        raise ValueError(f"pred {tuple(pred.shape)} and true {tuple(true.shape)} must have one shape")


# ---- the two element-wise losses (loss.py:41-47) ----------------------------------------------------------------------
@custom_op("mp::eltwise_loss_fwd_raw", mutates_args=(), device_types="cuda")
def _op_loss_fwd_raw(pred: Tensor, true: Tensor, kind: int, scale: float) -> Tuple[Tensor, Tensor]:
    """one engine call: (fp32 scalar scale * sum of terms, score like pred)"""
    _require_hip(pred, "pred")
    _require_hip(true, "true")
    _check_f32(pred, true)
    z, y = pred.contiguous(), true.contiguous()
    n = z.numel()
    score = torch.empty(z.shape, dtype=torch.float32, device=z.device)
    loss = torch.empty((), dtype=torch.float32, device=z.device)
    ws = _ws(n, z.device)
    with torch.cuda.device(z.device):
        check(E.lib().mp_eval_loss_fwd_f32(kind, ptr(z), ptr(y), n, scale, ptr(score), ptr(loss), ptr(ws), ws.numel(),
                                           _stream()), "mp_eval_loss_fwd_f32")
    return loss, score


@_op_loss_fwd_raw.register_fake
def _(pred, true, kind, scale):
    return pred.new_empty((), dtype=torch.float32), pred.new_empty(pred.shape, dtype=torch.float32)


@custom_op("mp::eltwise_loss_bwd_raw", mutates_args=(), device_types="cuda")
def _op_loss_bwd_raw(pred: Tensor, true: Tensor, g: Tensor, kind: int, scale: float) -> Tensor:
    _require_hip(pred, "pred")
    _check_f32(pred, true)
    z, y = pred.contiguous(), true.contiguous()
    gs = g.to(torch.float32).reshape(1).contiguous()
    dz = torch.empty(z.shape, dtype=torch.float32, device=z.device)
    with torch.cuda.device(z.device):
        check(E.lib().mp_eval_loss_bwd_f32(kind, ptr(z), ptr(y), z.numel(), ptr(gs), scale, ptr(dz), _stream()),
              "mp_eval_loss_bwd_f32")
    return dz


@_op_loss_bwd_raw.register_fake
def _(pred, true, g, kind, scale):
    return pred.new_empty(pred.shape, dtype=torch.float32)


@custom_op("mp::bce_logits", mutates_args=(), device_types="cuda")
def _op_bce_logits(pred: Tensor, true: Tensor, size_average: str = "mean") -> Tuple[Tensor, Tensor]:
    """(nn.BCEWithLogitsLoss(reduction=size_average)(pred, true), torch.sigmoid(pred)) in one pass"""
    return torch.ops.mp.eltwise_loss_fwd_raw(pred, true, E.BCE, _scale(pred.numel(), size_average))


@custom_op("mp::mse", mutates_args=(), device_types="cuda")
def _op_mse(pred: Tensor, true: Tensor, size_average: str = "mean") -> Tuple[Tensor, Tensor]:
    """(nn.MSELoss(reduction=size_average)(pred, true), pred as the score) in one pass"""
    return torch.ops.mp.eltwise_loss_fwd_raw(pred, true, E.MSE, _scale(pred.numel(), size_average))


def _loss_fake(pred, true, size_average="mean"):
    return pred.new_empty((), dtype=torch.float32), pred.new_empty(pred.shape, dtype=torch.float32)


_op_bce_logits.register_fake(_loss_fake)
_op_mse.register_fake(_loss_fake)


def _loss_setup(ctx, inputs, output):
    pred, true = inputs[0], inputs[1]
    size_average = inputs[2] if len(inputs) > 2 else "mean"
    ctx.save_for_backward(pred, true)
    ctx.scale = _scale(pred.numel(), size_average)
    ctx.mark_non_differentiable(output[1])      # the score is a report (the reference detaches it), not a path for gradients


def _loss_backward(kind):
    def backward(ctx, g, _g_score):
        pred, true = ctx.saved_tensors
        dz = torch.ops.mp.eltwise_loss_bwd_raw(pred, true, g, kind, ctx.scale) if ctx.needs_input_grad[0] else None
        return dz, None, None                   # the target gets no gradient
    return backward


register_autograd("mp::bce_logits", _loss_backward(E.BCE), setup_context=_loss_setup)
register_autograd("mp::mse", _loss_backward(E.MSE), setup_context=_loss_setup)


def bce_logits(pred, true, size_average="mean"):
    _check_f32(pred, true)
    return torch.ops.mp.bce_logits(pred, true, size_average)


def mse(pred, true, size_average="mean"):
    _check_f32(pred, true)
    return torch.ops.mp.mse(pred, true, size_average)


def compute_loss(pred, true, loss_fun=None, size_average=None):
    """graphgym/loss.py:11-50 -> (loss, pred_score).  Device tensors take the engine's passes (the multi-class branch
    nn.softmax_cross_entropy, the binary and mse branches mp::bce_logits / mp::mse, which are fp32 only); CPU tensors take
    the reference's own torch formulas."""
    loss_fun = cfg.model.loss_fun if loss_fun is None else loss_fun
    size_average = getattr(cfg.model, "size_average", "mean") if size_average is None else size_average
    # default manipulation for pred and true; if multi task binary classification, treat as flatten binary
    pred = pred.squeeze(-1) if pred.ndim > 1 else pred
    true = true.squeeze(-1) if true.ndim > 1 else true
    if true.ndim > 1 and loss_fun == "cross_entropy":
        pred, true = torch.flatten(pred), torch.flatten(true)
    if loss_fun == "cross_entropy":
        if pred.ndim > 1:       # multiclass
            if pred.is_cuda:
                return mpnn.softmax_cross_entropy(pred, true), F.log_softmax(pred, dim=-1)
            score = F.log_softmax(pred, dim=-1)
            return F.nll_loss(score, true), score
        true = true.float()     # binary
        if pred.is_cuda:
            return bce_logits(pred, true, size_average)
        return F.binary_cross_entropy_with_logits(pred, true, reduction=size_average), torch.sigmoid(pred)
    if loss_fun == "mse":
        true = true.float()
        if pred.is_cuda:
            loss, _ = mse(pred, true, size_average)
            return loss, pred           # the reference hands pred itself back
        return F.mse_loss(pred, true, reduction=size_average), pred
    raise ValueError('Loss func {} not supported'.format(loss_fun))


# ---- epoch statistics -----------------------------------------------------------------------------------------------------
def _ratio(num, den):
    """scikit-learn's zero_division default: 0.0 (it also warns)"""
    return num / den if den else 0.0


def binary_stats(tp, fp, tn, fn, two_u, p, n):
    """the five statistics of Logger.classification_binary from integer counts, in float64, unrounded.  Integer division
    in Python is correctly rounded, so equal counts give equal bits."""
    count = tp + fp + tn + fn
    return {"accuracy": _ratio(tp + tn, count), "precision": _ratio(tp, tp + fp), "recall": _ratio(tp, tp + fn),
            "f1": _ratio(2 * tp, 2 * tp + fp + fn),
            "auc": two_u / (2 * p * n) if (p and n) else float("nan")}       # one class only: scikit-learn 1.7 gives NaN


class Meter:
    """An epoch's statistics on the device: Logger.update_stats / write_epoch without the host copies.

    update() and update_logits() enqueue device passes and synchronise nothing; they allocate nothing the size of the
    epoch, except that the binary task keeps one fp32 score and one int8 label per example on the device (the AUC needs
    them).  compute() is one device-to-host copy of the state (for the binary task the sort and the pair count run in
    front of it) and returns write_epoch's dictionary: 'loss' and the task's keys, rounded with cfg.round, then the
    custom statistics."""

    def __init__(self, task_type, thresh=None):
        if task_type not in TASK_TYPES:
            raise ValueError('Task has to be regression or classification')
        self.task_type = task_type
        self.thresh = float(getattr(cfg.model, "thresh", 0.5) if thresh is None else thresh)
        self.state = None
        self.reset()

    def reset(self):
        """start a new epoch"""
        if self.state is not None:
            self.state.zero_()
        self._iter = 0
        self._examples = 0
        self._lr = 0.0
        self._params = 0
        self._time_used = 0.0
        self._scores, self._labels = [], []
        self._custom_stats = {}

    # ---- updates ------------------------------------------------------------------------------------------------------
    def _state_on(self, device):
        if self.state is None:
            self.state = torch.zeros(E.STATE_WORDS, dtype=torch.int64, device=device)
        elif self.state.device != device:
            raise ValueError(f"the meter's state lives on {self.state.device}, the batch on {device}")
        return self.state

    @staticmethod
    def _loss_args(loss, device):
        """(device fp32 [1] or None, host float): loss as a 0-d device tensor stays on the device"""
        if isinstance(loss, torch.Tensor):
            return loss.detach().to(device=device, dtype=torch.float32).reshape(1), 0.0
        return None, float(loss)

    def update(self, true, pred, loss, lr=0.0, time_used=0.0, params=0, **custom):
        """Logger.update_stats (logger.py:123-139): `pred` is compute_loss's pred_score (binary: scores [n] or [n, 1];
        multi-class: [n, C]; regression: [n]), `loss` a 0-d device tensor or a float.  No host synchronisation."""
        assert true.shape[0] == pred.shape[0]
        _require_hip(pred, "pred")
        _require_hip(true, "true")
        if pred.dtype != torch.float32:
            raise TypeError(f"the meter takes fp32 scores, got {pred.dtype}")
        pred, true = pred.detach(), true.detach()
        st = self._state_on(pred.device)
        n = pred.shape[0]
        ldev, lhost = self._loss_args(loss, pred.device)
        L, s = E.lib(), _stream
        with torch.cuda.device(pred.device):
            if self.task_type == "classification_multi":
                self._multi_scores(pred, true, ldev, lhost, st)
            elif self.task_type == "classification_binary":
                if pred.dim() > 1 and pred.shape[1] != 1:
                    raise ValueError(f"binary scores must be [n] or [n, 1], got {tuple(pred.shape)}")
                score = pred.reshape(n).contiguous()
                true = true.reshape(n)
                # fp32 labels (link_pred.link_batch's edge_label) go to the kernel as they are
                lab_f = true.contiguous() if true.dtype == torch.float32 else None
                lab_i = self._int_labels(true) if lab_f is None else None
                keep_s = torch.empty(n, dtype=torch.float32, device=pred.device)
                keep_l = torch.empty(n, dtype=torch.int8, device=pred.device)
                check(L.mp_eval_binary_f32(ptr(score), ptr(lab_i), ptr(lab_f), n, self.thresh, ptr(ldev), lhost, ptr(keep_s),
                                           ptr(keep_l), ptr(st), s()), "mp_eval_binary_f32")
                self._scores.append(keep_s)
                self._labels.append(keep_l)
            else:
                p = pred.reshape(n).contiguous()
                t = true.reshape(n).to(torch.float32).contiguous()
                ws = _ws(n, pred.device)
                check(L.mp_eval_regression_f32(ptr(p), ptr(t), n, ptr(ldev), lhost, ptr(st), ptr(ws), ws.numel(), s()),
                      "mp_eval_regression_f32")
        self._after(n, lr, time_used, params, custom)

    @staticmethod
    def _int_labels(true):
        """int64 labels; a float label that is no integer becomes -1 and is counted as invalid on the device"""
        if not true.is_floating_point():
            return true.to(torch.int64).contiguous()
        lab = true.to(torch.int64)
        return torch.where(lab.to(true.dtype) == true, lab, torch.full_like(lab, -1)).contiguous()

    def _multi_scores(self, pred, true, ldev, lhost, st):
        if pred.dim() != 2:
            raise ValueError(f"multi-class scores must be [n, C], got {tuple(pred.shape)}")
        z = pred if pred.stride(1) == 1 else pred.contiguous()
        n, c = z.shape
        lab = self._int_labels(true.reshape(n))
        if c > E.MAX_C:
            self._multi_torch(z, lab, None, st, ldev, lhost)
            return
        check(E.lib().mp_eval_multi_scores_f32(ptr(z), z.stride(0), n, ptr(lab), c, ptr(ldev), lhost, ptr(st), _stream()),
              "mp_eval_multi_scores_f32")

    def _multi_torch(self, z, lab, index, st, ldev, lhost):
        """C > 1024: the same statistics with torch on the device (no synchronisation either)"""
        warnings.warn(f"Meter: {z.shape[1]} classes are more than the engine's {E.MAX_C}; this update runs on torch")
        n_rows, c = z.shape
        rows = torch.arange(lab.numel(), device=z.device) if index is None else index
        ok = (lab >= 0) & (lab < c) & (rows >= 0) & (rows < n_rows)
        sel = z[torch.where(ok, rows, torch.zeros_like(rows))]
        y = torch.where(ok, lab, torch.zeros_like(lab))
        best = sel.argmax(dim=1)               # torch, too, returns the first of several maxima
        st[E.COUNT] += ok.sum()
        st[E.HITS] += ((best == y) & ok).sum()
        st[E.INVALID] += (~ok).sum()
        st[E.SIZE] += lab.numel()
        sd = st.view(torch.float64)
        if ldev is None and lhost is None:
            rl = F.cross_entropy(sel, y, reduction="none").double()
            sd[E.LOSS] += torch.where(ok, rl, torch.zeros_like(rl)).sum()
        else:
            sd[E.LOSS] += (ldev[0].double() if ldev is not None else lhost) * lab.numel()

    @torch.no_grad()
    def update_logits(self, pred, true, index=None):
        """The evaluation shortcut (train.py:72-79 in one step): raw model outputs in, statistics AND loss accumulated.
        Multi-class: one pass over logits [n_rows, C] (rows `index` when given, labels `true` [n_sel]) that never stores
        log_softmax.  Binary and regression: compute_loss's single pass (loss and score), then update()."""
        _require_hip(pred, "pred")
        if self.task_type != "classification_multi":
            if index is not None:
                pred = pred[index]
            loss, score = compute_loss(pred, true, "cross_entropy" if self.task_type == "classification_binary" else "mse")
            self.update(true, score, loss)
            return
        if pred.dtype != torch.float32:
            raise TypeError(f"the meter takes fp32 logits, got {pred.dtype}")
        if pred.dim() != 2:
            raise ValueError(f"logits must be [n_rows, C], got {tuple(pred.shape)}")
        st = self._state_on(pred.device)
        z = pred.detach()
        z = z if z.stride(1) == 1 else z.contiguous()
        lab = self._int_labels(true.detach().reshape(-1))
        idx = None if index is None else index.to(torch.int64).contiguous()
        n_sel = lab.numel()
        mpnn._check_ce_shapes(z, lab, idx)
        with torch.cuda.device(z.device):
            if z.shape[1] > E.MAX_C:
                self._multi_torch(z, lab, idx, st, None, None)
            else:
                ws = _ws(n_sel, z.device)
                check(E.lib().mp_eval_multi_logits_f32(ptr(z), z.stride(0), z.shape[0], ptr(lab), ptr(idx), n_sel, z.shape[1],
                                                       ptr(st), ptr(ws), ws.numel(), _stream()), "mp_eval_multi_logits_f32")
        self._after(n_sel, 0.0, 0.0, self._params, {})

    def _after(self, n, lr, time_used, params, custom):
        self._iter += 1
        self._examples += n
        self._lr, self._params = lr, params
        self._time_used += time_used
        for key, val in custom.items():        # logger.py:135-139 (host numbers)
            self._custom_stats[key] = self._custom_stats.get(key, 0) + val * n

    # ---- the epoch's result ---------------------------------------------------------------------------------------------
    def _auc_pass(self):
        """sort the kept scores once with their labels, the exclusive prefix count of negatives, the pair-count kernel"""
        st = self.state
        score = self._scores[0] if len(self._scores) == 1 else torch.cat(self._scores)
        label = self._labels[0] if len(self._labels) == 1 else torch.cat(self._labels)
        self._scores, self._labels = [score], [label]
        n = score.numel()
        s_sorted, order = torch.sort(score)
        l_sorted = label[order]
        cn = torch.zeros(n + 1, dtype=torch.int64, device=score.device)
        torch.cumsum(l_sorted == 0, 0, dtype=torch.int64, out=cn[1:])
        st[E.NAN:E.N + 1].zero_()               # compute() may run more than once per epoch
        with torch.cuda.device(score.device):
            check(E.lib().mp_eval_auc_pairs(ptr(s_sorted), ptr(l_sorted), ptr(cn), n, ptr(st), _stream()),
                  "mp_eval_auc_pairs")

    def counts(self):
        """the state on the host (ONE device-to-host copy): {name: int} for the counters, floats for the three sums"""
        names = ("count", "hits", "invalid", "tp", "fp", "tn", "fn", "nan", "two_u", "p", "n", "size")
        if self.state is None:
            return {**{k: 0 for k in names}, "loss": 0.0, "abs": 0.0, "sq": 0.0}
        if self.task_type == "classification_binary" and self._scores:
            self._auc_pass()
        host = self.state.cpu()
        out = dict(zip(names, host[:len(names)].tolist()))
        out.update(zip(("loss", "abs", "sq"), host.view(torch.float64)[E.LOSS:E.SQ + 1].tolist()))
        return out

    def raw(self):
        """the task's statistics in float64 before rounding, 'loss' included"""
        c = self.counts()
        if c["nan"]:
            raise ValueError(f"Input contains NaN: {c['nan']} scores of the epoch are NaN")
        if c["invalid"]:
            raise ValueError(f"{c['invalid']} examples of the epoch have a label or a row index out of range")
        out = {"loss": c["loss"] / c["size"] if c["size"] else float("nan")}
        if self.task_type == "classification_binary":
            out.update(binary_stats(c["tp"], c["fp"], c["tn"], c["fn"], c["two_u"], c["p"], c["n"]))
        elif self.task_type == "classification_multi":
            out["accuracy"] = _ratio(c["hits"], c["count"])
        else:
            mse_ = c["sq"] / c["count"] if c["count"] else float("nan")
            out.update({"mae": c["abs"] / c["count"] if c["count"] else float("nan"), "mse": mse_,
                        "rmse": math.sqrt(mse_)})
        return out

    def compute(self):
        """write_epoch's dictionary (logger.py:144-164 without epoch / eta / lr / params / time_iter, which are the
        attributes of the same names here): 'loss', the task's keys, the custom statistics"""
        digits = getattr(cfg, "round", 4)
        out = {k: round(v, digits) for k, v in self.raw().items()}
        for key, val in self._custom_stats.items():
            out[key] = val / self._examples
        return out

    @property
    def lr(self):
        return self._lr

    @property
    def params(self):
        return self._params

    def time_iter(self):
        return self._time_used / self._iter
