"""ctypes prototypes of include/mp_eval.h (csrc/evalmetrics.hip: losses and epoch metrics), a 1:1 transcription, applied
once onto the handle `_lib.lib()` returns.  A table of its own beside `_lib.PROTOTYPES`, as the header is a file of its
own beside mp_engine.h (see the header for why)."""
import ctypes as C

from . import _lib

_p, _i64, _i32, _f32, _f64, _sz = C.c_void_p, C.c_int64, C.c_int32, C.c_float, C.c_double, C.c_size_t
_psz = C.POINTER(C.c_size_t)

# enum mp_eval_word
COUNT, HITS, INVALID, TP, FP, TN, FN, NAN, TWO_U, P, N, SIZE, LOSS, ABS, SQ = range(15)
STATE_WORDS = 16
BCE, MSE = 0, 1
MAX_C = 1024            # above it the multi-class entries return MP_ERR_UNSUPPORTED

# name -> (restype, argtypes); order and types follow mp_eval.h
PROTOTYPES_EVAL = {
    "mp_eval_state_words": (C.c_int, []),
    "mp_eval_ws_bytes": (C.c_int, [_i64, _psz]),
    "mp_eval_loss_fwd_f32": (C.c_int, [C.c_int, _p, _p, _i64, _f32, _p, _p, _p, _sz, _p]),
    "mp_eval_loss_bwd_f32": (C.c_int, [C.c_int, _p, _p, _i64, _p, _f32, _p, _p]),
    "mp_eval_multi_logits_f32": (C.c_int, [_p, _i64, _i64, _p, _p, _i64, _i32, _p, _p, _sz, _p]),
    "mp_eval_multi_scores_f32": (C.c_int, [_p, _i64, _i64, _p, _i32, _p, _f64, _p, _p]),
    "mp_eval_binary_f32": (C.c_int, [_p, _p, _p, _i64, _f32, _p, _f64, _p, _p, _p, _p]),
    "mp_eval_regression_f32": (C.c_int, [_p, _p, _i64, _p, _f64, _p, _p, _sz, _p]),
    "mp_eval_auc_pairs": (C.c_int, [_p, _p, _p, _i64, _p, _p]),
}

_bound = False


def lib():
    """`_lib.lib()` with the prototypes above applied (once)"""
    global _bound
    h = _lib.lib()
    if not _bound:
        for name, (res, args) in PROTOTYPES_EVAL.items():
            fn = getattr(h, name)  # AttributeError if the export is missing
            fn.restype = res
            fn.argtypes = args
        _bound = True
    return h
