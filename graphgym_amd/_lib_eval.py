"""ctypes prototypes and constants of include/mp_eval.h (csrc/evalmetrics.hip: losses and epoch metrics), read from the
header itself (graphgym_amd/_abi.py) and applied once onto the handle `_lib.lib()` returns.  A table of its own beside
`_lib.PROTOTYPES`, as the header is a file of its own beside mp_engine.h (see the header for why)."""
from . import _abi, _lib

_H = _abi.header("mp_eval.h")
K = _H.constants
PROTOTYPES_EVAL = dict(_H.prototypes)   # name -> (restype, argtypes)

# enum mp_eval_word
COUNT, HITS, INVALID, TP, FP, TN, FN, NAN, TWO_U, P, N, SIZE, LOSS, ABS, SQ = (
    K["MP_EVAL_" + w] for w in "COUNT HITS INVALID TP FP TN FN NAN TWO_U P N SIZE LOSS ABS SQ".split())
STATE_WORDS = K["MP_EVAL_STATE_WORDS"]
BCE, MSE = K["MP_EVAL_BCE"], K["MP_EVAL_MSE"]
MAX_C = 1024            # above it the multi-class entries return MP_ERR_UNSUPPORTED

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
