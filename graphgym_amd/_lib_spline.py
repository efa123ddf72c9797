"""ctypes prototypes of include/mp_spline.h (csrc/spmm.hip: the one-gather, two-sum aggregation of the B-spline layer and
its adjoint), read from the header itself (graphgym_amd/_abi.py) and applied once onto the handle `_lib.lib()` returns.
A table of its own beside `_lib.PROTOTYPES`, as the header is a file of its own beside mp_engine.h (see the header for
why)."""
from . import _abi, _lib

_H = _abi.header("mp_spline.h")
PROTOTYPES_SPLINE = dict(_H.prototypes)   # name -> (restype, argtypes)

_bound = False


def lib():
    """`_lib.lib()` with the prototypes above applied (once)"""
    global _bound
    h = _lib.lib()
    if not _bound:
        for name, (res, args) in PROTOTYPES_SPLINE.items():
            fn = getattr(h, name)  # AttributeError if the export is missing
            fn.restype = res
            fn.argtypes = args
        _bound = True
    return h
