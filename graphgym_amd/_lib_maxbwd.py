"""ctypes prototypes of include/mp_maxbwd.h (csrc/spmm.hip: the max backward as a gather over the transposed pattern, what
ops.deterministic() selects), read from the header itself (graphgym_amd/_abi.py) and applied once onto the handle
`_lib.lib()` returns.  A table of its own beside `_lib.PROTOTYPES`, as the header is a file of its own beside
mp_engine.h (see the header for why)."""
from . import _abi, _lib

_H = _abi.header("mp_maxbwd.h")
PROTOTYPES_MAXBWD = dict(_H.prototypes)   # name -> (restype, argtypes)

_bound = False


def lib():
    """`_lib.lib()` with the prototypes above applied (once)"""
    global _bound
    h = _lib.lib()
    if not _bound:
        for name, (res, args) in PROTOTYPES_MAXBWD.items():
            fn = getattr(h, name)  # AttributeError if the export is missing
            fn.restype = res
            fn.argtypes = args
        _bound = True
    return h
