"""ctypes prototypes of include/mp_pair.h (csrc/pair.hip: the pair decoders of the link-prediction head and the entry
weights of their gradient), read from the header itself (graphgym_amd/_abi.py) and applied once onto the handle
`_lib.lib()` returns.  A table of its own beside `_lib.PROTOTYPES`, as the header is a file of its own beside
mp_engine.h (see the header for why)."""
from . import _abi, _lib

_H = _abi.header("mp_pair.h")
PROTOTYPES_PAIR = dict(_H.prototypes)   # name -> (restype, argtypes)

_bound = False


def lib():
    """`_lib.lib()` with the prototypes above applied (once)"""
    global _bound
    h = _lib.lib()
    if not _bound:
        for name, (res, args) in PROTOTYPES_PAIR.items():
            fn = getattr(h, name)  # AttributeError if the export is missing
            fn.restype = res
            fn.argtypes = args
        _bound = True
    return h
