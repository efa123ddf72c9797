"""ctypes prototypes and constants of include/mp_structure.h (csrc/centrality.hip: PageRank, betweenness, one-hot ids),
read from the header itself (graphgym_amd/_abi.py) and applied once onto the handle `_lib.lib()` returns.  A table of its
own beside `_lib.PROTOTYPES`, as the header is a file of its own beside mp_engine.h (see the header for why)."""
from . import _abi, _lib

_H = _abi.header("mp_structure.h")
K = _H.constants
PROTOTYPES_STRUCTURE = dict(_H.prototypes)   # name -> (restype, argtypes)

# enum mp_struct_limit
PAGERANK_LDS_NODES, PAGERANK_CHUNK = K["MP_STRUCT_PAGERANK_LDS_NODES"], K["MP_STRUCT_PAGERANK_CHUNK"]
BETWEENNESS_SLICE, BETWEENNESS_LDS_NODES, BETWEENNESS_MAX_NODES = (
    K["MP_STRUCT_BETWEENNESS_" + w] for w in "SLICE LDS_NODES MAX_NODES".split())
ONEHOT_STREAM = K["MP_STRUCT_ONEHOT_STREAM"]

_bound = False


def lib():
    """`_lib.lib()` with the prototypes above applied (once)"""
    global _bound
    h = _lib.lib()
    if not _bound:
        for name, (res, args) in PROTOTYPES_STRUCTURE.items():
            fn = getattr(h, name)  # AttributeError if the export is missing
            fn.restype = res
            fn.argtypes = args
        _bound = True
    return h
