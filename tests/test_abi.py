"""The C-ABI shared library: loads, exports every symbol include/mp_engine.h declares,
and its host-only entry points behave; the header reader the ctypes binding is derived with (graphgym_amd/_abi.py)
against header texts written here and against the C compiler's view of the real headers.  No device work here (CPU
suite)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from graphgym_amd import _abi, _lib, _lib_eval
from graphgym_amd import build as mpbuild

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mp_engine.h")


def declared_symbols():
    text = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mp_[a-z0-9_]+)\s*\(", text)))


def test_library_is_built_in_tree():
    mpbuild.build()
    assert os.path.exists(_lib.LIB_PATH)
    assert os.path.dirname(_lib.LIB_PATH).startswith(ROOT)


def test_every_declared_symbol_is_exported_and_bound():
    lib = _lib.lib()
    names = declared_symbols()
    assert len(names) >= 25
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mp_engine.h but not exported"
        assert n in _lib.PROTOTYPES, f"{n} has no ctypes prototype"
    for n in _lib.PROTOTYPES:
        assert n in names, f"ctypes binds {n} which the header does not declare"


SMALL_HEADER = """
/* a comment that names mp_fake(int x); and runs
 * over two lines */
#ifndef MP_SMALL_H
#define MP_SMALL_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
typedef void* mp_stream_t; /* hipStream_t */
enum mp_one { MP_A = 0, MP_B = 1, MP_C = 0x10 };
enum mp_many {
  MP_D = 4, /* mp_fake2(int) */
  MP_E = 5  // mp_fake3(
};
#define MP_B 1
#define MP_F 7
int mp_three(const int32_t* rowptr, int64_t n,
             float const* x, double p,
             size_t* bytes_host, mp_stream_t stream);
int mp_none(void);
int mp_empty();
const char* mp_text(int status);
int mp_scalars(int a, int32_t b, int64_t c, uint64_t d, float e, double f, size_t g);
typedef void* (*mp_alloc_fn)(size_t bytes, int32_t tag, void* user);
typedef struct mp_pair { int64_t n; /* mp_fake4( */ const float* x; size_t bytes; } mp_pair_t;
#ifdef __cplusplus
}
#endif
#endif /* MP_SMALL_H */
"""


def test_reader_on_a_small_header():
    h = _abi.parse(SMALL_HEADER)
    p = C.c_void_p
    assert h.prototypes == {
        "mp_three": (C.c_int, [p, C.c_int64, p, C.c_double, p, p]),          # broken over three lines, const either side
        "mp_none": (C.c_int, []), "mp_empty": (C.c_int, []),
        "mp_text": (C.c_char_p, [C.c_int]),
        "mp_scalars": (C.c_int, [C.c_int, C.c_int32, C.c_int64, C.c_uint64, C.c_float, C.c_double, C.c_size_t])}
    # one-line and many-line enumerator lists, a #define that repeats an enumerator's value; no include guard
    assert h.constants == {"MP_A": 0, "MP_B": 1, "MP_C": 16, "MP_D": 4, "MP_E": 5, "MP_F": 7}
    assert h.structs["mp_pair_t"]._fields_ == [("n", C.c_int64), ("x", p), ("bytes", C.c_size_t)]
    fn = h.callbacks["mp_alloc_fn"]
    assert fn._restype_ is p and fn._argtypes_ == (C.c_size_t, C.c_int32, p)


@pytest.mark.parametrize("text, names", [
    ("int mp_bad(int64_t n, long ld);", ("mp_bad", "'ld'", "long")),                   # a type outside the map
    ("int mp_bad(int64_t n, unsigned int* flags);", ("mp_bad", "'flags'")),
    ("long mp_bad(int64_t n);", ("mp_bad", "return", "long")),
    ("typedef struct mp_s { int64_t n; short k; } mp_s_t;", ("mp_s_t", "'k'", "short")),
    ("int mp_bad(int64_t);", ("mp_bad",)),                                             # a parameter without a name
    ("enum mp_e { MP_X = 1 };\n#define MP_X 2", ("MP_X", "1", "2")),                   # one name, two values
    ("enum mp_e { MP_X, MP_Y };", ("MP_X",)),                                          # no explicit value
    ("#define MP_SCALE 1.5f", ("MP_SCALE",)),
    ("#define MP_TWICE(x) (2 * (x))", ("MP_TWICE",)),
    ("static inline int mp_f(void) { return 0; }", ("mp_f",)),                         # not a declaration
    ("typedef int mp_index_t;", ("mp_index_t",)),                                      # a typedef the map does not hold
])
def test_reader_refuses_what_it_does_not_know(text, names):
    with pytest.raises(_abi.HeaderError) as e:
        _abi.parse(text)
    for n in names:
        assert n in str(e.value), (n, str(e.value))


def test_missing_header_is_an_import_error():
    with pytest.raises(ImportError, match="no_such_header.h"):
        _abi.header("no_such_header.h")


def test_compiler_agrees_with_the_reader(tmp_path):
    """every parsed constant, and the size and field offsets of mp_ego_result_t, as a host C program that includes the
    two headers prints them: the one check of the reader against something other than itself"""
    include = os.path.dirname(HEADER)
    consts = {**_lib.K, **_lib_eval.K}
    fields = [f for f, _ in _lib.EgoResult._fields_]
    src = ['#include <stddef.h>', '#include <stdio.h>', '#include "mp_engine.h"', '#include "mp_eval.h"',
           'int main(void) {']
    src += [f'  printf("{n} %lld\\n", (long long)({n}));' for n in consts]
    src += ['  printf("sizeof %zu\\n", sizeof(mp_ego_result_t));']
    src += [f'  printf("{f} %zu\\n", offsetof(mp_ego_result_t, {f}));' for f in fields]
    src += ['  return 0;', '}', '']
    (tmp_path / "abi.c").write_text("\n".join(src))
    subprocess.run([mpbuild._hipcc(), "-x", "c", "-I", include, str(tmp_path / "abi.c"), "-o", str(tmp_path / "abi")],
                   check=True, capture_output=True)
    out = subprocess.run([str(tmp_path / "abi")], check=True, capture_output=True, text=True).stdout
    seen = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    expected = dict(consts, sizeof=C.sizeof(_lib.EgoResult), **{f: getattr(_lib.EgoResult, f).offset for f in fields})
    assert len(consts) >= 50 and len(fields) == 12
    assert seen == expected


def test_abi_numbers_are_pinned():
    """a renumbering in the header must fail here, not silently follow"""
    assert _lib.K["MP_OK"] == _lib.MP_OK == 0
    assert _lib.K["MP_ERR_UNSUPPORTED"] == _lib.MP_ERR_UNSUPPORTED == 2
    assert _lib.K["MP_ERR_HIP"] == _lib.MP_ERR_HIP == 4
    assert _lib.K["MP_ERR_ALIGNMENT"] == _lib.MP_ERR_ALIGNMENT == 5
    assert _lib.K["MP_MAX"] == _lib.MAX == 2
    assert _lib.K["MP_COO_RECT"] == _lib.COO_RECT == 8
    assert _lib.K["MP_ACT_SILU"] == 6
    assert _lib.K["MP_EGO_TAG_EID"] == 6
    assert _lib_eval.K["MP_EVAL_STATE_WORDS"] == _lib_eval.STATE_WORDS == 16


def test_version_and_status_strings():
    lib = _lib.lib()
    assert lib.mp_version() >= 100
    assert lib.mp_status_str(0) == b"ok"
    assert b"workspace" in lib.mp_status_str(3)
    with pytest.raises(_lib.EngineError):
        _lib.check(1, "x")


def test_argument_validation_without_device():
    lib = _lib.lib()
    nb = C.c_size_t(0)
    assert lib.mp_spmm_plan_bytes(-1, 0, None, C.byref(nb)) == 1
    assert lib.mp_spmm_plan_bytes(10, 2**31, None, C.byref(nb)) == 2          # int32 index limit
    assert lib.mp_spmm_plan_bytes(1000, 10000, None, C.byref(nb)) == 0 and nb.value > 0
    default_bytes = nb.value
    assert lib.mp_spmm_plan_bytes(1000, 10000, (C.c_int32 * 4)(32, 4, 1024, 256), C.byref(nb)) == 1   # seg_cost too small
    assert lib.mp_spmm_plan_bytes(1000, 10000, (C.c_int32 * 4)(64, 1, 64, 64), C.byref(nb)) == 0 and nb.value > default_bytes
    counts = (C.c_int32 * 8)(10, 0, 3, 1, 4, 320, 1024, 256)
    assert lib.mp_spmm_ws_bytes(counts, 256, 0, 0, C.byref(nb)) == 0
    assert nb.value >= 3 * 256 * 4
    assert lib.mp_spmm_ws_bytes(counts, 256, 2, 0, C.byref(nb)) == 0    # max: values + argmax
    assert nb.value >= 2 * 3 * 256 * 4
    # null pointers are rejected before any launch
    assert lib.mp_spmm_csr_f32(None, None, None, 5, None, counts, None, 4, None, 4, 4, 0, None, 0, 0.0,
                               None, 0, None, None, 0, None) == 1


def test_ba_generator_host():
    from graphgym_amd import graphgen
    u, v = graphgen.ba_undirected_pairs(2000, 5, seed=3)
    assert u.size == 5 * (2000 - 5) and (u > v).all() and v.min() >= 0 and u.max() == 1999
    u2, v2 = graphgen.ba_undirected_pairs(2000, 5, seed=3)
    assert (u == u2).all() and (v == v2).all()                          # deterministic
    deg = np.bincount(np.concatenate([u, v]), minlength=2000)
    assert deg[5:].min() >= 5                                            # every new node made m links
    assert deg.max() > 5 * np.median(deg)                                # heavy tail
    ei = graphgen.ba_edge_index(500, 3, seed=1)
    key = (ei[1] * 500 + ei[0]).numpy()
    assert np.unique(key).size == key.size                               # deduplicated
    rev = (ei[0] * 500 + ei[1]).numpy()
    assert set(key.tolist()) == set(rev.tolist())                        # symmetric


def test_ops_refuse_cpu_tensors():
    import torch
    import graphgym_amd as ga
    ei = torch.tensor([[0, 1], [1, 0]])
    with pytest.raises(ga.EngineError):
        ga.CSRGraph.from_edge_index(ei, 2)


def test_powerlaw_cluster_generator_host():
    """Holme-Kim growth: same degree budget as BA, but triangles (clustering) like networkx's generator"""
    import networkx as nx
    from graphgym_amd import graphgen
    u, v = graphgen.powerlaw_cluster_undirected_pairs(4000, 4, 0.5, seed=2)
    assert (u > v).all() and v.min() >= 0 and u.max() == 3999 and u.size <= 4 * (4000 - 4)
    pairs = set(zip(u.tolist(), v.tolist()))
    assert len(pairs) == u.size                                          # links of one node are distinct
    G = nx.Graph(); G.add_edges_from(pairs)
    ref = nx.powerlaw_cluster_graph(4000, 4, 0.5, seed=2)
    ba_u, ba_v = graphgen.ba_undirected_pairs(4000, 4, seed=2)
    B = nx.Graph(); B.add_edges_from(zip(ba_u.tolist(), ba_v.tolist()))
    c, cref, cba = nx.average_clustering(G), nx.average_clustering(ref), nx.average_clustering(B)
    assert cba < 0.05 < c and abs(c - cref) < 0.5 * cref                 # triangle closing is really there
    u2, v2 = graphgen.powerlaw_cluster_undirected_pairs(4000, 4, 0.5, seed=2)
    assert (u == u2).all() and (v == v2).all()
