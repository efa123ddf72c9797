"""The pair decoders, host side (no device): the closure of include/mp_pair.h over the library's exports, the binding and
the poisoning cases (mirroring tests/test_spline_host.py), the argument checks of every entry before anything is
launched, the fakes' shapes, GNNEdgeHead on CPU tensors against the reference's three lines bit for bit, the route rule,
and the refusals of the wrappers."""
import ctypes as C
import os
import re

import pytest
import torch
import torch.nn.functional as F

import _pair_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mp_pair.h")
INVALID, UNSUPPORTED = 1, 2
FAKE = C.c_void_p(256)        # a non-null pointer that is never dereferenced
ENTRIES = ["mp_pair_bwd_weights_f32", "mp_pair_rnorm_f32", "mp_pair_score_f32", "mp_pair_sum_f32"]


# ---- the header's closure -----------------------------------------------------------------------------------------------

def declared_symbols(path=HEADER):
    text = re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(mp_pair_[a-z0-9_]+)\s*\(", text)))


def test_every_declared_symbol_is_exported_and_bound_and_the_reverse():
    from graphgym_amd import _lib, _lib_pair
    from graphgym_amd import build as mpbuild
    lib = _lib_pair.lib()
    names = declared_symbols()
    assert names == ENTRIES
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mp_pair.h but not exported"
        assert n in _lib_pair.PROTOTYPES_PAIR, f"{n} has no ctypes prototype"
    for n in _lib_pair.PROTOTYPES_PAIR:
        assert n.startswith("mp_pair_") and n in names, f"ctypes binds {n} which mp_pair.h does not declare"
        assert getattr(lib, n).argtypes == _lib_pair.PROTOTYPES_PAIR[n][1]
    # mp_engine.h has one older entry of this prefix, the negative sampler's pair-space count; none of this header's
    assert declared_symbols(os.path.join(ROOT, "include", "mp_engine.h")) == ["mp_pair_space_rows"]
    assert [n for n in _lib.PROTOTYPES if n.startswith("mp_pair_")] == ["mp_pair_space_rows"]
    assert HEADER in mpbuild.HEADERS and "pair.hip" in mpbuild.SOURCES
    assert "pair.hip" not in mpbuild.EXTRA_FLAGS


def test_every_entry_has_a_poisoning_case():
    """mirrors tests/test_poison_host.py::test_every_c_entry_has_a_case_or_a_reason for include/mp_pair.h"""
    import test_poison_pair_gpu as P
    from graphgym_amd import _lib_pair
    covered = set()
    for case in P.CASES:
        assert case.entries and case.exact and callable(case.run), case.name
        covered |= set(case.entries)
    every = set(declared_symbols())
    assert every == set(_lib_pair.PROTOTYPES_PAIR)
    assert covered == every, f"cases {sorted(covered)} against entries {sorted(every)}"


# ---- the C entries, before anything is launched -------------------------------------------------------------------------

def _lib():
    from graphgym_amd import _lib_pair
    return _lib_pair.lib()


def _rnorm(h=FAKE, ldh=8, N=10, d=8, eps=1e-8, r=FAKE, q=None):
    return _lib().mp_pair_rnorm_f32(h, ldh, N, d, eps, r, q, None)


def _score(h=FAKE, ldh=8, N=10, d=8, a=FAKE, b=FAKE, K=5, r=None, score=FAKE, bad=FAKE):
    return _lib().mp_pair_score_f32(h, ldh, N, d, a, b, K, r, score, bad, None)


def _sum(U=FAKE, ldu=8, V=FAKE, ldv=8, N=10, m=8, a=FAKE, b=FAKE, K=5, bias=None, z=FAKE, ldz=8, bad=FAKE):
    return _lib().mp_pair_sum_f32(U, ldu, V, ldv, N, m, a, b, K, bias, z, ldz, bad, None)


def _bwd(rowptr=FAKE, eid=FAKE, N=10, K=5, g=FAKE, score=None, r=None, q=None, a=FAKE, b=FAKE, w=FAKE, diag=None):
    return _lib().mp_pair_bwd_weights_f32(rowptr, eid, N, K, g, score, r, q, a, b, w, diag, None)


def test_rnorm_checks_its_arguments_before_any_launch():
    assert _rnorm(h=None) == INVALID and _rnorm(r=None) == INVALID
    assert _rnorm(N=-1) == INVALID and _rnorm(d=0) == INVALID and _rnorm(d=-3) == INVALID
    assert _rnorm(ldh=7) == INVALID
    assert _rnorm(eps=0.0) == INVALID and _rnorm(eps=-1.0) == INVALID
    assert _rnorm(N=2 ** 31) == UNSUPPORTED and _rnorm(d=2 ** 30, ldh=2 ** 30) == UNSUPPORTED
    assert _rnorm(N=0, h=None, r=None) == 0 and _rnorm(N=0, h=None, r=None, q=None) == 0


def test_score_checks_its_arguments_before_any_launch():
    for missing in ("h", "a", "b", "score", "bad"):
        assert _score(**{missing: None}) == INVALID, missing
    assert _score(N=-1) == INVALID and _score(K=-1) == INVALID and _score(d=0) == INVALID
    assert _score(ldh=7) == INVALID
    assert _score(N=2 ** 31) == UNSUPPORTED and _score(K=2 ** 30) == UNSUPPORTED
    assert _score(d=2 ** 30, ldh=2 ** 30) == UNSUPPORTED
    assert _score(K=0, h=None, a=None, b=None, score=None, bad=None) == 0


def test_sum_checks_its_arguments_before_any_launch():
    for missing in ("U", "V", "a", "b", "z", "bad"):
        assert _sum(**{missing: None}) == INVALID, missing
    assert _sum(N=-1) == INVALID and _sum(K=-1) == INVALID and _sum(m=0) == INVALID
    assert _sum(ldu=7) == INVALID and _sum(ldv=7) == INVALID and _sum(ldz=7) == INVALID
    assert _sum(N=2 ** 31) == UNSUPPORTED and _sum(K=2 ** 30) == UNSUPPORTED
    assert _sum(m=2 ** 30, ldu=2 ** 30, ldv=2 ** 30, ldz=2 ** 30) == UNSUPPORTED
    assert _sum(K=0, U=None, V=None, a=None, b=None, z=None, bad=None) == 0


def test_bwd_weights_checks_its_arguments_before_any_launch():
    for missing in ("rowptr", "eid", "g", "w"):
        assert _bwd(**{missing: None}) == INVALID, missing
    assert _bwd(N=-1) == INVALID and _bwd(K=-1) == INVALID
    # cosine: the pair ids with r; score, r and q with the diagonal
    assert _bwd(r=FAKE, a=None) == INVALID and _bwd(r=FAKE, b=None) == INVALID
    assert _bwd(diag=FAKE) == INVALID and _bwd(diag=FAKE, r=FAKE, q=FAKE) == INVALID
    assert _bwd(diag=FAKE, score=FAKE, q=FAKE) == INVALID and _bwd(diag=FAKE, score=FAKE, r=FAKE) == INVALID
    assert _bwd(N=2 ** 31) == UNSUPPORTED and _bwd(K=2 ** 30) == UNSUPPORTED
    assert _bwd(K=0, rowptr=None, eid=None, g=None, w=None, a=None, b=None) == 0


# ---- the operators --------------------------------------------------------------------------------------------------------

def test_fake_kernels_give_the_shapes():
    from graphgym_amd import ops  # noqa: F401
    h = torch.empty(5, 8, device="meta")
    idx = torch.empty(2, 7, dtype=torch.int64, device="meta")
    for cosine in (False, True):
        s = torch.ops.mp.pair_score(h, idx, cosine, 1e-8)
        assert s.shape == (7,) and s.dtype == torch.float32
    assert torch.ops.mp.pair_sum(h, h, idx, None).shape == (7, 8)
    assert torch.ops.mp.pair_sum(h, h, idx, torch.empty(8, device="meta")).shape == (7, 8)
    assert torch.ops.mp.pair_score_bwd_raw(torch.empty(7, device="meta"), h, idx, None, False, 1e-8).shape == (5, 8)
    dz = torch.empty(7, 8, device="meta")
    assert [tuple(t.shape) for t in torch.ops.mp.pair_sum_bwd_raw(dz, idx, 5, 3)] == [(5, 8), (5, 8)]
    assert [tuple(t.shape) for t in torch.ops.mp.pair_sum_bwd_raw(dz, idx, 5, 2)] == [(0,), (5, 8)]
    assert torch.ops.mp.pair_score(h, torch.empty(2, 0, dtype=torch.int64, device="meta"), False, 1e-8).shape == (0,)


def test_wrappers_refuse_other_dtypes_misshaped_indices_and_the_cpu():
    from graphgym_amd import ops
    from graphgym_amd._lib import EngineError
    idx = torch.zeros(2, 3, dtype=torch.int64)
    for dt in (torch.bfloat16, torch.float16, torch.float64):
        with pytest.raises(TypeError, match="float32 only"):
            ops.pair_score(torch.zeros(4, 4, dtype=dt), idx)
        with pytest.raises(TypeError, match="float32 only"):
            ops.pair_sum(torch.zeros(4, 4, dtype=dt), torch.zeros(4, 4), idx)
        with pytest.raises(TypeError, match="float32 only"):
            ops.pair_sum(torch.zeros(4, 4), torch.zeros(4, 4, dtype=dt), idx)
    for bad in (torch.zeros(3, 2, dtype=torch.int64), torch.zeros(6, dtype=torch.int64),
                torch.zeros(2, 3, dtype=torch.int32), torch.zeros(2, 6, dtype=torch.int64)[:, ::2]):
        with pytest.raises(ValueError, match="index"):
            ops.pair_score(torch.zeros(4, 4), bad)
        with pytest.raises(ValueError, match="index"):
            ops.pair_index(bad, 4)
    with pytest.raises(ValueError, match="eps"):
        ops.pair_score(torch.zeros(4, 4), idx, cosine=True, eps=0.0)
    with pytest.raises(EngineError, match="HIP device"):               # the engine has no CPU path
        ops.pair_score(torch.zeros(4, 4), idx)
    with pytest.raises(EngineError, match="HIP device"):
        ops.pair_sum(torch.zeros(4, 4), torch.zeros(4, 4), idx)


# ---- the head ---------------------------------------------------------------------------------------------------------------

def _head(decoding, d, dim_out, layers):
    import graphgym_amd.graphgym_plugin  # noqa: F401
    from graphgym_amd import harness as H
    from graphgym_amd.config import cfg
    old = (getattr(cfg.model, "edge_decoding", None), cfg.gnn.layers_post_mp)
    cfg.model.edge_decoding, cfg.gnn.layers_post_mp = decoding, layers
    try:
        torch.manual_seed(2)
        return H.GNNEdgeHead(d, dim_out)
    finally:
        cfg.gnn.layers_post_mp = old[1]
        if old[0] is None:
            delattr(cfg.model, "edge_decoding")
        else:
            cfg.model.edge_decoding = old[0]


@pytest.mark.parametrize("decoding", ["concat", "dot", "cosine_similarity"])
def test_head_on_cpu_tensors_is_the_reference_composition(decoding, monkeypatch):
    """CPU tensors never take the engine route, whatever the threshold: the three lines of head.py, bit for bit"""
    from graphgym_amd import harness as H
    monkeypatch.setattr(H, "PAIR_DECODE_MIN", 1)
    d, K = 16, 40
    head = _head(decoding, d, 3 if decoding == "concat" else 1, 1)
    h = R.features(d)
    idx = R.pairs(K)
    pred, label = head(H.Batch(node_feature=h.clone(), edge_label_index=idx, edge_label=torch.ones(K)))
    lin = head.layer_post_mp.model[0].model
    if decoding == "concat":
        want = F.linear(torch.cat((h[idx[0]], h[idx[1]]), -1), lin.weight, lin.bias)
    else:
        z = F.linear(h, lin.weight, lin.bias)
        want = R.score(z, idx, decoding != "dot")
    assert torch.equal(pred, want) and torch.equal(label, torch.ones(K))


def test_route_rule(monkeypatch):
    from graphgym_amd import harness as H
    f32, route = torch.float32, H.pair_decode_route
    monkeypatch.delenv("MP_PAIR_DECODE", raising=False)
    T = H.PAIR_DECODE_MIN
    assert isinstance(T, int) and T & (T - 1) == 0, "a power of two"
    assert T > H.PAIR_DECODE_FLOOR, "the tests that ran a GNNEdgeHead before the route existed keep the composition"
    assert route(True, f32, T // 64, 64) and route(True, f32, T // 256, 256)
    assert not route(True, f32, T // 64 - 1, 64) and not route(True, f32, 1, T - 1)
    assert not route(False, f32, T, 64), "CPU tensors"
    for dt in (torch.bfloat16, torch.float16, torch.float64):
        assert not route(True, dt, T, 64), dt
    monkeypatch.setenv("MP_PAIR_DECODE", "0")
    assert not route(True, f32, T, 64)
    monkeypatch.setenv("MP_PAIR_DECODE", "1")
    assert route(True, f32, T, 64)
    monkeypatch.setattr(H, "PAIR_DECODE_MIN", None)
    assert not route(True, f32, 1 << 40, 64)
    monkeypatch.setattr(H, "PAIR_DECODE_MIN", 1)
    assert route(True, f32, 1, 1) and not route(True, f32, 0, 64)
    # the concat decoding crosses later by a measured factor
    monkeypatch.undo()
    monkeypatch.delenv("MP_PAIR_DECODE", raising=False)
    C = H.PAIR_DECODE_CONCAT
    assert isinstance(C, int) and C >= 1 and C & (C - 1) == 0
    assert route(True, f32, T * C // 64, 64, concat=True) and not route(True, f32, T * C // 64 - 1, 64, concat=True)
    assert route(True, f32, T * C // 64 - 1, 64) or C == 1
