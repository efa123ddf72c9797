"""The zero-extent rule of the C ABI without a device: an entry point that receives an extent as an
argument takes NULL for the arrays of that extent when it is zero and returns MP_OK before any launch — the extent test
comes before the pointer test — while a NULL array at a non-zero extent is still refused with status 1.

Only calls that return before any launch or runtime call stand here (each entry point was read for it): the weight-gradient
entries at M = 0, which clear dW with a memset, are covered on the device (tests/test_degenerate_gpu.py: test_dense)."""
import ctypes as C

import pytest

from graphgym_amd import _lib

OK, INVALID = 0, 1
p = C.c_void_p(16)      # a live array: never dereferenced, every call below returns before any launch


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


@pytest.fixture(scope="module")
def counts():
    return (C.c_int32 * 8)(1, 0, 0, 1, 1, 320, 1024, 256)


def _spmm(L, counts, name, N, X, Y):
    if name == "mp_spmm_csr_epilogue_f32":
        return L.mp_spmm_csr_epilogue_f32(p, None, None, N, p, counts, X, 4, Y, 4, 4, 0, None, 0, 0.0, None, None, 0, 0,
                                          1e-12, None, 0, None)
    return getattr(L, name)(p, None, None, N, p, counts, X, 4, Y, 4, 4, 0, None, 0, 0.0, None, 0, None, None, 0, None)


@pytest.mark.parametrize("name", ["mp_spmm_csr_f32", "mp_spmm_csr_bf16", "mp_spmm_csr_epilogue_f32"])
def test_aggregation_of_an_operator_without_rows(L, counts, name):
    """N = 0: Y (and X of a square operator) have no address; rowptr, the plan and its counts still exist"""
    assert _spmm(L, counts, name, 0, None, None) == OK
    assert _spmm(L, counts, name, 0, p, None) == OK            # a rectangular operator: columns but no rows
    # unchanged: a NULL array of a non-zero extent, a missing structure at any extent
    assert _spmm(L, counts, name, 5, None, p) == INVALID
    assert _spmm(L, counts, name, 5, p, None) == INVALID
    assert getattr(L, "mp_spmm_csr_f32")(None, None, None, 0, p, counts, None, 4, None, 4, 4, 0, None, 0, 0.0, None, 0,
                                         None, None, 0, None) == INVALID
    assert getattr(L, "mp_spmm_csr_f32")(p, None, None, 0, None, counts, None, 4, None, 4, 4, 0, None, 0, 0.0, None, 0,
                                         None, None, 0, None) == INVALID
    assert _spmm(L, counts, name, -1, p, p) == INVALID


@pytest.mark.parametrize("name", ["mp_idgnn_agg_f32", "mp_idgnn_agg_bf16"])
def test_two_branch_aggregation_of_an_operator_without_rows(L, counts, name):
    f = getattr(L, name)
    call = lambda N, X, P, Q: f(p, None, None, N, p, counts, X, 4, P, 4, Q, 4, 4, None, 0, None)      # noqa: E731
    assert call(0, None, None, None) == OK
    assert call(5, p, p, None) == INVALID                          # unchanged: the second branch's output at N > 0
    assert call(5, None, p, p) == INVALID and call(5, p, None, p) == INVALID


def test_heads_max_da_without_entries(L):
    """nnz = 0: every per-entry array, and argmax / dY / V of an operator without rows, may be NULL"""
    f = L.mp_spmm_heads_max_da_f32
    assert f(None, None, 0, None, 8, None, 8, None, 8, 8, 4, None, None) == OK
    assert f(None, None, 0, p, 8, p, 8, p, 8, 8, 4, p, None) == OK
    # unchanged: NULL arrays at nnz > 0, bad head layouts and leading dimensions at any extent
    assert f(None, None, 10, None, 8, None, 8, None, 8, 8, 4, None, None) == INVALID
    for k in range(6):
        args = [p, p, 10, p, 8, p, 8, p, 8, 8, 4, p, None]
        args[(0, 1, 3, 5, 7, 11)[k]] = None
        assert f(*args) == INVALID, k
    assert f(None, None, 0, None, 8, None, 8, None, 8, 8, 3, None, None) == INVALID      # d % heads
    assert f(None, None, 0, None, 4, None, 8, None, 8, 8, 4, None, None) == INVALID      # ldm < d
    assert f(None, None, -1, None, 8, None, 8, None, 8, 8, 4, None, None) == INVALID


def test_edge_backward_without_entries_or_rows(L):
    """mp_spmm_edge_bwd_f32 gets both N and nnz: eid at nnz = 0, dY and argmax at N = 0 may be NULL (dM is pre-zeroed by
    the caller and untouched)"""
    f = L.mp_spmm_edge_bwd_f32          # (rowptr, eid, val, argmax, N, nnz, reduce, dY, ldy, d, dM, ldm, stream)
    assert f(p, None, None, None, 5, 0, 0, p, 8, 8, p, 8, None) == OK
    assert f(p, None, None, None, 5, 0, 2, p, 8, 8, None, 8, None) == OK          # max: no entry, no winner to read
    assert f(p, None, None, None, 0, 0, 2, None, 8, 8, None, 8, None) == OK
    # unchanged: NULL arrays at non-zero extents, the structure and the ranges at any extent
    for k in (1, 7, 10):
        args = [p, p, None, None, 5, 10, 0, p, 8, 8, p, 8, None]
        args[k] = None
        assert f(*args) == INVALID, k
    assert f(p, p, None, None, 5, 10, 2, p, 8, 8, p, 8, None) == INVALID          # max needs the argmax
    assert f(None, None, None, None, 5, 0, 0, p, 8, 8, p, 8, None) == INVALID     # rowptr
    assert f(p, None, None, None, 5, 0, 3, p, 8, 8, p, 8, None) == INVALID        # reduce out of range
    assert f(p, None, None, None, 5, 0, 0, p, 7, 8, p, 8, None) == INVALID        # ldy < d


def test_dense_fused_of_no_rows(L):
    """M = 0: P, Q and out have no address; the weights still exist"""
    f = L.mp_dense_fused_f32
    assert f(None, 12, p, None, 0, None, None, 0, None, 8, 0, 12, 8, None) == OK
    assert f(None, 12, p, None, 12, p, p, 1, None, 8, 0, 12, 8, None) == OK         # second branch: Q [0, F] is NULL too
    assert f(None, 12, None, None, 0, None, None, 0, None, 8, 0, 12, 8, None) == INVALID     # W has F rows at any M
    # unchanged at M > 0
    assert f(None, 12, p, None, 0, None, None, 0, p, 8, 10, 12, 8, None) == INVALID
    assert f(p, 12, p, None, 0, None, None, 0, None, 8, 10, 12, 8, None) == INVALID
    assert f(p, 12, p, p, 12, None, None, 0, p, 8, 10, 12, 8, None) == INVALID       # Q without W_id
    assert f(p, 12, p, None, 0, p, None, 0, p, 8, 10, 12, 8, None) == INVALID        # W_id without Q
    assert f(p, 11, p, None, 0, None, None, 0, p, 8, 10, 12, 8, None) == INVALID     # ldp < F
    assert f(None, 12, p, None, 0, None, None, 7, None, 8, 0, 12, 8, None) == INVALID    # a bad activation at any M


def test_entry_points_that_already_followed_the_rule(L):
    """the models of the rule (mp_rows_gather_f32, mp_sddmm_dot_f32, mp_gat_alpha_f32): NULL at extent 0, refused at
    a non-zero extent"""
    assert L.mp_rows_gather_f32(None, 4, None, 0, 4, None, 4, None) == OK
    assert L.mp_rows_gather_f32(None, 4, p, 3, 4, p, 4, None) == INVALID
    assert L.mp_sddmm_dot_f32(p, None, 5, 0, None, 4, None, 4, 4, 1, 1.0, None, None) == OK
    assert L.mp_sddmm_dot_f32(p, None, 5, 3, p, 4, p, 4, 4, 1, 1.0, p, None) == INVALID
    assert L.mp_gat_alpha_f32(p, None, 5, 0, 2, None, None, 0.2, None, None) == OK
    assert L.mp_gat_alpha_f32(p, None, 5, 3, 2, p, p, 0.2, p, None) == INVALID
