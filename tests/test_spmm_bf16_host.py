"""Argument validation of the bf16 aggregation entry points and their bindings, without a device (CPU suite).
Every case returns before anything is launched or dereferenced on the device."""
import ctypes as C

from graphgym_amd import _lib

INVALID, UNSUPPORTED = 1, 2
BIG_N = 2 ** 31
FAKE = C.c_void_p(256)        # a non-null pointer that is never dereferenced


def _counts():
    return (C.c_int32 * 8)(4, 0, 0, 1, 1, 320, 1024, 256)


def _spmm(N=10, d=8, X=FAKE, Y=FAKE, rowptr=FAKE, plan=FAKE, reduce=0, ldx=None):
    lib = _lib.lib()
    ld = d if ldx is None else ldx
    return lib.mp_spmm_csr_bf16(rowptr, FAKE, None, N, plan, _counts(), X, ld, Y, max(d, 1), d, reduce,
                                None, 0, 0.0, None, 0, None, None, 0, None)


def _idgnn(N=10, d=8, X=FAKE, P=FAKE, Q=FAKE):
    return _lib.lib().mp_idgnn_agg_bf16(FAKE, FAKE, None, N, FAKE, _counts(), X, max(d, 1), P, max(d, 1), Q,
                                        max(d, 1), d, None, 0, None)


def _max_bwd(N=10, d=8, col=FAKE, argmax=FAKE, dY=FAKE, dX=FAKE):
    return _lib.lib().mp_spmm_max_bwd_bf16(col, None, argmax, dY, max(d, 1), N, d, dX, max(d, 1), None)


def test_prototypes_exist():
    for name in ("mp_spmm_csr_bf16", "mp_idgnn_agg_bf16", "mp_spmm_max_bwd_bf16"):
        assert name in _lib.PROTOTYPES
        assert hasattr(_lib.lib(), name)
    # the bf16 forms take the fp32 forms' arguments, pointer for pointer
    assert _lib.PROTOTYPES["mp_spmm_csr_bf16"] == _lib.PROTOTYPES["mp_spmm_csr_f32"]
    assert _lib.PROTOTYPES["mp_idgnn_agg_bf16"] == _lib.PROTOTYPES["mp_idgnn_agg_f32"]
    assert _lib.PROTOTYPES["mp_spmm_max_bwd_bf16"] == _lib.PROTOTYPES["mp_spmm_max_bwd_f32"]


def test_spmm_null_pointers_and_widths():
    assert _spmm(X=None) == INVALID
    assert _spmm(Y=None) == INVALID
    assert _spmm(rowptr=None) == INVALID
    assert _spmm(plan=None) == INVALID
    assert _spmm(d=0) == INVALID
    assert _spmm(d=-3) == INVALID
    assert _spmm(d=8, ldx=4) == INVALID                   # ldx < d
    assert _spmm(reduce=3) == INVALID
    assert _spmm(N=-1) == INVALID
    assert _spmm(N=BIG_N) == UNSUPPORTED
    assert _spmm(N=0) == 0                                # nothing to do: no launch


def test_idgnn_null_pointers_and_widths():
    assert _idgnn(X=None) == INVALID
    assert _idgnn(P=None) == INVALID
    assert _idgnn(Q=None) == INVALID
    assert _idgnn(d=0) == INVALID
    assert _idgnn(N=BIG_N) == UNSUPPORTED


def test_max_bwd_null_pointers_and_widths():
    assert _max_bwd(col=None) == INVALID
    assert _max_bwd(argmax=None) == INVALID
    assert _max_bwd(dY=None) == INVALID
    assert _max_bwd(dX=None) == INVALID
    assert _max_bwd(d=0) == INVALID
    assert _max_bwd(N=BIG_N) == UNSUPPORTED
    assert _max_bwd(N=0) == 0
