"""The deterministic switch of graphgym_amd.ops and the pull-form max backward, without a device: the switch's
semantics, the argument checks of the three new C entries, the fake kernels of the two new operators, and the NumPy
restatement the GPU tests compare against (tests/_detref.py) held to a float64 evaluation in another formulation."""
import ctypes as C

import numpy as np
import pytest
import torch

import _detref as D
from _tol import assert_close_rows


@pytest.fixture()
def switch():
    """the override and torch's flag as they were, whatever a test sets"""
    from graphgym_amd import ops
    saved = ops._DETERMINISTIC
    torch_on, torch_warn = torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled()
    yield ops
    ops._DETERMINISTIC = saved
    torch.use_deterministic_algorithms(torch_on, warn_only=torch_warn)


# ---- the switch -------------------------------------------------------------------------------------------------------
def test_none_follows_torch(switch):
    ops = switch
    ops.set_deterministic(None)
    torch.use_deterministic_algorithms(False)
    assert ops.deterministic() is False
    torch.use_deterministic_algorithms(True)
    assert ops.deterministic() is True
    torch.use_deterministic_algorithms(True, warn_only=True)          # warn_only makes no difference
    assert ops.deterministic() is True
    torch.use_deterministic_algorithms(False)
    assert ops.deterministic() is False


def test_override_wins(switch):
    ops = switch
    torch.use_deterministic_algorithms(True)
    ops.set_deterministic(False)
    assert ops.deterministic() is False
    torch.use_deterministic_algorithms(False)
    ops.set_deterministic(True)
    assert ops.deterministic() is True
    ops.set_deterministic(None)
    assert ops.deterministic() is False
    for bad in (1, 0, "1", "on"):
        with pytest.raises(TypeError):
            ops.set_deterministic(bad)
    assert ops.deterministic() is False


@pytest.mark.parametrize("env, want", [("1", True), ("0", False), ("", None), (None, None)])
def test_env_sets_the_initial_override(switch, monkeypatch, env, want):
    ops = switch
    if env is None:
        monkeypatch.delenv("MP_DETERMINISTIC", raising=False)
    else:
        monkeypatch.setenv("MP_DETERMINISTIC", env)
    assert ops._env_deterministic() is want
    monkeypatch.setenv("MP_DETERMINISTIC", "yes")
    with pytest.raises(ValueError, match="MP_DETERMINISTIC"):
        ops._env_deterministic()


# ---- the C entries ----------------------------------------------------------------------------------------------------
def _pull_args(**over):
    """valid-looking host arguments of mp_spmm_max_bwd_pull_*: the entries must refuse what is wrong with them before
    anything is launched, so the addresses are never read"""
    buf = (C.c_int32 * 64)()
    a = C.cast(buf, C.c_void_p)
    counts = (C.c_int32 * 8)(1, 0, 0, 1, 1, 320, 1024, 256)
    v = dict(t_rowptr=a, t_col=a, t_pos=a, t_val=None, n_src=4, nnz=8, plan=a, counts=counts, argmax=a, lda=4, dY=a,
             ldy=4, d=4, dX=a, ldx=4, ws=None, ws_bytes=0, stream=None)
    v.update(over)
    return v


ORDER = ("t_rowptr", "t_col", "t_pos", "t_val", "n_src", "nnz", "plan", "counts", "argmax", "lda", "dY", "ldy", "d",
         "dX", "ldx", "ws", "ws_bytes", "stream")


def _call(name, heads=None, **over):
    from graphgym_amd import _lib_maxbwd
    v = _pull_args(**over)
    args = [v[k] for k in ORDER]
    if heads is not None:
        args.insert(4, heads)
    return getattr(_lib_maxbwd.lib(), name)(*args)


def test_header_is_closed_over_the_exports_and_the_binding():
    """include/mp_maxbwd.h in both directions: what it declares is exported and bound with the header's own types, and
    the binding names nothing else; none of it is in mp_engine.h's table"""
    import os
    import re
    from graphgym_amd import _lib, _lib_maxbwd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(root, "include", "mp_maxbwd.h")).read(), flags=re.S)
    names = sorted(set(re.findall(r"\b(mp_[a-z0-9_]+)\s*\(", text)))
    assert names == ["mp_spmm_heads_max_bwd_pull_f32", "mp_spmm_max_bwd_pull_bf16", "mp_spmm_max_bwd_pull_f32"]
    lib = _lib_maxbwd.lib()
    assert set(_lib_maxbwd.PROTOTYPES_MAXBWD) == set(names)
    for n in names:
        assert hasattr(lib, n), f"{n} declared in mp_maxbwd.h but not exported"
        assert getattr(lib, n).argtypes == _lib_maxbwd.PROTOTYPES_MAXBWD[n][1] and getattr(lib, n).restype is C.c_int
        assert n not in _lib.PROTOTYPES
    assert len(_lib_maxbwd.PROTOTYPES_MAXBWD["mp_spmm_max_bwd_pull_f32"][1]) == len(ORDER)
    assert len(_lib_maxbwd.PROTOTYPES_MAXBWD["mp_spmm_heads_max_bwd_pull_f32"][1]) == len(ORDER) + 1


@pytest.mark.parametrize("name, heads", [("mp_spmm_max_bwd_pull_f32", None), ("mp_spmm_max_bwd_pull_bf16", None),
                                         ("mp_spmm_heads_max_bwd_pull_f32", 2)])
def test_entries_validate_without_a_device(name, heads):
    from graphgym_amd import _lib
    buf = (C.c_float * 64)()
    tv = {"t_val": C.cast(buf, C.c_void_p)} if heads else {}
    INVALID, UNSUPPORTED = 1, _lib.MP_ERR_UNSUPPORTED
    for k in ("t_rowptr", "plan", "counts", "t_col", "t_pos", "argmax", "dY", "dX"):
        assert _call(name, heads, **{**tv, k: None}) == INVALID, k
    for k, bad in (("n_src", -1), ("nnz", -1), ("d", 0), ("d", -4), ("lda", 3), ("ldy", 3), ("ldx", 3)):
        assert _call(name, heads, **{**tv, k: bad}) == INVALID, (k, bad)
    assert _call(name, heads, **{**tv, "nnz": 2 ** 31}) == UNSUPPORTED
    assert _call(name, heads, **{**tv, "nnz": 2 ** 31 - 1}) == UNSUPPORTED
    assert _call(name, heads, **{**tv, "n_src": 2 ** 31}) == UNSUPPORTED
    assert _call(name, heads, **{**tv, "n_src": 0}) == _lib.MP_OK            # no row: nothing to write
    # a plan with hub pieces needs its workspace
    counts = (C.c_int32 * 8)(1, 1, 3, 1, 4, 320, 1024, 256)
    assert _call(name, heads, **{**tv, "counts": counts}) == 3
    if heads:
        assert _call(name, heads, t_val=None) == INVALID                     # the heads form has no implicit ones
        assert _call(name, 0, **tv) == INVALID
        assert _call(name, 3, **tv) == INVALID                               # d = 4 is no multiple of 3
        assert _call(name, 3, **{**tv, "d": 6, "lda": 6, "ldy": 6, "ldx": 6}) == UNSUPPORTED   # per head, by the caller


# ---- the fake kernels -------------------------------------------------------------------------------------------------
def _meta_graph(n_rows, n_cols):
    from graphgym_amd import CSRGraph
    rowptr = torch.zeros(n_rows + 1, dtype=torch.int32)
    return CSRGraph(rowptr, torch.zeros(0, dtype=torch.int32), None, None, n_rows, 0, n_cols)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_fake_kernels(dtype):
    from torch._subclasses.fake_tensor import FakeTensorMode
    import graphgym_amd  # noqa: F401
    g = _meta_graph(12, 7)                   # a rectangular operator: the gradient has one row per COLUMN
    with FakeTensorMode():
        dy = torch.empty((12, 10), dtype=dtype, device="cuda")
        am = torch.empty((12, 10), dtype=torch.int32, device="cuda")
        dx = torch.ops.mp.spmm_max_bwd_pull_raw(dy, am, g.handle)
        assert dx.shape == (7, 10) and dx.dtype == dtype and dx.device.type == "cuda"
        if dtype == torch.float32:
            w = torch.empty((0, 2), dtype=torch.float32, device="cuda")
            dv = torch.ops.mp.spmm_heads_max_bwd_pull_raw(dy, am, w, g.handle, 2)
            assert dv.shape == (7, 10) and dv.dtype == torch.float32 and dv.device.type == "cuda"


# ---- the host restatement ---------------------------------------------------------------------------------------------
def _host_case(kind, weighted, d, heads=1, seed=0):
    dst, src, N, w = D.edges(kind, seed)
    rows, cols, order = D.csr_host(dst, src, N)
    val = w[order] if weighted else None
    if heads > 1:
        val = np.stack([w[order] * (1 + 0.25 * h) for h in range(heads)], 1).astype(np.float32)
    x = D.features(N, d, seed, boost=(0, 1, 2))
    argmax = D.forward_max_host(rows, cols, val, x, N, heads)
    gt = D.transpose_host(rows, cols, N)
    dy = D.spread_dy((N, d), seed)
    return rows, cols, val, argmax, gt, dy, N


@pytest.mark.parametrize("weighted", [False, True], ids=["ones", "weighted"])
@pytest.mark.parametrize("kind", [k for k in D.GRAPHS if k != "rect"])
def test_host_restatement_against_float64(kind, weighted):
    for d in (1, 7):
        rows, cols, val, argmax, (rp, gc, gp), dy, N = _host_case(kind, weighted, d)
        if kind == "empty_dst":
            assert (argmax[::5] == -1).all()
        if kind == "no_out":
            assert (rp[1:][::4] == rp[:-1][::4]).all()
        hub = dict(hub_deg=D.STAR_PLAN[2], piece_edges=D.STAR_PLAN[3]) if kind == "star" else {}
        if kind == "star":
            assert rp[1] - rp[0] >= 300
        got = D.max_bwd_pull_host(rp, gc, gp, val, argmax, dy, **hub)
        ref = D.max_bwd_dense64(rows, cols, val, argmax, dy, N)
        mag = D.max_bwd_dense64(rows, cols, val, argmax, dy, N, absolute=True)
        # fp32 sums of up to a few hundred terms of either sign and magnitudes spread over 2^20: held to the sum of the
        # absolute terms (tests/_tol.py rule (d))
        assert_close_rows(got, ref, mag=mag, what=f"host {kind} weighted={weighted} d={d}")
        assert (got[rp[1:] == rp[:-1]] == 0).all()


def test_host_restatement_heads():
    rows, cols, val, argmax, (rp, gc, gp), dy, N = _host_case("multi", True, 12, heads=4)
    got = D.max_bwd_pull_host(rp, gc, gp, val, argmax, dy, heads=4)
    ref = D.max_bwd_dense64(rows, cols, val, argmax, dy, N, heads=4)
    mag = D.max_bwd_dense64(rows, cols, val, argmax, dy, N, heads=4, absolute=True)
    assert_close_rows(got, ref, mag=mag, what="host heads")


def test_ties_go_to_the_first_entry():
    """a repeated (destination, source) pair carries equal messages: only the first entry's pos wins, and the pull form
    counts the gradient once"""
    dst, src, N, _ = D.edges("multi")
    rows, cols, _ = D.csr_host(dst, src, N)
    same = (rows[1:] == rows[:-1]) & (cols[1:] == cols[:-1])
    assert same.sum() > 100
    argmax = D.forward_max_host(rows, cols, None, D.features(N, 3, boost=(0, 1, 2)), N)
    later = np.nonzero(same)[0] + 1
    assert not np.isin(argmax, later).any()
    rp, gc, gp = D.transpose_host(rows, cols, N)
    ones = np.ones((N, 3), dtype=np.float32)
    got = D.max_bwd_pull_host(rp, gc, gp, None, argmax, ones)
    assert got.sum() == (argmax >= 0).sum()


@pytest.mark.parametrize("kind", ["multi", "star"])
def test_another_order_changes_bits(kind):
    """the inputs of the bitwise GPU checks show an order: the same terms summed with every row's entries reversed
    differ in at least one row — otherwise equal bits would prove nothing"""
    rows, cols, val, argmax, (rp, gc, gp), dy, N = _host_case(kind, False, 7)
    a = D.max_bwd_pull_host(rp, gc, gp, None, argmax, dy)
    rc, rpos = D.reversed_rows(rp, gc, gp)
    b = D.max_bwd_pull_host(rp, rc, rpos, None, argmax, dy)
    assert (a.view(np.uint32) != b.view(np.uint32)).any(axis=1).sum() >= 1
    np.testing.assert_allclose(a, b, rtol=0, atol=1e-5 * np.abs(dy).max() * 300)
