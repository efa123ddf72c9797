"""The poisoning allocator shim of tests/_poison.py on CPU tensors (`cpu=True`), and the closure of the case table of
tests/test_poison_gpu.py over the C ABI: every entry of _lib.PROTOTYPES has a case or an admissible reason not to."""
import re

import pytest
import torch

import _poison as P
from _bigview import SENTINEL16
from _layout import SENTINEL

DTYPES = [torch.float32, torch.bfloat16, torch.float16, torch.int32, torch.int64, torch.uint8, torch.bool, torch.float64]
SHAPES = [(), (1,), (5,), (3, 5), (2, 0, 3), (0,), (7, 1, 2)]


@pytest.mark.parametrize("word", P.FILLS, ids=hex)
def test_shapes_dtypes_and_fill_patterns(word):
    real = (torch.empty, torch.empty_like)
    with P.poisoned(word, cpu=True) as p:
        assert torch.empty is not real[0]
        seen = 0
        for dtype in DTYPES:
            for shape in SHAPES:
                for t in (torch.empty(shape, dtype=dtype),
                          torch.empty(*shape, dtype=dtype) if shape else torch.empty((), dtype=dtype),
                          torch.empty_like(torch.zeros(shape, dtype=dtype)),
                          torch.zeros(3).new_empty(shape, dtype=dtype)):
                    assert t.shape == torch.Size(shape) and t.dtype == dtype and t.is_contiguous() and not t._is_view()
                    n = t.numel() * t.element_size()
                    seen += n
                    if t.numel():
                        assert t.data_ptr() % 16 == 0
                        es = t.element_size()
                        bits = P.raw_bits(t).reshape(-1)
                        if es == 1:
                            w32 = P.word32_for(word, 1)
                            want = torch.tensor([(w32 >> (8 * (k % 4))) & 0xFF for k in range(t.numel())], dtype=torch.uint8)
                            assert torch.equal(bits, want)
                        else:
                            assert bool((bits == P.signed(P.element_pattern(word, dtype), es)).all())
        assert p.bytes_seen == seen and p.allocations == len(p.buffers) == 4 * len(DTYPES) * len(SHAPES)
        for flat, nbytes, _ in p.buffers:
            assert flat.numel() == P.GUARD + (nbytes + 3) // 4 * 4 + P.GUARD and flat.dtype == torch.uint8
        p.check_guards()
    assert (torch.empty, torch.empty_like) == real and "new_empty" not in torch.Tensor.__dict__


def test_the_words():
    assert P.FILLS == (0, 1, SENTINEL)
    assert P.word16(SENTINEL) == SENTINEL16 and P.word16(1) == 1 and P.word16(0) == 0
    with P.poisoned(SENTINEL, cpu=True):
        f, b, i = torch.empty(4), torch.empty(4, dtype=torch.bfloat16), torch.empty(4, dtype=torch.int32)
    assert bool(torch.isnan(f).all()) and bool(torch.isnan(b).all()) and bool((i == SENTINEL).all())
    with P.poisoned(1, cpu=True):
        f, i, l = torch.empty(4), torch.empty(4, dtype=torch.int32), torch.empty(4, dtype=torch.int16)
    assert bool((f > 0).all()) and bool((f < 1e-40).all()) and bool((i == 1).all()) and bool((l == 1).all())


def test_guards_catch_writes_on_either_side():
    for shape, where, word in (((16,), 16, 0), ((16,), -1, 1), ((3, 5), 15, SENTINEL), ((5,), 7, 1)):
        with P.poisoned(word, cpu=True) as p:
            t = torch.empty(shape)
            t.zero_()
            p.check_guards()
            flat = torch.as_strided(t, (t.numel() + 8,), (1,), t.storage_offset() - 4)
            flat[4 + where] = 3.0
            with pytest.raises(AssertionError, match="guard bytes overwritten"):
                p.check_guards()
    with P.poisoned(1, cpu=True) as p:                 # an odd byte count: the round-up slack belongs to the guard
        t = torch.empty(5, dtype=torch.uint8)
        t.fill_(9)
        p.check_guards()
        torch.as_strided(t, (6,), (1,))[5] = 9
        with pytest.raises(AssertionError, match="guard bytes overwritten"):
            p.check_guards()


def test_restored_after_an_exception_too():
    real = (torch.empty, torch.empty_like)
    with pytest.raises(RuntimeError, match="boom"):
        with P.poisoned(1, cpu=True):
            assert torch.empty is not real[0]
            raise RuntimeError("boom")
    assert (torch.empty, torch.empty_like) == real and "new_empty" not in torch.Tensor.__dict__
    assert float(torch.zeros(2).new_empty(3).fill_(2.0).sum()) == 6.0


def test_pass_through_cases():
    with P.poisoned(SENTINEL) as p:                    # cpu=False: host tensors are torch's own
        t = torch.empty(8)
        assert p.allocations == 0 and p.passed_through == 1 and t.storage_offset() == 0
    with P.poisoned(SENTINEL, cpu=True) as p:
        dst = torch.zeros(4)
        assert torch.empty(4, out=dst) is dst
        c = torch.empty(4, dtype=torch.complex64)
        m = torch.empty(4, device="meta")
        assert p.allocations == 0 and c.storage_offset() == 0 and m.device.type == "meta"
        assert torch.empty(size=(2, 3)).shape == (2, 3) and p.allocations == 1
        g = torch.empty(3, requires_grad=True)
        assert g.requires_grad and g.is_leaf and p.allocations == 2
        # empty_like of a non-contiguous tensor keeps torch's strides and is only filled
        src = torch.zeros(4, 6).t()
        like = torch.empty_like(src)
        assert like.stride() == src.stride() and bool(torch.isnan(like).all()) and len(p.buffers) == 2
        assert p.allocations == 3
        # library code keeps working under the shim
        lin = torch.nn.Linear(4, 3)
        y = torch.nn.functional.layer_norm(lin(torch.ones(2, 4)), (3,))
        assert bool(torch.isfinite(y).all())
        p.check_guards()


def test_recorder_records_what_is_fetched():
    class Lib:
        def mp_one(self, a):
            return a + 1

        other = 5
    rec = P.Recorder(Lib())
    assert rec.mp_one(2) == 3 and rec.other == 5 and rec.mp_one(0) == 1
    assert rec.names() == {"mp_one"} and rec.seen == ["mp_one", "mp_one"]
    with pytest.raises(AttributeError):
        rec.mp_missing


def test_fill_hits_and_same_bits():
    base = torch.tensor([0.0, 2.0, 3.0])
    run = base.clone()
    run.view(torch.int32)[1] = 1
    assert P.fill_hits(run, base, 1) == 1 and P.fill_hits(base, base, 1) == 0 and not P.same_bits(run, base)
    nan = base.clone()
    nan.view(torch.int32)[2] = SENTINEL
    assert P.fill_hits(nan, base, SENTINEL) == 1 and P.same_bits(nan, nan.clone())
    assert not P.same_bits(torch.tensor([0.0]), torch.tensor([-0.0]))


# ---- the sums of the atomics cases are exact --------------------------------------------------------------------------
def test_the_atomics_operands_sum_exactly():
    """integers in [-8, 8] (gradients, features) times powers of two in [1/4, 4] (weights), summed by destination and by
    source at the degrees of the cases' graph — the hub row among them: float32 index_add_ gives the float64 sums, so the
    order of the additions cannot show in the bits"""
    import test_poison_gpu as T
    src, dst, w = T.hub_edges()
    assert int(torch.bincount(dst).max()) >= 1000 and set(w.tolist()) <= {0.25, 0.5, 1.0, 2.0, 4.0}
    d = 16
    x, dy = T.ints(T.N_NODES, d, seed=1), T.ints(T.N_NODES, d, seed=2)
    assert float(x.abs().max()) <= 8 and bool((x == x.round()).all())
    for idx, gathered in ((dst, x[src]), (src, dy[dst])):
        terms = gathered * w[:, None]
        s32 = torch.zeros(T.N_NODES, d).index_add_(0, idx, terms)
        s64 = torch.zeros(T.N_NODES, d, dtype=torch.float64).index_add_(0, idx, terms.double())
        assert torch.equal(s32.double(), s64)
        perm = torch.randperm(idx.numel(), generator=T.gen(3))
        assert torch.equal(torch.zeros(T.N_NODES, d).index_add_(0, idx[perm], terms[perm]), s32)
    deg = torch.zeros(T.N_NODES).index_add_(0, src, w)
    assert torch.equal(deg.double(), torch.zeros(T.N_NODES, dtype=torch.float64).index_add_(0, src, w.double()))
    # the attention-weighted max backward: a power of two per entry and head times an integer in [-2, 2]
    a, g = T.pow2(dst.numel(), 4), T.ints(dst.numel(), d, seed=5, lo=-2, hi=2)
    s32 = torch.zeros(T.N_NODES, d).index_add_(0, src, a[:, None] * g)
    s64 = torch.zeros(T.N_NODES, d, dtype=torch.float64).index_add_(0, src, (a[:, None] * g).double())
    assert torch.equal(s32.double(), s64)


# ---- coverage closure ---------------------------------------------------------------------------------------------
HOST_ONLY = "host-only: no device memory is touched"
PROBE = "probe or stream utility"
EXCLUDED = {
    "mp_version": HOST_ONLY, "mp_status_str": HOST_ONLY, "mp_last_hip_error": HOST_ONLY,
    "mp_collate_stage_cap": HOST_ONLY, "mp_code_reduce_max_codes": HOST_ONLY,
    "mp_lpt_partition_host": HOST_ONLY, "mp_gen_ba_edges_host": HOST_ONLY, "mp_gen_powerlaw_cluster_edges_host": HOST_ONLY,
    "mp_csr_from_coo_ws_bytes": HOST_ONLY, "mp_csr_transpose_ws_bytes": HOST_ONLY, "mp_spmm_plan_bytes": HOST_ONLY,
    "mp_spmm_ws_bytes": HOST_ONLY, "mp_bn_ws_bytes": HOST_ONLY, "mp_bn_act_ws_bytes": HOST_ONLY,
    "mp_bn_drop_ws_bytes": HOST_ONLY, "mp_dense_wgrad_ws_bytes": HOST_ONLY, "mp_code_reduce_ws_bytes": HOST_ONLY,
    "mp_copy_probe_f32": PROBE, "mp_read_probe_f32": PROBE, "mp_probe_copy_ms": PROBE, "mp_probe_gather_ms": PROBE,
    "mp_stream_create_cu_mask": PROBE, "mp_stream_destroy": PROBE,
}
_ADMISSIBLE = re.compile(r"^(mp_.*_host|mp_.*_bytes|mp_version|mp_status_str|mp_last_hip_error|mp_collate_stage_cap|"
                         r"mp_code_reduce_max_codes|mp_copy_probe_f32|mp_read_probe_f32|mp_probe_.*_ms|"
                         r"mp_stream_create_cu_mask|mp_stream_destroy)$")


def test_every_c_entry_has_a_case_or_a_reason():
    """a new C entry fails here until someone gives it a case in tests/test_poison_gpu.py"""
    import test_poison_gpu as T                        # the table imports without touching a device
    from graphgym_amd import _lib
    covered = set()
    for case in T.CASES:
        assert case.entries and case.exact and callable(case.run), case.name
        assert case.unspecified is None or "mp_engine.h" in case.unspecified[0], f"{case.name}: quote the header line"
        covered |= set(case.entries)
    names = [c.name for c in T.CASES]
    assert len(names) == len(set(names))
    every = set(_lib.PROTOTYPES)
    assert covered <= every, f"cases name entries that do not exist: {sorted(covered - every)}"
    assert not (covered & set(EXCLUDED)), f"both covered and excluded: {sorted(covered & set(EXCLUDED))}"
    assert set(EXCLUDED) <= every, f"excluded names that do not exist: {sorted(set(EXCLUDED) - every)}"
    for name, reason in EXCLUDED.items():
        assert _ADMISSIBLE.match(name) and reason in (HOST_ONLY, PROBE), f"{name}: not an admissible exclusion"
    missing = every - covered - set(EXCLUDED)
    assert not missing, f"C entries without a case: {sorted(missing)}"
