"""The barrier structure of the hot-column tile kernels (fused_hot.hip: agg_dense_pc_kernel<..., HOT = true> of fused_pc.h, built in
a translation unit of their own), checked on the emitted code as tests/test_emitted_barriers.py checks fused.o: two
loops with b1 + b2 each, 3 barriers outside them, + 2 with a self term.  Also: that object holds the hot kernels and
nothing else.  CPU only."""
from test_emitted_barriers import _template_args, barriers_by_loop, disassemble, kernels_of


def test_hot_kernels_hold_equal_barrier_counts(tmp_path):
    ks = kernels_of(disassemble("fused_hot.o", tmp_path), "agg_dense_pc_kernel")
    assert len(ks) == 18                                          # sum / mean (± self term) and max at F = 128 / 256 / 512, ± weights
    seen = set()
    for sym, ins in ks.items():
        # <W, WEIGHTED, KH, NCB, PF, BF16X3, TR, NP, NC, HAS_S, AGG_ONLY, MAXR, HOT>
        targs = _template_args(sym, "agg_dense_pc_kernel")
        assert targs[10] and targs[12], sym                       # aggregation-only, hot
        has_s = targs[9]
        loops, outside = barriers_by_loop(ins)
        assert loops == [2, 2], (sym, loops, outside)
        assert outside == 3 + (2 if has_s else 0), (sym, loops, outside)
        seen.add(has_s)
    assert seen == {False, True}


def test_no_hot_kernel_in_the_plain_object(tmp_path):
    ks = kernels_of(disassemble("fused.o", tmp_path), "agg_dense_pc_kernel")
    assert ks and not any(len(t) > 12 and t[12] for t in (_template_args(s, "agg_dense_pc_kernel") for s in ks))
