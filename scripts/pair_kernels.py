"""The workload behind the kernel table of the pair decoders: ops.pair_score (dot, cosine) and
ops.pair_sum forward + backward on link_batch of BA(NODES, 5) at ratio 1, d in WIDTHS, a few repetitions each, and
mp_sddmm_dot_stream_f32 on the same pairs (as int32) for comparison.  Run it under the profiler for the table,

    rocprofv3 --kernel-trace --stats -d OUT -- python scripts/pair_kernels.py

or alone: it prints the forward kernels' time from device events and the bytes they have to move
(score: 2 K d 4 + 16 K + 4 K; sum: the same with K m 4 written)."""
import ctypes as C
import json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import graphgym_amd as ga
from graphgym_amd import _lib, graphgen, ops, pair_ops
from graphgym_amd._lib import check, ptr
from graphgym_amd.link_pred import link_batch, link_split

dev = torch.device("cuda:0")
n = int(os.environ.get("NODES", "1000000"))
WIDTHS = [int(v) for v in os.environ.get("WIDTHS", "64,128,256").split(",")]
REPS = int(os.environ.get("REPS", "5"))


def ms(fn):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(REPS):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / REPS


ei = graphgen.ba_edge_index(n, 5, seed=12345, device=dev)
base = ga.CSRGraph.from_edge_index(ei, n)
splits = link_split(base, torch.tensor([0, n]), (0.8, 0.2), generator=torch.Generator().manual_seed(0))
index = link_batch(splits["train"], torch.zeros((n, 1), device=dev), ratio=1.0, seed=1, offset=0).edge_label_index.contiguous()
K = index.size(1)
a32, b32 = index[0].to(torch.int32), index[1].to(torch.int32)
gen = torch.Generator(device=dev).manual_seed(7)
pi = ops.pair_index(index, n)
pi.role_operators()
for d in WIDTHS:
    h = torch.empty((n, d), device=dev).uniform_(-1.0, 1.0, generator=gen).requires_grad_(True)
    g = torch.empty(K, device=dev).uniform_(-1.0, 1.0, generator=gen)
    rec = {"n": n, "K": K, "d": d, "score_bytes": 2 * K * d * 4 + 20 * K, "sum_bytes": 3 * K * d * 4 + 16 * K}
    with torch.no_grad():
        r = pair_ops._raw_rnorm(h, 1e-8)
        rec["score_dot_ms"] = ms(lambda: pair_ops._raw_pair_score(h, index))
        rec["score_cosine_ms"] = ms(lambda: pair_ops._raw_pair_score(h, index, r))
        rec["rnorm_ms"] = ms(lambda: pair_ops._raw_rnorm(h, 1e-8))
        rec["sum_ms"] = ms(lambda: pair_ops._raw_pair_sum(h, h, index))
        s = torch.empty(K, device=dev)
        L = _lib.lib()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rec["sddmm_stream_ms"] = ms(lambda: check(L.mp_sddmm_dot_stream_f32(ptr(a32), ptr(b32), K, ptr(h), h.stride(0),
                                                                            ptr(h), h.stride(0), d, 1, 1.0, ptr(s), stream)))
        rec["sddmm_equal"] = bool(torch.allclose(s, pair_ops._raw_pair_score(h, index)[0], rtol=1e-4, atol=1e-4))
    for cosine in (False, True):
        def step():
            h.grad = None
            ops.pair_score(h, index, cosine=cosine, pair_index=pi).backward(g)
        rec["fwd_bwd_cosine_ms" if cosine else "fwd_bwd_dot_ms"] = ms(step)
    for k in ("score_dot", "score_cosine", "sddmm_stream"):
        rec[k + "_TBps"] = round(rec["score_bytes"] / rec[k + "_ms"] / 1e9, 3)
    rec["sum_TBps"] = round(rec["sum_bytes"] / rec["sum_ms"] / 1e9, 3)
    print(json.dumps(rec), flush=True)
    del h
    torch.cuda.empty_cache()
