"""scripts/agg_hot_pmc.py — the bench graph, d = 256: 4 launches with MP_AGG_HOT_MB=0 (the plain tile kernel), then 4 with the default budget
(the hot kernel): for per-dispatch kernel traces and counters, one rocprofv3 pass per counter:
    rocprofv3 --pmc FETCH_SIZE --output-format csv -d OUT -- python scripts/agg_hot_pmc.py"""
import os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import graphgym_amd as ga
from graphgym_amd import _lib, graphgen, ops
dev = torch.device("cuda:0")
n, d = 10_000_000, 256
ei = graphgen.ba_edge_index(n, 5, seed=12345, device=dev)
g = ga.CSRGraph.from_edge_index(ei, n, add_self_loops=True).gcn_norm("row")
del ei
x = torch.empty((n, d), dtype=torch.float32, device=dev)
x.uniform_(-1.0, 1.0, generator=torch.Generator(device=dev).manual_seed(7))
y = torch.empty((n, d), dtype=torch.float32, device=dev)
for mb in ("0", str(ops.AGG_HOT_MB)):
    os.environ["MP_AGG_HOT_MB"] = mb
    ops._raw_spmm(g, x, _lib.SUM, out=y)      # (the tag is built here, outside the 4 launches)
    torch.cuda.synchronize()
    for _ in range(4):
        ops._raw_spmm(g, x, _lib.SUM, out=y)
    torch.cuda.synchronize()
print("ok", ops.AGG_HOT_CALLS)
