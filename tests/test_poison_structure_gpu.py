"""No mp_struct_* entry may depend on the contents of its fresh allocations: the cases of tests/test_poison_gpu.py for the
centrality layer (include/mp_structure.h), under the same harness (tests/_poison.py through that file's `differential`:
the three fills in their order, the recorder, the guards) and the same checks 1-4 of its docstring.

Every output (values, iteration counts, ids), every workspace (PageRank's ping-pong vectors, 1/deg and partial sums;
betweenness' partial vectors and its level / sigma / delta slabs) is a `torch.empty`, and the results under the three
fills are equal bit for bit: every sum of these entries has a fixed order.  The graphs take every form: PageRank's LDS
and large form in one batch, betweenness' LDS and workspace form in one batch, isolated nodes (dangling sums), more than
one chunk and more than one source slice."""
import networkx as nx
import pytest
import torch

import _centrality_ref as CR
import _structure_ref as R
from test_poison_gpu import Case, differential


def _batch(dev, big):
    graphs = R.pc_graphs(3) + [CR.path_with_isolated(), nx.path_graph(1),
                               CR.with_isolated(nx.powerlaw_cluster_graph(big, 3, 0.5, seed=2))]
    return R.base_of(graphs, dev)


def run_pagerank(dev):
    from graphgym_amd import _lib_structure as LS
    from graphgym_amd import structure
    base, gp = _batch(dev, LS.PAGERANK_LDS_NODES + 100)           # the last graph: three chunks of the large form
    out, iters = structure.node_pagerank(base, gp, return_iters=True)
    alone, iters1 = structure.node_pagerank(base, gp, alpha=0.5, tol=1e-9, return_iters=True)
    assert int(iters.min()) >= 1 and int(iters1.min()) >= 1
    return out, iters, alone, iters1


def run_betweenness(dev):
    from graphgym_amd import _lib_structure as LS
    from graphgym_amd import structure
    base, gp = _batch(dev, LS.BETWEENNESS_LDS_NODES + 30)         # the last graph keeps its vectors in the workspace
    small, gp_small = R.base_of(R.ba_graphs(3), dev)
    return structure.node_betweenness_centrality(base, gp), structure.node_betweenness_centrality(small, gp_small)


def run_onehot(dev):
    from graphgym_amd import structure
    base, gp = _batch(dev, 300)
    return structure.node_onehot(base, gp, seed=3), structure.node_onehot(base, seed=3)


CASES = [
    Case("struct_pagerank", ("mp_struct_pagerank",), run_pagerank),
    Case("struct_betweenness", ("mp_struct_betweenness",), run_betweenness),
    Case("struct_onehot", ("mp_struct_onehot",), run_onehot),
]
# (the *_ws_bytes entries are host-only: no device memory is touched; tests/test_centrality_host.py closes the list)


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_no_struct_entry_depends_on_fresh_allocations(dev, monkeypatch, case):
    from graphgym_amd import _lib_structure
    _lib_structure.lib()                 # bound before the recorder stands in: binding fetches every entry by name
    seen = differential(case.run, dev, monkeypatch, case.entries, what=case.name)
    print(f"{case.name}: {seen} bytes through the shim")
