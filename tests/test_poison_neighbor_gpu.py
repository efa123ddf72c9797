"""No mp_nbr_* entry may depend on the contents of its fresh allocations: the cases of tests/test_poison_gpu.py for
include/mp_neighbor.h, under the same harness (tests/_poison.py through that file's `differential`: the three fills in
their order, the recorder, the guards) and the same checks 1-4 of its docstring; check 5 is the NumPy restatement of
the sampler, which every returned tensor must equal.

The graph is that file's hub graph (320 nodes, one row of 1 300 entries, one row in twenty empty), so a batch holds rows
taken whole, rows drawn through the in-group sort (the hub at fanouts 4 and 200) and empty rows.  Plans, seeds,
bitmaps, ranks, frontiers and outputs are all built inside the poisoned context.  Integers only: the results under
the three fills are equal bit for bit."""
import pytest
import torch

from test_poison_gpu import Case, differential, hub_graph

SIZES = ([4, 200, 3], [-1, 2], [200])
SEEDS = [3, 40, 41, 3, 319]                   # the hub, a repeat, the last node


def _fields(b):
    return (b.orig_node, b.graph.rowptr, b.graph.col, b.base_entry, b.hop, b.seed_index, b.edge_index)


def run_neighbor(dev):
    from graphgym_amd import neighbor as NB
    g = hub_graph(dev, weighted=False)
    out = []
    for sizes in SIZES:
        plan = NB.plan_neighbor(g, sizes, 7, torch.arange(1, 320, 3, device=dev))
        for step in (0, plan.num_batches - 1):
            out.append(NB.seeds(plan, 5, step))
            out += _fields(NB.neighbor_batch(plan, 5, step))
        out += _fields(NB.neighbor_batch_nodes(plan, torch.tensor(SEEDS, device=dev), 5, 1))
    return tuple(out)


def oracle_neighbor(outs):
    from graphgym_amd import neighbor as NB
    from graphgym_amd.link_pred import _on_cpu
    h = _on_cpu(hub_graph(outs[0].device, weighted=False))
    want = []
    for sizes in SIZES:
        plan = NB.plan_neighbor(h, sizes, 7, torch.arange(1, 320, 3))
        for step in (0, plan.num_batches - 1):
            want.append(NB.seeds_host(plan, 5, step))
            want += _fields(NB.neighbor_batch_host(plan, 5, step))
        want += _fields(NB.neighbor_batch_host(plan, 5, 1, torch.tensor(SEEDS)))
    assert len(want) == len(outs)
    for i, (o, w) in enumerate(zip(outs, want)):
        assert o.dtype == w.dtype and torch.equal(o.cpu(), w), f"output {i}"


CASES = [
    Case("neighbor", ("mp_nbr_seeds", "mp_nbr_mark", "mp_nbr_count", "mp_nbr_fill", "mp_bitmap_mark",
                      "mp_bitmap_word_counts", "mp_bitmap_nodes"), run_neighbor, oracle=oracle_neighbor),
]


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_no_neighbor_entry_depends_on_fresh_allocations(dev, monkeypatch, case):
    from graphgym_amd import _lib_neighbor
    _lib_neighbor.lib()               # bound before the recorder stands in: binding fetches every entry by name
    seen = differential(case.run, dev, monkeypatch, case.entries, case.oracle, what=case.name)
    print(f"{case.name}: {seen} bytes through the shim")
