"""The cache-key contract (graph.tensor_stamp) on CPU tensors, and the three holder caches that need no device once
their builder is stubbed: layers.get_graph, layers.seed_graph_cache, encoders.cached_codes.  The colliding pairs come from
tests/_alias.py, which asserts for each that the keys used before tensor_stamp could not tell its two tensors apart."""
import types

import pytest
import torch

import _alias

CPU = torch.device("cpu")
N_NODES = 96


def _all_pairs():
    out = []
    for n, unique in ((40, True), (3, True), (40, False), (2, True)):
        for sc in _alias.index_scenarios(n, unique):
            out.append((f"index-{sc}-{n}{'u' if unique else ''}", lambda sc=sc, n=n, u=unique:
                        _alias.index_pair(sc, CPU, n, N_NODES, unique=u)))
    out.append(("index-stride-40-int32", lambda: _alias.index_pair("stride", CPU, 40, N_NODES, dtype=torch.int32)))
    for sc in _alias.EDGE_SCENARIOS:
        out.append((f"edges-{sc}", lambda sc=sc: _alias.edge_pair(sc, CPU, 50, N_NODES)))
    for sc in _alias.CODE_SCENARIOS:
        out.append((f"codes-{sc}", lambda sc=sc: _alias.code_pair(sc, CPU, 6, 6, 7)))
    return out


PAIRS = _all_pairs()


def test_one_element_index_tensors_have_no_colliding_pair():
    assert _alias.index_scenarios(1) == () and _alias.index_scenarios(1, unique=False) == ()
    buf = torch.tensor([77, 5])
    for v in (buf[:1], buf[::2], buf.view(torch.int32)[:1], buf.view(torch.int16)[:1], buf.view(torch.uint8)[:1]):
        assert v.data_ptr() == buf.data_ptr() and v.numel() == 1 and int(v[0]) == 77


@pytest.mark.parametrize("name,make", PAIRS, ids=[p[0] for p in PAIRS])
def test_stamp_tells_every_alias_pair_apart(name, make):
    from graphgym_amd.graph import tensor_stamp
    A, B = make()
    assert tensor_stamp(A) != tensor_stamp(B)
    assert tensor_stamp(A) == tensor_stamp(A) and tensor_stamp(B) == tensor_stamp(B)
    assert hash(tensor_stamp(A)) is not None                       # a dictionary key


def test_stamp_holds_device_dtype_address_shape_strides_version():
    from graphgym_amd.graph import tensor_stamp
    t = torch.arange(12).view(3, 4)[:, 1:3]
    s = tensor_stamp(t)
    for part in (t.device, t.dtype, t.data_ptr(), (3, 2), (4, 1), t._version):
        assert part in s


def test_stamp_is_equal_for_the_same_tensor_and_for_a_fresh_slice_of_equal_geometry():
    from graphgym_amd.graph import tensor_stamp
    ids = torch.arange(50)
    a, b = ids[:17], ids[:17]
    assert a is not b and tensor_stamp(a) == tensor_stamp(b)
    assert tensor_stamp(ids[3:20:2]) == tensor_stamp(ids[3:20:2])
    assert tensor_stamp(ids[:17]) != tensor_stamp(ids[:18]) and tensor_stamp(ids[:17]) != tensor_stamp(ids[1:18])
    ei = torch.arange(40).view(2, 20)
    assert tensor_stamp(ei[:, :9]) == tensor_stamp(ei[:, :9]) and tensor_stamp(ei.t()) == tensor_stamp(ei.t())
    assert tensor_stamp(ids.detach()) == tensor_stamp(ids)


IN_PLACE = {
    "copy_": lambda t: t.copy_(torch.flip(t.clone(), (0,))),
    "setitem": lambda t: t.__setitem__(0, 1),
    "add_": lambda t: t.add_(1),
    "randperm_out": lambda t: torch.randperm(t.numel(), out=t, generator=torch.Generator().manual_seed(1)),
}


@pytest.mark.parametrize("op", sorted(IN_PLACE))
def test_stamp_sees_every_in_place_torch_op(op):
    from graphgym_amd.graph import tensor_stamp
    t = torch.arange(10, 30)
    view = t[:]                                                    # a view shares the version counter
    before, before_view = tensor_stamp(t), tensor_stamp(view)
    IN_PLACE[op](t)
    assert tensor_stamp(t) != before and tensor_stamp(view) != before_view
    assert tensor_stamp(t)[:-1] == before[:-1]                     # only the version moved


def test_stamp_cannot_see_a_rewrite_through_data():
    """the contract's blind spot, pinned so that nobody relies on the opposite: `.data` has a version counter of its own"""
    from graphgym_amd.graph import tensor_stamp
    t = torch.arange(10)
    before = tensor_stamp(t)
    t.data.add_(1)
    assert tensor_stamp(t) == before and int(t[0]) == 1


# ------------------------------------------------------------------------------------- the holder caches, builder stubbed
def _stub_graph(n=N_NODES):
    from graphgym_amd.graph import CSRGraph
    g = CSRGraph(torch.zeros(n + 1, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), None,
                 torch.zeros(0, dtype=torch.int32), n, 0)
    return g


@pytest.fixture
def builds(monkeypatch):
    """CSRGraph.from_edge_index replaced by a recorder that keeps a COPY of the edge list it was given (no device is needed:
    the builder never runs; what is under test is whether it is reached, and with what)"""
    from graphgym_amd.graph import CSRGraph
    seen = []

    def record(cls, edge_index, num_nodes, edge_weight=None, **kw):
        seen.append((edge_index.clone().to(torch.int64), int(num_nodes), dict(kw)))
        return _stub_graph(int(num_nodes))
    monkeypatch.setattr(CSRGraph, "from_edge_index", classmethod(record))
    return seen


@pytest.mark.parametrize("scenario", _alias.EDGE_SCENARIOS)
def test_get_graph_rebuilds_for_an_aliasing_edge_list(builds, scenario):
    from graphgym_amd import layers
    A, B = _alias.edge_pair(scenario, CPU, 50, N_NODES)
    holder = types.SimpleNamespace()
    gA = layers.get_graph(holder, A, N_NODES, dst_row=0)
    assert len(builds) == 1 and torch.equal(builds[0][0], A.long())
    assert layers.get_graph(holder, A, N_NODES, dst_row=0) is gA and len(builds) == 1         # unchanged: a hit
    gB = layers.get_graph(holder, B, N_NODES, dst_row=0)
    assert len(builds) == 2 and gB is not gA, "the aliasing edge list was answered from the cache"
    assert torch.equal(builds[1][0], B.long()) and builds[1][2]["dst_row"] == 0
    assert layers.get_graph(holder, B, N_NODES, dst_row=0) is gB and len(builds) == 2


def test_get_graph_hits_on_a_fresh_view_of_equal_geometry_and_keys_on_num_nodes(builds):
    from graphgym_amd import layers
    buf = torch.randint(0, N_NODES, (2, 80), generator=torch.Generator().manual_seed(3))
    holder = types.SimpleNamespace()
    g = layers.get_graph(holder, buf[:, :50], N_NODES)
    assert layers.get_graph(holder, buf[:, :50], N_NODES) is g and len(builds) == 1
    assert layers.get_graph(holder, buf[:, :50], N_NODES, loops="add") is not g and len(builds) == 2   # another policy
    assert layers.get_graph(holder, buf[:, :50], N_NODES) is g and len(builds) == 2
    assert layers.get_graph(holder, buf[:, :50], N_NODES + 1) is not g and len(builds) == 3


@pytest.mark.parametrize("op", sorted(IN_PLACE))
def test_get_graph_rebuilds_after_an_in_place_update(builds, op):
    from graphgym_amd import layers
    ei = torch.stack([torch.arange(20), torch.arange(20).flip(0)])
    holder = types.SimpleNamespace()
    layers.get_graph(holder, ei, 20)
    layers.get_graph(holder, ei, 20)
    assert len(builds) == 1
    old = ei.clone()
    IN_PLACE[op](ei[1])                                             # through a view: the version counter is shared
    assert not torch.equal(old, ei)
    layers.get_graph(holder, ei, 20)
    assert len(builds) == 2 and torch.equal(builds[1][0], ei) and torch.equal(builds[0][0], old)


@pytest.mark.parametrize("scenario", _alias.EDGE_SCENARIOS)
def test_seed_graph_cache_does_not_answer_for_an_aliasing_edge_list(builds, scenario):
    from graphgym_amd import layers
    A, B = _alias.edge_pair(scenario, CPU, 50, N_NODES)
    seeded = _stub_graph()
    seeded.symmetric = True
    holder = types.SimpleNamespace()
    layers.seed_graph_cache(holder, A, N_NODES, seeded, "none")
    assert layers.get_graph(holder, A, N_NODES) is seeded and not builds                       # the seed is found
    assert layers.get_graph(holder, A, N_NODES, loops="remove") is seeded and not builds
    got = layers.get_graph(holder, B, N_NODES)
    assert got is not seeded and len(builds) == 1 and torch.equal(builds[0][0], B.long())
    # ... and after an in-place update of the seeded list
    layers.seed_graph_cache(holder, A, N_NODES, seeded, "none")
    A[0, 0] = (int(A[0, 0]) + 1) % N_NODES
    assert layers.get_graph(holder, A, N_NODES) is not seeded and len(builds) == 2
    assert torch.equal(builds[1][0], A.long())


@pytest.fixture
def checks(monkeypatch):
    """ops.check_codes replaced by a recorder that keeps a copy of the codes it was given"""
    from graphgym_amd import ops
    seen = []

    def record(codes, dims, what="codes"):
        seen.append((codes.clone().to(torch.int64), tuple(dims), what))
        return codes.to(torch.int32).contiguous()
    monkeypatch.setattr(ops, "check_codes", record)
    return seen


@pytest.mark.parametrize("scenario", _alias.CODE_SCENARIOS)
def test_cached_codes_rechecks_an_aliasing_code_tensor(checks, scenario):
    from graphgym_amd import encoders
    R = K = 6
    A, B = _alias.code_pair(scenario, CPU, R, K, 7)
    dims = [7] * K
    holder = types.SimpleNamespace()
    a = encoders.cached_codes(holder, "node_feature", A, dims)
    assert len(checks) == 1 and torch.equal(a.long(), A.long())
    assert encoders.cached_codes(holder, "node_feature", A, dims) is a and len(checks) == 1      # unchanged: a hit
    b = encoders.cached_codes(holder, "node_feature", B, dims)
    assert len(checks) == 2, "the aliasing codes were answered from the cache"
    assert torch.equal(checks[1][0], B.long()) and torch.equal(b.long(), B.long())
    assert encoders.cached_codes(holder, "node_feature", B, dims) is b and len(checks) == 2


def test_cached_codes_hits_on_the_encoders_own_fresh_column_slice(checks):
    """_TablesEncoder.encode passes feature[:, :K], a new strided view on every call"""
    from graphgym_amd import encoders
    feature = torch.randint(0, 7, (30, 9), generator=torch.Generator().manual_seed(4))
    holder = types.SimpleNamespace()
    a = encoders.cached_codes(holder, "node_feature", feature[:, :3], [7, 7, 7])
    assert encoders.cached_codes(holder, "node_feature", feature[:, :3], [7, 7, 7]) is a and len(checks) == 1
    b = encoders.cached_codes(holder, "edge_feature", feature[:, :3], [7, 7, 7])                # another field: its own entry
    assert len(checks) == 2 and b is not a
    assert encoders.cached_codes(holder, "node_feature", feature[:, :3], [7, 7, 7]) is a and len(checks) == 2


@pytest.mark.parametrize("op", sorted(IN_PLACE))
def test_cached_codes_rechecks_after_an_in_place_update(checks, op):
    from graphgym_amd import encoders
    codes = torch.arange(24).view(6, 4) % 5
    holder = types.SimpleNamespace()
    encoders.cached_codes(holder, "node_feature", codes, [30] * 4)
    old = codes.clone()
    IN_PLACE[op](codes[:, 0])
    assert not torch.equal(old, codes)
    out = encoders.cached_codes(holder, "node_feature", codes, [30] * 4)
    assert len(checks) == 2 and torch.equal(checks[1][0], codes) and torch.equal(out.long(), codes)


def test_checked_codes_lose_their_mark_on_an_in_place_update(monkeypatch):
    """ops.check_codes marks its result as checked against `dims`; ops.embed_sum skips the check for a marked tensor.  An
    in-place update after the check voids the mark (the codes could have left the tables)."""
    from graphgym_amd import ops
    monkeypatch.setattr(ops, "_require_hip", lambda t, name: None)
    codes = torch.tensor([[1, 2], [3, 0]], dtype=torch.int32)
    out = ops.check_codes(codes, [4, 4])
    assert out is codes and out._mp_checked_dims == (4, 4) and out._mp_checked_version == out._version
    out.add_(3)
    assert out._mp_checked_version != out._version
    table = torch.zeros(8, 2)
    with pytest.raises(IndexError):
        ops.embed_sum(out, table, [0, 4])                           # checked again: 6 is outside [0, 4)
