"""The path's operators as PyTorch custom ops (torch.ops.mp.*): registered with schemas and fake kernels (CPU
suite: no device needed), torch.library.opcheck on the GPU (schema, fake tensors, autograd registration, AOT
dispatch of forward + backward)."""
import pytest
import torch

NAMES = ["spmm", "idgnn_agg", "agg_dense", "agg_dense_id", "dense_fused", "bn_act",
         "spmm_raw", "spmm_rows_raw", "spmm_max_bwd_raw", "idgnn_agg_raw", "agg_dense_raw", "agg_dense_id_raw",
         "id_branch_t_raw", "dense_fused_raw", "dense_wgrad_raw", "dense_wgrad_relu_raw", "bn_fwd_raw", "bn_bwd_raw",
         "softmax_ce", "softmax_ce_rows_raw", "softmax_ce_bwd_raw"]


# every mp:: op graphgym_amd/ops.py registers, with its full schema: argument names, order, types and defaults are what
# torch.compile, export and saved graphs hold on to
SCHEMAS = {
    "spmm_raw": "mp::spmm_raw(Tensor x, SymInt graph, SymInt variant, SymInt reduce, Tensor? S, float self_scale, Tensor? bias, bool relu, bool want_argmax) -> (Tensor, Tensor)",
    "spmm_rows_raw": "mp::spmm_rows_raw(Tensor x, SymInt graph, SymInt variant, Tensor rows) -> Tensor",
    "spmm_max_bwd_raw": "mp::spmm_max_bwd_raw(Tensor dy, Tensor argmax, SymInt graph) -> Tensor",
    "idgnn_agg_raw": "mp::idgnn_agg_raw(Tensor x, SymInt graph, Tensor id_index) -> (Tensor, Tensor)",
    "agg_dense_raw": "mp::agg_dense_raw(Tensor x, Tensor W, Tensor? bias, SymInt graph, SymInt variant, SymInt reduce, Tensor? S, float self_scale, bool relu, bool want_P) -> (Tensor, Tensor)",
    "agg_dense_id_raw": "mp::agg_dense_id_raw(Tensor x, Tensor W, Tensor W_id, Tensor? bias, SymInt graph, Tensor id_index, float self_scale, bool relu, bool want_P) -> (Tensor, Tensor, Tensor)",
    "id_branch_t_raw": "mp::id_branch_t_raw(Tensor gm, SymInt graph, Tensor id_index) -> Tensor",
    "dense_fused_raw": "mp::dense_fused_raw(Tensor P, Tensor W, Tensor? Q, Tensor? W_id, Tensor? bias, bool relu) -> Tensor",
    "dense_wgrad_raw": "mp::dense_wgrad_raw(Tensor X, Tensor G, bool want_w, bool want_b) -> (Tensor, Tensor)",
    "dense_wgrad_relu_raw": "mp::dense_wgrad_relu_raw(Tensor X, Tensor G, Tensor Y, bool want_b, bool want_gm=True) -> (Tensor, Tensor, Tensor)",
    "spmm": "mp::spmm(Tensor x, SymInt graph, SymInt reduce, float self_scale, Tensor? bias, bool relu) -> (Tensor, Tensor)",
    "idgnn_agg": "mp::idgnn_agg(Tensor x, SymInt graph, Tensor id_index) -> (Tensor, Tensor)",
    "dense_fused": "mp::dense_fused(Tensor P, Tensor W, Tensor? Q, Tensor? W_id, Tensor? bias, bool relu) -> Tensor",
    "agg_dense": "mp::agg_dense(Tensor x, Tensor W, Tensor? bias, SymInt graph, SymInt reduce, float self_scale, bool relu, bool want_P) -> (Tensor, Tensor)",
    "agg_dense_id": "mp::agg_dense_id(Tensor x, Tensor W, Tensor W_id, Tensor? bias, SymInt graph, Tensor id_index, float self_scale, bool relu, bool want_P) -> (Tensor, Tensor, Tensor)",
    "spmm_edge_raw": "mp::spmm_edge_raw(Tensor x, Tensor m, Tensor? t, Tensor? bias, SymInt graph, SymInt reduce, bool want_argmax) -> (Tensor, Tensor)",
    "spmm_edge_bwd_raw": "mp::spmm_edge_bwd_raw(Tensor dy, Tensor argmax, SymInt graph, SymInt reduce, SymInt n_edges) -> Tensor",
    "spmm_edge_dt_raw": "mp::spmm_edge_dt_raw(Tensor dy, Tensor argmax, SymInt graph, SymInt reduce) -> Tensor",
    "spmm_edge": "mp::spmm_edge(Tensor x, Tensor m, Tensor? t, Tensor? bias, SymInt graph, SymInt reduce) -> (Tensor, Tensor)",
    "edge_att_alpha": "mp::edge_att_alpha(Tensor? a_dst, Tensor a_src, Tensor a_edge, SymInt graph, float slope) -> Tensor",
    "edge_att_alpha_bwd_raw": "mp::edge_att_alpha_bwd_raw(Tensor dalpha, Tensor alpha, Tensor? a_dst, Tensor a_src, Tensor a_edge, SymInt graph, float slope, SymInt want) -> (Tensor, Tensor, Tensor)",
    "spmm_edge_heads": "mp::spmm_edge_heads(Tensor w, Tensor x, Tensor m, Tensor? t, Tensor? bias, SymInt graph, SymInt heads, SymInt reduce) -> (Tensor, Tensor)",
    "spmm_edge_heads_bwd_raw": "mp::spmm_edge_heads_bwd_raw(Tensor dy, Tensor w, Tensor x, Tensor m, Tensor? t, Tensor argmax, SymInt graph, SymInt heads, SymInt reduce, SymInt want) -> (Tensor, Tensor, Tensor, Tensor)",
    "embed_sum": "mp::embed_sum(Tensor codes, Tensor table, SymInt[] offsets) -> Tensor",
    "embed_sum_bwd_raw": "mp::embed_sum_bwd_raw(Tensor dy, Tensor codes, SymInt[] offsets, SymInt n_codes, bool disjoint) -> Tensor",
    "spmm_code": "mp::spmm_code(Tensor x, Tensor table, Tensor? bias, Tensor qe, SymInt graph, SymInt reduce) -> (Tensor, Tensor)",
    "spmm_code_bwd_raw": "mp::spmm_code_bwd_raw(Tensor dy, Tensor argmax, Tensor qe, SymInt graph, SymInt reduce, SymInt n_codes) -> Tensor",
}


def test_ops_are_registered_with_schemas():
    import re
    import graphgym_amd  # noqa: F401  (importing the package registers the ops)
    from graphgym_amd import nn as _nn, ops as _ops  # noqa: F401
    for n in NAMES:
        op = getattr(torch.ops.mp, n).default
        assert op._schema.name == "mp::" + n
    s = str(torch.ops.mp.spmm.default._schema)
    assert "Tensor x" in s and "graph" in s and "Tensor? bias" in s
    assert not torch.ops.mp.spmm.default._schema.is_mutable
    with open(_ops.__file__) as f:
        registered = re.findall(r'custom_op\("mp::(\w+)"', f.read())
    assert sorted(registered) == sorted(SCHEMAS)                # the table covers every op of ops.py, and nothing else
    for n, schema in SCHEMAS.items():
        op = getattr(torch.ops.mp, n).default
        assert str(op._schema) == schema, n
        assert not op._schema.is_mutable, n


def test_fake_kernels_give_shapes_without_a_device():
    """tracing (torch.compile, export, opcheck) sees shapes and dtypes through register_fake, no kernel runs"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    from graphgym_amd import graph, nn as _nn, ops as _ops  # noqa: F401
    g = graph.CSRGraph(torch.zeros(11, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), None, None, 10, 0)
    with FakeTensorMode():
        x = torch.empty(10, 64, device="cuda")
        W = torch.empty(64, 32, device="cuda")
        Wi = torch.empty(64, 32, device="cuda")
        ids = torch.empty(3, dtype=torch.int64, device="cuda")
        y, am = torch.ops.mp.spmm(x, g.handle, 2, 0.0, None, False)
        assert y.shape == (10, 64) and am.shape == (10, 64) and am.dtype == torch.int32
        P, Q = torch.ops.mp.idgnn_agg(x, g.handle, ids)
        assert P.shape == Q.shape == (10, 64)
        out, Pk = torch.ops.mp.agg_dense(x, W, None, g.handle, 0, 1.0, True, False)
        assert out.shape == (10, 32) and Pk.numel() == 0
        out, Pk, xid = torch.ops.mp.agg_dense_id(x, W, Wi, None, g.handle, ids, 0.0, True, True)
        assert out.shape == (10, 32) and Pk.shape == (10, 64) and xid.shape == (3, 64)
        assert torch.ops.mp.dense_fused(x, W, x, Wi, None, True).shape == (10, 32)
        yb, mean, invstd, var = torch.ops.mp.bn_act(x, None, None, 1e-5, True)
        assert yb.shape == (10, 64) and mean.shape == invstd.shape == var.shape == (64,)
    with pytest.raises(Exception):
        from graphgym_amd.graph import from_handle
        from_handle(10 ** 9)                                  # a dead handle is an error, not a silent default


def test_fake_results_in_every_state():
    """every op of ops.py with a flag that decides what comes back EMPTY (an op cannot return None): shape and dtype of
    every result with the flag on and off, on an edgeless operator and on a rectangular one with entries"""
    from torch._subclasses.fake_tensor import FakeTensorMode
    from graphgym_amd import graph, ops as _ops  # noqa: F401
    f32, i32, E = torch.float32, torch.int32, (0,)
    g0 = graph.CSRGraph(torch.zeros(11, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), None, None, 10, 0)
    g1 = graph.CSRGraph(torch.zeros(11, dtype=torch.int32), torch.zeros(23, dtype=torch.int32), None, None, 10, 23,
                        num_cols=12)
    mp = torch.ops.mp

    def check(res, *expected):
        got = [(tuple(t.shape), t.dtype) for t in (res if isinstance(res, tuple) else (res,))]
        assert got == [(tuple(s), dt) for s, dt in expected], (got, expected)

    with FakeTensorMode():
        new = lambda *shape, dtype=f32: torch.empty(*shape, dtype=dtype, device="cuda")      # noqa: E731
        ids = new(3, dtype=torch.int64)
        W, Wi, b32 = new(64, 32), new(64, 32), new(32)
        for g, nc, nnz in ((g0, 10, 0), (g1, 12, 23)):
            h, x, sq, dy = g.handle, new(nc, 64), new(10, 64), new(10, 64)
            m, qe, table = new(30, 64), new(nnz, dtype=i32), new(7, 64)
            # ---- the aggregations: y [N, d] and argmax [N, d] int32 or empty (want_argmax; reduce == MAX) ---------------
            for on in (False, True):
                am = ((10, 64) if on else E, i32)
                check(mp.spmm_raw(x, h, 0, 2 if on else 0, None, 0.0, None, False, on), ((10, 64), f32), am)
                check(mp.spmm_edge_raw(x, m, None, None, h, 2, on), ((10, 64), f32), am)
            for variant in (1, 2):      # the transposed operators: one row per column
                check(mp.spmm_raw(dy, h, variant, 0, None, 0.0, None, False, False), ((nc, 64), f32), (E, i32))
                check(mp.spmm_raw(dy, h, variant, 0, None, 0.0, None, False, True), ((nc, 64), f32), ((nc, 64), i32))
            for reduce in (0, 1, 2):
                am = ((10, 64) if reduce == 2 else E, i32)
                check(mp.spmm_edge(x, m, dy, None, h, reduce), ((10, 64), f32), am)
                check(mp.spmm_code(x, table, None, qe, h, reduce), ((10, 64), f32), am)
                for heads in (1, 4):
                    check(mp.spmm_edge_heads(new(nnz, heads), x, m, None, None, h, heads, reduce), ((10, 64), f32), am)
                check(mp.spmm(x, h, reduce, 0.0, None, False), ((10, 64), f32), am)
            check(mp.spmm(x.bfloat16(), h, 2, 0.0, None, False), ((10, 64), torch.bfloat16), ((10, 64), i32))
            # ---- aggregate -> transform: out [N, d_out], the aggregated rows or empty (want_P) [, x[id]] -----------------
            for on in (False, True):
                P = ((10, 64) if on else E, f32)
                check(mp.agg_dense_raw(x, W, None, h, 0, 0, None, 0.0, True, on), ((10, 32), f32), P)
                check(mp.agg_dense_raw(dy, W, None, h, 1, 0, None, 0.0, False, on), ((nc, 32), f32),
                      ((nc, 64) if on else E, f32))
                check(mp.agg_dense(sq, W, b32, h, 1, 0.0, False, on), ((10, 32), f32), P)
                check(mp.agg_dense_id_raw(sq, W, Wi, None, h, ids, 0.0, True, on), ((10, 32), f32), P, ((3, 64), f32))
                check(mp.agg_dense_id(sq, W, Wi, None, h, ids, 1.0, False, on), ((10, 32), f32), P, ((3, 64), f32))
            check(mp.idgnn_agg_raw(x, h, ids), ((10, 64), f32), ((10, 64), f32))
            check(mp.idgnn_agg(x, h, ids), ((10, 64), f32), ((10, 64), f32))
            # ---- the want bits of the attention backward ops -----------------------------------------------------------
            H = 4
            a_dst, a_src, a_edge, alpha = new(10, H), new(nc, H), new(30, H), new(nnz, H)
            check(mp.edge_att_alpha(a_dst, a_src, a_edge, h, 0.2), ((nnz, H), f32))
            for want in (1, 2, 4, 7):
                for ad in (a_dst, None):
                    check(mp.edge_att_alpha_bwd_raw(alpha, alpha, ad, a_src, a_edge, h, 0.2, want),
                          ((10, H) if (want & 1 and ad is not None) else E, f32),
                          ((nc, H) if want & 2 else E, f32), ((30, H) if want & 4 else E, f32))
            w, am = new(nnz, H), new(10, 64, dtype=i32)
            for want in (1, 2, 4, 8, 15):
                for t in (dy, None):
                    check(mp.spmm_edge_heads_bwd_raw(dy, w, x, m, t, am, h, H, 2, want),
                          ((nnz, H) if want & 1 else E, f32), ((nc, 64) if want & 2 else E, f32),
                          ((30, 64) if want & 4 else E, f32), ((10, 64) if (want & 8 and t is not None) else E, f32))
        # ---- the weight-gradient passes ---------------------------------------------------------------------------------
        X, G = new(10, 64), new(10, 32)
        for want_w in (False, True):
            for want_b in (False, True):
                check(mp.dense_wgrad_raw(X, G, want_w, want_b), ((64, 32) if want_w else E, f32),
                      ((32,) if want_b else E, f32))
        for want_b in (False, True):
            for want_gm in (False, True):
                check(mp.dense_wgrad_relu_raw(X, G, G, want_b, want_gm), ((64, 32), f32), ((32,) if want_b else E, f32),
                      ((10, 32) if want_gm else E, f32))
            check(mp.dense_wgrad_relu_raw(X, G, G, want_b), ((64, 32), f32), ((32,) if want_b else E, f32),
                  ((10, 32), f32))


@pytest.mark.gpu
def test_opcheck(dev):
    import graphgym_amd as ga
    from graphgym_amd import nn as _nn, ops  # noqa: F401
    gen = torch.Generator().manual_seed(0)
    n, F, d = 300, 64, 32
    ei = torch.randint(0, n, (2, 4000), generator=gen)
    ei = torch.cat([ei, ei.flip(0)], 1)
    w = torch.rand(ei.size(1), generator=gen) + 0.1
    g = ga.CSRGraph.from_edge_index(ei.to(dev), n, w.to(dev))
    h = g.handle
    ids = torch.arange(0, n, 11, device=dev)

    def t(*shape, grad=True):
        return torch.randn(*shape, generator=gen).to(dev).requires_grad_(grad)
    cases = [
        (torch.ops.mp.spmm.default, (t(n, F), h, 0, 0.5, t(F), True)),
        (torch.ops.mp.spmm.default, (t(n, F), h, 1, 0.0, None, False)),
        (torch.ops.mp.spmm.default, (t(n, F), h, 2, 0.0, None, False)),
        (torch.ops.mp.idgnn_agg.default, (t(n, F), h, ids)),
        (torch.ops.mp.dense_fused.default, (t(n, F), t(F, d), t(n, F), t(F, d), t(d), True)),
        (torch.ops.mp.dense_fused.default, (t(n, F), t(F, d), None, None, None, False)),
        (torch.ops.mp.agg_dense.default, (t(n, F), t(F, d), t(d), h, 0, 1.0, True, True)),
        (torch.ops.mp.agg_dense.default, (t(n, F), t(F, d), None, h, 1, 0.0, False, True)),
        (torch.ops.mp.agg_dense_id.default, (t(n, F), t(F, d), t(F, d), t(d), h, ids, 0.0, True, True)),
        (torch.ops.mp.bn_act.default, (t(n, F), t(F), t(F), 1e-5, True)),
        (torch.ops.mp.spmm_raw.default, (t(n, F, grad=False), h, 1, 0, None, 0.0, None, False, False)),
        (torch.ops.mp.dense_wgrad_raw.default, (t(n, F, grad=False), t(n, d, grad=False), True, True)),
        (torch.ops.mp.dense_wgrad_relu_raw.default, (t(n, F, grad=False), t(n, d, grad=False),
                                                     torch.relu(t(n, d, grad=False)), True)),
        (torch.ops.mp.softmax_ce.default, (t(n, 7), torch.randint(0, 7, (n // 2,), generator=gen).to(dev),
                                           torch.randperm(n, generator=gen)[: n // 2].to(dev))),
    ]
    for op, args in cases:
        res = torch.library.opcheck(op, args, raise_exception=True)
        assert all(v == "SUCCESS" for v in res.values()), (op, res)


@pytest.mark.gpu
def test_layers_run_on_the_registered_ops(dev):
    """a layer's forward + backward dispatches torch.ops.mp.* (seen by a dispatch-mode tracer), not opaque Python"""
    import graphgym_amd as ga  # noqa: F401
    from graphgym_amd import layers as L
    from torch.utils._python_dispatch import TorchDispatchMode

    seen = set()

    class Spy(TorchDispatchMode):
        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            name = str(func)
            if name.startswith("mp."):
                seen.add(name.split(".")[1])
            return func(*args, **(kwargs or {}))

    gen = torch.Generator().manual_seed(1)
    n, F = 400, 64
    ei = torch.randint(0, n, (2, 3000), generator=gen)
    ei = torch.cat([ei, ei.flip(0)], 1).to(dev)
    x = torch.randn(n, F, generator=gen).to(dev).requires_grad_(True)
    ids = torch.arange(0, n, 9, device=dev)
    layer = L.IDGCN(F, activation=torch.relu, in_features=F).to(dev)
    with Spy():
        layer([x, ei, ids]).sum().backward()
    assert "agg_dense_id" in seen or "agg_dense_id_raw" in seen, seen
    assert ({"dense_wgrad_raw", "dense_wgrad_relu_raw"} & seen) and "agg_dense_raw" in seen, seen   # the backward formula is registered ops too
