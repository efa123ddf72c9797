"""The edge-feature attention operators as PyTorch custom ops (torch.ops.mp.edge_att_alpha, torch.ops.mp.spmm_edge_heads
and their backward launches): registered with schemas and fake kernels (CPU suite: no device needed), torch.library.opcheck
on the GPU — as tests/test_torch_ops.py checks the other operators."""
import pytest
import torch

NAMES = ["edge_att_alpha", "edge_att_alpha_bwd_raw", "spmm_edge_heads", "spmm_edge_heads_bwd_raw"]


def test_ops_are_registered_with_schemas():
    from graphgym_amd import ops  # noqa: F401
    for n in NAMES:
        op = getattr(torch.ops.mp, n).default
        assert op._schema.name == "mp::" + n and not op._schema.is_mutable
    s = str(torch.ops.mp.edge_att_alpha.default._schema)
    assert "Tensor? a_dst" in s and "Tensor a_src" in s and "Tensor a_edge" in s and "graph" in s
    s = str(torch.ops.mp.spmm_edge_heads.default._schema)
    assert "Tensor w" in s and "Tensor x" in s and "Tensor m" in s and "Tensor? t" in s and "Tensor? bias" in s


def test_fake_kernels_give_shapes_without_a_device():
    from torch._subclasses.fake_tensor import FakeTensorMode
    from graphgym_amd import graph, ops  # noqa: F401
    g = graph.CSRGraph(torch.zeros(11, dtype=torch.int32), torch.zeros(23, dtype=torch.int32), None, None, 10, 23)
    with FakeTensorMode():
        a_n = torch.empty(10, 4, device="cuda")
        a_e = torch.empty(30, 4, device="cuda")
        al = torch.ops.mp.edge_att_alpha(a_n, a_n, a_e, g.handle, 0.2)
        assert al.shape == (23, 4) and al.dtype == torch.float32
        assert torch.ops.mp.edge_att_alpha(None, a_n, a_e, g.handle, 0.2).shape == (23, 4)
        dd, dsrc, de = torch.ops.mp.edge_att_alpha_bwd_raw(al, al, a_n, a_n, a_e, g.handle, 0.2, 7)
        assert dd.shape == (10, 4) and dsrc.shape == (10, 4) and de.shape == (30, 4)
        dd, dsrc, de = torch.ops.mp.edge_att_alpha_bwd_raw(al, al, None, a_n, a_e, g.handle, 0.2, 7)
        assert dd.numel() == 0 and dsrc.shape == (10, 4) and de.shape == (30, 4)
        dd, dsrc, de = torch.ops.mp.edge_att_alpha_bwd_raw(al, al, a_n, a_n, a_e, g.handle, 0.2, 4)
        assert dd.numel() == 0 and dsrc.numel() == 0 and de.shape == (30, 4)
        x = torch.empty(10, 64, device="cuda")
        m = torch.empty(30, 64, device="cuda")
        y, am = torch.ops.mp.spmm_edge_heads(al, x, m, x, None, g.handle, 4, 2)
        assert y.shape == (10, 64) and am.shape == (10, 64) and am.dtype == torch.int32
        y, am = torch.ops.mp.spmm_edge_heads(al, x, m, None, None, g.handle, 4, 0)
        assert y.shape == (10, 64) and y.dtype == torch.float32 and am.numel() == 0
        dw, dx, dm, dt = torch.ops.mp.spmm_edge_heads_bwd_raw(y, al, x, m, x, am, g.handle, 4, 0, 15)
        assert dw.shape == (23, 4) and dx.shape == (10, 64) and dm.shape == (30, 64) and dt.shape == (10, 64)
        dw, dx, dm, dt = torch.ops.mp.spmm_edge_heads_bwd_raw(y, al, x, m, None, am, g.handle, 4, 0, 4 | 8)
        assert dw.numel() == 0 and dx.numel() == 0 and dm.shape == (30, 64) and dt.numel() == 0


@pytest.mark.gpu
def test_opcheck(dev):
    import graphgym_amd as ga
    from graphgym_amd import ops
    gen = torch.Generator().manual_seed(0)
    n, d, H = 300, 32, 4
    ei = torch.randint(0, n, (2, 4000), generator=gen)
    g = ga.CSRGraph.from_edge_index(ei.to(dev), n)
    h = g.handle

    def t(*shape, grad=True):
        return torch.randn(*shape, generator=gen).to(dev).requires_grad_(grad)
    E = ei.size(1)
    w, x, m, tt = t(g.nnz, H, grad=False), t(n, d, grad=False), t(E, d, grad=False), t(n, d, grad=False)
    win = ops._raw_spmm_edge_heads(g, w, x, m, tt, None, H, ops._lib.MAX, True)[1]
    none = torch.empty(0, dtype=torch.int32, device=dev)
    alpha = torch.ops.mp.edge_att_alpha(None, t(n, H, grad=False), t(E, H, grad=False), h, 0.2)
    cases = [
        (torch.ops.mp.edge_att_alpha.default, (t(n, H), t(n, H), t(E, H), h, 0.2)),
        (torch.ops.mp.edge_att_alpha.default, (None, t(n, H), t(E, H), h, 0.2)),
        (torch.ops.mp.edge_att_alpha_bwd_raw.default, (t(g.nnz, H, grad=False), alpha, t(n, H, grad=False),
                                                       t(n, H, grad=False), t(E, H, grad=False), h, 0.2, 7)),
        (torch.ops.mp.edge_att_alpha_bwd_raw.default, (t(g.nnz, H, grad=False), alpha, None,
                                                       t(n, H, grad=False), t(E, H, grad=False), h, 0.2, 4)),
        (torch.ops.mp.spmm_edge_heads.default, (t(g.nnz, H), t(n, d), t(E, d), t(n, d), t(d), h, H, 0)),
        (torch.ops.mp.spmm_edge_heads.default, (t(g.nnz, H), t(n, d), t(E, d), None, None, h, H, 1)),
        (torch.ops.mp.spmm_edge_heads.default, (t(g.nnz, H), t(n, d), t(E, d), t(n, d), t(d), h, H, 2)),
        (torch.ops.mp.spmm_edge_heads.default, (t(g.nnz, 1), t(n, d), t(E, d), t(n, d), None, h, 1, 0)),
        # the other rungs of the head ladder under max (1 head) and with 3 heads (one launch per head, d = 24)
        (torch.ops.mp.spmm_edge_heads.default, (t(g.nnz, 1), t(n, d), t(E, d), t(n, d), t(d), h, 1, 2)),
        (torch.ops.mp.spmm_edge_heads.default, (t(g.nnz, 3), t(n, 24), t(E, 24), t(n, 24), t(24), h, 3, 1)),
        (torch.ops.mp.spmm_edge_heads.default, (t(g.nnz, 3), t(n, 24), t(E, 24), None, None, h, 3, 2)),
        (torch.ops.mp.spmm_edge_heads_bwd_raw.default, (t(n, d, grad=False), w, x, m, tt, none, h, H, 1, 15)),
        (torch.ops.mp.spmm_edge_heads_bwd_raw.default, (t(n, d, grad=False), w, x, m, tt, win, h, H, 2, 15)),
        (torch.ops.mp.spmm_edge_heads_bwd_raw.default, (t(n, d, grad=False), w, x, m, None, none, h, H, 0, 5)),
    ]
    for op, args in cases:
        res = torch.library.opcheck(op, args, raise_exception=True)
        assert all(v == "SUCCESS" for v in res.values()), (op, res)
