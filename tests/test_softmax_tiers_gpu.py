"""The row softmax's three tiers (attn.hip: one lane per row up to 16 entries, a 16-lane group up to 2048, the whole
workgroup beyond) with rows ON the boundaries between them, through the three operators that run on that body:
ops.edge_softmax, ops.gat_alpha, ops.edge_att_alpha.  One workgroup holds all 64 rows; more than 16 of them are medium, so
its 16 groups work the medium queue off in two passes; a lane of a group keeps its first four trips (64 entries) in
registers, so 63 / 64 / 65 is a boundary too.  Against the float64 / float32 references of the other attention tests at
the tolerances of tests/_tol.py; every row sums to one; a second call gives the same bits."""
import pytest
import torch

import _edgeatt_ref as EA
from _tol import both, close
from oracle import ref_ops as R

pytestmark = pytest.mark.gpu

N = 64
# entries per row.  The boundaries and their neighbours, each also one below: the graph with inserted self loops has one
# entry more in every row
EDGE = [0, 1, 14, 15, 16, 17, 62, 63, 64, 65, 80, 2046, 2047, 2048, 2049, 4100]
MEDIUM = [20, 33, 48, 100, 129, 200, 256, 300, 400]
COUNTS = EDGE + MEDIUM + [(5 * i) % 17 for i in range(N - len(EDGE) - len(MEDIUM))]


def _edges(seed=0):
    """[2, E] source -> destination without self loops, row r with COUNTS[perm[r]] entries, in a shuffled input order"""
    g = torch.Generator().manual_seed(seed)
    counts = torch.tensor(COUNTS)[torch.randperm(N, generator=g)]
    dst = torch.repeat_interleave(torch.arange(N), counts)
    src = torch.randint(0, N - 1, (dst.numel(),), generator=g)
    src = src + (src >= dst).long()
    ei = torch.stack([src, dst])
    return ei[:, torch.randperm(ei.size(1), generator=g)], counts


@pytest.fixture(scope="module")
def tiers(dev):
    """(graph, graph with a self loop inserted into every row, the input edges)"""
    import graphgym_amd as ga
    ei, counts = _edges()
    assert 14_000 <= ei.size(1) <= 16_000
    g = ga.CSRGraph.from_edge_index(ei.to(dev), N)
    gl = ga.CSRGraph.from_edge_index(ei.to(dev), N, add_self_loops=True)
    deg, degl = torch.diff(g.rowptr.cpu()).long(), torch.diff(gl.rowptr.cpu()).long()
    assert torch.equal(deg, counts) and torch.equal(degl, counts + 1)
    want = {0, 1, 15, 16, 17, 63, 64, 65, 80, 2047, 2048, 2049, 4100}
    assert want <= set(deg.tolist()) and want - {0, 80, 4100} <= set(degl.tolist())
    for d in (deg, degl):
        assert int(((d > 16) & (d <= 2048)).sum()) >= 17 and int((d > 2048).sum()) >= 2
    assert int((gl.eid < 0).sum()) == N and int((g.eid < 0).sum()) == 0
    return g, gl, ei


def _softmax_terms(alpha64, dl64, rows):
    """|alpha_e| (|dalpha_e| + sum_row |alpha dalpha|): the absolute terms of a softmax row's gradient (tests/_tol.py
    rule (d), as test_parity_gpu.test_row_softmax_with_hub_rows)"""
    rowdot = torch.zeros(N, alpha64.size(1), dtype=torch.float64).index_add_(0, rows, (alpha64 * dl64).abs())
    return alpha64.abs() * (dl64.abs() + rowdot[rows])


def _rows_sum_to_one(p, rows, what):
    sums = torch.zeros(N, p.size(1), dtype=torch.float64).index_add_(0, rows, p.detach().cpu().double())
    has = torch.bincount(rows, minlength=N) > 0
    assert float((sums[has] - 1.0).abs().max()) <= 1e-5, what


@pytest.mark.parametrize("heads", [1, 3])
def test_edge_softmax_on_tier_boundaries(dev, tiers, heads):
    from graphgym_amd import ops
    G = tiers[0]
    rows = G.row_ids().cpu().long()
    gen = torch.Generator().manual_seed(70 + heads)
    s = torch.randn(G.nnz, heads, generator=gen) * 3
    up = torch.randn(G.nnz, heads, generator=gen)
    sg = s.to(dev).requires_grad_(True)
    p = ops.edge_softmax(G, sg)
    p.backward(up.to(dev))

    def ref(c):
        sr = c(s).clone().requires_grad_(True)
        pr = R.softmax(sr, rows, N)
        pr.backward(c(up))
        return pr.detach(), sr.grad
    r64, r32 = both(ref)
    what = f"tier boundaries: edge_softmax H={heads}"
    close(p, (r64[0], r32[0]), what=what)
    close(sg.grad, (r64[1], r32[1]), what=what + " backward", mag=_softmax_terms(r64[0], up.double(), rows))
    _rows_sum_to_one(p, rows, what)
    assert torch.equal(p.detach(), ops.edge_softmax(G, sg.detach())), what


@pytest.mark.parametrize("heads", [1, 4])
def test_gat_alpha_on_tier_boundaries(dev, tiers, heads):
    from graphgym_amd import ops
    G = tiers[0]
    rows, cols = G.row_ids().cpu().long(), G.col.cpu().long()
    gen = torch.Generator().manual_seed(80 + heads)
    a_dst, a_src = torch.randn(N, heads, generator=gen), torch.randn(N, heads, generator=gen)
    dal = torch.randn(G.nnz, heads, generator=gen)
    adg, asg = a_dst.to(dev).requires_grad_(True), a_src.to(dev).requires_grad_(True)
    alpha = ops.gat_alpha(G, adg, asg, 0.2)
    alpha.backward(dal.to(dev))

    def ref(c):
        adr, asr = c(a_dst).clone().requires_grad_(True), c(a_src).clone().requires_grad_(True)
        r = R.softmax(torch.nn.functional.leaky_relu(adr[rows] + asr[cols], 0.2), rows, N)
        r.backward(c(dal))
        return r.detach(), adr.grad, asr.grad
    r64, r32 = both(ref)
    what = f"tier boundaries: gat_alpha H={heads}"
    close(alpha, (r64[0], r32[0]), what=what)
    terms = _softmax_terms(r64[0], dal.double(), rows)
    zero = torch.zeros(N, heads, dtype=torch.float64)
    close(adg.grad, (r64[1], r32[1]), what=what + " d_dst",
          mag=torch.maximum(zero.index_add(0, rows, terms), r64[1].abs()))
    close(asg.grad, (r64[2], r32[2]), what=what + " d_src",
          mag=torch.maximum(zero.index_add(0, cols, terms), r64[2].abs()))
    _rows_sum_to_one(alpha, rows, what)
    assert torch.equal(alpha.detach(), ops.gat_alpha(G, adg.detach(), asg.detach(), 0.2)), what


@pytest.mark.parametrize("has_dst", [True, False], ids=["dst", "nodst"])
def test_edge_att_alpha_on_tier_boundaries(dev, tiers, has_dst):
    from graphgym_amd import ops
    _, G, ei = tiers
    heads, E = 2, ei.size(1)
    rows, cols, eids = G.row_ids().cpu().long(), G.col.cpu().long(), G.eid.cpu().long()
    gen = torch.Generator().manual_seed(90 + has_dst)
    a_dst = torch.randn(N, heads, generator=gen) if has_dst else None
    a_src, a_edge = torch.randn(N, heads, generator=gen), torch.randn(E, heads, generator=gen)
    dal = torch.randn(G.nnz, heads, generator=gen)
    leaf_dev = lambda t: None if t is None else t.to(dev).requires_grad_(True)      # noqa: E731
    dd, sd, ed = leaf_dev(a_dst), leaf_dev(a_src), leaf_dev(a_edge)
    alpha = ops.edge_att_alpha(G, dd, sd, ed, 0.2)
    alpha.backward(dal.to(dev))

    def ref(c):
        leaf = lambda t: None if t is None else c(t).detach().clone().requires_grad_(True)    # noqa: E731
        ad, asr, ae = leaf(a_dst), leaf(a_src), leaf(a_edge)
        al = EA.edge_att_alpha(rows, cols, eids, ad, asr, ae, N, 0.2)
        al.backward(c(dal))
        return [al.detach(), asr.grad, ae.grad] + ([ad.grad] if ad is not None else [])
    r64, r32 = both(ref)
    what = f"tier boundaries: edge_att_alpha dst={has_dst}"
    close(alpha, (r64[0], r32[0]), what=what)
    terms = _softmax_terms(r64[0], dal.double(), rows)
    zero = torch.zeros(N, heads, dtype=torch.float64)
    has = eids >= 0
    mag_e = torch.zeros(E, heads, dtype=torch.float64)
    mag_e[eids[has]] = terms[has]
    close(sd.grad, (r64[1], r32[1]), what=what + " d_src", mag=zero.index_add(0, cols, terms))
    close(ed.grad, (r64[2], r32[2]), what=what + " d_edge", mag=mag_e)
    if has_dst:
        close(dd.grad, (r64[3], r32[3]), what=what + " d_dst", mag=zero.index_add(0, rows, terms))
    _rows_sum_to_one(alpha, rows, what)
    again = ops.edge_att_alpha(G, None if dd is None else dd.detach(), sd.detach(), ed.detach(), 0.2)
    assert torch.equal(alpha.detach(), again), what
