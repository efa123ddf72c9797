"""The hot-column form of the tile aggregation (mp_agg_rows_tiles_hot_f32, MP_AGG_HOT_MB): the same bits as the plain
tile kernel, the tag it reads, the gate that keeps small operators on the plain kernel, and stream capture."""
import pytest
import torch

import graphgym_amd as ga
from graphgym_amd import _lib, ops

pytestmark = pytest.mark.gpu


def graph(dev, n, E, seed, weighted, hubs):
    g = torch.Generator().manual_seed(seed)
    dst = torch.randint(0, n, (E,), generator=g)
    src = torch.randint(0, n, (E,), generator=g)
    src[: E // 4] = torch.randint(0, 40, (E // 4,), generator=g)        # a few much-used columns
    if hubs:                                                            # long rows cut between producer waves
        k = E // 3
        dst[:k] = torch.randint(0, 4, (k,), generator=g) * 1000 + 17
    keep = dst % 11 != 3                                                 # empty rows
    dst, src = dst[keep], src[keep]
    w = (torch.rand(dst.numel(), generator=g) + 0.1) if weighted else None
    G = ga.CSRGraph.from_edge_index(torch.stack([dst, src]).to(dev), n, None if w is None else w.to(dev), dst_row=0)
    return G


@pytest.fixture
def small_gate(monkeypatch):
    monkeypatch.setenv("MP_AGG_TILES", "1")
    monkeypatch.setattr(ops, "AGG_TILES_MIN_ROWS", 1)
    monkeypatch.setattr(ops, "AGG_HOT_MIN_BYTES", 1)


@pytest.mark.parametrize("d", [128, 256, 512])
@pytest.mark.parametrize("reduce,weighted,hubs,self_scale", [
    ("sum", True, True, 0.0), ("sum", False, False, 0.0), ("sum", True, False, 1.5),   # (the self term: a sum form)
    ("mean", True, True, 0.0), ("mean", False, False, 0.0),
    ("max", True, True, 0.0), ("max", False, False, 0.0)])
def test_hot_kernel_has_the_same_bits(dev, small_gate, monkeypatch, reduce, d, weighted, hubs, self_scale):
    n = 4099                                                              # a ragged last tile
    G = graph(dev, n, 60000, n + d, weighted, hubs)
    x = torch.randn(n, d, generator=torch.Generator().manual_seed(d)).to(dev)
    red = _lib.REDUCE[reduce]
    S = x if self_scale else None
    monkeypatch.setenv("MP_AGG_HOT_MB", "0")
    hot0, tiles0 = ops.AGG_HOT_CALLS, ops.AGG_TILES_CALLS
    y0, _ = ops._raw_spmm(G, x, red, S=S, self_scale=self_scale)
    assert ops.AGG_HOT_CALLS == hot0 and ops.AGG_TILES_CALLS == tiles0 + 1
    for mb in ("0.05", "1", "64"):                                       # some columns hot, most, every one
        monkeypatch.setenv("MP_AGG_HOT_MB", mb)
        y1, _ = ops._raw_spmm(G, x, red, S=S, self_scale=self_scale)
        assert torch.equal(y1, y0), mb
    assert ops.AGG_HOT_CALLS == hot0 + 3


def test_the_tag(dev, small_gate, monkeypatch):
    n, d = 3000, 256
    G = graph(dev, n, 40000, 5, True, False).gcn_norm()
    col = G.col.clone()
    x = torch.randn(n, d, device=dev)
    mb = (30 * d * 4 + 100) / (1 << 20)                                   # 30 rows of 1 KiB
    monkeypatch.setenv("MP_AGG_HOT_MB", repr(mb))
    ops._raw_spmm(G, x, _lib.SUM)
    ops._raw_spmm(G, x, _lib.MEAN)
    t = G.hot_col(int(mb * (1 << 20)), d * 4)
    assert t is not None and torch.equal(t & 0x7fffffff, G.col)
    assert torch.equal(G.col, col)                                        # g.col is never modified
    counts = torch.bincount(G.col.long(), minlength=n)
    hot = torch.zeros(n, dtype=torch.bool, device=dev)
    hot[G.col[t < 0].long()] = True
    assert int(hot.sum()) == 30                                           # the budget's rows, no more
    assert int(counts[hot].min()) >= int(counts[~hot].max())              # ... and the most used ones
    owner = getattr(G, "_pattern_of", None) or G
    assert len(owner.__dict__["_hot_col"]) == 1                           # one copy per pattern and budget


def test_below_the_gate_the_plain_kernel_runs(dev, monkeypatch):
    monkeypatch.setenv("MP_AGG_TILES", "1")
    monkeypatch.setattr(ops, "AGG_TILES_MIN_ROWS", 1)
    monkeypatch.delenv("MP_AGG_HOT_MB", raising=False)
    n, d = 3000, 256                                                      # X of 3 MB: far below AGG_HOT_MIN_BYTES
    G = graph(dev, n, 40000, 6, True, False)
    x = torch.randn(n, d, device=dev)
    hot0, tiles0 = ops.AGG_HOT_CALLS, ops.AGG_TILES_CALLS
    ops._raw_spmm(G, x, _lib.SUM)
    assert ops.AGG_TILES_CALLS == tiles0 + 1 and ops.AGG_HOT_CALLS == hot0
    assert "_hot_col" not in (getattr(G, "_pattern_of", None) or G).__dict__


def test_capture_builds_no_tag(dev, small_gate, monkeypatch):
    n, d = 3000, 256
    monkeypatch.setenv("MP_AGG_HOT_MB", "1")
    x = torch.randn(n, d, device=dev)
    for prebuilt in (False, True):
        G = graph(dev, n, 40000, 7, True, True)
        G.max_row_entries()
        y = torch.empty(n, d, device=dev)
        if prebuilt:
            ops._raw_spmm(G, x, _lib.SUM, out=y)
        eager = y.clone() if prebuilt else ops._raw_spmm(G, x, _lib.SUM)[0]
        had = "_hot_col" in G.__dict__
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops._raw_spmm(G, x, _lib.SUM, out=y)                              # (warm: a counter slot for this stream)
        torch.cuda.current_stream().wait_stream(s)
        cg = torch.cuda.CUDAGraph()
        if not prebuilt:
            G.__dict__.pop("_hot_col", None)
        before = len(G.__dict__.get("_hot_col", {}))
        with torch.cuda.graph(cg):
            ops._raw_spmm(G, x, _lib.SUM, out=y)
        assert len(G.__dict__.get("_hot_col", {})) == before                # nothing built under capture
        y.zero_()
        cg.replay()
        torch.cuda.synchronize()
        assert torch.equal(y, eager)
        assert had or prebuilt
