"""Every operator family on edgeless, empty and one-element inputs (tests/_degenerate.py): a graph without edges, without
nodes, with one node, one edge, a last row alone, row degrees on the plan's hub and piece limits; widths 1 and 3; the
smallest heads; dense products of zero and one row; index sets of length 0 and 1.

The expected value is always the float64 evaluation of the family's own oracle on the same fp32 inputs (tests/_tol.py:
both, close, close_all at their defaults).  assert_close_rows returns silently on an empty tensor, so every comparison is
preceded by asserts on type, shape, dtype, device and finiteness: an empty result has the reference's shape.  Every
differentiable input requires a gradient; every .grad must be a tensor of the input's shape — zeros where nothing flows —
equal to the float64 autograd of the oracle.  Conventions of the project: max of a row without entries is 0 with argmax
-1; mean divides by max(count, 1).

A (family, case) pair is either compared or pinned with pytest.raises against the exception type of the torch reference;
the last test counts both kinds and asserts that the table was visited in full."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _att_ref as AR
import _degenerate as D
import _edgeatt_ref as EAR
import _edgeconv_ref as ER
import _ogb_ref as OR
import _skip_ref as SR
from _tol import both, close, close_all
from oracle import ref_ops as R

pytestmark = pytest.mark.gpu

POOL_CASES = ("zero-graphs", "gaps")
TABLE = {
    "graph": D.TAGS, "spmm": D.TAGS, "fused_eval": D.TAGS, "idgnn": D.TAGS, "agg_dense": D.TAGS,
    "edge_values": D.TAGS, "spmm_edge": D.TAGS, "spmm_edge_heads": D.TAGS, "spmm_code": D.TAGS,
    "pooling": POOL_CASES, "attention": D.TAGS, "fake": D.TAGS,
    "dense": tuple(f"M{m}" for m in D.DENSE_ROWS), "rows": tuple(f"n{n}" for n in D.INDEX_LENGTHS),
    "embed_sum": tuple(f"R{r}" for r in D.INDEX_LENGTHS),
    "bn": ("N2-d1",), "bn_raises": ("N0", "N1"), "dropout": ("N0",), "softmax_ce": ("empty-index",),
    "layers": tuple(f"{f}/{t}" for f in (
        "GeneralConv", "GCNConv", "SAGEConv", "GATConv", "GINConv", "GeneralIDConv", "GATIDConv", "GeneralEdgeConv",
        "GeneralSampleEdgeConv", "GeneralAddAttConv", "GeneralMulAttConv", "GeneralEdgeAttConvv1",
        "GeneralEdgeAttConvv2") for t in ("edgeless", "one-bare", "one-loop")),
}
VISITS = {}


def visit(family, case, kind="compared"):
    assert case in TABLE[family], (family, case)
    VISITS[(family, case)] = kind


def check_result(t, ref, what, dtype=torch.float32):
    """what assert_close_rows does not look at, and all it would look at on an empty tensor"""
    assert isinstance(t, torch.Tensor), (what, type(t))
    assert t.is_cuda, (what, t.device)
    assert tuple(t.shape) == tuple(ref.shape), (what, tuple(t.shape), tuple(ref.shape))
    assert t.dtype == dtype, (what, t.dtype)
    assert bool(torch.isfinite(t.float()).all()), what


def run_op(dev, what, eng, ref, ins, params=(), grads=True, positive=False):
    """eng(**device tensors) against ref(c, **cast CPU tensors), forward and backward.  ins: name -> CPU fp32 tensor, every
    one of them differentiated; params: the names compared with one scale for the tensor (weights, biases).  The
    upstream gradient is seeded by `what` and has the oracle's output shape (empty where that is empty); positive: it is
    drawn from [0.25, 1) like the operands of the long sums (tests/_degenerate.py: pos).  Returns the engine's output and
    the float64 reference."""
    names = list(ins)
    d_ins = {k: ins[k].to(dev).requires_grad_(grads) for k in names}
    out = eng(**d_ins)

    def oracle(c):
        leaves = {k: c(ins[k]).clone().requires_grad_(True) for k in names}
        o = ref(c, **leaves)
        dy = c((D.pos if positive else D.rnd)(D.gen_of(what, "dy"), *o.shape))
        gr = [torch.zeros_like(leaves[k]) for k in names]
        if o.requires_grad:
            got = torch.autograd.grad(o, [leaves[k] for k in names], dy, allow_unused=True)
            gr = [z if g is None else g for g, z in zip(got, gr)]
        return (o.detach(), dy) + tuple(gr)

    r64, r32 = both(oracle)
    check_result(out, r64[0], what)
    (close if out.dim() >= 2 else close_all)(out, (r64[0], r32[0]), what=what)
    if not grads:
        return out, r64[0]
    assert out.requires_grad, f"{what}: the result is cut off from its inputs"
    out.backward(r64[1].float().to(dev))
    for i, k in enumerate(names):
        g = d_ins[k].grad
        assert g is not None, f"{what}: d{k} is None"
        check_result(g, ins[k], f"{what} d{k}")
        cmp = close_all if (k in params or g.dim() < 2) else close
        cmp(g, (r64[2 + i], r32[2 + i]), what=f"{what} d{k}")
    return out, r64[0]


def opcheck_fake(op, args):
    """the registered fake gives the real call's shapes and dtypes (as tests/test_torch_ops.py does on ordinary inputs)"""
    res = torch.library.opcheck(op, args, test_utils=("test_faketensor",), raise_exception=True)
    assert all(v == "SUCCESS" for v in res.values()), (op, res)


def agg_ref(c, dst, src, w, x, n, reduce, self_scale=0.0, bias=None, relu=False):
    y = R.coo_aggregate(dst, src, None if w is None else c(w), x, n, reduce)
    if self_scale:
        y = y + self_scale * x
    if bias is not None:
        y = y + bias
    return torch.relu(y) if relu else y


@pytest.fixture
def ga():
    import graphgym_amd
    return graphgym_amd


# ---- graph construction --------------------------------------------------------------------------------------------
def _eq(t, a, what, dtype=torch.int32):
    assert isinstance(t, torch.Tensor) and t.is_cuda, what
    assert t.dtype == dtype, (what, t.dtype)
    assert tuple(t.shape) == tuple(a.shape), (what, tuple(t.shape), a.shape)
    assert np.array_equal(t.cpu().numpy(), a.astype(t.cpu().numpy().dtype)), what


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("tag", D.TAGS)
def test_graph_construction(dev, ga, monkeypatch, tag, weighted):
    G, dst, src, w = D.build(ga, dev, tag, weighted, monkeypatch)
    n = D.NUM_NODES[tag]
    ei = torch.stack([dst, src]).to(dev)
    wd = None if w is None else w.to(dev)
    for rm, add in ((False, False), (False, True), (True, False), (True, True)):
        what = f"{tag} w={weighted} remove={rm} add={add}"
        Gx = ga.CSRGraph.from_edge_index(ei, n, wd, dst_row=0, remove_self_loops=rm, add_self_loops=add)
        rp, col, val, eid = D.numpy_csr(dst, src, w, n, rm, add)
        assert Gx.num_nodes == n and Gx.nnz == col.size, what
        _eq(Gx.rowptr, rp, what + " rowptr")
        _eq(Gx.col, col, what + " col")
        _eq(Gx.eid, eid, what + " eid")
        assert (Gx.val is None) == (val is None), what
        if val is not None:
            _eq(Gx.val, val, what + " val", torch.float32)
    rp, col, val, eid = D.numpy_csr(dst, src, w, n)
    rows = np.repeat(np.arange(n), np.diff(rp))
    _eq(G.row_ids(), rows, f"{tag} row_ids")
    deg = np.diff(rp)
    assert G.max_row_entries() == (int(deg.max()) if n else 0)
    # plan: the segment count of the configuration in force, the hub and piece counts the degrees imply
    cfgp = D.PLAN_LIMITS if tag == "limits" else (320, 4, 1024, 256)
    counts = G.plan()[1]
    assert counts[0] == max(-(-(col.size + cfgp[1] * n) // cfgp[0]), 1), tuple(counts)
    hub = deg[deg > cfgp[2]]
    assert (counts[1], counts[2]) == (hub.size, int((-(-hub // cfgp[3])).sum())), tuple(counts)
    # from_csr on the same arrays
    Gc = ga.CSRGraph.from_csr(G.rowptr, G.col, G.val, n)
    assert Gc.nnz == col.size and Gc.num_nodes == n
    _eq(Gc.row_ids(), rows, f"{tag} from_csr row_ids")
    # the sorted transpose: rows = sources, entries of one (source, row) pair in CSR order, pos = their CSR position
    T = G._transpose_sorted()
    trp, tcol, tval, tpos = D.numpy_csr(torch.from_numpy(col), torch.from_numpy(rows),
                                        None if val is None else torch.from_numpy(val), n)
    _eq(T.rowptr, trp, f"{tag} t.rowptr")
    _eq(T.col, tcol, f"{tag} t.col")
    _eq(T.pos, tpos, f"{tag} t.pos")
    if val is not None:
        _eq(T.val, tval, f"{tag} t.val", torch.float32)
    # an operator equals its transpose when pattern and values do (an operator without entries does)
    sym = bool(np.array_equal(rp, trp) and np.array_equal(col, tcol) and (val is None or np.array_equal(val, tval)))
    assert Gc.is_symmetric(run=True) == sym, tag
    Tt = Gc.transpose()
    assert (Tt is Gc) == sym and Tt.nnz == col.size and Tt.num_nodes == n
    _eq(Tt.rowptr, trp, f"{tag} transpose().rowptr")
    _eq(Tt.col, tcol, f"{tag} transpose().col")
    # identity marks, with no and with one identity node
    for n_id in D.INDEX_LENGTHS:
        if n_id > n:
            continue
        ids = torch.arange(n - n_id, n, device=dev)
        marked = col.copy()
        marked[np.isin(col, ids.cpu().numpy())] |= -2 ** 31
        _eq(G.mark_ids(ids), marked, f"{tag} mark_ids n_id={n_id}")
    # the gcn-norm path on the operator with one inserted loop per node
    Gl = ga.CSRGraph.from_edge_index(ei, n, wd, dst_row=0, add_self_loops=True)
    Gn = Gl.gcn_norm("row")
    lrp, lcol, lval, _ = D.numpy_csr(dst, src, w, n, False, True)
    lrows = torch.from_numpy(np.repeat(np.arange(n), np.diff(lrp)))
    lv = torch.ones(lcol.size) if lval is None else torch.from_numpy(lval)

    def norm(c):
        degs = torch.zeros(n, dtype=c(lv).dtype).index_add_(0, lrows, c(lv))
        dinv = degs.pow(-0.5)
        dinv = torch.where(torch.isfinite(dinv), dinv, torch.zeros_like(dinv))
        return dinv[lrows] * c(lv) * dinv[torch.from_numpy(lcol)], dinv

    r64, r32 = both(norm)
    check_result(Gn.val, r64[0], f"{tag} gcn_norm val")
    check_result(Gn.dinv, r64[1], f"{tag} gcn_norm dinv")
    close_all(Gn.val, (r64[0], r32[0]), what=f"{tag} gcn_norm val")
    close_all(Gn.dinv, (r64[1], r32[1]), what=f"{tag} gcn_norm dinv")
    visit("graph", tag)


# ---- aggregation ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", D.TAGS)
def test_spmm(dev, ga, monkeypatch, tag):
    from graphgym_amd import ops
    n = D.NUM_NODES[tag]
    for weighted in (False, True):
        G, dst, src, w = D.build(ga, dev, tag, weighted, monkeypatch)
        for d in D.widths(tag):
            for reduce in ("sum", "mean", "max"):
                for self_scale, has_bias, relu in ((0.0, False, False), (0.5, True, True)):
                    what = f"spmm {tag} w={weighted} d={d} {reduce} s={self_scale} b={has_bias} relu={relu}"
                    gen = D.gen_of(what)
                    ins = {"x": D.pos(gen, n, d)}
                    if has_bias:
                        ins["bias"] = D.gate_bias(gen, d)
                    run_op(dev, what,
                           lambda x, bias=None: ops.spmm(G, x, reduce, self_scale=self_scale, bias=bias, relu=relu),
                           lambda c, x, bias=None: agg_ref(c, dst, src, w, x, n, reduce, self_scale, bias, relu),
                           ins, params=("bias",), positive=True)
                    # bf16: the fp32 kernel's value on the widened operand, rounded once: bit for bit
                    xb = ins["x"].to(dev).bfloat16()
                    bd = ins["bias"].to(dev) if has_bias else None
                    yb = ops.spmm(G, xb, reduce, self_scale=self_scale, bias=bd, relu=relu)
                    y32 = ops.spmm(G, xb.float(), reduce, self_scale=self_scale, bias=bd, relu=relu)
                    check_result(yb, y32, what + " bf16", torch.bfloat16)
                    assert torch.equal(yb.view(torch.int16), y32.bfloat16().view(torch.int16)), what + " bf16"
    visit("spmm", tag)


@pytest.mark.parametrize("tag", D.TAGS)
def test_spmm_fused_eval(dev, ga, monkeypatch, tag):
    from graphgym_amd import ops
    n = D.NUM_NODES[tag]
    for weighted in (False, True):
        G, dst, src, w = D.build(ga, dev, tag, weighted, monkeypatch)
        for d in D.widths(tag):
            for l2 in (False, True):
                what = f"fused_eval {tag} w={weighted} d={d} l2={l2}"
                gen = D.gen_of(what)
                x, cs, ct = D.rnd(gen, n, d), torch.rand(d, generator=gen) + 0.5, D.rnd(gen, d)

                def ref(c):
                    y = torch.relu(agg_ref(c, dst, src, w, c(x), n, "sum", 0.5) * c(cs) + c(ct))
                    return F.normalize(y, p=2, dim=-1, eps=1e-12) if l2 else y
                y = ops.spmm_fused_eval(G, x.to(dev), "sum", self_scale=0.5, col_scale=cs.to(dev), col_shift=ct.to(dev),
                                        relu=True, l2norm=l2)
                r64, r32 = both(ref)
                check_result(y, r64, what)
                close(y, (r64, r32), what=what)
            # an all-zero row normalises to zero: no self term, no shift, rows without entries
            what = f"fused_eval {tag} w={weighted} d={d} zero rows"
            x = D.rnd(D.gen_of(what), n, d)
            y = ops.spmm_fused_eval(G, x.to(dev), "sum", l2norm=True)
            r64, r32 = both(lambda c: F.normalize(agg_ref(c, dst, src, w, c(x), n, "sum"), p=2, dim=-1, eps=1e-12))
            check_result(y, r64, what)
            close(y, (r64, r32), what=what)
    visit("fused_eval", tag)


@pytest.mark.parametrize("tag", D.TAGS)
def test_idgnn_aggregate(dev, ga, monkeypatch, tag):
    from graphgym_amd import ops
    n = D.NUM_NODES[tag]
    for weighted in (False, True):
        G, dst, src, w = D.build(ga, dev, tag, weighted, monkeypatch)
        for d in D.widths(tag):
            for n_id in D.INDEX_LENGTHS:
                if n_id > n:
                    continue
                what = f"idgnn {tag} w={weighted} d={d} n_id={n_id}"
                ids = torch.arange(n - n_id, n)
                sel = torch.zeros(n, 1)
                sel[ids] = 1
                idd = ids.to(dev)
                ins = {"x": D.pos(D.gen_of(what), n, d)}
                # (P, Q) side by side, so that one upstream gradient reaches both
                run_op(dev, what, lambda x: torch.cat(ops.idgnn_aggregate(G, idd, x), 1),
                       lambda c, x: torch.cat([agg_ref(c, dst, src, w, x, n, "sum"),
                                               agg_ref(c, dst, src, w, x * c(sel), n, "sum")], 1), ins, positive=True)
    visit("idgnn", tag)


@pytest.mark.parametrize("tag", D.TAGS)
def test_agg_dense_and_sage_concat(dev, ga, monkeypatch, tag):
    """the one-kernel layer's operators: at widths 1 and 3 they take their documented two-kernel order, at 64 (limits) the
    one kernel; agg_dense_id returns None outside the one kernel (its contract), and then the pair it stands for runs"""
    from graphgym_amd import ops
    n = D.NUM_NODES[tag]
    for weighted in (False, True):
        G, dst, src, w = D.build(ga, dev, tag, weighted, monkeypatch)
        for d in D.widths(tag):
            k = 2 if d < 64 else 32
            for reduce, self_scale, relu in (("sum", 1.0, True), ("mean", 0.0, False)):
                what = f"agg_dense {tag} w={weighted} d={d} {reduce}"
                gen = D.gen_of(what)
                ins = {"x": D.pos(gen, n, d), "W": D.pos(gen, d, k) / 4, "bias": D.gate_bias(gen, k)}
                run_op(dev, what,
                       lambda x, W, bias: ops.agg_dense(G, x, W, bias=bias, relu=relu, self_scale=self_scale,
                                                        reduce=reduce),
                       lambda c, x, W, bias: (lambda y: torch.relu(y) if relu else y)(
                           agg_ref(c, dst, src, w, x, n, reduce, self_scale) @ W + bias),
                       ins, params=("W", "bias"), positive=True)
            # the operator's backward runs on the transposed operator: there is no max form, and it says so
            with pytest.raises(ValueError, match="max"):
                ops.agg_dense(G, torch.zeros(n, d, device=dev), torch.zeros(d, k, device=dev), reduce="max")
            what = f"sage_concat {tag} w={weighted} d={d}"
            gen = D.gen_of(what)
            ins = {"x": D.pos(gen, n, d), "Ws": D.pos(gen, d, k) / 4, "Wn": D.pos(gen, d, k) / 4,
                   "bias": D.gate_bias(gen, 2 * k)}
            run_op(dev, what, lambda x, Ws, Wn, bias: ops.sage_concat(G, x, Ws, Wn, bias=bias, relu=True),
                   lambda c, x, Ws, Wn, bias: torch.relu(
                       torch.cat([x @ Ws, agg_ref(c, dst, src, w, x, n, "mean") @ Wn], 1) + bias),
                   ins, params=("Ws", "Wn", "bias"), positive=True)
            for n_id in D.INDEX_LENGTHS:
                if n_id > n:
                    continue
                what = f"agg_dense_id {tag} w={weighted} d={d} n_id={n_id}"
                gen = D.gen_of(what)
                ids = torch.arange(n - n_id, n)
                sel = torch.zeros(n, 1)
                sel[ids] = 1
                idd = ids.to(dev)
                ins = {"x": D.pos(gen, n, d), "W": D.pos(gen, d, k) / 4, "W_id": D.pos(gen, d, k) / 4,
                       "bias": D.gate_bias(gen, k)}

                def eng(x, W, W_id, bias):
                    y = ops.agg_dense_id(G, x, W, W_id, idd, bias=bias, relu=True)
                    if y is None:
                        assert not ops.agg_dense_supported(G, x, W), what
                        P, Q = ops.idgnn_aggregate(G, idd, x)
                        y = ops.dense_fused(P, W, Q, W_id, bias=bias, relu=True)
                    return y
                run_op(dev, what, eng,
                       lambda c, x, W, W_id, bias: torch.relu(
                           agg_ref(c, dst, src, w, x @ W + (x * c(sel)) @ W_id, n, "sum") + bias),
                       ins, params=("W", "W_id", "bias"), positive=True)
    visit("agg_dense", tag)


@pytest.mark.parametrize("tag", D.TAGS)
def test_spmm_edge_values(dev, ga, monkeypatch, tag):
    from graphgym_amd import ops
    n = D.NUM_NODES[tag]
    G, dst, src, _ = D.build(ga, dev, tag, False, monkeypatch)
    rows, cols, _, _ = D.csr_lists(G)
    for H, d in D.HEAD_SHAPES:
        for reduce in ("sum", "mean", "max"):
            what = f"edge_values {tag} H={H} d={d} {reduce}"
            gen = D.gen_of(what)
            ins = {"a": torch.rand(G.nnz, H, generator=gen) + 0.25, "V": D.rnd(gen, n, d)}
            run_op(dev, what, lambda a, V: ops.spmm_edge_values(G, a, V, heads=H, reduce=reduce),
                   lambda c, a, V: AR.edge_values_agg(rows, cols, a, V, n, H, reduce), ins)
    visit("edge_values", tag)


def _edge_inputs(gen, G, n, E, d, with_t, with_bias):
    ins = {"x": D.rnd(gen, n, d), "m": D.rnd(gen, E, d)}
    if with_t:
        ins["t"] = D.rnd(gen, n, d)
    if with_bias:
        ins["bias"] = D.rnd(gen, d)
    return ins


@pytest.mark.parametrize("tag", D.TAGS)
def test_spmm_edge(dev, ga, monkeypatch, tag):
    from graphgym_amd import ops
    n = D.NUM_NODES[tag]
    for weighted in (False, True):
        # with inserted loops too: entries without an input edge (eid < 0) read and drop row 0 of m
        for loops in (False, True):
            G, dst, src, w = D.build(ga, dev, tag, weighted, monkeypatch, **({"add_self_loops": True} if loops else {}))
            rows, cols, eids, val = D.csr_lists(G)
            for d in D.widths(tag):
                for reduce in ("sum", "mean", "max"):
                    for with_t, with_bias in ((False, False), (True, True)):
                        what = f"spmm_edge {tag} w={weighted} loops={loops} d={d} {reduce} t={with_t}"
                        ins = _edge_inputs(D.gen_of(what), G, n, dst.numel(), d, with_t, with_bias)
                        run_op(dev, what,
                               lambda x, m, t=None, bias=None: ops.spmm_edge(G, x, m, reduce, t=t, bias=bias),
                               lambda c, x, m, t=None, bias=None: ER.edge_agg(
                                   rows, cols, eids, None if val is None else c(val), x, m, t, bias, n, reduce),
                               ins, params=("bias",))
    visit("spmm_edge", tag)


@pytest.mark.parametrize("tag", D.TAGS)
def test_spmm_edge_heads(dev, ga, monkeypatch, tag):
    from graphgym_amd import ops
    n = D.NUM_NODES[tag]
    for loops in (False, True):
        G, dst, src, _ = D.build(ga, dev, tag, False, monkeypatch, **({"add_self_loops": True} if loops else {}))
        rows, cols, eids, _ = D.csr_lists(G)
        for H, d in D.HEAD_SHAPES:
            for reduce in ("sum", "mean", "max"):
                for with_t, with_bias in ((False, False), (True, True)):
                    what = f"spmm_edge_heads {tag} loops={loops} H={H} d={d} {reduce} t={with_t}"
                    gen = D.gen_of(what)
                    ins = {"w": torch.rand(G.nnz, H, generator=gen) + 0.25}
                    ins.update(_edge_inputs(gen, G, n, dst.numel(), d, with_t, with_bias))
                    run_op(dev, what,
                           lambda w, x, m, t=None, bias=None: ops.spmm_edge_heads(G, w, x, m, t=t, heads=H,
                                                                                  reduce=reduce, bias=bias),
                           lambda c, w, x, m, t=None, bias=None: EAR.edge_heads_agg(rows, cols, eids, w, x, m, t, bias, n,
                                                                                    H, reduce),
                           ins, params=("bias",))
    visit("spmm_edge_heads", tag)


@pytest.mark.parametrize("tag", D.TAGS)
def test_spmm_code(dev, ga, monkeypatch, tag):
    from graphgym_amd import ops
    n, C = D.NUM_NODES[tag], 5
    for weighted in (False, True):
        G, dst, src, w = D.build(ga, dev, tag, weighted, monkeypatch)
        rows, cols, eids, val = D.csr_lists(G)
        codes = torch.randint(0, C, (dst.numel(),), generator=D.gen_of(tag, "codes")).to(torch.int32)
        q = codes.long()[eids]
        cd = codes.to(dev)
        for d in D.widths(tag):
            for reduce in ("sum", "mean", "max"):
                what = f"spmm_code {tag} w={weighted} d={d} {reduce}"
                gen = D.gen_of(what)
                ins = {"x": D.rnd(gen, n, d), "table": D.rnd(gen, C, d), "bias": D.rnd(gen, d)}
                run_op(dev, what, lambda x, table, bias: ops.spmm_code(G, x, table, cd, reduce, bias=bias),
                       lambda c, x, table, bias: OR.spmm_code(rows, cols, q, None if val is None else c(val), x, table,
                                                              bias, n, reduce),
                       ins, params=("table", "bias"))
    visit("spmm_code", tag)


@pytest.mark.parametrize("case", POOL_CASES)
def test_pooling(dev, case):
    """zero graphs (no node either), and a batch whose first, middle and last graph has no node"""
    from graphgym_amd import pooling
    batch, size = (torch.zeros(0, dtype=torch.int64), 0) if case == "zero-graphs" else (torch.tensor([1, 1, 3]), 5)
    nn_ = batch.numel()
    nodes = torch.arange(nn_)
    for d in D.WIDTHS:
        for name, reduce in (("add", "sum"), ("mean", "mean"), ("max", "max")):
            what = f"pool {case} d={d} {name}"
            ins = {"x": D.rnd(D.gen_of(what), nn_, d)}
            run_op(dev, what, lambda x: pooling.pooling_dict[name](x, batch.to(dev), size=size),
                   lambda c, x: R.coo_aggregate(batch, nodes, None, x, size, reduce), ins)
    visit("pooling", case)


# ---- attention pieces -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", D.TAGS)
def test_attention_pieces(dev, ga, monkeypatch, tag):
    from graphgym_amd import ops
    n = D.NUM_NODES[tag]
    G, dst, src, _ = D.build(ga, dev, tag, False, monkeypatch)
    rows, cols, eids, _ = D.csr_lists(G)
    E = dst.numel()
    for H, d in D.HEAD_SHAPES:
        dh = d // H
        what = f"sddmm_dot {tag} H={H} d={d}"
        gen = D.gen_of(what)
        run_op(dev, what, lambda Q, K: ops.sddmm_dot(G, Q, K, heads=H, scale=0.5),
               lambda c, Q, K: 0.5 * (Q[rows].view(-1, H, dh) * K[cols].view(-1, H, dh)).sum(-1),
               {"Q": D.rnd(gen, n, d), "K": D.rnd(gen, n, d)})
        what = f"gat_alpha {tag} H={H}"
        gen = D.gen_of(what)
        run_op(dev, what, lambda a_dst, a_src: ops.gat_alpha(G, a_dst, a_src, 0.2),
               lambda c, a_dst, a_src: AR.segment_softmax(F.leaky_relu(a_dst[rows] + a_src[cols], 0.2), rows, n),
               {"a_dst": D.rnd(gen, n, H), "a_src": D.rnd(gen, n, H)})
        for with_dst in (True, False):
            what = f"edge_att_alpha {tag} H={H} dst={with_dst}"
            gen = D.gen_of(what)
            ins = {"a_src": D.rnd(gen, n, H), "a_edge": D.rnd(gen, E, H)}
            if with_dst:
                ins["a_dst"] = D.rnd(gen, n, H)
            run_op(dev, what, lambda a_src, a_edge, a_dst=None: ops.edge_att_alpha(G, a_dst, a_src, a_edge, 0.2),
                   lambda c, a_src, a_edge, a_dst=None: EAR.edge_att_alpha(rows, cols, eids, a_dst, a_src, a_edge, n,
                                                                           0.2), ins)
        what = f"edge_softmax {tag} H={H}"
        run_op(dev, what, lambda s: ops.edge_softmax(G, s), lambda c, s: AR.segment_softmax(s, rows, n),
               {"s": D.rnd(D.gen_of(what), G.nnz, H) * 3})
    what = f"sddmm_add {tag}"
    gen = D.gen_of(what)
    run_op(dev, what, lambda ai, aj: ops.sddmm_add(G, ai, aj, 0.2),
           lambda c, ai, aj: F.leaky_relu(ai[rows] + aj[cols], 0.2).view(-1, 1),
           {"ai": D.rnd(gen, n), "aj": D.rnd(gen, n)})
    visit("attention", tag)


# ---- dense ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M", D.DENSE_ROWS)
def test_dense(dev, M):
    """dense_fused with and without the second branch, concat_dense and nn.Linear at zero rows and one row: at M = 0 the
    result is [0, d] and every weight and bias gradient is zeros of the parameter's shape"""
    from graphgym_amd import nn as mnn, ops
    for Fi, d in ((1, 1), (3, 2), (8, 4)):
        for relu in (False, True):
            for second in (False, True):
                for has_bias in (False, True):
                    what = f"dense_fused M={M} F={Fi} d={d} relu={relu} second={second} bias={has_bias}"
                    gen = D.gen_of(what)
                    ins = {"P": D.rnd(gen, M, Fi), "W": D.rnd(gen, Fi, d)}
                    if second:
                        ins.update(Q=D.rnd(gen, M, Fi), W_id=D.rnd(gen, Fi, d))
                    if has_bias:
                        ins["bias"] = D.rnd(gen, d)

                    def ref(c, P, W, Q=None, W_id=None, bias=None):
                        y = P @ W
                        y = y if Q is None else y + Q @ W_id
                        y = y if bias is None else y + bias
                        return torch.relu(y) if relu else y
                    run_op(dev, what, lambda P, W, Q=None, W_id=None, bias=None: ops.dense_fused(P, W, Q, W_id, bias, relu),
                           ref, ins, params=("W", "W_id", "bias"))
            what = f"concat_dense M={M} F={Fi} d={d} relu={relu}"
            gen = D.gen_of(what)
            ins = {"x": D.rnd(gen, M, Fi), "m": D.rnd(gen, M, Fi), "Ws": D.rnd(gen, Fi, d), "Wn": D.rnd(gen, Fi, d),
                   "bias": D.rnd(gen, 2 * d)}
            run_op(dev, what, lambda x, m, Ws, Wn, bias: ops.concat_dense(x, m, Ws, Wn, bias, relu=relu),
                   lambda c, x, m, Ws, Wn, bias: (lambda y: torch.relu(y) if relu else y)(
                       torch.cat([x @ Ws, m @ Wn], 1) + bias),
                   ins, params=("Ws", "Wn", "bias"))
            what = f"Linear M={M} F={Fi} d={d} relu={relu}"
            gen = D.gen_of(what)
            lin = mnn.Linear(Fi, d, bias=True, relu=relu).to(dev)
            ins = {"x": D.rnd(gen, M, Fi), "weight": D.rnd(gen, d, Fi), "bias": D.rnd(gen, d)}

            run_op(dev, what, lambda x, weight, bias: _linear_through(lin, x, weight, bias),
                   lambda c, x, weight, bias: (lambda y: torch.relu(y) if relu else y)(F.linear(x, weight, bias)),
                   ins, params=("weight", "bias"))
    visit("dense", f"M{M}")


def _linear_through(lin, x, weight, bias):
    """the module's forward with the given leaves as its parameters (torch.func.functional_call): gradients reach them"""
    return torch.func.functional_call(lin, {"weight": weight, "bias": bias}, (x,))


# ---- rows and codes -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_idx", D.INDEX_LENGTHS)
def test_rows(dev, n_idx):
    from graphgym_amd import ops
    n = 5
    ids = torch.tensor([3][:n_idx], dtype=torch.int64)
    idd = ids.to(dev)
    for d in D.WIDTHS:
        what = f"gather_rows n={n_idx} d={d}"
        run_op(dev, what, lambda x: ops.gather_rows(x, idd), lambda c, x: x[ids], {"x": D.rnd(D.gen_of(what), n, d)})
        what = f"index_add_rows n={n_idx} d={d}"
        gen = D.gen_of(what)
        run_op(dev, what, lambda h, u: ops.index_add_rows(h, idd, u), lambda c, h, u: h.index_add(0, ids, u),
               {"h": D.rnd(gen, n, d), "u": D.rnd(gen, n_idx, d)})
        # the same on a source without rows at all
        if n_idx == 0:
            what = f"gather_rows from nothing d={d}"
            run_op(dev, what, lambda x: ops.gather_rows(x, idd), lambda c, x: x[ids], {"x": D.rnd(D.gen_of(what), 0, d)})
    visit("rows", f"n{n_idx}")


@pytest.mark.parametrize("n_rows", D.INDEX_LENGTHS)
def test_embed_sum(dev, n_rows):
    from graphgym_amd import ops
    dims = (3, 2)
    offsets = [0, 3]
    gen = D.gen_of("embed_sum codes", n_rows)
    codes = torch.stack([torch.randint(0, k, (n_rows,), generator=gen) for k in dims], 1)
    cd = codes.to(dev)
    for d in D.WIDTHS:
        what = f"embed_sum R={n_rows} d={d}"
        run_op(dev, what, lambda table: ops.embed_sum(cd, table, offsets),
               lambda c, table: OR.encode(codes, [table[:3], table[3:]]),
               {"table": D.rnd(D.gen_of(what), sum(dims), d)}, params=("table",))
    visit("embed_sum", f"R{n_rows}")


# ---- step ops -------------------------------------------------------------------------------------------------------
def test_bn_at_two_rows(dev):
    """the BatchNorm passes at N = 2, the smallest size that stays on the engine (its pivot reads rows 0, N / 2, N - 1),
    and d = 1: bn_act, the fused activation, both skip forms and the keyed dropout behind each"""
    import torch.nn as tnn
    from graphgym_amd import nn as mnn
    N, d, eps = 2, 1, 1e-5
    P = lambda w, b: {"bn.weight": w, "bn.bias": b}      # noqa: E731

    for relu in (False, True):
        what = f"bn_act N=2 d=1 relu={relu}"
        gen = D.gen_of(what)
        ins = {"x": D.rnd(gen, N, d), "w": torch.rand(d, generator=gen) + 0.5, "b": D.rnd(gen, d)}
        run_op(dev, what, lambda x, w, b: torch.ops.mp.bn_act(x, w, b, eps, relu)[0],
               lambda c, x, w, b: (torch.relu if relu else (lambda y: y))(SR._bn(x, P(w, b), "bn", eps)),
               ins, params=("w", "b"))
    p = 0.25
    for act in (tnn.ReLU(), tnn.LeakyReLU(0.1), tnn.ELU(), None):
        for with_drop in (False, True):
            if act is None and not with_drop:
                continue
            what = f"bn_act_module N=2 d=1 act={type(act).__name__} drop={with_drop}"
            gen = D.gen_of(what)
            ins = {"x": D.rnd(gen, N, d), "w": torch.rand(d, generator=gen) + 0.5, "b": D.rnd(gen, d)}
            bn = mnn.BatchNorm1d(d, eps=eps).to(dev).train()
            drop = mnn.Dropout(p, seed=D.seed_of(what)).train() if with_drop else None
            keep = mnn.dropout_keep_host(drop.seed, 0, N, d, p) if with_drop else None

            def eng(x, w, b):
                if drop is not None:
                    drop.set_stream(drop.seed, 0)
                return torch.func.functional_call(
                    _BnAct(bn, act, drop), {"bn.weight": w, "bn.bias": b}, (x,))

            def ref(c, x, w, b):
                y = SR._bn(x, P(w, b), "bn", eps)
                if keep is not None:
                    y = y * c(keep.float()) * mnn.dropout_scale(p)
                return y if act is None else act(y)
            run_op(dev, what, eng, ref, ins, params=("w", "b"))
    for mode in ("skipsum", "skipconcat"):
        for with_drop in (False, True):
            for relu in (False, True):
                what = f"bn_skip_act N=2 d=1 {mode} drop={with_drop} relu={relu}"
                gen = D.gen_of(what)
                ins = {"x": D.rnd(gen, N, d), "skip": D.rnd(gen, N, d), "w": torch.rand(d, generator=gen) + 0.5,
                       "b": D.rnd(gen, d)}
                bn = mnn.BatchNorm1d(d, eps=eps).to(dev).train()
                drop = mnn.Dropout(p, seed=D.seed_of(what)).train() if with_drop else None
                keep = mnn.dropout_keep_host(drop.seed, 0, N, d, p) if with_drop else None

                def eng(x, skip, w, b):
                    if drop is not None:
                        drop.set_stream(drop.seed, 0)
                    return torch.func.functional_call(_BnSkip(bn, mode, relu, drop), {"bn.weight": w, "bn.bias": b},
                                                      (x, skip))

                def ref(c, x, skip, w, b):
                    y = SR._bn(x, P(w, b), "bn", eps)
                    if keep is not None:
                        y = y * c(keep.float()) * mnn.dropout_scale(p)
                    z = skip + y if mode == "skipsum" else torch.cat((skip, y), 1)
                    return torch.relu(z) if relu else z
                run_op(dev, what, eng, ref, ins, params=("w", "b"))
    x = D.rnd(D.gen_of("bn fake"), N, d).to(dev)
    opcheck_fake(torch.ops.mp.bn_act.default, (x, torch.ones(d, device=dev), torch.zeros(d, device=dev), eps, True))
    visit("bn", "N2-d1")


class _BnAct(torch.nn.Module):
    def __init__(self, bn, act, drop):
        super().__init__()
        self.bn, self.act, self.drop = bn, act, drop

    def forward(self, x):
        from graphgym_amd import nn as mnn
        return mnn.bn_act_module(self.bn, x, self.act, self.drop)


class _BnSkip(torch.nn.Module):
    def __init__(self, bn, mode, relu, drop):
        super().__init__()
        self.bn, self.mode, self.relu, self.drop = bn, mode, relu, drop

    def forward(self, x, skip):
        from graphgym_amd import nn as mnn
        return mnn.bn_skip_act(self.bn, x, skip, self.mode, relu=self.relu, drop=self.drop)


@pytest.mark.parametrize("N", [0, 1])
def test_batchnorm_does_what_torch_does_below_two_rows(dev, N):
    """nn.BatchNorm1d in training mode on zero rows or one row never reaches the engine: it raises what
    torch.nn.BatchNorm1d raises (one row: "Expected more than 1 value per channel") and, where torch raises nothing (no
    row), returns what torch returns, an empty [0, d]"""
    from graphgym_amd import nn as mnn
    x = torch.zeros(N, 3)
    try:
        want = torch.nn.BatchNorm1d(3).train()(x)
    except Exception as e:      # noqa: BLE001  (whatever torch raises is what is pinned)
        with pytest.raises(type(e)):
            torch.nn.BatchNorm1d(3).train()(x)
        for relu in (False, True):
            with pytest.raises(type(e)):
                mnn.BatchNorm1d(3, relu=relu).to(dev).train()(x.to(dev))
        visit("bn_raises", f"N{N}", "raised")
        return
    for relu in (False, True):
        got = mnn.BatchNorm1d(3, relu=relu).to(dev).train()(x.to(dev).requires_grad_(True))
        check_result(got, want, f"BatchNorm1d N={N} relu={relu}")
        assert got.requires_grad
    visit("bn_raises", f"N{N}")


def test_dropout_of_nothing(dev):
    from graphgym_amd import nn as mnn
    for d in D.WIDTHS:
        what = f"dropout N=0 d={d}"
        drop = mnn.Dropout(0.5, seed=7).train()
        run_op(dev, what, lambda x: drop(x), lambda c, x: x * 2.0, {"x": torch.zeros(0, d)})
        run_op(dev, what + " op", lambda x: torch.ops.mp.dropout_keyed(x, 32768, 7, 0), lambda c, x: x * 2.0,
               {"x": torch.zeros(0, d)})
        opcheck_fake(torch.ops.mp.dropout_keyed.default, (torch.zeros(0, d, device=dev), 32768, 7, 0))
    visit("dropout", "N0")


def test_softmax_ce_with_an_empty_index(dev):
    """torch.ops.mp.softmax_ce with no labelled row: the value is what F.cross_entropy(logits[index], labels,
    reduction="mean") gives on the CPU in float64 — its NaN included — and the gradient is zeros of the logits' shape"""
    from graphgym_amd import nn as mnn  # noqa: F401
    n, C = 5, 3
    z = D.rnd(D.gen_of("ce"), n, C)
    idx = torch.zeros(0, dtype=torch.int64)
    y = torch.zeros(0, dtype=torch.int64)
    zr = z.double().requires_grad_(True)
    want = F.cross_entropy(zr[idx], y, reduction="mean")
    want.backward()
    zd = z.to(dev).requires_grad_(True)
    got = torch.ops.mp.softmax_ce(zd, y.to(dev), idx.to(dev))
    assert got.is_cuda and got.shape == want.shape and got.dtype == torch.float32
    assert torch.allclose(got.cpu().double(), want.detach(), rtol=0, atol=0, equal_nan=True), (got, want)
    got.backward()
    assert zd.grad is not None and zd.grad.shape == z.shape and zd.grad.dtype == torch.float32
    assert torch.allclose(zd.grad.cpu().double(), zr.grad, rtol=0, atol=0, equal_nan=True), (zd.grad, zr.grad)
    assert float(zr.grad.abs().max()) == 0.0
    opcheck_fake(torch.ops.mp.softmax_ce.default, (z.to(dev), y.to(dev), idx.to(dev)))
    visit("softmax_ce", "empty-index")


# ---- layers ---------------------------------------------------------------------------------------------------------
LAYER_TAGS = ("edgeless", "one-bare", "one-loop")
LAYER_FAMILIES = ("GeneralConv", "GCNConv", "SAGEConv", "GATConv", "GINConv", "GeneralIDConv", "GATIDConv",
                  "GeneralEdgeConv", "GeneralSampleEdgeConv", "GeneralAddAttConv", "GeneralMulAttConv",
                  "GeneralEdgeAttConvv1", "GeneralEdgeAttConvv2")
FI, DO, EDIM = 4, 4, 2


def _layer_case(family, n, ei, ids):
    """(module, args after x as a function of the extra inputs, extra inputs' shapes, oracle(x, extra, p), parameters
    left out of the comparison) of one layer family on the edges ei [2, E] = (source, destination)"""
    import types
    from graphgym_amd import attconv, edgeattconv, edgeconv, layers as L
    from graphgym_amd.config import cfg
    from oracle import ref_layers as RL
    E = ei.size(1)
    ef = {"ef": (E, EDIM)}
    if family == "GeneralConv":
        return (L.GeneralConvLayer(FI, DO, bias=True), lambda e: ((ei,), {}), {},
                lambda x, e, p: RL.general_conv(x, ei, p["weight"], p["weight_self"], p["bias"], "add"), ())
    if family == "GCNConv":
        return (L.GCNConvLayer(FI, DO, bias=True, order="transform_first"), lambda e: ((ei,), {}), {},
                lambda x, e, p: RL.pyg_gcn_conv(x, ei, p["weight"], p["bias"]), ())
    if family == "SAGEConv":
        return (L.SAGEConvLayer(FI, DO, bias=True), lambda e: ((ei,), {}), {},
                lambda x, e, p: RL.pyg_sage_conv(x, ei, p["lin_l.weight"], p["lin_l.bias"], p["lin_r.weight"]), ())
    if family == "GATConv":
        return (L.GATConvLayer(FI, DO, bias=True), lambda e: ((ei,), {}), {},
                lambda x, e, p: RL.pyg_gat_conv(x, ei, p["lin_l.weight"].t(), p["att_r"].view(1, -1),
                                                p["att_l"].view(1, -1), p["bias"]), ())
    if family == "GINConv":
        mlp = torch.nn.Sequential(torch.nn.Linear(FI, DO), torch.nn.ReLU(), torch.nn.Linear(DO, DO))
        return (L.GINConvLayer(mlp), lambda e: ((ei,), {}), {},
                lambda x, e, p: RL.pyg_gin_conv(x, ei, lambda h: torch.relu(
                    h @ p["nn.0.weight"].t() + p["nn.0.bias"]) @ p["nn.2.weight"].t() + p["nn.2.bias"]), ())
    if family == "GeneralIDConv":
        return (L.GeneralIDConvLayer(FI, DO, bias=True, order="transform_first"), lambda e: ((ei, ids), {}), {},
                lambda x, e, p: RL.generalid_conv(x, ei, ids, p["weight"], p["weight_id"], p["bias"], "add"), ())
    if family == "GATIDConv":
        return (L.GATIDConvLayer(FI, DO, bias=True), lambda e: ((ei, ids), {}), {},
                lambda x, e, p: RL.gatid_conv(x, ei, ids, p["weight"], p["weight_id"], p["att"], p["bias"]), ())
    if family == "GeneralEdgeConv":
        return (edgeconv.GeneralEdgeConvLayer(FI, DO, bias=True), lambda e: ((ei,), {"edge_feature": e["ef"]}), ef,
                lambda x, e, p: ER.edge_conv(x, e["ef"], ei, None, p["linear_msg.weight"], p["linear_self.weight"],
                                             p["bias"], "both", "concat", "add"), ())
    if family == "GeneralSampleEdgeConv":
        # the batch-level module: keep_edge = 0 drops every edge of the batch (the layer then sees an edgeless graph)
        class Sampled(torch.nn.Module):
            def __init__(self):
                super().__init__()
                self.inner = edgeconv.GeneralSampleEdgeConv(FI, DO, bias=True)

            def forward(self, x, edge_feature):
                batch = types.SimpleNamespace(node_feature=x, edge_index=ei, edge_feature=edge_feature)
                return self.inner(batch).node_feature
        none = ei[:, :0]
        assert cfg.gnn.keep_edge == 0.0
        return (Sampled(), lambda e: ((e["ef"],), {}), ef,
                lambda x, e, p: ER.edge_conv(x, e["ef"][:0], none, None, p["inner.model.linear_msg.weight"],
                                             p["inner.model.linear_self.weight"], p["inner.model.bias"], "both",
                                             "concat", "add"), ())
    if family in ("GeneralAddAttConv", "GeneralMulAttConv"):
        kind = "add" if family == "GeneralAddAttConv" else "mul"
        cls = attconv.GeneralAddAttConvLayer if kind == "add" else attconv.GeneralMulAttConvLayer
        heads = int(cfg.gnn.att_heads)
        return (cls(FI, DO, bias=True), lambda e: ((ei,), {}), {},
                lambda x, e, p: AR.att_conv(kind, x, p["linear_msg.weight"], p.get("att"), p.get("bias_att"), p["bias"],
                                            ei, None, heads, "add")[0], ())
    version = 1 if family == "GeneralEdgeAttConvv1" else 2
    cls = edgeattconv.GeneralEdgeAttConvv1Layer if version == 1 else edgeattconv.GeneralEdgeAttConvv2Layer
    return (cls(FI, DO, bias=True), lambda e: ((ei,), {"edge_feature": e["ef"]}), ef,
            lambda x, e, p: EAR.edge_att_conv(x, e["ef"], ei, None, p, version, int(cfg.gnn.att_heads), "add", "both"),
            ("linear_key.weight", "linear_key.bias"))          # (v2's key transform takes no part in the forward)


@pytest.mark.parametrize("tag", LAYER_TAGS)
@pytest.mark.parametrize("family", LAYER_FAMILIES)
def test_layers(dev, monkeypatch, family, tag):
    """one module of every layer family, one forward and one backward, on a graph without edges, on one bare node and on
    one node with a loop; parameters from a seed; outputs and gradients against the family's own oracle"""
    from graphgym_amd.config import cfg
    for name, v in (("agg", "add"), ("normalize_adj", False), ("self_msg", "concat"), ("msg_direction", "both"),
                    ("att_heads", 1 if family == "GeneralMulAttConv" else 2), ("keep_edge", 0.0)):
        monkeypatch.setattr(cfg.gnn, name, v)
    monkeypatch.setattr(cfg.dataset, "edge_dim", EDIM)
    n = D.NUM_NODES[tag]
    dst, src = D.edges(tag)
    ei = torch.stack([src, dst])                                # source -> destination, PyG's flow
    ids = torch.tensor([n - 1])
    what = f"layer {family} {tag}"
    layer, call, extra, _, unused = _layer_case(family, n, ei.to(dev), ids.to(dev))     # (the oracle keeps CPU edges)
    layer = layer.to(dev).train()
    ref_of = _layer_case(family, n, ei, ids)[3]
    gen = D.gen_of(what)
    pnames = [k for k, _ in layer.named_parameters() if not k.endswith(unused or ("\0",))]
    ins = {"x": D.rnd(gen, n, FI)}
    ins.update({k: D.rnd(gen, *shape) for k, shape in extra.items()})
    ins.update({k: D.rnd(gen, *dict(layer.named_parameters())[k].shape) / 2 for k in pnames})

    def eng(x, **kw):
        args, kwargs = call(kw)
        return torch.func.functional_call(layer, {k: kw[k] for k in pnames}, (x,) + args, kwargs)

    run_op(dev, what, eng, lambda c, x, **kw: ref_of(x, kw, kw), ins, params=tuple(pnames))
    visit("layers", f"{family}/{tag}")


# ---- the registered fakes on the degenerate inputs ------------------------------------------------------------------
@pytest.mark.parametrize("tag", D.TAGS)
def test_fake_kernels_on_degenerate_inputs(dev, ga, monkeypatch, tag):
    """torch.library.opcheck(test_faketensor): the registered fake returns the real call's shapes and dtypes"""
    from graphgym_amd import nn as mnn, ops  # noqa: F401
    n, d, H = D.NUM_NODES[tag], 4, 2
    G, dst, src, w = D.build(ga, dev, tag, True, monkeypatch)
    h, E = G.handle, dst.numel()
    gen = D.gen_of("fake", tag)
    t = lambda *s: D.rnd(gen, *s).to(dev)      # noqa: E731
    n_id = min(n, 1)
    ids = torch.arange(n - n_id, n, device=dev)
    codes = torch.randint(0, 3, (E,), generator=gen).to(torch.int32).to(dev)
    qe = ops.entry_codes(G, codes)[0]
    cases = [
        (torch.ops.mp.spmm.default, (t(n, d), h, 0, 0.5, t(d), True)),
        (torch.ops.mp.spmm.default, (t(n, d), h, 1, 0.0, None, False)),
        (torch.ops.mp.spmm.default, (t(n, d), h, 2, 0.0, None, False)),
        (torch.ops.mp.idgnn_agg.default, (t(n, d), h, ids)),
        (torch.ops.mp.agg_dense.default, (t(n, d), t(d, 2), t(2), h, 0, 1.0, True, True)),
        (torch.ops.mp.spmm_edge.default, (t(n, d), t(E, d), t(n, d), t(d), h, 0)),
        (torch.ops.mp.spmm_edge.default, (t(n, d), t(E, d), None, None, h, 2)),
        (torch.ops.mp.edge_att_alpha.default, (t(n, H), t(n, H), t(E, H), h, 0.2)),
        (torch.ops.mp.spmm_edge_heads.default, (torch.rand(G.nnz, H, generator=gen).to(dev), t(n, d), t(E, d), t(n, d),
                                                t(d), h, H, 0)),
        (torch.ops.mp.spmm_edge_heads.default, (torch.rand(G.nnz, H, generator=gen).to(dev), t(n, d), t(E, d), None, None,
                                                h, H, 2)),
        (torch.ops.mp.spmm_code.default, (t(n, d), t(3, d), t(d), qe, h, 0)),
        (torch.ops.mp.spmm_code.default, (t(n, d), t(3, d), None, qe, h, 2)),
        (torch.ops.mp.dense_fused.default, (t(min(n, 1), d), t(d, 2), t(min(n, 1), d), t(d, 2), t(2), True)),
        (torch.ops.mp.embed_sum.default, (torch.zeros(min(n, 1), 2, dtype=torch.int32, device=dev), t(5, d), [0, 3])),
    ]
    for op, args in cases:
        opcheck_fake(op, args)
    visit("fake", tag)


def test_zz_every_pair_was_visited():
    """no (family, case) pair skipped, xfailed or filtered out: each was compared or pinned with pytest.raises"""
    want = {(f, c) for f, cases in TABLE.items() for c in cases}
    missing = sorted(want - set(VISITS))
    assert not missing, f"{len(missing)} (family, case) pairs were not visited: {missing}"
    kinds = {k: sum(1 for v in VISITS.values() if v == k) for k in ("compared", "raised")}
    assert kinds["compared"] + kinds["raised"] == len(want) and 1 <= kinds["raised"] <= len(TABLE["bn_raises"]), kinds
