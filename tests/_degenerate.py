"""The degenerate inputs of tests/test_degenerate_gpu.py, once: graphs without edges, without nodes, with one node, rows
whose degree sits on the plan's hub and piece limits; the widths, head shapes, dense row counts and index-set lengths
used with them.  Everything comes from seeded generators; an empty tensor's values are simply empty.

Every graph is built with CSRGraph.from_edge_index(..., dst_row=0): edge_index[0] = destination (the CSR row),
edge_index[1] = source (the column).

    tag        nodes  edges
    null         0    none
    one-bare     1    none
    one-loop     1    (0, 0)
    edgeless     5    none
    one-edge     5    3 -> 1
    last-row    70    3 edges, all into row 69
    limits       8    row degrees 0, 63, 64, 65, 127, 128, 129, 1; sources uniform over the 8 nodes (repeats allowed);
                      built under PLAN_CONFIG = (64, 1, 64, 64): hub_deg = 64, piece_edges = 64

What an (operator family, case) pair does on the device, found by reading each wrapper and entry point before the first
run.  R = returns before any launch, Z = launches and loops zero times over the empty extent, E = reads an element that
must exist (and does exist):

    graph construction   null, one-bare, edgeless: mp_csr_from_coo, mp_csr_transpose memset rowptr and return (R for the
                         sort); mp_csr_row_ids, mp_csr_is_symmetric, mp_csr_scale_f32, mp_mark_id_sources R at nnz = 0;
                         mp_spmm_plan_build launches its header and segment kernels, whose binary search over rowptr reads
                         nothing at N = 0 (Z); mp_gcn_norm_edges launches the row-degree kernel over N rows of no entries
                         (Z) and is R at N = 0.  The other cases are ordinary small builds.
    aggregation          (spmm, fused_eval, idgnn, agg_dense, sage_concat, pooling)  null: agg_common R at N = 0.
                         one-bare, edgeless: one wave per segment walks its rows, the entry walk runs zero times (col, val
                         are never read: Z) and every row is flushed through the epilogue, which reads S[row] and bias (E:
                         both exist).  last-row: 69 rows flushed empty, then one row.  limits: the hub pieces and the
                         finalize kernel.  The backward runs the same kernel on the transposed operator (same classes);
                         max backward: mp_spmm_max_bwd_f32 reads col[e] only for argmax >= 0 — the wrapper returns zeros at
                         nnz = 0 (R).  An operator without COLUMNS (the per-edge operator of an edgeless graph; the
                         transposed operator of an empty index set has no ROWS instead and is R) gets a one-row X that
                         nothing reads (Z).
    edge aggregation     (spmm_edge, spmm_edge_heads, spmm_code, spmm_edge_values)  the kernels read row 0 of m for an
                         inserted loop, so m always has a row (E); at nnz = 0 the wrappers return before any launch (R)
                         with y = bias and argmax = -1, because col / eid / the head weights have no address.
    attention pieces     sddmm_dot, sddmm_add, gat_alpha, edge_att_alpha: R at nnz = 0 or N = 0 inside the entry point;
                         edge_softmax and its backward: R in the wrapper (the entry point cannot see nnz).
    dense                M = 0: R inside mp_dense_fused_f32 / the weight-gradient entries (memset of dW, db); M = 1: one
                         block, rows beyond M masked (E: row 0).
    rows and codes       n = 0 / R = 0: R inside the entry points; the table gradient at R = 0 is zeros from the wrapper.
    step ops             BatchNorm at N = 2 reads rows 0, N / 2 = 1 and N - 1 = 1 for its pivot (E: they exist); N < 2 never
                         reaches the engine (torch's own error).  dropout_keyed R at N = 0.  softmax_ce R at n_sel = 0.
"""
import numpy as np
import torch

PLAN_LIMITS = (64, 1, 64, 64)                 # {seg_cost, row_cost, hub_deg, piece_edges} of the `limits` case
LIMIT_DEGREES = (0, 63, 64, 65, 127, 128, 129, 1)

TAGS = ("null", "one-bare", "one-loop", "edgeless", "one-edge", "last-row", "limits")
NUM_NODES = {"null": 0, "one-bare": 1, "one-loop": 1, "edgeless": 5, "one-edge": 5, "last-row": 70, "limits": 8}

WIDTHS = (1, 3)                               # plus 64 for `limits` only
HEAD_SHAPES = ((1, 1), (2, 2), (3, 3), (4, 8))    # (H, d): dh = 1 is the smallest head, H = 3 takes the per-head fallback
DENSE_ROWS = (0, 1)
INDEX_LENGTHS = (0, 1)


def widths(tag):
    return WIDTHS + ((64,) if tag == "limits" else ())


def seed_of(*key):
    """a generator seed from a key of strings / ints (stable across processes, unlike hash())"""
    s = 0
    for k in key:
        for ch in str(k):
            s = (s * 131 + ord(ch)) % (2 ** 31 - 1)
        s = (s * 131 + 7) % (2 ** 31 - 1)
    return s


def gen_of(*key):
    return torch.Generator().manual_seed(seed_of(*key))


def rnd(gen, *shape):
    """uniform in [-1, 1); an empty shape gives an empty tensor"""
    return torch.rand(*shape, generator=gen) * 2 - 1


def pos(gen, *shape):
    """uniform in [0.25, 1): the operands (and upstream gradients) of the families whose outputs are long sums — spmm,
    idgnn_aggregate, agg_dense, sage_concat on the 129-entry rows of `limits`, at width 1 where a row is one number.
    The tests hold every row to 1e-5 of its own magnitude; a sequential fp32 sum of n terms is only good to n * 2^-24 of
    the sum of their ABSOLUTE values, so a signed sum that cancels to a hundredth of its terms cannot meet that bar in any
    arithmetic.  With terms of one sign the two coincide and n * 2^-24 = 7.7e-6 at n = 129 stays inside the bar."""
    return torch.rand(*shape, generator=gen) * 0.75 + 0.25


def gate_bias(gen, d):
    """a bias for those families that keeps ReLU at work without cancellation: -20 on every third column (below any
    pre-activation of a row of fewer than about 30 entries, so that short rows are cut to exactly zero and the 63- to
    129-entry rows of `limits` pass with half their magnitude left), pos() elsewhere"""
    b = pos(gen, d)
    b[::3] = -20.0
    return b


def edges(tag):
    """(dst, src) int64 [E] of a case, in input order"""
    if tag in ("null", "one-bare", "edgeless"):
        return torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64)
    if tag == "one-loop":
        return torch.tensor([0]), torch.tensor([0])
    if tag == "one-edge":
        return torch.tensor([1]), torch.tensor([3])                     # 3 -> 1
    if tag == "last-row":
        return torch.tensor([69, 69, 69]), torch.tensor([0, 35, 69])
    if tag == "limits":
        gen = gen_of("limits-edges")
        dst = torch.repeat_interleave(torch.arange(8), torch.tensor(LIMIT_DEGREES))
        src = torch.randint(0, 8, (dst.numel(),), generator=gen)
        perm = torch.randperm(dst.numel(), generator=gen)              # input order is not row order
        return dst[perm], src[perm]
    raise KeyError(tag)


def weights(tag):
    """positive entry values [E] of a case's weighted form"""
    return torch.rand(edges(tag)[0].numel(), generator=gen_of(tag, "weights")) + 0.5


def numpy_csr(dst, src, w, n, remove_self_loops=False, add_self_loops=False, fill=1.0):
    """(rowptr [n + 1], col, val or None, eid) as the engine stores them: rows ascending, inside a row columns
    ascending, entries of one (row, column) in input order; an inserted loop has eid -1 - node and value `fill`"""
    dst, src = dst.numpy().astype(np.int64), src.numpy().astype(np.int64)
    eid = np.arange(dst.size, dtype=np.int64)
    val = None if w is None else w.numpy().astype(np.float32)
    if remove_self_loops:
        keep = dst != src
        dst, src, eid = dst[keep], src[keep], eid[keep]
        val = None if val is None else val[keep]
    if add_self_loops:
        loop = np.arange(n, dtype=np.int64)
        dst, src, eid = np.concatenate([dst, loop]), np.concatenate([src, loop]), np.concatenate([eid, -1 - loop])
        if val is not None or fill != 1.0:
            val = np.concatenate([np.ones(dst.size - n, np.float32) if val is None else val,
                                  np.full(n, fill, np.float32)])
    order = np.lexsort((np.arange(dst.size), src, dst))     # stable: (row, column, position)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(dst, minlength=n)[:n], out=rowptr[1:])
    return rowptr, src[order], None if val is None else val[order], eid[order]


def expected_plan_counts(tag):
    """(hub rows, hub pieces) the degrees of a case imply under PLAN_LIMITS: a row of more than hub_deg entries is a hub,
    cut into ceil(deg / piece_edges) pieces"""
    dst = edges(tag)[0]
    deg = np.bincount(dst.numpy(), minlength=max(NUM_NODES[tag], 1))
    hub = deg[deg > PLAN_LIMITS[2]]
    return int(hub.size), int(((hub + PLAN_LIMITS[3] - 1) // PLAN_LIMITS[3]).sum())


def build(ga, dev, tag, weighted, monkeypatch=None, **kw):
    """(G, dst, src, w or None) of a case on the device; `limits` needs the monkeypatch fixture (PLAN_CONFIG) and has its
    hub and piece counts asserted: otherwise the case is not the one it claims to be"""
    dst, src = edges(tag)
    w = weights(tag) if weighted else None
    n = NUM_NODES[tag]
    if tag == "limits":
        assert monkeypatch is not None, "the limits case is built under PLAN_CONFIG"
        monkeypatch.setattr(ga.CSRGraph, "PLAN_CONFIG", PLAN_LIMITS)
    G = ga.CSRGraph.from_edge_index(torch.stack([dst, src]).to(dev), n, None if w is None else w.to(dev), dst_row=0, **kw)
    if tag == "limits" and not kw:
        counts = G.plan()[1]
        assert (counts[1], counts[2]) == expected_plan_counts(tag) == (4, 9), tuple(counts)
        assert (counts[6], counts[7]) == PLAN_LIMITS[2:]
    return G, dst, src, w


def csr_lists(G):
    """(rows, cols, eids, val or None) of the stored entries on the CPU, int64 / fp32"""
    rows = G.row_ids().cpu().long()
    return rows, G.col.cpu().long(), G.eid.cpu().long(), None if G.val is None else G.val.cpu()
