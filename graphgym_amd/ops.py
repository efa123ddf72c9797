"""Differentiable operators over CSRGraph on the C-ABI entry points of libmpengine.so (include/mp_engine.h).

Three layers, in the order of the file: launchers (`_raw_*` and their kin: one per entry point or ladder of entry points;
they choose the kernel form, allocate the outputs and own the stand-ins for arrays without an address; tests and
benchmarks reach them by name), the `torch.autograd.Function` classes of the attention pieces and the concatenating
transforms, and the registered operators `torch.ops.mp.*`: `*_raw` ops without autograd around the launchers, and the
un-suffixed ops whose backward formulas are built from `*_raw` ops.  What the op families share (results and fake
kernels, the `want` bits, the gradient by source, the setup_context, the bias gradient, the wrappers' checks) is written
once under "what the registered operators share"; the per-head backward stands before `_SpmmEdgeValues`.

    spmm(g, x, reduce)           SparseAdj.matmul (sparse_adj.py:91-97); PyG propagate
    idgnn_aggregate(g, id, x)    two-branch form of gcn_id (TfgIDLayer.py:510-517)
    index_add_rows(h, id, u)     tensor_scatter_nd_add / index_add_ (K10)
    edge_softmax / sddmm_*       GAT pieces (TfgIDLayer.py:333-355; idconv.py:317-332)
    spmm_edge(g, x, m, reduce)   aggregation of messages with an edge feature (generalconv.py:203-209)
    edge_att_alpha / spmm_edge_heads   attention over messages with an edge feature (attconv.py:342-360)
    embed_sum(codes, table, offsets)   rows of stacked embedding tables summed per item (feature_encoder.py:74-81)
    spmm_code(g, x, table, codes, reduce)   aggregation of messages with a coded edge term (generalconv_ogb.py:115-118)
    spline_agg / spline_fold(g, w, x)    one gather into two weighted sums, and its adjoint (SplineConv, layer.py:177-186)
    pair_score / pair_sum(.., index)     the link-prediction head's pair decodings without a [K, d] tensor (head.py:62-85)
"""
import ctypes as C
import os

import torch

from . import _lib, placement
from ._lib import check, lib, ptr
from .graph import CSRGraph, _require_hip, _stream, tensor_stamp


# ---- the deterministic switch ----------------------------------------------------------------------
# The backwards that scatter with float atomics (max through the argmax, gather_rows / index_add_rows with repeated
# ids, the cross-entropy over a repeated index, the by-node sums of the attention scores) have a second form without
# them: a gather over an inverted index on the aggregation kernel, the same bits every run.  The choice is made here,
# where the backward is dispatched, never inside a kernel; with the switch off every op launches what it always did.
def _env_deterministic():
    v = os.environ.get("MP_DETERMINISTIC")
    if v is None or v == "":
        return None
    if v not in ("0", "1"):
        raise ValueError(f"MP_DETERMINISTIC must be 0 or 1, got {v!r}")
    return v == "1"


_DETERMINISTIC = _env_deterministic()       # None: follow torch.are_deterministic_algorithms_enabled()


def set_deterministic(mode):
    """True / False: the engine's reproducible backward forms on / off, whatever torch's flag says; None (the default,
    unless MP_DETERMINISTIC=0|1 was set at import): follow torch.use_deterministic_algorithms (warn_only or not)"""
    global _DETERMINISTIC
    if mode is not None and not isinstance(mode, bool):
        raise TypeError(f"set_deterministic takes True, False or None, got {mode!r}")
    _DETERMINISTIC = mode


def deterministic():
    """do the backward passes run their atomics-free forms?"""
    return torch.are_deterministic_algorithms_enabled() if _DETERMINISTIC is None else _DETERMINISTIC


def _f32c(t, name):
    _require_hip(t, name)
    if t.dtype != torch.float32:
        raise TypeError(f"{name} must be float32 (the path aggregates in fp32), got {t.dtype}")
    return t if t.stride(-1) == 1 and t.dim() == 2 else t.contiguous()


def _agg_in(t, name):
    """an operand of the aggregation: float32, or bfloat16 (stored as bf16, aggregated in fp32); rows unit-stride"""
    _require_hip(t, name)
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(f"{name} must be float32 or bfloat16 (the path aggregates in fp32), got {t.dtype}")
    return t if t.stride(-1) == 1 and t.dim() == 2 else t.contiguous()


def _plan_ws(g, device, d, reduce, two_branch):
    """the plan of g and the workspace a plan-based aggregation of width d needs: (plan, counts, ws, ws_bytes)"""
    plan, counts = g.plan()
    nb = C.c_size_t(0)
    check(lib().mp_spmm_ws_bytes(counts, d, reduce, 1 if two_branch else 0, C.byref(nb)))
    ws = torch.empty(nb.value, dtype=torch.uint8, device=device) if nb.value else None
    return plan, counts, ws, nb.value


def _raw_spmm(g, x, reduce, S=None, self_scale=0.0, bias=None, relu=False, want_argmax=False,
              col_override=None, out=None):
    """one launch of mp_spmm_csr_f32 — or, for plain sum / mean / max (values only, no argmax) at d = 128 / 256 / 512 on
    a large operator, of mp_agg_rows_tiles_f32 (the same aggregation on the producer/consumer tile structure: 2-5 %
    faster; MP_AGG_TILES=0 keeps the plan-based kernel; for an X of >= AGG_HOT_MIN_BYTES its hot-column form,
    mp_agg_rows_tiles_hot_f32: _hot_col) —; x [n_src, d] -> y [N, d] (written into `out` when given).  A bf16 x goes
    to mp_spmm_csr_bf16: bf16 x, S and y, fp32 accumulation, bias passed as fp32; every output is that of
    mp_spmm_csr_f32 on x.float() with the same plan, rounded once to bf16.  The tile kernels have no bf16 form."""
    L = lib()
    N, d = g.num_nodes, x.size(1)
    if x.size(0) == 0 and N > 0 and g.nnz == 0:
        # an operator without columns (and so without entries): nothing reads X, the entry point — which cannot see the
        # column count — wants an address; the rows still get their self term, bias and activation
        x = x.new_zeros((1, d))
    y = out if out is not None else placement.empty_or_torch((N, d), x.device, reads=(x,), dtype=x.dtype)
    if (x.dtype == torch.float32 and reduce in (_lib.SUM, _lib.MEAN, _lib.MAX) and d in AGG_TILES_WIDTHS
            and N >= AGG_TILES_MIN_ROWS and bias is None
            and not relu and not want_argmax and col_override is None and not (reduce != _lib.SUM and S is not None)
            and os.environ.get("MP_AGG_TILES", "1") != "0"
            and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 and y.stride(0) % 4 == 0 and y.data_ptr() % 16 == 0
            and (S is None or (S.stride(0) % 4 == 0 and S.data_ptr() % 16 == 0))
            and g.nnz > 0 and g.max_row_entries() <= FUSED_MAX_ROW):
        global AGG_TILES_CALLS, AGG_HOT_CALLS
        AGG_TILES_CALLS += 1
        col_hot = _hot_col(g, x)
        with torch.cuda.device(x.device):
            if col_hot is not None:
                AGG_HOT_CALLS += 1
                check(L.mp_agg_rows_tiles_hot_f32(ptr(g.rowptr), ptr(col_hot), ptr(g.val), N, reduce, ptr(x), x.stride(0),
                                                  d, ptr(S), S.stride(0) if S is not None else 0, float(self_scale),
                                                  ptr(y), y.stride(0), _stream()), "mp_agg_rows_tiles_hot_f32")
            else:
                check(L.mp_agg_rows_tiles_f32(ptr(g.rowptr), ptr(g.col), ptr(g.val), N, reduce, ptr(x), x.stride(0), d,
                                              ptr(S), S.stride(0) if S is not None else 0, float(self_scale),
                                              ptr(y), y.stride(0), _stream()), "mp_agg_rows_tiles_f32")
        return y, None
    if x.dtype == torch.bfloat16:
        name = "mp_spmm_csr_bf16"
        if S is not None:
            S = S.to(torch.bfloat16)
        if bias is not None:
            bias = bias.detach().to(torch.float32).contiguous()
    else:
        name = "mp_spmm_csr_f32"
    argmax = torch.empty((N, d), dtype=torch.int32, device=x.device) if want_argmax else None
    plan, counts, ws, ws_bytes = _plan_ws(g, x.device, d, reduce, False)
    with torch.cuda.device(x.device):
        col = g.col if col_override is None else col_override
        check(getattr(L, name)(ptr(g.rowptr), ptr(col), ptr(g.val), N, ptr(plan), counts,
                               ptr(x), x.stride(0), ptr(y), y.stride(0), d, reduce,
                               ptr(S), S.stride(0) if S is not None else 0, float(self_scale),
                               ptr(bias), _lib.ACT_RELU if relu else _lib.ACT_NONE, ptr(argmax),
                               ptr(ws), ws_bytes, _stream()), name)
    return y, argmax


# (spmm: registered operator mp::spmm, below)


def spmm_fused_eval(g, x, reduce="sum", self_scale=0.0, col_scale=None, col_shift=None, relu=False,
                    l2norm=False, l2_eps=1e-12):
    """Inference-only aggregation with the layer's post-ops folded into the row flush:
    act((agg + self_scale * x) * col_scale + col_shift), then optional row L2 normalisation
    (graphgym/models/layer.py:26-47, gnn.py:79-80 with BatchNorm in eval mode).  No autograd."""
    x = _f32c(x.detach(), "x")
    L = lib()
    N, d = g.num_nodes, x.size(1)
    y = torch.empty((N, d), dtype=torch.float32, device=x.device)
    red = _lib.REDUCE[reduce]
    plan, counts, ws, ws_bytes = _plan_ws(g, x.device, d, red, False)
    S = x if self_scale != 0.0 else None
    with torch.cuda.device(x.device):
        cs = None if col_scale is None else col_scale.detach().contiguous()
        ct = None if col_shift is None else col_shift.detach().contiguous()
        st = L.mp_spmm_csr_epilogue_f32(ptr(g.rowptr), ptr(g.col), ptr(g.val), N, ptr(plan), counts, ptr(x),
                                        x.stride(0), ptr(y), y.stride(0), d, red, ptr(S),
                                        S.stride(0) if S is not None else 0, float(self_scale), ptr(cs), ptr(ct),
                                        _lib.ACT_RELU if relu else _lib.ACT_NONE, 1 if l2norm else 0,
                                        float(l2_eps), ptr(ws), ws_bytes, _stream())
        if st == 2 and l2norm:   # row wider than one wave: normalise in a second pass
            check(L.mp_spmm_csr_epilogue_f32(ptr(g.rowptr), ptr(g.col), ptr(g.val), N, ptr(plan), counts, ptr(x),
                                             x.stride(0), ptr(y), y.stride(0), d, red, ptr(S),
                                             S.stride(0) if S is not None else 0, float(self_scale), ptr(cs),
                                             ptr(ct), _lib.ACT_RELU if relu else _lib.ACT_NONE, 0, float(l2_eps),
                                             ptr(ws), ws_bytes, _stream()), "mp_spmm_csr_epilogue_f32")
            return torch.nn.functional.normalize(y, p=2, dim=-1, eps=l2_eps)
        check(st, "mp_spmm_csr_epilogue_f32")
    return y


def _raw_dense_fused(P, W, Q, W_id, bias, relu):
    """out = act(P @ W [+ Q @ W_id] + bias) on the engine's MFMA kernel; None if the shapes are outside
    what the kernel covers (the caller then composes library ops)"""
    L = lib()
    M, F = P.shape
    d = W.size(1)
    if Q is None and dense_x3_supported(P, F, d):
        return _raw_dense_x3(P, W, bias, relu)
    out = placement.empty_or_torch((M, d), P.device, reads=(P, Q), streaming=True)
    Wc = W.contiguous()
    Wi = None if W_id is None else W_id.contiguous()
    b = None if bias is None else bias.contiguous()
    with torch.cuda.device(P.device):
        st = L.mp_dense_fused_f32(ptr(P), P.stride(0), ptr(Wc), ptr(Q), Q.stride(0) if Q is not None else 0,
                                  ptr(Wi), ptr(b), _lib.ACT_RELU if relu else _lib.ACT_NONE, ptr(out),
                                  out.stride(0), M, F, d, _stream())
    if st in (_lib.MP_ERR_UNSUPPORTED, _lib.MP_ERR_ALIGNMENT):
        return None
    check(st, "mp_dense_fused_f32")
    return out


X3_WIDTHS = (64, 128, 256)
X3_MIN_ROWS = int(os.environ.get("MP_X3_MIN_ROWS", 1 << 17))   # below this the persistent 256-row blocks do not fill the chip


def _split_w(W, trans=False):
    """W -> the engine's three-way bf16 split of W (or of W^T): [3, K / 8, n, 8] bf16 (mp_split_w_bf16x3; one
    small launch, so nothing is cached across calls)"""
    Wc = W.detach()
    if Wc.stride(1) != 1 and Wc.stride(0) == 1:      # a transposed view (nn.Linear's weight.t()): split its base
        Wc, trans = Wc.t(), not trans
    elif Wc.stride(1) != 1:
        Wc = Wc.contiguous()
    K, n = (Wc.size(1), Wc.size(0)) if trans else (Wc.size(0), Wc.size(1))
    sp = torch.empty((3, K // 8, n, 8), dtype=torch.bfloat16, device=Wc.device)
    with torch.cuda.device(Wc.device):
        check(lib().mp_split_w_bf16x3(ptr(Wc), Wc.stride(0), K, n, 1 if trans else 0, ptr(sp), _stream()),
              "mp_split_w_bf16x3")
    return sp


def dense_x3_supported(P, K, n, out=None):
    """shapes the streaming transform takes (mp_dense_x3_f32): [M, K] @ [K, n] with n = 64 / 128 / 256, K % 32 == 0,
    K >= 64, 16-byte-aligned rows on both sides, and enough rows to fill the chip; MP_X3=0 turns it off (A/B timing)"""
    return (os.environ.get("MP_X3", "1") != "0" and P.dim() == 2 and P.size(0) >= X3_MIN_ROWS and n in X3_WIDTHS
            and K % 32 == 0 and K >= 64 and P.size(1) == K and P.stride(1) == 1 and P.stride(0) % 4 == 0
            and P.data_ptr() % 16 == 0 and P.dtype == torch.float32
            and (out is None or (out.stride(1) == 1 and out.stride(0) % 4 == 0 and out.data_ptr() % 16 == 0)))


def _raw_dense_x3(P, W, bias=None, relu=False, trans=False, out=None):
    """act(P @ W + bias) (trans: P @ W^T) on the streaming kernel; the caller has checked dense_x3_supported"""
    M, K = P.shape
    n = W.size(0) if trans else W.size(1)
    sp = _split_w(W, trans)
    if out is None:
        out = placement.empty_or_torch((M, n), P.device, reads=(P,), streaming=True)
    b = None if bias is None else bias.detach().contiguous()
    if b is not None and b.data_ptr() % 16:
        b = b.clone()                        # a slice of a longer bias: the kernel reads it in 16-byte groups
    with torch.cuda.device(P.device):
        check(lib().mp_dense_x3_f32(ptr(P), P.stride(0), ptr(sp), ptr(b), _lib.ACT_RELU if relu else _lib.ACT_NONE,
                                    ptr(out), out.stride(0), M, K, n, _stream()), "mp_dense_x3_f32")
    return out


def times_wt(g, W):
    """g @ W^T — the input gradient of a transform: the streaming kernel at its shapes, else the library GEMM"""
    if dense_x3_supported(g, W.size(1), W.size(0)):
        return _raw_dense_x3(g, W, trans=True)
    return torch.mm(g, W.detach().t())


FUSED_WIDTHS = (64, 128, 256, 512)
AGG_TILES_CALLS = 0                   # launches of mp_agg_rows_tiles_f32 by this process (tests assert the dispatch)
AGG_TILES_WIDTHS = (128, 256, 512)   # widths of mp_agg_rows_tiles_f32 (d = 128: 10.04 -> 9.85 ms; d = 64 stays on the plan-based kernel)
AGG_TILES_MIN_ROWS = 1 << 21    # crossover against the plan-based kernel on BA graphs (d = 256): 1e6 rows 2.15 vs 1.73 ms, 2e6 3.72 vs 3.82, 3e6 5.45 vs 5.82, 1e7 19.6 vs 20.6
FUSED_MAX_ROW = 1 << 18      # longer rows (star-like hubs) go to the plan-based kernel, which spreads them over many waves
AGG_HOT_CALLS = 0           # launches of mp_agg_rows_tiles_hot_f32 by this process
AGG_HOT_MB = 256            # MP_AGG_HOT_MB (read per call; 0 = off): the rows of X kept cache-resident by the tile aggregation
# X below this keeps the plain kernel: at d = 256, hot (256 MB) against plain, 0.25 GiB of X 1.005 vs 0.885 ms, 0.5 GiB
# 1.485 vs 1.399, 1 GiB 2.226 vs 2.237, 9.8 GiB 18.48 vs 20.62 (profiles/r05_hot_ab_small.jsonl, r05_hot_ab.jsonl).  With
# AGG_TILES_MIN_ROWS = 2^21 a square operator at d >= 128 is past it anyway: it decides for rectangular ones.
AGG_HOT_MIN_BYTES = int(os.environ.get("MP_AGG_HOT_MIN_BYTES", 1 << 30))


def _hot_col(g, x):
    """the tagged column indices for mp_agg_rows_tiles_hot_f32 (graph.py, CSRGraph.hot_col), or None: X below
    AGG_HOT_MIN_BYTES, a zero budget, or none built yet under stream capture"""
    row_bytes = x.size(1) * x.element_size()
    if x.size(0) * row_bytes < AGG_HOT_MIN_BYTES:
        return None
    mb = float(os.environ.get("MP_AGG_HOT_MB", AGG_HOT_MB))
    return g.hot_col(int(mb * (1 << 20)), row_bytes) if mb > 0 else None


def agg_dense_supported(g, x, W):
    """shapes the one-kernel aggregate -> transform takes (mp_agg_dense_f32); MP_FUSED=0 in the environment
    turns the path off (A/B timing against the two-kernel order)"""
    if os.environ.get("MP_FUSED", "1") == "0":
        return False
    return (x.size(1) in FUSED_WIDTHS and W.size(1) % 2 == 0 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0
            and (x.size(1) < 512 or W.size(1) <= 512)
            and g.nnz > 0 and g.max_row_entries() <= FUSED_MAX_ROW)


BF16X3_MIN_ROWS = 1 << 14   # below this the split of W (one ~5 us launch per call) costs more than the shorter MFMA phase saves
                            # (round 2: 2^19, set on the one-role kernel; an ego batch of 1.5 * 10^5 rows at F = 512 ran the
                            # exact-f32 product at 1.24 ms per layer, MFMA-bound)


def _split_bf16_t(W):
    """W [F, d] fp32 -> [3, F / 8, d, 8] bf16: W split three ways, plane s = bf16(W - sum of the planes before it)
    (24 mantissa bits in all), in the layout the bf16x3 product of mp_agg_dense_f32 loads (a lane's 8 k-values of a
    column contiguous, neighbouring columns neighbours).  Split afresh on every call (mp_split_w_bf16x3, one ~5 us
    launch): nothing observable from Python says W is unchanged — `w.data.uniform_()` (the reference's own
    reset_parameters idiom, idconv.py:125-128) rewrites a weight without touching `_version`, and a cached split
    would then multiply by the old weights silently."""
    return _split_w(W)


def _raw_agg_dense(g, x, W, bias=None, relu=False, S=None, self_scale=0.0, want_P=False, reduce=_lib.SUM,
                   out=None, defer_act=None, bf16x3=None, residual=None):
    """out = act((reduce_j w_ij x[j] + self_scale * S) W + bias) in one launch (into the view `out` when given);
    returns (out, P or None) with P the aggregated rows; defer_act [N] uint8: rows stored without the activation.
    bf16x3: run the product on the bf16 matrix pipe with three-way split operands (fp32-accurate, 3/8 of the MFMA
    cycles); default: on for N >= BF16X3_MIN_ROWS unless MP_BF16X3=0."""
    L = lib()
    N, F, d = g.num_nodes, x.size(1), W.size(1)
    Wc = W.contiguous()
    if bf16x3 is None:
        bf16x3 = N >= BF16X3_MIN_ROWS and os.environ.get("MP_BF16X3", "1") != "0"
    Wsp = _split_bf16_t(Wc) if bf16x3 else None
    b = None if bias is None else bias.contiguous()
    if out is None:
        out = placement.empty_or_torch((N, d), x.device, reads=(x,))
    P = placement.empty_or_torch((N, F), x.device, reads=(x,)) if want_P else None
    with torch.cuda.device(x.device):
        args = (ptr(g.rowptr), ptr(g.col), ptr(g.val), N, reduce, ptr(x), x.stride(0), F,
                ptr(S), S.stride(0) if S is not None else 0, float(self_scale), ptr(Wc),
                Wc.stride(0), d, ptr(b), _lib.ACT_RELU if relu else _lib.ACT_NONE, ptr(defer_act),
                ptr(P), P.stride(0) if P is not None else 0, ptr(out), out.stride(0), ptr(Wsp))
        if residual is None:
            check(L.mp_agg_dense_f32(*args, _stream()), "mp_agg_dense_f32")
        else:   # out = act(... + residual); the residual may be `out` itself
            check(L.mp_agg_dense_add_f32(*args, ptr(residual), residual.stride(0), _stream()), "mp_agg_dense_add_f32")
    return out, P


def _launch_dense_wgrad(P, G, Y=None, want_bias=False, want_gm=False, gm_out=None):
    """one weight-gradient pass, mp_dense_wgrad_f32 or (Y given) mp_dense_wgrad_relu_f32: sizes and allocates the workspace
    and the outputs; (P^T g, column sums of g or None, g or None) with g = G or G * [Y > 0]; None when the shape is
    outside the kernel"""
    L = lib()
    M, F = P.shape
    d = G.size(1)
    out = torch.empty((F, d), dtype=torch.float32, device=P.device)
    db = torch.empty(d, dtype=torch.float32, device=P.device) if want_bias else None
    # the masked gradient is written only when an input-gradient launch will read it (a first layer has none)
    # (gm_out: a [M, d] view to receive it, e.g. one half of a concatenated gradient)
    gm = gm_out if gm_out is not None else (
        placement.empty_or_torch((M, d), P.device, reads=(G, Y, P), streaming=True) if want_gm else None)
    with torch.cuda.device(P.device):
        nb = C.c_size_t(0)
        check(L.mp_dense_wgrad_ws_bytes(M, F, d, C.byref(nb)))
        ws = torch.empty(max(nb.value, 1), dtype=torch.uint8, device=P.device)
        tail = (M, F, d, ptr(out), ptr(db), ptr(ws), nb.value, _stream())
        if Y is None:
            name, st = "mp_dense_wgrad_f32", L.mp_dense_wgrad_f32(ptr(P), P.stride(0), ptr(G), G.stride(0), *tail)
        else:
            name, st = "mp_dense_wgrad_relu_f32", L.mp_dense_wgrad_relu_f32(
                ptr(P), P.stride(0), ptr(G), G.stride(0), ptr(Y), Y.stride(0), ptr(gm),
                gm.stride(0) if gm is not None else 0, *tail)
    if st in (_lib.MP_ERR_UNSUPPORTED, _lib.MP_ERR_ALIGNMENT):
        return None
    check(st, name)
    return out, db, gm


def _raw_dense_wgrad(P, G, want_bias=False):
    """P^T @ G on the engine's split-K MFMA kernel (None when the shape is outside it); with want_bias the pair
    (P^T @ G, column sums of G) — the bias gradient comes out of the same pass over G"""
    r = _launch_dense_wgrad(P, G, want_bias=want_bias) or (None, None)
    return r[:2] if want_bias else r[0]


def _raw_dense_wgrad_relu(P, G, Y, want_bias=False, want_gm=True, gm_out=None):
    """(P^T (G * [Y > 0]), its column sums or None, G * [Y > 0]) in one pass (mp_dense_wgrad_relu_f32): the weight-gradient
    kernel masks the incoming gradient by the forward's ReLU pattern as it reads it and writes the masked gradient out
    for the input-gradient launch; None when the shape is outside the kernel"""
    return _launch_dense_wgrad(P, G, Y, want_bias, want_gm, gm_out)


def _wgrad_and_bias(X, g, need_w, need_b):
    """(X^T g, sum_m g[m]) for a transform's backward pass: one kernel when both are wanted (bf16: library GEMM, the
    column sums in fp32, cast)"""
    if g.dtype == torch.bfloat16:
        return (X.t() @ g if need_w else None), (g.float().sum(0).to(g.dtype) if need_b else None)
    if need_w and need_b:
        dW, db = _raw_dense_wgrad(X, g, want_bias=True)
        if dW is not None:
            return dW, db
    dW = None
    if need_w:
        dW = _raw_dense_wgrad(X, g)
        if dW is None:
            dW = X.t() @ g
    return dW, (g.sum(0) if need_b else None)


def _concat_wgrad(a, b, g, out, ku, relu, need_wa, need_wb, has_bias, need_gm):
    """the weight side of the backward of out = act([a Wa ‖ b Wb] + bias): (g masked by the ReLU — None if nobody reads
    it —, dWa, dWb, dba, dbb).  b None: its rows were not kept (no dWb)"""
    if relu and need_wa and need_wb and b is not None:
        # the ReLU mask rides in the two weight-gradient passes (one per half of the output), which also leave the masked
        # halves in one buffer for the input-gradient launches (no threshold_backward pass); the buffer is written only
        # when an input gradient will read it (a first layer has none)
        mg = placement.empty_or_torch(tuple(g.shape), g.device, reads=(g, out), streaming=True) if need_gm else None
        rs = _raw_dense_wgrad_relu(a, g[:, :ku], out[:, :ku], want_bias=has_bias, want_gm=need_gm,
                                   gm_out=None if mg is None else mg[:, :ku])
        rn = None if rs is None else _raw_dense_wgrad_relu(b, g[:, ku:], out[:, ku:], want_bias=has_bias,
                                                           want_gm=need_gm,
                                                           gm_out=None if mg is None else mg[:, ku:])
        if rs is not None and rn is not None:
            return mg, rs[0], rn[0], rs[1], rn[1]
    if relu:
        g = torch.ops.aten.threshold_backward(g, out, 0.0)
    dWa, dba = _wgrad_and_bias(a, g[:, :ku], need_wa, has_bias)
    dWb, dbb = _wgrad_and_bias(b, g[:, ku:], need_wb, has_bias)
    return g, dWa, dWb, dba, dbb


def _dense_into(out_view, P, W, bias, relu):
    """out_view[:, :] = act(P @ W + bias) written in place through the kernel's output leading dimension"""
    L = lib()
    M, F = P.shape
    d = W.size(1)
    if dense_x3_supported(P, F, d, out_view):
        _raw_dense_x3(P, W, bias, relu, out=out_view)
        return
    Wc = W.contiguous()
    b = None if bias is None else bias.contiguous()
    with torch.cuda.device(P.device):
        check(L.mp_dense_fused_f32(ptr(P), P.stride(0), ptr(Wc), None, 0, None, ptr(b),
                                   _lib.ACT_RELU if relu else _lib.ACT_NONE, ptr(out_view), out_view.stride(0), M, F, d,
                                   _stream()), "mp_dense_fused_f32")


class _ConcatDense(torch.autograd.Function):
    """out = act([x @ Ws ‖ m @ Wn] + bias): both halves written straight into one buffer (no cat, no separate
    bias / activation passes) — the combine step of tfg MeanGraphSage / IDSAGE.call (TfgIDLayer.py:100-117)"""
    @staticmethod
    def forward(ctx, x, m, Ws, Wn, bias, relu):
        x, m = _f32c(x, "x"), _f32c(m, "m")
        ku, kn = Ws.size(1), Wn.size(1)
        out = placement.empty_or_torch((x.size(0), ku + kn), x.device, reads=(x, m), streaming=True)
        b = None if bias is None else bias.detach()
        _dense_into(out[:, :ku], x, Ws.detach(), None if b is None else b[:ku], relu)
        _dense_into(out[:, ku:], m, Wn.detach(), None if b is None else b[ku:], relu)
        ctx.relu, ctx.ku, ctx.has_bias = relu, ku, bias is not None
        ctx.save_for_backward(x, m, Ws, Wn, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, g):
        x, m, Ws, Wn, out = ctx.saved_tensors
        ku = ctx.ku
        g, dWs, dWn, dbs, dbn = _concat_wgrad(x, m, g.contiguous(), out, ku, ctx.relu, ctx.needs_input_grad[2],
                                              ctx.needs_input_grad[3], ctx.has_bias,
                                              ctx.needs_input_grad[0] or ctx.needs_input_grad[1])
        dx = times_wt(g[:, :ku], Ws) if ctx.needs_input_grad[0] else None     # strided views: the kernels take leading dimensions
        dm = times_wt(g[:, ku:], Wn) if ctx.needs_input_grad[1] else None
        db = torch.cat([dbs, dbn]) if ctx.has_bias else None
        return dx, dm, dWs, dWn, db, None


def concat_dense(x, m, Ws, Wn, bias=None, relu=False):
    if x.dtype == torch.bfloat16:     # no bf16 transform kernel: library ops
        _require_hip(x, "x")
        out = torch.cat([x @ Ws, m @ Wn], dim=1)
        out = out if bias is None else out + bias
        return torch.relu(out) if relu else out
    return _ConcatDense.apply(x, m, Ws, Wn, bias, bool(relu))


class _SageConcatFused(torch.autograd.Function):
    """out = act([x Ws ‖ mean_j(x_j) Wn] + bias) (TfgIDLayer.py:100-117): the self half is one MFMA kernel, the
    neighbour half is the one-kernel aggregate -> transform writing into the same buffer; the backward pass
    runs the aggregate -> transform kernel on the transposed mean operator."""
    @staticmethod
    def forward(ctx, x, Ws, Wn, bias, g, relu, grad_mode):
        x = _f32c(x, "x")
        ku, kn = Ws.size(1), Wn.size(1)
        out = placement.empty_or_torch((x.size(0), ku + kn), x.device, reads=(x,))
        b = None if bias is None else bias.detach()
        _dense_into(out[:, :ku], x, Ws.detach(), None if b is None else b[:ku], relu)
        _, P = _raw_agg_dense(g, x, Wn.detach(), None if b is None else b[ku:], relu,
                              want_P=ctx.needs_input_grad[2] and grad_mode, reduce=_lib.MEAN,
                              out=out[:, ku:])
        ctx.g, ctx.relu, ctx.ku, ctx.has_bias = g, relu, ku, bias is not None
        ctx.save_for_backward(x, P, Ws, Wn, out if relu else None)
        return out

    @staticmethod
    def backward(ctx, gout):
        x, P, Ws, Wn, out = ctx.saved_tensors
        ku = ctx.ku
        gm, dWs, dWn, dbs, dbn = _concat_wgrad(x, P, gout.contiguous(), out, ku, ctx.relu, ctx.needs_input_grad[1],
                                               ctx.needs_input_grad[2], ctx.has_bias, ctx.needs_input_grad[0])
        gs, gn = (gm[:, :ku], gm[:, ku:]) if gm is not None else (None, None)
        db = torch.cat([dbs, dbn]) if ctx.has_bias else None
        dx = None
        if ctx.needs_input_grad[0]:
            dx = times_wt(gs, Ws)
            gt = ctx.g.transpose_mean()
            Wnt = Wn.detach().t().contiguous()
            if agg_dense_supported(gt, gn, Wnt) and dx.stride(1) == 1 and dx.stride(0) % 2 == 0:
                # dx = gs Ws^T + (A^T gn) Wn^T: the second term's launch adds the first as it stores
                _raw_agg_dense(gt, gn, Wnt, out=dx, residual=dx)
            else:
                T, _ = _raw_spmm(gt, gn.contiguous(), _lib.SUM)
                dx.add_(T @ Wnt)
        return dx, dWs, dWn, db, None, None, None


def sage_concat(g, x, Ws, Wn, bias=None, relu=False):
    """act([x Ws ‖ mean-aggregate(x) Wn] + bias); one-kernel aggregate -> transform for the neighbour half when
    the shapes allow, else the aggregation kernel + concat_dense"""
    if (agg_dense_supported(g, x, Wn) and x.dtype == torch.float32 and Ws.size(1) % 2 == 0
            and g.num_cols == g.num_nodes):
        return _SageConcatFused.apply(x, Ws, Wn, bias, g, bool(relu), torch.is_grad_enabled())
    return concat_dense(x, spmm(g, x, "mean"), Ws, Wn, bias, relu=relu)


_IDS_OPS = {}


def _ids_operator(ids, n, clamp=False):
    """the [n x K] operator of an id list ids [K] int64 with entries in [0, n): row r holds the positions k with
    ids[k] == r in ascending order (a stable sort, then rowptr by binary search: no atomics).  Summing rows u [K, d]
    over it on the aggregation kernel is index_add over ids in a fixed order.  Cached per id tensor (tensor_stamp).
    clamp: an id outside [0, n) is listed under row 0 (the caller hands a zero row for it)."""
    stamp = (tensor_stamp(ids), int(n), bool(clamp))
    hit = _IDS_OPS.get(stamp)
    if hit is None:
        if len(_IDS_OPS) > 8:
            _IDS_OPS.clear()
        order = torch.sort(torch.where((ids >= 0) & (ids < n), ids, torch.zeros_like(ids)) if clamp else ids, stable=True)
        rowptr = torch.searchsorted(order.values, torch.arange(n + 1, dtype=ids.dtype, device=ids.device))
        op = CSRGraph(rowptr.to(torch.int32), order.indices.to(torch.int32), None, None, n, ids.numel(), ids.numel())
        hit = _IDS_OPS[stamp] = (op, ids)         # holding `ids` keeps its address from being reused
    return hit[0]


def _sum_rows_by_ids(ids, n, u, clamp=False):
    """out[r] = sum of u[k] over the k with ids[k] == r, k ascending -> [n, d]: the deterministic index_add"""
    return _raw_spmm(_ids_operator(ids, n, clamp), u, _lib.SUM)[0]


def _entry_sums(g, ds, by_source):
    """ds [nnz, H] fp32 summed over the entries of every destination (an [N x nnz] operator over g.rowptr, col = arange)
    or of every source (the same over the transposed pattern's rowptr, col = its pos) on the aggregation kernel: the
    by-node sums of a per-entry gradient in a fixed order.  Both operators are cached on the graph and share the plan
    of the pattern they stand on."""
    key = "_entry_sum_src" if by_source else "_entry_sum_dst"
    op = g.__dict__.get(key)
    if op is None:
        if by_source:
            gt = g._transpose_sorted()
            op = CSRGraph(gt.rowptr, gt.pos, None, None, gt.num_nodes, g.nnz, g.nnz)
            op._plan = gt.plan()
        else:
            op = CSRGraph(g.rowptr, torch.arange(g.nnz, dtype=torch.int32, device=g.device), None, None, g.num_nodes,
                          g.nnz, g.nnz)
            op._plan = g.plan()
        g.__dict__[key] = op
    return _raw_spmm(op, ds.contiguous(), _lib.SUM)[0]


class _IndexAddRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, id_index, u):
        u = _f32c(u, "u")
        ids = id_index.to(torch.int64).contiguous()
        ctx.save_for_backward(ids)
        if deterministic():
            h = _f32c(h, "h")
            return h + _sum_rows_by_ids(ids, h.size(0), u)
        h = _f32c(h, "h").clone()
        L = lib()
        with torch.cuda.device(h.device):
            check(L.mp_rows_scatter_add_f32(ptr(h), h.stride(0), ptr(ids), ids.numel(), h.size(1),
                                            ptr(u), u.stride(0), _stream()), "mp_rows_scatter_add_f32")
        return h

    @staticmethod
    def backward(ctx, dh):
        (ids,) = ctx.saved_tensors
        return dh, None, gather_rows(dh.contiguous(), ids)


def index_add_rows(h, id_index, u):
    """out = h ; out[id[k]] += u[k]   (tensor_scatter_nd_add, TfgIDLayer.py:107,165,330,515;
    index_add_, idconv.py:67,155,251,310,375)"""
    if h.dtype == torch.bfloat16:     # bf16: the library op
        _require_hip(h, "h")
        return h.index_add(0, id_index.to(torch.int64), u)
    return _IndexAddRows.apply(h, id_index, u)


class _GatherRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, ids):
        x = _f32c(x, "x")
        L = lib()
        ids = ids.to(torch.int64).contiguous()
        out = torch.empty((ids.numel(), x.size(1)), dtype=torch.float32, device=x.device)
        with torch.cuda.device(x.device):
            check(L.mp_rows_gather_f32(ptr(x), x.stride(0), ptr(ids), ids.numel(), x.size(1), ptr(out),
                                       out.stride(0), _stream()), "mp_rows_gather_f32")
        ctx.save_for_backward(ids)
        ctx.n = x.size(0)
        return out

    @staticmethod
    def backward(ctx, dout):
        (ids,) = ctx.saved_tensors
        if deterministic():
            return _sum_rows_by_ids(ids, ctx.n, _f32c(dout, "dout")), None
        dx = torch.zeros((ctx.n, dout.size(1)), dtype=torch.float32, device=dout.device)
        L = lib()
        dout = dout.contiguous()
        with torch.cuda.device(dout.device):
            check(L.mp_rows_scatter_add_f32(ptr(dx), dx.stride(0), ptr(ids), ids.numel(), dx.size(1),
                                            ptr(dout), dout.stride(0), _stream()))
        return dx, None


def gather_rows(x, ids):
    """x[ids]  (tf.gather / index_select of the identity rows)"""
    if x.dtype == torch.bfloat16:     # bf16: the library op
        _require_hip(x, "x")
        return x.index_select(0, ids.to(torch.int64))
    return _GatherRows.apply(x, ids)


# ---- attention pieces --------------------------------------------------------

def _agg_of_nothing(N, d, x, bias=None, want_argmax=False, out=None):
    """(y, argmax or None) of an aggregation over an operator without entries, whose per-entry arrays have no address to
    hand to a kernel (the zero-extent rule): every row is empty, so y = 0 + bias — a destination's own
    term t rides in the entries and goes with them — and argmax = -1"""
    y = out if out is not None else torch.empty((N, d), dtype=x.dtype, device=x.device)
    if bias is None:
        y.zero_()
    else:
        y.copy_(bias.detach().to(y.dtype).expand(N, d))
    return y, (torch.full((N, d), -1, dtype=torch.int32, device=x.device) if want_argmax else None)


def _row0_if_none(m, width, device):
    """m, the operand read through an entry's input position — or, where it has no rows (every entry is an inserted loop),
    one row of zeros: the kernel still reads (and drops) row 0, and wants an address for it"""
    return m if m.size(0) else torch.zeros((1, width), dtype=torch.float32, device=device)


def _entry_empty(nnz, device, *cols):
    """an uninitialised float32 per-entry output [max(nnz, 1), *cols]: at least one row, so that the kernel gets an
    address also for an operator without entries; the caller returns its first nnz rows"""
    return torch.empty((max(nnz, 1),) + cols, dtype=torch.float32, device=device)


def _raw_sddmm_dot(g, A, B, heads, scale, idx=None):
    """s[e, h] = scale * <A[row_e, slice h], B[idx[e], slice h]>; idx [nnz] int32: the row of B an entry reads (default:
    its column, g.col)"""
    L = lib()
    idx = g.col if idx is None else idx
    s = _entry_empty(g.nnz * heads, A.device)
    with torch.cuda.device(A.device):
        st = L.mp_sddmm_dot_stream_f32(ptr(g.row_ids()), ptr(idx), g.nnz, ptr(A), A.stride(0), ptr(B),
                                       B.stride(0), A.size(1), heads, float(scale), ptr(s), _stream())
        if st == 2:   # head layout the entry-balanced kernel does not cover
            st = L.mp_sddmm_dot_f32(ptr(g.rowptr), ptr(idx), g.num_nodes, g.nnz, ptr(A), A.stride(0),
                                    ptr(B), B.stride(0), A.size(1), heads, float(scale), ptr(s), _stream())
        check(st, "mp_sddmm_dot")
    return s[:g.nnz * heads].view(g.nnz, heads)


HEADS_ONE_LAUNCH = (2, 4, 8)     # head counts of mp_spmm_csr_heads_reduce_f32 / mp_spmm_csr_edge_heads_f32 beside 1


def _raw_heads_agg(g, w, x, heads, reduce=_lib.SUM, want_argmax=False, edge=None, one_launch=True):
    """y[r, slice h] = reduce_e w[e, h] x[col_e, slice h] -> (y, argmax [N, d] int32 or None); with edge = (m, t, bias)
    the message is (x[col_e] + m[eid_e] + t[r])[slice h] and bias is added (m [E, d] by the entry's input position, t
    [N, d] or None, bias [d] or None).  The ladder over the head count, once for both forms:
      1 head            the aggregation itself with val = w (_raw_spmm — so a large sum still goes to the tile kernels — or
                        _raw_spmm_edge)
      2, 4 or 8 heads   one launch: full-row loads, every lane applies the weight of the head its columns belong to
                        (mp_spmm_csr_heads_reduce_f32 / mp_spmm_csr_edge_heads_f32)
      other counts, or a head layout the one launch does not take (status 2): the one-head call per head on column slices
    one_launch=False sends 2, 4 and 8 heads through the per-head form too (tests, tests/perf/bench_edgeatt.py): the same
    terms in the same order, the same bits, and the slower form as this function runs it — by 1.5 % on 2e7 entries,
    where the copies of w's columns cost more than the H launches save, and threefold on 2e5 entries.
    The entry values of g take no part: they belong in w."""
    N, d = g.num_nodes, x.size(1)
    if heads < 1 or d % heads:
        raise ValueError(f"{'V' if edge is None else 'x'} has {d} columns, not a multiple of heads = {heads}")
    m = t = bias = eid = None
    if edge is not None:
        m, t, bias = edge
        eid = _eid_checked(g, m.size(0))
        m = _row0_if_none(m, d, x.device)
    if g.nnz == 0:              # no entry: col, eid and w have no address; every row is empty
        return _agg_of_nothing(N, d, x, bias, want_argmax)

    def one_head(vals, cs=slice(None), out=None):
        gh = g.with_values(vals.contiguous())
        if edge is None:
            return _raw_spmm(gh, x[:, cs], reduce, want_argmax=want_argmax, out=out)
        gh.__dict__["_eid_max"] = g.__dict__.get("_eid_max")     # (checked on g above: no second read of it per head)
        return _raw_spmm_edge(gh, x[:, cs], m[:, cs], None if t is None else t[:, cs],
                              None if bias is None else bias[cs], reduce, want_argmax, out=out)

    if heads == 1:
        return one_head(w.reshape(-1))
    y = placement.empty_or_torch((N, d), x.device, reads=(x,) if edge is None else (x, m))
    argmax = torch.empty((N, d), dtype=torch.int32, device=x.device) if want_argmax else None
    if one_launch and heads in HEADS_ONE_LAUNCH:
        L = lib()
        w = w.contiguous()
        plan, counts, ws, ws_bytes = _plan_ws(g, x.device, d, reduce, False)
        with torch.cuda.device(x.device):
            if edge is None:
                name = "mp_spmm_csr_heads_reduce_f32"
                st = L.mp_spmm_csr_heads_reduce_f32(ptr(g.rowptr), ptr(g.col), ptr(w), N, ptr(plan), counts, heads,
                                                    reduce, ptr(x), x.stride(0), ptr(y), y.stride(0), d, ptr(argmax),
                                                    ptr(ws), ws_bytes, _stream())
            else:
                name = "mp_spmm_csr_edge_heads_f32"
                st = L.mp_spmm_csr_edge_heads_f32(ptr(g.rowptr), ptr(g.col), ptr(eid), ptr(w), N, ptr(plan), counts,
                                                  heads, ptr(x), x.stride(0), ptr(m), m.stride(0), ptr(t),
                                                  t.stride(0) if t is not None else 0, ptr(y), y.stride(0), d, reduce,
                                                  ptr(bias), ptr(argmax), ptr(ws), ws_bytes, _stream())
        if st != 2:
            check(st, name)
            return y, argmax
    g.plan()                                     # built once, shared by the per-head graphs below
    dh = d // heads
    for h in range(heads):
        cs = slice(h * dh, (h + 1) * dh)
        _, am = one_head(w[:, h], cs, out=y[:, cs])
        if want_argmax:
            argmax[:, cs] = am
    return y, argmax


# the ladder under the names and argument orders the callers use
def _raw_spmm_heads(g, a, V, heads):
    """y[i, slice h] = sum_e a[e,h] V[col_e, slice h]"""
    return _raw_heads_agg(g, a, V, heads)[0]


def _raw_spmm_heads_reduce(g, a, V, heads, reduce):
    """sum / mean / max of a[e,h] V[col_e, slice h] over each row -> (y, argmax [N, d] int32 for max, else None)"""
    return _raw_heads_agg(g, a, V, heads, reduce, want_argmax=reduce == _lib.MAX)


def _raw_spmm_edge_heads(g, w, x, m, t=None, bias=None, heads=1, reduce=_lib.SUM, want_argmax=False, one_launch=True):
    """the two-gather form: reduce_e w[e, h] (x[col_e] + m[eid_e] + t[r])[slice h] + bias -> (y, argmax or None)"""
    return _raw_heads_agg(g, w, x, heads, reduce, want_argmax, edge=(m, t, bias), one_launch=one_launch)


class _SddmmDot(torch.autograd.Function):
    """s[e,h] = scale * <Q[row_e, slice h], K[col_e, slice h]>"""
    @staticmethod
    def forward(ctx, Q, K, g, heads, scale):
        Q, K = _f32c(Q, "Q"), _f32c(K, "K")
        ctx.g, ctx.heads, ctx.scale = g, heads, scale
        ctx.save_for_backward(Q, K)
        return _raw_sddmm_dot(g, Q, K, heads, scale)

    @staticmethod
    def backward(ctx, ds):
        Q, K = ctx.saved_tensors
        g, heads = ctx.g, ctx.heads
        ds = (ds * ctx.scale).contiguous()
        # dQ[i, slice h] = sum_e ds[e,h] K[col_e, slice h]   (an aggregation over in-edges)
        dQ = _raw_spmm_heads(g, ds, K, heads)
        # dK[j, slice h] = sum_{e: col_e = j} ds[e,h] Q[row_e, slice h]   (over out-edges)
        dK = _heads_grad_by_source(g, ds, K, heads, False, Q)
        return dQ, dK, None, None, None


def sddmm_dot(g, Q, K, heads=1, scale=1.0):
    return _SddmmDot.apply(Q, K, g, int(heads), float(scale))


class _SddmmAdd(torch.autograd.Function):
    """s[e] = leaky_relu(ai[row_e] + aj[col_e])"""
    @staticmethod
    def forward(ctx, ai, aj, g, slope):
        L = lib()
        ai, aj = ai.contiguous(), aj.contiguous()
        s = _entry_empty(g.nnz, ai.device)
        with torch.cuda.device(ai.device):
            check(L.mp_sddmm_add_f32(ptr(g.rowptr), ptr(g.col), g.num_nodes, g.nnz, ptr(ai), ptr(aj),
                                     float(slope), ptr(s), _stream()), "mp_sddmm_add_f32")
        s = s[:g.nnz]
        ctx.g, ctx.slope = g, slope
        ctx.save_for_backward(s)
        return s.view(g.nnz, 1)

    @staticmethod
    def backward(ctx, ds):
        (s,) = ctx.saved_tensors
        g = ctx.g
        gs = ds.reshape(-1) * torch.where(s > 0, torch.ones_like(s), torch.full_like(s, ctx.slope))
        if deterministic():
            gs = gs.view(-1, 1)
            return _entry_sums(g, gs, False).view(-1), _entry_sums(g, gs, True).view(-1), None, None
        dai = torch.zeros(g.num_nodes, dtype=torch.float32, device=s.device)
        daj = torch.zeros(g.num_nodes, dtype=torch.float32, device=s.device)
        dai.index_add_(0, g.row_ids().long(), gs)
        daj.index_add_(0, g.col.long(), gs)
        return dai, daj, None, None


def sddmm_add(g, ai, aj, slope=0.2):
    return _SddmmAdd.apply(ai, aj, g, float(slope))


def _raw_row_softmax_bwd(g, p, dp):
    """ds = p * (dp - sum over the row of p * dp), per head (mp_csr_row_softmax_bwd_f32); p, dp [nnz, H]"""
    p, dp = p.contiguous(), dp.contiguous()
    ds = torch.empty_like(p)
    if g.nnz:
        with torch.cuda.device(p.device):
            check(lib().mp_csr_row_softmax_bwd_f32(ptr(g.rowptr), g.num_nodes, p.size(1), ptr(p), ptr(dp), ptr(ds),
                                                   _stream()), "mp_csr_row_softmax_bwd_f32")
    return ds


_EA_DST, _EA_SRC, _EA_EDGE = 1, 2, 4


def _alpha_bwd(g, alpha, dalpha, a_dst, a_src, a_edge, slope, which):
    """(d_dst, d_src, d_edge) of the additive coefficients alpha = softmax_row(leaky_relu(a_dst[row] + a_src[col] +
    a_edge[eid])) (gat_alpha: a_edge None; edge_att_alpha: a_dst may be None), each computed when its bit of `which`
    (1, 2, 4) is set and its term exists, None otherwise: the row softmax backward, the slope mask on the recomputed
    pre-activation, sums by destination and by source; an input edge belongs to at most one entry, so d_edge is an
    indexed store into zeros"""
    ds = _raw_row_softmax_bwd(g, alpha, dalpha)
    rows, cols = g.row_ids().long(), g.col.long()
    pre = a_src[cols] if a_dst is None else a_dst[rows] + a_src[cols]
    if a_edge is not None and a_edge.size(0):
        eidc, has = _eid_clamped(g)
        eidc = eidc.long()
        ae = a_edge[eidc]
        pre = pre + (ae if has is None else torch.where(has[:, None], ae, torch.zeros_like(ae)))
    ds = ds * torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, slope))
    d_dst = d_src = d_edge = None
    det = deterministic()
    if which & _EA_DST and a_dst is not None:
        d_dst = _entry_sums(g, ds, False) if det else torch.zeros_like(a_dst).index_add_(0, rows, ds)
    if which & _EA_SRC:
        d_src = _entry_sums(g, ds, True) if det else torch.zeros_like(a_src).index_add_(0, cols, ds)
    if which & _EA_EDGE and a_edge is not None:
        d_edge = torch.zeros_like(a_edge)
        if a_edge.size(0):
            if has is None:
                d_edge[eidc] = ds
            else:
                d_edge[eidc[has]] = ds[has]
    return d_dst, d_src, d_edge


class _GatAlpha(torch.autograd.Function):
    """alpha[e, h] = softmax over destination row of leaky_relu(a_dst[row_e, h] + a_src[col_e, h]): one launch for all
    heads, scores never stored (mp_gat_alpha_f32)"""
    @staticmethod
    def forward(ctx, a_dst, a_src, g, slope):
        L = lib()
        ad = a_dst.contiguous().float()
        asr = a_src.contiguous().float()
        H = ad.size(1)
        alpha = _entry_empty(g.nnz, ad.device, H)
        with torch.cuda.device(ad.device):
            check(L.mp_gat_alpha_f32(ptr(g.rowptr), ptr(g.col), g.num_nodes, g.nnz, H, ptr(ad), ptr(asr), float(slope),
                                     ptr(alpha), _stream()), "mp_gat_alpha_f32")
        alpha = alpha[:g.nnz]
        ctx.g, ctx.slope = g, slope
        ctx.save_for_backward(alpha, ad, asr)
        return alpha

    @staticmethod
    def backward(ctx, dalpha):
        alpha, ad, asr = ctx.saved_tensors
        which = (_EA_DST if ctx.needs_input_grad[0] else 0) | (_EA_SRC if ctx.needs_input_grad[1] else 0)
        d_dst, d_src, _ = _alpha_bwd(ctx.g, alpha, dalpha, ad, asr, None, ctx.slope, which)
        return d_dst, d_src, None, None


def gat_alpha(g, a_dst, a_src, slope=0.2):
    """additive attention coefficients [nnz, H] for per-node terms a_dst, a_src [N, H] (idconv.py:319-327)"""
    return _GatAlpha.apply(a_dst, a_src, g, float(slope))


class _EdgeSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, s, g):
        L = lib()
        s = s.contiguous()
        heads = s.size(1)
        p = torch.empty_like(s)
        if g.nnz:               # (the entry point cannot see nnz: without entries s and p have no address)
            with torch.cuda.device(s.device):
                check(L.mp_csr_row_softmax_f32(ptr(g.rowptr), g.num_nodes, heads, ptr(s), ptr(p), _stream()),
                      "mp_csr_row_softmax_f32")
        ctx.g = g
        ctx.save_for_backward(p)
        return p

    @staticmethod
    def backward(ctx, dp):
        (p,) = ctx.saved_tensors
        return _raw_row_softmax_bwd(ctx.g, p, dp), None


def edge_softmax(g, s):
    """softmax of the per-entry scores over each destination row, per head; s [nnz, H]"""
    return _EdgeSoftmax.apply(s, g)


def _raw_heads_max_da(g, argmax, dy, V, heads, idx=None):
    """da[e, h] = sum over the columns c of head h that entry e won (argmax[row_e, c] == e) of dy[row_e, c] V[col_e, c]
    (mp_spmm_heads_max_da_f32; head layouts it does not take: per head on column slices).  idx [nnz] int32: the row of V
    an entry reads in the place of its column"""
    L = lib()
    nnz, d = g.nnz, V.size(1)
    idx = g.col if idx is None else idx
    da = _entry_empty(nnz, V.device, heads)
    with torch.cuda.device(V.device):
        st = L.mp_spmm_heads_max_da_f32(ptr(g.row_ids()), ptr(idx), nnz, ptr(argmax), argmax.stride(0), ptr(dy),
                                        dy.stride(0), ptr(V), V.stride(0), d, heads, ptr(da), _stream())
        if st != 2:
            check(st, "mp_spmm_heads_max_da_f32")
            return da[:nnz]
        dh = d // heads
        one = _entry_empty(nnz, V.device)
        for h in range(heads):
            cs = slice(h * dh, (h + 1) * dh)
            check(L.mp_spmm_heads_max_da_f32(ptr(g.row_ids()), ptr(idx), nnz, ptr(argmax[:, cs]), argmax.stride(0),
                                             ptr(dy[:, cs]), dy.stride(0), ptr(V[:, cs]), V.stride(0), dh, 1, ptr(one),
                                             _stream()), "mp_spmm_heads_max_da_f32")
            da[:, h] = one
    return da[:nnz]


# ---- the backward of y[i, slice h] = reduce_e w[e, h] V[col_e, slice h], once for spmm_edge_values and spmm_edge_heads ------
def _mean_dy(g, dy):
    """the mean's backward is the sum's on dy / (row entry count)"""
    return (dy / g.entry_counts().clamp(min=1.0)[:, None]).contiguous()


def _heads_grad_by_source(g, w, like, heads, is_max, dy, argmax=None):
    """the gradient of the operand gathered by source, shaped like `like`: max scatters w * dy through the argmax into
    zeros (float atomics; nothing to launch without entries) — under deterministic() it gathers them over the
    transposed pattern (mp::spmm_heads_max_bwd_pull_raw) —, sum aggregates dy over the transposed pattern with w
    permuted to its order; a mean's dy comes pre-divided (_mean_dy)"""
    if is_max and deterministic():
        from . import maxbwd_ops           # (imports this module: bound late); mp::spmm_heads_max_bwd_pull_raw's launcher
        return maxbwd_ops._raw_heads_max_bwd_pull(g, dy, argmax, w, heads)
    if is_max:
        dV = torch.zeros_like(like)
        if g.nnz:
            with torch.cuda.device(dy.device):
                check(lib().mp_spmm_heads_max_bwd_f32(ptr(g.col), ptr(w), heads, ptr(argmax), g.num_nodes, like.size(1),
                                                      ptr(dy), dy.stride(0), ptr(dV), dV.stride(0), _stream()),
                      "mp_spmm_heads_max_bwd_f32")
        return dV
    gt = g._transpose_sorted()     # (per-entry values are permuted through gt.pos: also when A^T = A)
    return _raw_spmm_heads(gt, w[gt.pos.long()].contiguous(), dy, heads)


def _heads_grad_weights(g, V, heads, is_max, dy, argmax=None, idx=None):
    """dw[e, h] = <dy[row_e], V[idx_e]>_h (idx: the entry's column by default): a per-entry dot — for max over the columns
    the entry won only; a mean's dy comes pre-divided"""
    if is_max:
        return _raw_heads_max_da(g, argmax, dy, V, heads, idx=idx)
    return _raw_sddmm_dot(g, dy, V, heads, 1.0, idx=idx)


class _SpmmEdgeValues(torch.autograd.Function):
    """y[i, slice h] = sum / mean / max over row i's entries e of a[e,h] V[col_e, slice h], differentiable in a and V.
    sum: da a per-entry dot, dV the aggregation over the transposed pattern; mean: the sum's backward on dy / (row entry
    count); max: dV scattered through the argmax (float atomics), da as a masked per-entry dot"""
    @staticmethod
    def forward(ctx, a, V, g, heads, reduce):
        # a dense [nnz, H]: the kernels (the dV scatter of max among them) read a[e * H + h], whatever the caller's strides
        a, V = _f32c(a.reshape(g.nnz, heads), "a").contiguous(), _f32c(V, "V")
        y, argmax = _raw_spmm_heads_reduce(g, a, V, heads, reduce)
        ctx.g, ctx.heads, ctx.reduce = g, heads, reduce
        ctx.save_for_backward(a, V, argmax)
        return y

    @staticmethod
    def backward(ctx, dy):
        a, V, argmax = ctx.saved_tensors
        g, heads = ctx.g, ctx.heads
        dy = dy.contiguous()
        is_max = ctx.reduce == _lib.MAX
        if ctx.reduce == _lib.MEAN:
            dy = _mean_dy(g, dy)
        da = _heads_grad_weights(g, V, heads, is_max, dy, argmax) if ctx.needs_input_grad[0] else None
        dV = _heads_grad_by_source(g, a, V, heads, is_max, dy, argmax) if ctx.needs_input_grad[1] else None
        return da, dV, None, None, None


def spmm_edge_values(g, a, V, heads=1, reduce="sum"):
    """y[i, slice h] = reduce over row i's entries e of a[e,h] V[col_e, slice h]; a [nnz, H], V [n, d] fp32.
    reduce: "sum" (or "add"), "mean", "max" (argmax ties: the first entry in CSR order)"""
    return _SpmmEdgeValues.apply(a, V, g, int(heads), _checked_reduce(reduce))


# =========================================================================================
# Registered operators: torch.ops.mp.*
#
# The path's operators as PyTorch custom ops (torch.library): schemas, fake (meta) kernels for tracing /
# torch.compile / opcheck, autograd formulas built from other registered ops.  A graph crosses the boundary as
# an int handle (CSRGraph.handle): custom ops take tensors and scalars only, and the CSR, its plan and its cached
# transpose belong to the batch, not to a call.  `*_raw` ops have no autograd: a launcher behind a schema (one launch,
# one ladder of launches, or a backward step composed of a few); the un-suffixed ops are what the layers call, and their
# backward formulas call `*_raw` ops.  Every op has its explicit signature and one register_fake line (the last block of
# the file); the BatchNorm and loss ops (mp::bn_*, mp::softmax_ce) live in nn.py.
#
#   mp::spmm            y = act(reduce_j w_ij x_j + s x_i + b)         SparseAdj.matmul, sparse_adj.py:91-97
#       spmm_raw (any graph variant, argmax on request), spmm_rows_raw, spmm_max_bwd_raw
#       (the max backward without atomics, deterministic(): spmm_max_bwd_pull_raw / spmm_heads_max_bwd_pull_raw of
#       graphgym_amd/maxbwd_ops.py)
#   mp::idgnn_agg       (P, Q) = (A x, A S x)                          gcn_id two-branch form, TfgIDLayer.py:510-517
#       idgnn_agg_raw
#   mp::agg_dense       act((A x + s x) W + b), one launch             aggregate -> kernel product, TfgIDLayer.py:510-523
#   mp::agg_dense_id    act(A (x W + S x W_id) + b)                    gcn_id / GCNIDConvLayer, idconv.py:150-177
#       agg_dense_raw, agg_dense_id_raw, id_branch_t_raw
#   mp::dense_fused     act(P W [+ Q W_id] + b)                        the transform after the aggregation
#       dense_fused_raw, dense_wgrad_raw, dense_wgrad_relu_raw
#   mp::spmm_edge       y = reduce_e w_e (x_j + m_e + t_i) + b         GeneralEdgeConvLayer.message, generalconv.py:203-209
#       spmm_edge_raw, spmm_edge_bwd_raw (dm), spmm_edge_dt_raw (dt)
#   mp::edge_att_alpha  softmax_i lrelu(a_dst_i + a_src_j + a_edge_e)  GeneralEdgeAttConvv1Layer.message, attconv.py:352-357
#       edge_att_alpha_bwd_raw (d_dst, d_src, d_edge by the bits of `want`)
#   mp::spmm_edge_heads y = reduce_e w_eh (x_j + m_e + t_i)^h + b      ... attconv.py:358-360
#       spmm_edge_heads_bwd_raw (dw, dx, dm, dt by the bits of `want`)
#   mp::embed_sum       out_r = sum_k table[off_k + codes_rk]          AtomEncoder.forward, feature_encoder.py:74-81
#       embed_sum_bwd_raw
#   mp::spmm_code       y = reduce_e w_e (x_j + table[q_e]) + b        GeneralOGBConvLayer.message, generalconv_ogb.py:115-118
#       spmm_code_bwd_raw (dtable)
# =========================================================================================
from typing import List, Optional, Tuple   # noqa: E402

from torch.library import custom_op, register_autograd   # noqa: E402

from .graph import from_handle   # noqa: E402

Tensor = torch.Tensor


# ---- what the registered operators share ------------------------------------------------------------------------------
# An operator can return neither None nor one tensor twice: a result that is not computed comes back as an EMPTY (0,)
# tensor of its own.  Each family has one results function.  Called with the op's arguments it is the family's fake kernel
# (every op keeps its own register_fake line, at the end of the file); given `launched`, what the launcher returned, with
# None for what it did not write, it makes the real op's results: what comes back empty is written once per family.
def _none_if_empty(t):
    return None if t is None or t.numel() == 0 else t


def _empty_like_none(ref, dtype=torch.float32):
    return torch.empty((0,), dtype=dtype, device=ref.device)


def _or_empty(ref, results, dtype=torch.float32):
    return tuple(_empty_like_none(ref, dtype) if t is None else t for t in results)


def _op_rows(graph, variant=0):
    """rows of a graph variant: the transposed operators (1, 2) have one row per column"""
    g = from_handle(graph)
    return g.num_nodes if variant == 0 else g.num_cols


def _agg_results(x, graph, want_argmax, variant=0, launched=None):
    """(y [n, d], argmax [n, d] int32 or EMPTY) of spmm, spmm_edge, spmm_edge_heads, spmm_code and the *_raw ops under
    them; the un-suffixed ops write the argmax for max and only then"""
    if launched is not None:
        return _or_empty(x, launched, torch.int32)
    shape = (_op_rows(graph, variant), x.size(1))
    return x.new_empty(shape), x.new_empty(shape if want_argmax else (0,), dtype=torch.int32)


def _agg_dense_results(x, W, graph, want_P, variant=0, id_index=None, launched=None):
    """(out [n, W columns], the aggregated rows P [n, d] or EMPTY [, x[id]]) of agg_dense, agg_dense_id and their *_raw
    ops; P comes back only when asked for, also where the two-kernel order had to compute it"""
    if launched is not None:
        out, P, *x_id = launched
        return _or_empty(x, (out, P if want_P else None, *x_id))
    x_id = () if id_index is None else (x.new_empty((id_index.numel(), x.size(1))),)
    n = _op_rows(graph, variant)
    return (x.new_empty((n, W.size(1))), x.new_empty((n, x.size(1)) if want_P else (0,)), *x_id)


def _wgrad_results(X, G, want_w=True, want_b=False, want_gm=None, launched=None):
    """(X^T g [F, d] or EMPTY, the column sums of g [d] or EMPTY [, the masked gradient g [M, d] or EMPTY]) of
    dense_wgrad_raw and (want_gm given) dense_wgrad_relu_raw"""
    if launched is not None:
        return _or_empty(G, launched)
    gm = () if want_gm is None else (G.new_empty(G.shape if want_gm else (0,)),)
    return (G.new_empty((X.size(1), G.size(1)) if want_w else (0,)), G.new_empty((G.size(1),) if want_b else (0,)), *gm)


def _idgnn_results(x, graph):
    """(P, Q), both [N, d]"""
    shape = (_op_rows(graph), x.size(1))
    return x.new_empty(shape), x.new_empty(shape)


# The `want` protocol of the *_bwd_raw ops that return several gradients: gradient i is computed when bit i of `want` is
# set and its operand exists, and comes back EMPTY otherwise.  The backward formula packs the bits (_want_bits) and turns
# the results it did not ask for into None (_want_grads); _want_results is the ops' results function (shapes[i] None:
# the operand does not exist).
def _want_bits(*needs):
    return sum(1 << i for i, need in enumerate(needs) if need)


def _want_results(ref, want, shapes=None, launched=None):
    if launched is not None:
        return _or_empty(ref, launched)
    return tuple(ref.new_empty(shape if (want >> i & 1 and shape is not None) else (0,)) for i, shape in enumerate(shapes))


def _want_grads(want, results):
    return tuple(t if want >> i & 1 else None for i, t in enumerate(results))


def _graph_setup(ctx, graph, reduce=None, bias=None):
    """the common lines of the graph ops' setup_context: no zero-filled gradients for the outputs nobody used (the saved
    rows, the argmax), the handle and — to keep it alive until the backward — the graph itself"""
    ctx.set_materialize_grads(False)
    ctx.graph, ctx.g_alive = graph, from_handle(graph)
    ctx.reduce, ctx.has_bias = reduce, bias is not None


def _bias_grad(dy, bf16_to=None):
    """the column sums of dy; bf16_to (spmm alone has a bf16 form): a dy that is not float32 is summed in fp32 and cast"""
    if bf16_to is None or dy.dtype == torch.float32:
        return dy.sum(0)
    return dy.float().sum(0).to(bf16_to)


def _transposed_variant(reduce):
    """the graph variant that carries the backward of a sum (1: the transpose) or a mean (2: its entries w / count(row))"""
    return 1 if reduce == _lib.SUM else 2


def _grad_by_source(graph, reduce, dy, argmax, self_scale=0.0):
    """the gradient of the operand a plain aggregation gathers by source (spmm; x of spmm_edge and spmm_code): max scatters
    dy through the argmax (float atomics; under deterministic() the pull form gathers it), sum and mean run the same kernel on the transposed operator; a self term
    self_scale * x[i] adds self_scale * dy"""
    if reduce == _lib.MAX:
        if deterministic():
            from . import maxbwd_ops  # noqa: F401  (registers the op; imports this module: bound late)
            dx = torch.ops.mp.spmm_max_bwd_pull_raw(dy, argmax, graph)
        else:
            dx = torch.ops.mp.spmm_max_bwd_raw(dy, argmax, graph)
        return dx + self_scale * dy if self_scale != 0.0 else dx
    return torch.ops.mp.spmm_raw(dy, graph, _transposed_variant(reduce), _lib.SUM, dy if self_scale != 0.0 else None,
                                 self_scale, None, False, False)[0]


def _checked_reduce(reduce):
    """the engine's code of the reduce name a public wrapper was given"""
    if reduce not in _lib.REDUCE:
        raise ValueError(f"reduce must be one of {sorted(_lib.REDUCE)}, got {reduce!r}")
    return _lib.REDUCE[reduce]


def _check_edge_f32(op, keys, **operands):
    """the float32 check of an edge-feature wrapper on the operands it was given, in their order"""
    for name, v in operands.items():
        if v is not None:
            _edge_f32(v, name, op, keys)


# ---- raw launches -------------------------------------------------------------------------
@custom_op("mp::spmm_raw", mutates_args=(), device_types="cuda")
def _op_spmm_raw(x: Tensor, graph: int, variant: int, reduce: int, S: Optional[Tensor], self_scale: float,
                 bias: Optional[Tensor], relu: bool, want_argmax: bool) -> Tuple[Tensor, Tensor]:
    g = from_handle(graph).variant(variant)
    x = _agg_in(x, "x")
    if x.size(0) != g.num_cols:
        raise ValueError(f"x has {x.size(0)} rows, the operator has {g.num_cols} columns")
    Sc = None if S is None else (_f32c(S, "S") if x.dtype == torch.float32 else _agg_in(S, "S"))
    return _agg_results(x, graph, want_argmax, variant, launched=_raw_spmm(
        g, x, reduce, S=Sc, self_scale=self_scale, bias=None if bias is None else bias.contiguous(), relu=relu,
        want_argmax=want_argmax))


@custom_op("mp::spmm_rows_raw", mutates_args=(), device_types="cuda")
def _op_spmm_rows_raw(x: Tensor, graph: int, variant: int, rows: Tensor) -> Tensor:
    """sum aggregation over the listed rows only of a graph variant: an [len(rows), n] operator"""
    sub = from_handle(graph).variant(variant).select_rows(rows)
    y, _ = _raw_spmm(sub, _agg_in(x, "x"), _lib.SUM)
    return y


@custom_op("mp::spmm_max_bwd_raw", mutates_args=(), device_types="cuda")
def _op_spmm_max_bwd_raw(dy: Tensor, argmax: Tensor, graph: int) -> Tensor:
    g = from_handle(graph)
    dy = dy.contiguous()
    N, d = dy.shape
    dx = torch.zeros((g.num_cols, d), dtype=torch.float32, device=dy.device)
    if g.nnz == 0:              # no entry won anything (the entry point cannot see nnz: col has no address)
        return dx.to(dy.dtype)
    # a bf16 gradient is accumulated in fp32 and rounded once
    name = "mp_spmm_max_bwd_bf16" if dy.dtype == torch.bfloat16 else "mp_spmm_max_bwd_f32"
    with torch.cuda.device(dy.device):
        check(getattr(lib(), name)(ptr(g.col), ptr(g.val), ptr(argmax), ptr(dy), dy.stride(0), N, d, ptr(dx),
                                   dx.stride(0), _stream()), name)
    return dx.to(dy.dtype)


@custom_op("mp::idgnn_agg_raw", mutates_args=(), device_types="cuda")
def _op_idgnn_agg_raw(x: Tensor, graph: int, id_index: Tensor) -> Tuple[Tensor, Tensor]:
    g = from_handle(graph)
    x = _agg_in(x, "x")
    L = lib()
    N, d = g.num_nodes, x.size(1)
    P = placement.empty_or_torch((N, d), x.device, reads=(x,), dtype=x.dtype)
    Q = placement.empty_or_torch((N, d), x.device, reads=(x,), dtype=x.dtype)
    if (x.dtype == torch.float32 and d in AGG_TILES_WIDTHS and N >= AGG_TILES_MIN_ROWS
            and os.environ.get("MP_AGG_TILES", "1") != "0"
            and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0 and g.nnz > 0 and id_index.numel() > 0
            and g.max_row_entries() <= FUSED_MAX_ROW):
        # the tile structure (round 4): P in the pass of mp_agg_rows_tiles_f32, which also writes the zero rows of Q;
        # the rows of Q next to an identity node come from their few identity entries, gathered from x[id] by a small
        # kernel the call launches behind the tile kernel
        global AGG_TILES_CALLS
        AGG_TILES_CALLS += 1
        br = g.id_branch(id_index)
        Z = x.index_select(0, id_index.to(torch.int64))
        with torch.cuda.device(x.device):
            check(L.mp_idgnn_agg_tiles_f32(ptr(g.rowptr), ptr(g.col), ptr(g.val), N, ptr(x), x.stride(0), d, ptr(br.defer),
                                           ptr(br.rows), ptr(br.crp), ptr(br.slot), ptr(br.val), br.n_rows, ptr(Z),
                                           Z.stride(0), ptr(P), P.stride(0), ptr(Q), Q.stride(0), _stream()),
                  "mp_idgnn_agg_tiles_f32")
        return P, Q
    # plan-based: mp_idgnn_agg_f32, or mp_idgnn_agg_bf16 (fp32 accumulation); the tile kernels have no bf16 form
    name = "mp_idgnn_agg_bf16" if x.dtype == torch.bfloat16 else "mp_idgnn_agg_f32"
    col_marked = g.mark_ids(id_index)
    plan, counts, ws, ws_bytes = _plan_ws(g, x.device, d, _lib.SUM, True)
    with torch.cuda.device(x.device):
        check(getattr(L, name)(ptr(g.rowptr), ptr(col_marked), ptr(g.val), N, ptr(plan), counts,
                               ptr(x), x.stride(0), ptr(P), P.stride(0), ptr(Q), Q.stride(0), d,
                               ptr(ws), ws_bytes, _stream()), name)
    return P, Q


def _agg_dense_kernel_ok(g, x, W, S=None, reduce=_lib.SUM):
    """the one-kernel aggregate -> transform covers these operands (shapes, alignment, row lengths; a mean with a self
    term is outside it: mp_agg_dense_f32 refuses that pair)"""
    return (agg_dense_supported(g, x, W) and x.dtype == torch.float32 and not (reduce == _lib.MEAN and S is not None)
            and (S is None or (S.stride(0) % 4 == 0 and S.data_ptr() % 16 == 0)))


@custom_op("mp::agg_dense_raw", mutates_args=(), device_types="cuda")
def _op_agg_dense_raw(x: Tensor, W: Tensor, bias: Optional[Tensor], graph: int, variant: int, reduce: int,
                      S: Optional[Tensor], self_scale: float, relu: bool, want_P: bool) -> Tuple[Tensor, Tensor]:
    """act((reduce_j w_ij x_j + s S_i) W + b): ONE launch where mp_agg_dense_f32 covers the operands, otherwise the
    aggregation kernel followed by the fused transform; returns (out, aggregated rows or an empty tensor)"""
    g = from_handle(graph).variant(variant)
    x = _agg_in(x, "x")
    Sc = None if S is None else (_f32c(S, "S") if x.dtype == torch.float32 else _agg_in(S, "S"))
    Wd = W.detach()
    if _agg_dense_kernel_ok(g, x, Wd, Sc, reduce):
        out, P = _raw_agg_dense(g, x, Wd, None if bias is None else bias.detach(), relu, S=Sc,
                                self_scale=self_scale, want_P=want_P, reduce=reduce)
    else:
        P, _ = _raw_spmm(g, x, reduce, S=Sc, self_scale=self_scale)
        out = _dense_any(P, Wd, None, None, bias, relu)
    return _agg_dense_results(x, W, graph, want_P, variant, launched=(out, P))


@custom_op("mp::agg_dense_id_raw", mutates_args=(), device_types="cuda")
def _op_agg_dense_id_raw(x: Tensor, W: Tensor, W_id: Tensor, bias: Optional[Tensor], graph: int, id_index: Tensor,
                         self_scale: float, relu: bool, want_P: bool) -> Tuple[Tensor, Tensor, Tensor]:
    """act((A x + s x) W + b + A_id Z), Z = x[id] W_id: the one-kernel layer with the activation deferred on the rows
    next to an identity node, then mp_id_fixup_f32 on those rows; returns (out, aggregated rows or empty, x[id])"""
    g = from_handle(graph)
    x = _f32c(x, "x")
    br = g.id_branch(id_index)
    ids = id_index.to(torch.int64)
    x_id = x.index_select(0, ids)
    Z = torch.mm(x_id, W_id.detach())
    Wd = W.detach()
    S = x if self_scale != 0.0 else None
    b = None if bias is None else bias.detach()
    if _agg_dense_kernel_ok(g, x, Wd, S):
        out, P = _raw_agg_dense(g, x, Wd, b, relu, S=S, self_scale=self_scale, want_P=want_P, defer_act=br.defer)
        act = _lib.ACT_RELU if relu else _lib.ACT_NONE
    else:   # shapes outside the one-kernel layer: aggregation kernel, transform without activation, then the fix-up
        P, _ = _raw_spmm(g, x, _lib.SUM, S=S, self_scale=self_scale)
        out = _dense_any(P, Wd, None, None, b, False)
        act = _lib.ACT_NONE
    with torch.cuda.device(x.device):
        check(lib().mp_id_fixup_f32(ptr(br.rows), ptr(br.crp), ptr(br.slot), ptr(br.val), br.n_rows, ptr(Z),
                                    Z.stride(0), ptr(out), out.stride(0), out.size(1), act, _stream()),
              "mp_id_fixup_f32")
    if relu and act == _lib.ACT_NONE:
        out = torch.relu_(out)
    return _agg_dense_results(x, W, graph, want_P, id_index=id_index, launched=(out, P, x_id))


@custom_op("mp::id_branch_t_raw", mutates_args=(), device_types="cuda")
def _op_id_branch_t_raw(gm: Tensor, graph: int, id_index: Tensor) -> Tensor:
    """T = A_id^T g  [n_id, d]: the gradient reaching Z = x[id] W_id"""
    br = from_handle(graph).id_branch(id_index)
    T, _ = _raw_spmm(br.t, _f32c(gm, "g"), _lib.SUM)
    return T


def _dense_any(P, W, Q, W_id, bias, relu):
    """act(P W [+ Q W_id] + b): the engine's MFMA kernel where it pays / applies, library GEMMs otherwise (bf16: library
    GEMMs, bias and ReLU)"""
    if P.dtype == torch.bfloat16:
        _require_hip(P, "P")
        out = P @ W.to(P.dtype)
        if Q is not None:
            out = out + Q @ W_id.to(P.dtype)
        if bias is not None:
            out = out + bias.to(P.dtype)
        return torch.relu(out) if relu else out
    Pc = _f32c(P, "P")
    Qc = None if Q is None else _f32c(Q, "Q")
    out = None
    if Qc is None and bias is None and not relu and not dense_x3_supported(Pc, Pc.size(1), W.size(1)):
        # a plain product outside the streaming kernel's shapes has nothing to fuse: the library GEMM; the general
        # MFMA kernel earns its keep when bias / activation / a second product ride along
        return torch.mm(Pc, W)
    out = _raw_dense_fused(Pc, W, Qc, W_id, bias, relu)
    if out is None:     # shape outside the fused kernel: library GEMMs
        out = Pc @ W
        if Qc is not None:
            out = out + Qc @ W_id
        if bias is not None:
            out = out + bias
        if relu:
            out = torch.relu(out)
    return out


@custom_op("mp::dense_fused_raw", mutates_args=(), device_types="cuda")
def _op_dense_fused_raw(P: Tensor, W: Tensor, Q: Optional[Tensor], W_id: Optional[Tensor], bias: Optional[Tensor],
                        relu: bool) -> Tensor:
    return _dense_any(P, W.detach(), Q, None if W_id is None else W_id.detach(),
                      None if bias is None else bias.detach(), relu)


@custom_op("mp::dense_wgrad_raw", mutates_args=(), device_types="cuda")
def _op_dense_wgrad_raw(X: Tensor, G: Tensor, want_w: bool, want_b: bool) -> Tuple[Tensor, Tensor]:
    """(X^T G, column sums of G) in one pass over G (either may be skipped: an empty tensor comes back)"""
    return _wgrad_results(X, G, launched=_wgrad_and_bias(X, G.contiguous() if G.stride(-1) != 1 else G, want_w, want_b))


@custom_op("mp::dense_wgrad_relu_raw", mutates_args=(), device_types="cuda")
def _op_dense_wgrad_relu_raw(X: Tensor, G: Tensor, Y: Tensor, want_b: bool,
                             want_gm: bool = True) -> Tuple[Tensor, Tensor, Tensor]:
    """(X^T gm, column sums of gm, gm) with gm = G * [Y > 0]: the ReLU backward folded into the weight-gradient pass;
    want_gm False: gm is not written (nobody reads it) and comes back empty"""
    Gc = G if (G.stride(-1) == 1 and G.dim() == 2) else G.contiguous()
    Yc = Y if Y.stride(-1) == 1 else Y.contiguous()
    Xc = X if X.stride(-1) == 1 else X.contiguous()
    r = _raw_dense_wgrad_relu(Xc, Gc, Yc, want_bias=want_b, want_gm=want_gm) if Gc.dtype == torch.float32 else None
    if r is None:     # shape outside the kernel: separate passes
        gm = torch.ops.aten.threshold_backward(Gc, Yc, 0.0)
        r = _wgrad_and_bias(Xc, gm, True, want_b) + (gm if want_gm else None,)
    return _wgrad_results(X, G, launched=r)


def _masked_grads(P, gout, out, relu, need_w, need_b, need_gm=True):
    """(gm, dW, db) for a transform with an optional ReLU epilogue: with ReLU and a weight gradient wanted the mask rides
    in the weight-gradient pass (one kernel); otherwise threshold_backward / plain weight gradient.  need_gm False
    (no input gradient will be taken): gm may come back None and is not written."""
    if relu and need_w and P is not None and P.numel() > 0:
        dW, db, gm = torch.ops.mp.dense_wgrad_relu_raw(P, gout, out, need_b, need_gm)
        return (gm if need_gm else None), dW, _none_if_empty(db)
    gm = gout.contiguous()
    if relu:
        gm = torch.ops.aten.threshold_backward(gm, out, 0.0)
    if need_w or need_b:
        dW, db = torch.ops.mp.dense_wgrad_raw(P, gm, need_w, need_b)
        return gm, _none_if_empty(dW), _none_if_empty(db)
    return gm, None, None


# ---- differentiable operators ---------------------------------------------------------------
@custom_op("mp::spmm", mutates_args=(), device_types="cuda")
def _op_spmm(x: Tensor, graph: int, reduce: int, self_scale: float, bias: Optional[Tensor],
             relu: bool) -> Tuple[Tensor, Tensor]:
    return torch.ops.mp.spmm_raw(x, graph, 0, reduce, x if self_scale != 0.0 else None, self_scale, bias, relu,
                                 reduce == _lib.MAX)


def _spmm_setup(ctx, inputs, output):
    x, graph, reduce, self_scale, bias, relu = inputs
    y, argmax = output
    _graph_setup(ctx, graph, reduce, bias)
    ctx.self_scale, ctx.relu = self_scale, relu
    ctx.bias_dtype = None if bias is None else bias.dtype
    ctx.save_for_backward(y if relu else None, argmax)


def _spmm_backward(ctx, dy, _dargmax):
    y, argmax = ctx.saved_tensors
    if dy is None:
        return None, None, None, None, None, None
    dy = dy.contiguous()
    if ctx.relu:
        dy = torch.ops.aten.threshold_backward(dy, y, 0.0)    # one vectorised pass
    dbias = _bias_grad(dy, bf16_to=ctx.bias_dtype) if (ctx.has_bias and ctx.needs_input_grad[4]) else None
    dx = _grad_by_source(ctx.graph, ctx.reduce, dy, argmax, ctx.self_scale) if ctx.needs_input_grad[0] else None
    return dx, None, None, None, dbias, None


register_autograd("mp::spmm", _spmm_backward, setup_context=_spmm_setup)


def spmm(g, x, reduce="sum", self_scale=0.0, bias=None, relu=False):
    """y[i] = act( reduce_{j in N(i)} w_ij x[j] + self_scale * x[i] + bias )   (torch.ops.mp.spmm)

    reduce: 'sum'/'add' | 'mean' | 'max'.  The gradient flows to x and bias; entry values
    of g are constants here (attention weights go through spmm_edge_values)."""
    _require_hip(x, "x")
    r = _lib.REDUCE[reduce]
    if r == _lib.MAX and not (torch.is_grad_enabled() and (x.requires_grad or (bias is not None and bias.requires_grad))):
        # nothing will be differentiated: no argmax written (and the tile kernel may take the launch)
        return torch.ops.mp.spmm_raw(x, g.handle, 0, r, x if self_scale != 0.0 else None, float(self_scale), bias,
                                     bool(relu), False)[0]
    return torch.ops.mp.spmm(x, g.handle, r, float(self_scale), bias, bool(relu))[0]


@custom_op("mp::idgnn_agg", mutates_args=(), device_types="cuda")
def _op_idgnn_agg(x: Tensor, graph: int, id_index: Tensor) -> Tuple[Tensor, Tensor]:
    return torch.ops.mp.idgnn_agg_raw(x, graph, id_index)


def _idgnn_setup(ctx, inputs, output):
    x, graph, id_index = inputs
    _graph_setup(ctx, graph)
    ctx.save_for_backward(id_index)


def _idgnn_backward(ctx, dP, dQ):
    (id_index,) = ctx.saved_tensors
    if dP is None and dQ is None:
        return None, None, None
    if dP is None:                            # only Q was used downstream
        dP = torch.zeros_like(dQ)
    dx = torch.ops.mp.spmm_raw(dP.contiguous(), ctx.graph, 1, _lib.SUM, None, 0.0, None, False, False)[0]
    if dQ is None:
        return dx, None, None
    # Q = A S x  =>  dx[id] += (A^T dQ)[id]: only the identity nodes' rows of A^T are needed, an
    # aggregation over their out-edges alone (an [n_id, N] operator), not a second full pass
    t = torch.ops.mp.spmm_rows_raw(dQ.contiguous(), ctx.graph, 1, id_index)
    return dx.index_add(0, id_index.to(torch.int64), t), None, None


register_autograd("mp::idgnn_agg", _idgnn_backward, setup_context=_idgnn_setup)


def idgnn_aggregate(g, id_index, x, col_marked=None):
    """(P, Q) with P = A x and Q = A S x, S selecting the identity nodes' rows: one pass over
    the edges.  P @ W + Q @ W_id equals A (x W + S x W_id) of gcn_id (TfgIDLayer.py:510-517)."""
    _require_hip(x, "x")
    return torch.ops.mp.idgnn_agg(x, g.handle, id_index)


@custom_op("mp::dense_fused", mutates_args=(), device_types="cuda")
def _op_dense_fused(P: Tensor, W: Tensor, Q: Optional[Tensor], W_id: Optional[Tensor], bias: Optional[Tensor],
                    relu: bool) -> Tensor:
    return torch.ops.mp.dense_fused_raw(P, W, Q, W_id, bias, relu)


def _dense_setup(ctx, inputs, output):
    P, W, Q, W_id, bias, relu = inputs
    ctx.relu, ctx.has_q, ctx.has_bias = relu, Q is not None, bias is not None
    ctx.save_for_backward(P, W, Q, W_id, output if relu else None)


def _dense_backward(ctx, g):
    P, W, Q, W_id, out = ctx.saved_tensors
    need = ctx.needs_input_grad
    # the weight and bias gradients come out of one pass of the engine's split-K kernel, which also applies the ReLU
    # mask to g on the way; g @ W^T is the streaming transform with W^T (library GEMM outside its shapes)
    need_gm = need[0] or (ctx.has_q and (need[2] or need[3]))
    g, dW, db = _masked_grads(P, g, out, ctx.relu, need[1], ctx.has_bias and need[4], need_gm)
    dP = times_wt(g, W) if need[0] else None
    dQ = times_wt(g, W_id) if (ctx.has_q and need[2]) else None
    dWid = torch.ops.mp.dense_wgrad_raw(Q, g, True, False)[0] if (ctx.has_q and need[3]) else None
    return dP, dW, dQ, dWid, db, None


register_autograd("mp::dense_fused", _dense_backward, setup_context=_dense_setup)


def dense_fused(P, W, Q=None, W_id=None, bias=None, relu=False):
    """act(P @ W [+ Q @ W_id] + bias) in one kernel (torch.ops.mp.dense_fused; mp_dense_fused_f32)"""
    _require_hip(P, "P")
    return torch.ops.mp.dense_fused(P, W, Q, W_id, bias, bool(relu))


@custom_op("mp::agg_dense", mutates_args=(), device_types="cuda")
def _op_agg_dense(x: Tensor, W: Tensor, bias: Optional[Tensor], graph: int, reduce: int, self_scale: float,
                  relu: bool, want_P: bool) -> Tuple[Tensor, Tensor]:
    return torch.ops.mp.agg_dense_raw(x, W, bias, graph, 0, reduce, x if self_scale != 0.0 else None, self_scale, relu,
                                      want_P)


def _agg_dense_setup(ctx, inputs, output):
    x, W, bias, graph, reduce, self_scale, relu, want_P = inputs
    out, P = output
    _graph_setup(ctx, graph, reduce, bias)
    ctx.self_scale, ctx.relu, ctx.want_P = self_scale, relu, want_P
    ctx.save_for_backward(P, W, out if relu else None, None if want_P else x)


def _agg_rows_again(ctx, x):
    """the aggregated rows P of agg_dense / agg_dense_id where the forward did not keep them (called outside grad mode
    bookkeeping) and the weight gradient needs them"""
    return torch.ops.mp.spmm_raw(x, ctx.graph, 0, ctx.reduce, x if ctx.self_scale != 0.0 else None, ctx.self_scale, None,
                                 False, False)[0]


def _agg_dense_dx(ctx, gm, W):
    """(A^T g + s g) W^T: the same one-kernel layer on the transposed operator"""
    return torch.ops.mp.agg_dense_raw(gm, W.t().contiguous(), None, ctx.graph, _transposed_variant(ctx.reduce), _lib.SUM,
                                      gm if ctx.self_scale != 0.0 else None, ctx.self_scale, False, False)[0]


def _agg_dense_backward(ctx, gout, _gP):
    P, W, out, x = ctx.saved_tensors
    need = ctx.needs_input_grad
    if gout is None:
        return None, None, None, None, None, None, None, None
    if not ctx.want_P and need[1]:
        P = _agg_rows_again(ctx, x)
    gm, dW, db = _masked_grads(P, gout, out, ctx.relu, need[1], ctx.has_bias and need[2], need[0])
    return (_agg_dense_dx(ctx, gm, W) if need[0] else None), dW, db, None, None, None, None, None


register_autograd("mp::agg_dense", _agg_dense_backward, setup_context=_agg_dense_setup)


def agg_dense(g, x, W, bias=None, relu=False, self_scale=0.0, reduce="sum"):
    """act((reduce_{j in N(i)} w_ij x[j] + self_scale * x[i]) W + bias)  (torch.ops.mp.agg_dense): aggregation and
    the feature transform that follows it in ONE kernel (mp_agg_dense_f32) when the shapes allow
    (agg_dense_supported), otherwise the aggregation kernel followed by the fused transform"""
    _require_hip(x, "x")
    if g.num_cols != g.num_nodes and self_scale != 0.0:
        raise ValueError("the self term needs a square operator")
    if _lib.REDUCE[reduce] == _lib.MAX:
        # the backward runs on the transposed (mean) operator: a max has no such form, and no layer asks for it
        raise ValueError("agg_dense takes reduce 'sum' / 'add' or 'mean', not 'max' (spmm + dense_fused has the max)")
    want_P = torch.is_grad_enabled() and W.requires_grad     # inference: no aggregated rows written
    return torch.ops.mp.agg_dense(x, W, bias, g.handle, _lib.REDUCE[reduce], float(self_scale), bool(relu), want_P)[0]


@custom_op("mp::agg_dense_id", mutates_args=(), device_types="cuda")
def _op_agg_dense_id(x: Tensor, W: Tensor, W_id: Tensor, bias: Optional[Tensor], graph: int, id_index: Tensor,
                     self_scale: float, relu: bool, want_P: bool) -> Tuple[Tensor, Tensor, Tensor]:
    return torch.ops.mp.agg_dense_id_raw(x, W, W_id, bias, graph, id_index, self_scale, relu, want_P)


def _agg_dense_id_setup(ctx, inputs, output):
    x, W, W_id, bias, graph, id_index, self_scale, relu, want_P = inputs
    out, P, x_id = output
    _graph_setup(ctx, graph, _lib.SUM, bias)
    ctx.self_scale, ctx.relu, ctx.want_P = self_scale, relu, want_P
    ctx.save_for_backward(P, W, W_id, x_id, id_index, out if relu else None, None if want_P else x)


def _agg_dense_id_backward(ctx, gout, _gP, _gxid):
    P, W, W_id, x_id, id_index, out, x = ctx.saved_tensors
    need = ctx.needs_input_grad
    if gout is None:
        return None, None, None, None, None, None, None, None, None
    if not ctx.want_P and need[1]:
        P = _agg_rows_again(ctx, x)
    gm, dW, db = _masked_grads(P, gout, out, ctx.relu, need[1], ctx.has_bias and need[3], need[0] or need[2])
    # identity branch: T = A_id^T g [n_id, d_out];  dW_id = x_id^T T ;  dx[id] += T W_id^T
    T = torch.ops.mp.id_branch_t_raw(gm, ctx.graph, id_index) if (need[0] or need[2]) else None
    dWid = torch.mm(x_id.t(), T) if need[2] else None
    dx = None
    if need[0]:
        dx = _agg_dense_dx(ctx, gm, W).index_add(0, id_index.to(torch.int64), torch.mm(T, W_id.t()))
    return dx, dW, dWid, db, None, None, None, None, None


register_autograd("mp::agg_dense_id", _agg_dense_id_backward, setup_context=_agg_dense_id_setup)


def agg_dense_id(g, x, W, W_id, id_index, bias=None, relu=False, self_scale=0.0):
    """act(A (x W + S x W_id) + bias) with S selecting the identity nodes' rows (torch.ops.mp.agg_dense_id): one
    aggregate -> transform launch plus the identity branch's small product and row fix-up; None when the shapes are
    outside the one-kernel layer (the caller then runs idgnn_aggregate + dense_fused)"""
    _require_hip(x, "x")
    if not (agg_dense_supported(g, x, W) and x.dtype == torch.float32 and g.num_cols == g.num_nodes):
        return None
    want_P = torch.is_grad_enabled() and W.requires_grad
    return torch.ops.mp.agg_dense_id(x, W, W_id, bias, g.handle, id_index, float(self_scale), bool(relu), want_P)[0]


# ---- two-gather aggregation: messages with an edge feature (generalconv.py:203-209) ---------------------------------
_EDGE_KEYS = "keys generaledgeconv and generalsampleedgeconv"
_EDGE_ATT_KEYS = "attention keys generaledgeattconvv1 and generaledgeattconvv2"


def _edge_f32(t, name, op, keys):
    """an operand of `op`, one of the operators with an edge feature (`keys`: the layer keys it serves, for the
    message): float32 only, rows unit-stride"""
    _require_hip(t, name)
    if t.dtype != torch.float32:
        raise TypeError(f"{op} is float32 only: {name} is {t.dtype} (the edge-feature {keys} have no bfloat16 or "
                        "float16 form)")
    return t if t.dim() == 2 and t.stride(1) == 1 else t.contiguous()


def _edge_operands(g, op, keys, x, m, t, bias):
    """x, m, t, bias of spmm_edge / spmm_edge_heads, checked against g and each other: float32, x one row per column of
    the operator, m as wide as x, t [N, d]; rows unit-stride, bias contiguous"""
    x, m = _edge_f32(x, "x", op, keys), _edge_f32(m, "m", op, keys)
    t = None if t is None else _edge_f32(t, "t", op, keys)
    if x.size(0) != g.num_cols or m.size(1) != x.size(1):
        raise ValueError(f"x is {tuple(x.shape)}, m is {tuple(m.shape)}: the operator has {g.num_cols} columns and both "
                         "operands share one width")
    if t is not None and tuple(t.shape) != (g.num_nodes, x.size(1)):
        raise ValueError(f"t is {tuple(t.shape)}, expected {(g.num_nodes, x.size(1))}")
    if bias is not None and bias.dtype != torch.float32:
        raise TypeError(f"{op} is float32 only: bias is {bias.dtype}")
    return x, m, t, None if bias is None else bias.contiguous()


def _eid_checked(g, n_edges):
    """g.eid, after checking once per graph that every stored entry's input position is below n_edges"""
    if g.eid is None:
        raise ValueError("spmm_edge needs a graph that knows the input position of its entries (CSRGraph.eid): build it "
                         "with CSRGraph.from_edge_index")
    top = g.__dict__.get("_eid_max")
    if top is None:
        top = int(g.eid.max().item()) if g.nnz else -1
        g.__dict__["_eid_max"] = top
    if n_edges <= top:
        raise ValueError(f"m has {n_edges} rows, the graph's entries come from input edges up to {top}")
    return g.eid


def _raw_spmm_edge(g, x, m, t=None, bias=None, reduce=_lib.SUM, want_argmax=False, out=None, eid=None):
    """one launch of mp_spmm_csr_edge_f32 (+ the hub launches of its plan): y[r] = reduce_e val_e (x[col_e] + m[eid_e] +
    t[r]) + bias -> (y, argmax [N, d] int32 or None).  eid: another per-entry row index into m in the place of g.eid
    (spmm_code: the entry's code, checked by its caller)"""
    L = lib()
    N, d = g.num_nodes, x.size(1)
    if eid is None:
        eid = _eid_checked(g, m.size(0))
    if g.nnz == 0:          # no entry: col and eid have no address; every row is empty
        return _agg_of_nothing(N, d, x, bias, want_argmax, out)
    m = _row0_if_none(m, d, x.device)
    y = out if out is not None else placement.empty_or_torch((N, d), x.device, reads=(x, m))
    argmax = torch.empty((N, d), dtype=torch.int32, device=x.device) if want_argmax else None
    plan, counts, ws, ws_bytes = _plan_ws(g, x.device, d, reduce, False)
    with torch.cuda.device(x.device):
        check(L.mp_spmm_csr_edge_f32(ptr(g.rowptr), ptr(g.col), ptr(eid), ptr(g.val), N, ptr(plan), counts, ptr(x),
                                     x.stride(0), ptr(m), m.stride(0), ptr(t), t.stride(0) if t is not None else 0,
                                     ptr(y), y.stride(0), d, reduce, ptr(bias), ptr(argmax), ptr(ws), ws_bytes,
                                     _stream()), "mp_spmm_csr_edge_f32")
    return y, argmax


@custom_op("mp::spmm_edge_raw", mutates_args=(), device_types="cuda")
def _op_spmm_edge_raw(x: Tensor, m: Tensor, t: Optional[Tensor], bias: Optional[Tensor], graph: int, reduce: int,
                      want_argmax: bool) -> Tuple[Tensor, Tensor]:
    g = from_handle(graph)
    x, m, t, bias = _edge_operands(g, "spmm_edge", _EDGE_KEYS, x, m, t, bias)
    return _agg_results(x, graph, want_argmax, launched=_raw_spmm_edge(g, x, m, t, bias, reduce, want_argmax))


@custom_op("mp::spmm_edge_bwd_raw", mutates_args=(), device_types="cuda")
def _op_spmm_edge_bwd_raw(dy: Tensor, argmax: Tensor, graph: int, reduce: int, n_edges: int) -> Tensor:
    """dm [n_edges, d] of spmm_edge (mp_spmm_edge_bwd_f32): rows of input edges the operator does not hold stay zero"""
    g = from_handle(graph)
    dy = dy if dy.stride(-1) == 1 else dy.contiguous()
    N, d = dy.shape
    dm = torch.zeros((n_edges, d), dtype=torch.float32, device=dy.device)
    if n_edges == 0:            # (the entry point cannot see n_edges: every entry is an inserted loop, dm has no address)
        return dm
    with torch.cuda.device(dy.device):
        check(lib().mp_spmm_edge_bwd_f32(ptr(g.rowptr), ptr(g.eid), ptr(g.val), ptr(_none_if_empty(argmax)), N, g.nnz,
                                         reduce, ptr(dy), dy.stride(0), d, ptr(dm), dm.stride(0), _stream()),
              "mp_spmm_edge_bwd_f32")
    return dm


@custom_op("mp::spmm_edge_dt_raw", mutates_args=(), device_types="cuda")
def _op_spmm_edge_dt_raw(dy: Tensor, argmax: Tensor, graph: int, reduce: int) -> Tensor:
    """dt [N, d] of spmm_edge, elementwise: t[r] rides in every entry of row r — (the sum of the row's values [over its
    entry count for mean]) * dy; max: each column's winner carries it once — val[argmax] * dy, 0 for an empty row"""
    g = from_handle(graph)
    if g.nnz == 0:              # no entry carries t
        return torch.zeros_like(dy)
    if reduce == _lib.MAX:
        dt = dy if g.val is None else g.val[argmax.clamp(min=0).long()] * dy
        return torch.where(argmax >= 0, dt, torch.zeros_like(dt))
    c = g.entry_counts() if g.val is None else g.degree("row")
    if reduce == _lib.MEAN:
        c = c / g.entry_counts().clamp(min=1.0)
    return c[:, None] * dy


@custom_op("mp::spmm_edge", mutates_args=(), device_types="cuda")
def _op_spmm_edge(x: Tensor, m: Tensor, t: Optional[Tensor], bias: Optional[Tensor], graph: int,
                  reduce: int) -> Tuple[Tensor, Tensor]:
    return torch.ops.mp.spmm_edge_raw(x, m, t, bias, graph, reduce, reduce == _lib.MAX)


def _spmm_edge_setup(ctx, inputs, output):
    x, m, t, bias, graph, reduce = inputs
    _graph_setup(ctx, graph, reduce, bias)
    ctx.n_edges, ctx.has_t = m.size(0), t is not None
    ctx.save_for_backward(output[1])


def _spmm_edge_backward(ctx, dy, _dargmax):
    (argmax,) = ctx.saved_tensors
    if dy is None:
        return None, None, None, None, None, None
    dy = dy.contiguous()
    need = ctx.needs_input_grad
    dx = dm = dt = dbias = None
    if need[0]:
        dx = _grad_by_source(ctx.graph, ctx.reduce, dy, argmax)
    if need[1]:
        dm = torch.ops.mp.spmm_edge_bwd_raw(dy, argmax, ctx.graph, ctx.reduce, ctx.n_edges)
    if ctx.has_t and need[2]:
        dt = torch.ops.mp.spmm_edge_dt_raw(dy, argmax, ctx.graph, ctx.reduce)
    if ctx.has_bias and need[3]:
        dbias = _bias_grad(dy)
    return dx, dm, dt, dbias, None, None


register_autograd("mp::spmm_edge", _spmm_edge_backward, setup_context=_spmm_edge_setup)


def spmm_edge(g, x, m, reduce="sum", t=None, bias=None):
    """y[i] = reduce_{e = (i <- j)} w_e (x[j] + m[eid_e] + t[i]) + bias   (torch.ops.mp.spmm_edge)

    The aggregation of messages that carry an edge feature (GeneralEdgeConvLayer.message, generalconv.py:203-209): x
    [n, d] is gathered by source, m [E, d] by the entry's position in the input edge_index (g.eid; an inserted self loop
    has none and gets no m term), t [N, d] is the destination's own term.  One pass, no per-entry tensor.  reduce:
    'sum'/'add' | 'mean' | 'max' (ties: the first entry in CSR order).  float32 only; the gradient flows to x, m, t and
    bias, the entry values of g are constants; no float atomics except in dx of 'max' (mp_spmm_max_bwd_f32)."""
    r = _checked_reduce(reduce)
    _check_edge_f32("spmm_edge", _EDGE_KEYS, x=x, m=m, t=t, bias=bias)
    _eid_checked(g, m.size(0))
    return torch.ops.mp.spmm_edge(x, m, t, bias, g.handle, r)[0]


# ---- attention over messages with an edge feature (attconv.py:342-360) ----------------------------------------------
def _eid_clamped(g):
    """g.eid with the inserted loops (eid < 0) pointed at row 0, and the mask of the entries that have an input edge (None:
    all of them); cached on g"""
    hit = g.__dict__.get("_eid_clamped")
    if hit is None:
        eid = g.eid
        if g.nnz and bool((eid < 0).any()):
            hit = (eid.clamp(min=0).contiguous(), eid >= 0)
        else:
            hit = (eid, None)
        g.__dict__["_eid_clamped"] = hit
    return hit


@custom_op("mp::edge_att_alpha", mutates_args=(), device_types="cuda")
def _op_edge_att_alpha(a_dst: Optional[Tensor], a_src: Tensor, a_edge: Tensor, graph: int, slope: float) -> Tensor:
    g = from_handle(graph)
    op = "edge_att_alpha"
    asr = _edge_f32(a_src, "a_src", op, _EDGE_ATT_KEYS).contiguous()
    aed = _edge_f32(a_edge, "a_edge", op, _EDGE_ATT_KEYS).contiguous()
    ad = None if a_dst is None else _edge_f32(a_dst, "a_dst", op, _EDGE_ATT_KEYS).contiguous()
    H = asr.size(1)
    if asr.size(0) != g.num_cols or aed.size(1) != H or (ad is not None and tuple(ad.shape) != (g.num_nodes, H)):
        raise ValueError(f"a_src is {tuple(asr.shape)}, a_edge {tuple(aed.shape)}, a_dst "
                         f"{None if ad is None else tuple(ad.shape)}: expected [{g.num_cols}, H], [E, H], "
                         f"[{g.num_nodes}, H]")
    eid = _eid_checked(g, aed.size(0))
    aed = _row0_if_none(aed, H, asr.device)
    alpha = torch.empty((g.nnz, H), dtype=torch.float32, device=asr.device)
    with torch.cuda.device(asr.device):
        check(lib().mp_edge_att_alpha_f32(ptr(g.rowptr), ptr(g.col), ptr(eid), g.num_nodes, g.nnz, H, ptr(ad), ptr(asr),
                                          ptr(aed), float(slope), ptr(alpha), _stream()), "mp_edge_att_alpha_f32")
    return alpha


@custom_op("mp::edge_att_alpha_bwd_raw", mutates_args=(), device_types="cuda")
def _op_edge_att_alpha_bwd_raw(dalpha: Tensor, alpha: Tensor, a_dst: Optional[Tensor], a_src: Tensor, a_edge: Tensor,
                               graph: int, slope: float, want: int) -> Tuple[Tensor, Tensor, Tensor]:
    """(d_dst, d_src, d_edge) of edge_att_alpha (_alpha_bwd), each computed when its bit of `want` (1, 2, 4) is set and
    empty otherwise"""
    return _want_results(alpha, want, launched=_alpha_bwd(from_handle(graph), alpha, dalpha, a_dst, a_src, a_edge, slope,
                                                          want))


def _edge_att_alpha_setup(ctx, inputs, output):
    a_dst, a_src, a_edge, graph, slope = inputs
    ctx.graph, ctx.slope, ctx.g_alive = graph, slope, from_handle(graph)
    ctx.has_dst = a_dst is not None
    ctx.save_for_backward(output, a_dst, a_src, a_edge)


def _edge_att_alpha_backward(ctx, dalpha):
    alpha, a_dst, a_src, a_edge = ctx.saved_tensors
    need = ctx.needs_input_grad
    want = _want_bits(ctx.has_dst and need[0], need[1], need[2])      # _EA_DST, _EA_SRC, _EA_EDGE
    if not want:
        return (None,) * 5
    return _want_grads(want, torch.ops.mp.edge_att_alpha_bwd_raw(dalpha, alpha, a_dst, a_src, a_edge, ctx.graph,
                                                                 ctx.slope, want)) + (None, None)


register_autograd("mp::edge_att_alpha", _edge_att_alpha_backward, setup_context=_edge_att_alpha_setup)


def edge_att_alpha(g, a_dst, a_src, a_edge, slope=0.2):
    """alpha[e, h] = softmax over the entries of e's destination row of leaky_relu(a_dst[row_e, h] + a_src[col_e, h] +
    a_edge[eid_e, h])   (torch.ops.mp.edge_att_alpha) -> [nnz, H]

    The attention coefficients of GeneralEdgeAttConvv1Layer / v2 (attconv.py:352-357): a_src [n, H] by source, a_edge
    [E, H] by the entry's position in the input edge_index (g.eid; an inserted self loop has no edge term), a_dst [N, H]
    by destination or None.  One launch for all heads, the scores are never stored.  float32 only; differentiable in
    all three."""
    _check_edge_f32("edge_att_alpha", _EDGE_ATT_KEYS, a_dst=a_dst, a_src=a_src, a_edge=a_edge)
    _eid_checked(g, a_edge.size(0))
    return torch.ops.mp.edge_att_alpha(a_dst, a_src, a_edge, g.handle, float(slope))


@custom_op("mp::spmm_edge_heads", mutates_args=(), device_types="cuda")
def _op_spmm_edge_heads(w: Tensor, x: Tensor, m: Tensor, t: Optional[Tensor], bias: Optional[Tensor], graph: int,
                        heads: int, reduce: int) -> Tuple[Tensor, Tensor]:
    g = from_handle(graph)
    op = "spmm_edge_heads"
    if heads < 1 or x.size(1) % heads:
        raise ValueError(f"x has {x.size(1)} columns, not a multiple of heads = {heads}")
    x, m, t, bias = _edge_operands(g, op, _EDGE_ATT_KEYS, x, m, t, bias)
    # w dense [nnz, H]: the kernels read w[e * H + h], whatever the caller's strides
    w = _edge_f32(w.reshape(g.nnz, heads), "w", op, _EDGE_ATT_KEYS).contiguous()
    is_max = reduce == _lib.MAX
    return _agg_results(x, graph, is_max, launched=_raw_spmm_edge_heads(g, w, x, m, t, bias, heads, reduce, is_max))


_EH_W, _EH_X, _EH_M, _EH_T = 1, 2, 4, 8


@custom_op("mp::spmm_edge_heads_bwd_raw", mutates_args=(), device_types="cuda")
def _op_spmm_edge_heads_bwd_raw(dy: Tensor, w: Tensor, x: Tensor, m: Tensor, t: Optional[Tensor], argmax: Tensor,
                                graph: int, heads: int, reduce: int,
                                want: int) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(dw, dx, dm, dt) of spmm_edge_heads, each computed when its bit of `want` (1, 2, 4, 8) is set and empty otherwise"""
    g = from_handle(graph)
    op = "spmm_edge_heads"
    dy = dy if (dy.dim() == 2 and dy.stride(1) == 1) else dy.contiguous()
    x, m = _edge_f32(x, "x", op, _EDGE_ATT_KEYS), _edge_f32(m, "m", op, _EDGE_ATT_KEYS)
    t = None if t is None else _edge_f32(t, "t", op, _EDGE_ATT_KEYS)
    w = w.reshape(g.nnz, heads).contiguous()
    N, d = dy.shape
    hw = d // heads
    E = m.size(0)
    is_max = reduce == _lib.MAX
    dw = dx = dm = dt = None
    dy0 = dy
    if reduce == _lib.MEAN and want & (_EH_W | _EH_X | _EH_T):      # (dm's kernel divides by itself: it reads dy0)
        dy = _mean_dy(g, dy)
    eidc, has = _eid_clamped(g)
    if want & _EH_X:
        dx = _heads_grad_by_source(g, w, x, heads, is_max, dy, argmax)
    if want & _EH_M:
        dm = torch.zeros((E, d), dtype=torch.float32, device=dy.device)
        if E and g.nnz:
            with torch.cuda.device(dy.device):
                check(lib().mp_spmm_edge_heads_bwd_f32(ptr(g.rowptr), ptr(g.eid), ptr(w), heads,
                                                       ptr(argmax if is_max else None), N, g.nnz, reduce, ptr(dy0),
                                                       dy0.stride(0), d, ptr(dm), dm.stride(0), _stream()),
                      "mp_spmm_edge_heads_bwd_f32")
    if want & _EH_T and t is not None:
        if g.nnz == 0:  # no entry carries t
            dt = torch.zeros_like(dy)
        elif is_max:   # each column's winner carries t once
            am = argmax.long()
            head_of = torch.arange(d, device=dy.device) // hw
            dt = w.reshape(-1)[(am.clamp(min=0) * heads + head_of)] * dy
            dt = torch.where(am >= 0, dt, torch.zeros_like(dt))
        else:          # t[r] rides in every entry of row r: the per-head row sums of w, on the aggregation kernel
            ones = torch.ones((g.num_cols, heads), dtype=torch.float32, device=dy.device)
            rs = _raw_spmm_heads(g, w, ones, heads)                        # [N, H]
            dt = (rs[:, :, None] * dy.view(N, heads, hw)).reshape(N, d)
    if want & _EH_W:
        # dw[e, h] = <dy[row_e], x[col_e] + m[eid_e] + t[row_e]>_h: three per-entry dots (max: over the columns e won)
        dw = _heads_grad_weights(g, x, heads, is_max, dy, argmax)
        dwm = _heads_grad_weights(g, _row0_if_none(m, d, dy.device), heads, is_max, dy, argmax, idx=eidc)
        dw = dw + (dwm if has is None else torch.where(has[:, None], dwm, torch.zeros_like(dwm)))
        if t is not None:
            if is_max:
                dw = dw + _raw_heads_max_da(g, argmax, dy, t, heads, idx=g.row_ids())
            else:
                dw = dw + (dy.view(N, heads, hw) * t.view(N, heads, hw)).sum(-1)[g.row_ids().long()]
    return _want_results(dy, want, launched=(dw, dx, dm, dt))


def _spmm_edge_heads_setup(ctx, inputs, output):
    w, x, m, t, bias, graph, heads, reduce = inputs
    _graph_setup(ctx, graph, reduce, bias)
    ctx.heads, ctx.has_t, ctx.w_shape = heads, t is not None, w.shape
    ctx.save_for_backward(w, x, m, t, output[1])


def _spmm_edge_heads_backward(ctx, dy, _dargmax):
    w, x, m, t, argmax = ctx.saved_tensors
    if dy is None:
        return (None,) * 8
    need = ctx.needs_input_grad
    want = _want_bits(need[0], need[1], need[2], ctx.has_t and need[3])      # _EH_W, _EH_X, _EH_M, _EH_T
    dw = dx = dm = dt = None
    if want:
        dw, dx, dm, dt = _want_grads(want, torch.ops.mp.spmm_edge_heads_bwd_raw(dy, w, x, m, t, argmax, ctx.graph,
                                                                                ctx.heads, ctx.reduce, want))
        dw = dw.reshape(ctx.w_shape) if dw is not None else None
    dbias = _bias_grad(dy) if (ctx.has_bias and need[4]) else None
    return dw, dx, dm, dt, dbias, None, None, None


register_autograd("mp::spmm_edge_heads", _spmm_edge_heads_backward, setup_context=_spmm_edge_heads_setup)


def spmm_edge_heads(g, w, x, m, t=None, heads=1, reduce="sum", bias=None):
    """y[i, slice h] = reduce_{e = (i <- j)} w[e, h] (x[j] + m[eid_e] + t[i])[slice h] + bias   (torch.ops.mp.spmm_edge_heads)

    spmm_edge with one weight per entry AND head — the propagate of GeneralEdgeAttConvv1Layer / v2 (attconv.py:358-360)
    with w = norm * alpha [nnz, H]; x [n, d] by source, m [E, d] by the entry's input position (g.eid; an inserted self
    loop gets no m term), t [N, d] the destination's own term.  The entry values of g take no part.  2, 4 and 8 heads run
    in one launch (mp_spmm_csr_edge_heads_f32), every other head count above one runs one launch of
    mp_spmm_csr_edge_f32 per head on column slices.  reduce: 'sum'/'add' | 'mean' | 'max'
    (ties: the first entry in CSR order).  float32 only; the gradient flows to w, x, m, t and bias; no float atomics
    except in dx of 'max' (mp_spmm_heads_max_bwd_f32), which is therefore not bitwise reproducible."""
    r = _checked_reduce(reduce)
    _check_edge_f32("spmm_edge_heads", _EDGE_ATT_KEYS, w=w, x=x, m=m, t=t, bias=bias)
    if int(heads) < 1 or x.size(1) % int(heads):
        raise ValueError(f"x has {x.size(1)} columns, not a multiple of heads = {heads}")
    _eid_checked(g, m.size(0))
    return torch.ops.mp.spmm_edge_heads(w, x, m, t, bias, g.handle, int(heads), r)[0]


# ---- integer-coded features (feature_encoder.py:13-103) and the coded edge term (generalconv_ogb.py:30-35,115-118) ----
def code_reduce_cap():
    """the largest number of table rows mp_code_reduce_f32 takes"""
    return int(lib().mp_code_reduce_max_codes())


def code_reduce_path(n_codes):
    """'kernel' (mp_code_reduce_f32) or 'operator' (the plan-based aggregation on the transposed one-hot operator) for a
    table reduction whose items are known ahead of the call (embed_sum's backward; sum and mean of spmm_code).  Above
    code_reduce_cap() rows only the operator exists.  Below it the choice follows the measurement
    (profiles/ogb_bench.json): at N = 10^6 the operator took 0.41 ms against the kernel's 1.15 ms for
    the 60 bond codes and 2.20 ms against 5.45 ms for the 173 atom rows, so the operator is the default; MP_CODE_REDUCE=kernel
    takes the kernel (it needs no operator build and a workspace of a sixteenth of dY).  The winners of a max
    aggregation differ per column and have no operator form: they always run on the kernel."""
    if n_codes > code_reduce_cap():
        return "operator"
    return "kernel" if os.environ.get("MP_CODE_REDUCE", "operator") == "kernel" else "operator"


_OFFSETS = {}


def _offsets_dev(offsets, device):
    """the K table offsets as an int32 device tensor (one per (offsets, device))"""
    key = (tuple(int(o) for o in offsets), str(device))
    t = _OFFSETS.get(key)
    if t is None:
        t = _OFFSETS[key] = torch.tensor(key[0], dtype=torch.int32, device=device)
    return t


def check_codes(codes, dims, what="codes"):
    """the int32 copy of integer features [R, K] (K = len(dims)) the kernels read, after checking every column k against
    [0, dims[k]) — IndexError as nn.Embedding raises.  One device-to-host read: callers cache the result per batch."""
    if codes.dim() != 2 or codes.size(1) != len(dims) or codes.is_floating_point():
        raise ValueError(f"{what} must be an integer tensor [R, {len(dims)}], got {codes.dtype} {tuple(codes.shape)}")
    if codes.size(0):
        lo, hi = codes.amin(0).cpu().tolist(), codes.amax(0).cpu().tolist()
        for k, dim in enumerate(dims):
            if lo[k] < 0 or hi[k] >= dim:
                raise IndexError(f"{what}[:, {k}] holds {lo[k] if lo[k] < 0 else hi[k]}: index out of range "
                                 f"[0, {dim})")
    _require_hip(codes, what)
    out = codes.to(torch.int32).contiguous()
    out._mp_checked_dims = tuple(int(v) for v in dims)
    out._mp_checked_version = out._version        # (an in-place update afterwards voids the check)
    return out


def _raw_embed_sum(codes, table, off, out=None):
    """one launch of mp_embed_sum_f32 -> out [R, d]"""
    R, K = codes.shape
    d = table.size(1)
    out = torch.empty((R, d), dtype=torch.float32, device=table.device) if out is None else out
    with torch.cuda.device(table.device):
        check(lib().mp_embed_sum_f32(ptr(codes), K, ptr(off), ptr(table), table.stride(0), R, d, ptr(out), out.stride(0),
                                     _stream()), "mp_embed_sum_f32")
    return out


def _raw_code_reduce(dy, codes, n_codes, K=0, off=None, disjoint=False, rowptr=None, rows=None, w=None, sel=None):
    """one call of mp_code_reduce_f32 -> (dT [n_codes, d], number of partial slabs).  Items of row r: K per row (codes
    [R, K] + off; disjoint: the K codes of a row lie in K separate tables), the entries rowptr[r] .. rowptr[r+1] (codes,
    w and rows per entry), or one per column (sel [R, d])"""
    L = lib()
    R, d = dy.shape
    nb, ns = C.c_size_t(0), C.c_int32(0)
    check(L.mp_code_reduce_ws_bytes(R, n_codes, d, C.byref(ns), C.byref(nb)), "mp_code_reduce_ws_bytes")
    ws = torch.empty(max(nb.value, 1), dtype=torch.uint8, device=dy.device)
    dT = torch.empty((n_codes, d), dtype=torch.float32, device=dy.device)
    with torch.cuda.device(dy.device):
        check(L.mp_code_reduce_f32(ptr(rowptr), ptr(rows), K, ptr(codes), ptr(off), 1 if disjoint else 0, ptr(w),
                                   ptr(sel), sel.stride(0) if sel is not None else 0, R, n_codes, ptr(dy),
                                   dy.stride(0), d, ptr(dT), dT.stride(0), ptr(ws), nb.value, _stream()),
              "mp_code_reduce_f32")
    return dT, ns.value


_ONEHOT_T = {}     # (stamp of the codes tensor, offsets, n_codes) -> (codes, operator): holding codes keeps its address unique


def _code_reduce_fallback(dy, codes, offsets, n_codes):
    """dTable of embed_sum on the transposed one-hot operator: row (off_k + code) <- item row, one entry per item, summed
    by the plan kernel — deterministic (a table row with many items takes the hub path).  offsets: the K host integers.
    The operator is kept per codes tensor (graph.tensor_stamp: a batch's checked codes are one tensor for all
    steps), for the last few of them."""
    offsets = tuple(int(o) for o in offsets)
    key = (tensor_stamp(codes), offsets, int(n_codes))
    hit = _ONEHOT_T.get(key)
    if hit is None:
        if len(_ONEHOT_T) >= 8:
            _ONEHOT_T.clear()
        R, K = codes.shape
        dst = (codes.long() + _offsets_dev(offsets, codes.device).long()[None]).reshape(-1)
        src = torch.arange(R, device=codes.device).repeat_interleave(K)
        hit = _ONEHOT_T[key] = (codes, CSRGraph.from_edge_index(torch.stack([src, dst]), n_codes, num_cols=max(R, 1)))
    return torch.ops.mp.spmm_raw(dy, hit[1].handle, 0, _lib.SUM, None, 0.0, None, False, False)[0]


@custom_op("mp::embed_sum", mutates_args=(), device_types="cuda")
def _op_embed_sum(codes: Tensor, table: Tensor, offsets: List[int]) -> Tensor:
    table = _edge_f32(table, "table", "embed_sum", "encoders and generalogbconv")
    return _raw_embed_sum(codes, table, _offsets_dev(offsets, table.device))


@custom_op("mp::embed_sum_bwd_raw", mutates_args=(), device_types="cuda")
def _op_embed_sum_bwd_raw(dy: Tensor, codes: Tensor, offsets: List[int], n_codes: int, disjoint: bool) -> Tensor:
    """dTable [n_codes, d] of embed_sum: the transposed one-hot operator or mp_code_reduce_f32 (code_reduce_path).
    disjoint: the caller's promise that the K codes of a row lie in K separate tables (embed_sum: codes checked against
    tables at strictly increasing offsets), which lets K = 3 / 9 update all K accumulators of a row at once"""
    dy = dy if dy.dim() == 2 and dy.stride(1) == 1 else dy.contiguous()
    if dy.size(0) == 0:         # no item: nothing reaches the table
        return torch.zeros((n_codes, dy.size(1)), dtype=torch.float32, device=dy.device)
    if code_reduce_path(n_codes) == "operator":
        return _code_reduce_fallback(dy, codes, offsets, n_codes)
    return _raw_code_reduce(dy, codes, n_codes, K=codes.size(1), off=_offsets_dev(offsets, dy.device),
                            disjoint=disjoint)[0]


def _embed_sum_setup(ctx, inputs, output):
    codes, table, offsets = inputs
    ctx.n_codes = table.size(0)
    ctx.offsets = [int(o) for o in offsets]
    ctx.save_for_backward(codes)


def _embed_sum_backward(ctx, dy):
    (codes,) = ctx.saved_tensors
    dtable = None
    if ctx.needs_input_grad[1]:
        off = ctx.offsets
        # the forward's contract: every code was checked against its own table, so increasing offsets separate them
        disjoint = all(a < b for a, b in zip(off, off[1:]))
        dtable = torch.ops.mp.embed_sum_bwd_raw(dy, codes, off, ctx.n_codes, disjoint)
    return None, dtable, None


register_autograd("mp::embed_sum", _embed_sum_backward, setup_context=_embed_sum_setup)


def embed_sum(codes, table, offsets):
    """out[r] = ((0 + table[off_0 + codes[r, 0]]) + table[off_1 + codes[r, 1]]) + ...   (torch.ops.mp.embed_sum)

    The sum of embedding rows of the reference's encoders (AtomEncoder.forward, feature_encoder.py:74-81) with the K
    tables stacked into `table` [C, d] (float32, any leading dimension) at the row offsets `offsets`; the additions run
    in the reference's order, so the bits are those of its fp32 loop.  codes [R, K]: the int32 tensor check_codes
    returned for these tables is taken as it is; any other integer tensor is checked here (IndexError outside a
    table).  The gradient flows to table, without float atomics (code_reduce_path: the aggregation on the transposed one-hot
    operator, or mp_code_reduce_f32 up to code_reduce_cap() rows)."""
    offsets = [int(o) for o in offsets]
    dims = tuple(b - a for a, b in zip(offsets, offsets[1:] + [table.size(0)]))
    if getattr(codes, "_mp_checked_dims", None) != dims or codes.dtype != torch.int32 \
            or getattr(codes, "_mp_checked_version", None) != codes._version:
        codes = check_codes(codes, dims)
    if table.dtype != torch.float32:
        raise TypeError(f"embed_sum is float32 only: table is {table.dtype}")
    return torch.ops.mp.embed_sum(codes, table, offsets)


def entry_codes(g, codes):
    """codes [E] int32 per INPUT edge -> per stored entry of g (q of the entry's input edge, -1 for an inserted self
    loop), with the largest entry code and the smallest input code; cached on g for this codes tensor (graph.tensor_stamp)"""
    hit = g.__dict__.get("_entry_codes")
    stamp = tensor_stamp(codes)                    # (not the tensor's identity: an in-place update must be seen)
    if hit is None or hit[4] != stamp:
        eid = g.eid
        if eid is None:
            raise ValueError("spmm_code needs a graph that knows the input position of its entries (CSRGraph.eid)")
        if g.nnz and int(eid.max().item()) >= codes.numel():
            raise ValueError(f"codes has {codes.numel()} rows, the graph's entries come from input edges up to "
                             f"{int(eid.max().item())}")
        q = codes[eid.clamp(min=0).long()] if codes.numel() else torch.full_like(eid, -1)
        q = torch.where(eid >= 0, q, torch.full_like(q, -1)).to(torch.int32).contiguous()
        top = int(q.max().item()) if g.nnz else -1
        low = int(codes.min().item()) if codes.numel() else 0
        hit = (codes, q, top, low, stamp)
        g.__dict__["_entry_codes"] = hit
    return hit[1], hit[2], hit[3]


@custom_op("mp::spmm_code", mutates_args=(), device_types="cuda")
def _op_spmm_code(x: Tensor, table: Tensor, bias: Optional[Tensor], qe: Tensor, graph: int,
                  reduce: int) -> Tuple[Tensor, Tensor]:
    g = from_handle(graph)
    x, table, _, bias = _edge_operands(g, "spmm_code", "key generalogbconv", x, table, None, bias)
    is_max = reduce == _lib.MAX
    return _agg_results(x, graph, is_max, launched=_raw_spmm_edge(g, x, table, None, bias, reduce, is_max, eid=qe))


@custom_op("mp::spmm_code_bwd_raw", mutates_args=(), device_types="cuda")
def _op_spmm_code_bwd_raw(dy: Tensor, argmax: Tensor, qe: Tensor, graph: int, reduce: int, n_codes: int) -> Tensor:
    """dTable [n_codes, d] of spmm_code (mp_code_reduce_f32): sum / mean over the entries of each row with weights val
    (/ the row's entry count), max over each column's winning entry"""
    g = from_handle(graph)
    dy = dy if dy.dim() == 2 and dy.stride(1) == 1 else dy.contiguous()
    if g.nnz == 0:              # no entry: nothing reaches the table
        return torch.zeros((n_codes, dy.size(1)), dtype=torch.float32, device=dy.device)
    if reduce == _lib.MAX:
        return _raw_code_reduce(dy, qe, n_codes, w=g.val, sel=argmax)[0]
    w = g.val
    if reduce == _lib.MEAN:        # entry weights val / (entry count of the row), cached on the graph — the mean folded into
        # the weights and not into dy (_mean_dy): (1 / count) * val is its own order of multiplications, kept as it is
        w = g.__dict__.get("_mean_entry_w")
        if w is None:
            w = (1.0 / g.entry_counts().clamp(min=1.0))[g.row_ids().long()]
            w = g.__dict__["_mean_entry_w"] = (w if g.val is None else w * g.val).contiguous()
    if code_reduce_path(n_codes) == "operator":
        return _entry_reduce_fallback(dy, g, qe, w, reduce, n_codes)
    return _raw_code_reduce(dy, qe, n_codes, rowptr=g.rowptr, rows=g.row_ids(), w=w)[0]


def _entry_reduce_fallback(dy, g, qe, w, reduce, n_codes):
    """dTable of spmm_code (sum / mean) on the transposed one-hot operator of the entries: row q_e <- the entry's row,
    value w_e, entries without a code left out; cached on g (the op's graph handle names it) for this qe by
    graph.tensor_stamp"""
    cache = g.__dict__.setdefault("_code_onehot_t", {})
    hit = cache.get((reduce, n_codes))
    if hit is None or hit[2] != tensor_stamp(qe):
        keep = torch.nonzero(qe >= 0).view(-1)
        ei = torch.stack([g.row_ids().long()[keep], qe.long()[keep]])
        op = CSRGraph.from_edge_index(ei, n_codes, None if w is None else w[keep], num_cols=max(g.num_nodes, 1))
        hit = cache[(reduce, n_codes)] = (qe, op, tensor_stamp(qe))
    return torch.ops.mp.spmm_raw(dy, hit[1].handle, 0, _lib.SUM, None, 0.0, None, False, False)[0]


def _spmm_code_setup(ctx, inputs, output):
    x, table, bias, qe, graph, reduce = inputs
    _graph_setup(ctx, graph, reduce, bias)
    ctx.n_codes = table.size(0)
    ctx.save_for_backward(output[1], qe)


def _spmm_code_backward(ctx, dy, _dargmax):
    argmax, qe = ctx.saved_tensors
    if dy is None:
        return None, None, None, None, None, None
    dy = dy.contiguous()
    need = ctx.needs_input_grad
    dx = dtable = dbias = None
    if need[0]:
        dx = _grad_by_source(ctx.graph, ctx.reduce, dy, argmax)
    if need[1]:
        dtable = torch.ops.mp.spmm_code_bwd_raw(dy, argmax, qe, ctx.graph, ctx.reduce, ctx.n_codes)
    if ctx.has_bias and need[2]:
        dbias = _bias_grad(dy)
    return dx, dtable, dbias, None, None, None


register_autograd("mp::spmm_code", _spmm_code_backward, setup_context=_spmm_code_setup)


def spmm_code(g, x, table, codes, reduce="sum", bias=None):
    """y[i] = reduce_{e = (i <- j)} w_e (x[j] + table[codes[eid_e]]) + bias   (torch.ops.mp.spmm_code)

    spmm_edge whose edge term is a row of a small table chosen by an integer code per INPUT edge (the bond term of
    GeneralOGBConvLayer.message, generalconv_ogb.py:115-118): codes [E] int32 in [0, table rows), checked once per
    (graph, codes) pair; an inserted self loop has no table term.  The forward is the two-gather launch with the entry's
    code in the place of its input position; nothing of size [E, d] exists in either direction.  The gradient flows to
    x, table and bias; dtable has no float atomics (code_reduce_path: the one-hot operator or mp_code_reduce_f32; 'max'
    always the kernel), dx of 'max' does (mp_spmm_max_bwd_f32).
    float32 only; table rows up to code_reduce_cap()."""
    r = _checked_reduce(reduce)
    _check_edge_f32("spmm_code", "key generalogbconv", x=x, table=table, bias=bias)
    if codes.dtype != torch.int32 or codes.dim() != 1:
        raise ValueError(f"codes must be int32 [E], got {codes.dtype} {tuple(codes.shape)}")
    if table.size(0) > code_reduce_cap():
        raise ValueError(f"spmm_code takes tables of up to {code_reduce_cap()} rows, got {table.size(0)}")
    qe, top, low = entry_codes(g, codes)
    if top >= table.size(0) or low < 0:
        raise IndexError(f"codes reach {top if top >= table.size(0) else low}: index out of range [0, {table.size(0)})")
    return torch.ops.mp.spmm_code(x, table, bias, qe, g.handle, r)[0]


# ---- fake kernels: one line per signature; the results functions are under "what the registered operators share" ------
_op_spmm_raw.register_fake(lambda x, graph, variant, reduce, S, self_scale, bias, relu, want_argmax:
                           _agg_results(x, graph, want_argmax, variant))
_op_spmm_rows_raw.register_fake(lambda x, graph, variant, rows: x.new_empty((rows.numel(), x.size(1))))
_op_spmm_max_bwd_raw.register_fake(lambda dy, argmax, graph: dy.new_empty((_op_rows(graph, 1), dy.size(1))))
_op_idgnn_agg_raw.register_fake(lambda x, graph, id_index: _idgnn_results(x, graph))
_op_agg_dense_raw.register_fake(lambda x, W, bias, graph, variant, reduce, S, self_scale, relu, want_P:
                                _agg_dense_results(x, W, graph, want_P, variant))
_op_agg_dense_id_raw.register_fake(lambda x, W, W_id, bias, graph, id_index, self_scale, relu, want_P:
                                   _agg_dense_results(x, W, graph, want_P, id_index=id_index))
_op_id_branch_t_raw.register_fake(lambda gm, graph, id_index: gm.new_empty((id_index.numel(), gm.size(1))))
_op_dense_fused_raw.register_fake(lambda P, W, Q, W_id, bias, relu: P.new_empty((P.size(0), W.size(1))))
_op_dense_wgrad_raw.register_fake(lambda X, G, want_w, want_b: _wgrad_results(X, G, want_w, want_b))
_op_dense_wgrad_relu_raw.register_fake(lambda X, G, Y, want_b, want_gm=True: _wgrad_results(X, G, True, want_b, want_gm))
_op_spmm.register_fake(lambda x, graph, reduce, self_scale, bias, relu: _agg_results(x, graph, reduce == _lib.MAX))
_op_idgnn_agg.register_fake(lambda x, graph, id_index: _idgnn_results(x, graph))
_op_dense_fused.register_fake(lambda P, W, Q, W_id, bias, relu: P.new_empty((P.size(0), W.size(1))))
_op_agg_dense.register_fake(lambda x, W, bias, graph, reduce, self_scale, relu, want_P:
                            _agg_dense_results(x, W, graph, want_P))
_op_agg_dense_id.register_fake(lambda x, W, W_id, bias, graph, id_index, self_scale, relu, want_P:
                               _agg_dense_results(x, W, graph, want_P, id_index=id_index))
_op_spmm_edge_raw.register_fake(lambda x, m, t, bias, graph, reduce, want_argmax: _agg_results(x, graph, want_argmax))
_op_spmm_edge_bwd_raw.register_fake(lambda dy, argmax, graph, reduce, n_edges: dy.new_empty((n_edges, dy.size(1))))
_op_spmm_edge_dt_raw.register_fake(lambda dy, argmax, graph, reduce: dy.new_empty(dy.shape))
_op_spmm_edge.register_fake(lambda x, m, t, bias, graph, reduce: _agg_results(x, graph, reduce == _lib.MAX))
_op_edge_att_alpha.register_fake(lambda a_dst, a_src, a_edge, graph, slope:
                                 a_src.new_empty((from_handle(graph).nnz, a_src.size(1))))
_op_edge_att_alpha_bwd_raw.register_fake(lambda dalpha, alpha, a_dst, a_src, a_edge, graph, slope, want: _want_results(
    alpha, want, (None if a_dst is None else a_dst.shape, a_src.shape, a_edge.shape)))
_op_spmm_edge_heads.register_fake(lambda w, x, m, t, bias, graph, heads, reduce: _agg_results(x, graph, reduce == _lib.MAX))
_op_spmm_edge_heads_bwd_raw.register_fake(lambda dy, w, x, m, t, argmax, graph, heads, reduce, want: _want_results(
    dy, want, (w.shape, x.shape, m.shape, None if t is None else dy.shape)))
_op_embed_sum.register_fake(lambda codes, table, offsets: table.new_empty((codes.size(0), table.size(1))))
_op_embed_sum_bwd_raw.register_fake(lambda dy, codes, offsets, n_codes, disjoint: dy.new_empty((n_codes, dy.size(1))))
_op_spmm_code.register_fake(lambda x, table, bias, qe, graph, reduce: _agg_results(x, graph, reduce == _lib.MAX))
_op_spmm_code_bwd_raw.register_fake(lambda dy, argmax, qe, graph, reduce, n_codes: dy.new_empty((n_codes, dy.size(1))))


# ---- one gather, two sums: the B-spline layer's aggregation and its adjoint (spline_ops.py, over the helpers above) ----
from .spline_ops import _raw_spline, spline_agg, spline_fold   # noqa: E402,F401


# ---- the pair decoders of the link-prediction head (pair_ops.py, over the helpers above) ------------------------------
from .pair_ops import PairIndex, pair_index, pair_score, pair_sum   # noqa: E402,F401
