/*
 * mp_spline.h — C ABI of the B-spline aggregation of libmpengine.so (csrc/spmm.hip: SplineAggRows, SplineFoldRows).
 *
 * What it replaces: the propagate of pyg.nn.SplineConv(dim_in, dim_out, dim=1, kernel_size=2) as
 * graphgym/models/layer.py:177-186 builds and calls it (key 'splineconv').  With one pseudo-coordinate u per edge, an
 * open spline of degree 1 and two kernel matrices W0, W1, the message of an entry is c0 x_j W0 + c1 x_j W1 with two
 * scalar coefficients of its own, so the layer is two weighted neighbour sums of the same rows of X over the same
 * sparsity pattern followed by one transform (or the transform first and one sum of two half rows).
 *
 * The conventions are those of mp_engine.h (device pointers, caller-owned buffers, everything enqueued on `stream`,
 * nothing allocates, nothing synchronises, mp_status return codes).  This header is separate from mp_engine.h, and its
 * entries are bound from a table of their own (graphgym_amd/_lib_spline.py), because the closure tests over mp_engine.h
 * name every entry of that header; the closures over this one are tests/test_spline_host.py and
 * tests/test_poison_spline_gpu.py.
 *
 * Every entry name starts with mp_spline_.
 *
 * The operator.  rowptr [N + 1] / col [nnz] is the engine's CSR with the plan / counts_host of mp_spmm_plan_build; its
 * entry values take no part.  w [nnz, 2] fp32 (dense, row stride 2) holds the two weights of every stored entry in
 * ENTRY order.  Both entries are sums: a caller who wants a mean folds 1 / count(row) into w.  Rows longer than the
 * plan's hub_deg go through the piece / finalize path of mp_spmm_csr_f32 (partial sums in the workspace, added in piece
 * order).  No atomics: the same bits every run.  An empty row gives zeros.  The two entries are each other's adjoint:
 * with t the transposed pattern and pos its entries' positions in this one (mp_csr_transpose),
 *   <mp_spline_agg(A, w, X), G> = <X, mp_spline_fold(A^T, w[pos], G)>.
 * fp32 only.  Any d >= 1; a leading dimension below its row's width, d <= 0 or N < 0: MP_ERR_INVALID_ARG;
 * N >= 2^31 or d >= 2^30: MP_ERR_UNSUPPORTED; a workspace below mp_spmm_ws_bytes': MP_ERR_WORKSPACE.  N = 0 returns
 * MP_OK without a launch; col and w may be NULL for an operator without entries.
 */
#ifndef MP_SPLINE_H
#define MP_SPLINE_H

#include "mp_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One gather, two sums:
 *   Y[r, 0:d]  = sum_{e in row r} w[e, 0] * X[col[e], :]
 *   Y[r, d:2d] = sum_{e in row r} w[e, 1] * X[col[e], :]
 * X [n, d] with ldx >= d, Y [N, 2d] with ldy >= 2d: the two sums are the two halves of one row, so a transform with
 * the stacked matrix [W0; W1] reads them without a copy.  Every row of X an entry names is loaded once and meets both
 * weights in registers.  The lane vector is as wide as X, Y and Y + d allow (16, 8 or 4 bytes; Y + d is 16-byte
 * aligned only when d % 4 == 0).  Workspace: mp_spmm_ws_bytes(counts_host, d, MP_SUM, 1). */
int mp_spline_agg_f32(const int32_t* rowptr, const int32_t* col, const float* w, int64_t N, const int32_t* plan,
                      const int32_t* counts_host, const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t d, void* ws,
                      size_t ws_bytes, mp_stream_t stream);

/* Two half rows gathered, one sum:
 *   Y[r, :] = sum_{e in row r} ( w[e, 0] * Z[col[e], 0:d] + w[e, 1] * Z[col[e], d:2d] )
 * Z [n, 2d] with ldz >= 2d, Y [N, d] with ldy >= d.  The input gradient of mp_spline_agg_f32 on the transposed pattern
 * (Z = dY) and the forward of the transform-first order (Z = x [W0 | W1]), whose input gradient is in turn
 * mp_spline_agg_f32 on the transpose.  An entry's term is formed as fma(w1, z1, w0 * z0) and added to the row's sum in
 * entry order.  Workspace: mp_spmm_ws_bytes(counts_host, d, MP_SUM, 0). */
int mp_spline_fold_f32(const int32_t* rowptr, const int32_t* col, const float* w, int64_t N, const int32_t* plan,
                       const int32_t* counts_host, const float* Z, int64_t ldz, float* Y, int64_t ldy, int32_t d, void* ws,
                       size_t ws_bytes, mp_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MP_SPLINE_H */
