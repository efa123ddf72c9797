/*
 * mp_maxbwd.h — C ABI of the max backward in pull form of libmpengine.so (csrc/spmm.hip: MaxBwdRows).
 *
 * What it replaces: the float-atomic scatters mp_spmm_max_bwd_f32 / _bf16 and mp_spmm_heads_max_bwd_f32 of mp_engine.h
 * — the gradient of the operand a reduce = MP_MAX aggregation gathers by source — wherever the caller wants the same
 * bits every run (graphgym_amd.ops.deterministic()).  The same gradient, gathered over the TRANSPOSED pattern on the plan
 * kernel instead of scattered: no atomics, every element of dX written exactly once (no zeroing by the caller):
 *   dX[j, c] = sum over the entries t of row j of the transposed operator, in stored order, of
 *              [argmax[t_col[t]*lda + c] == t_pos[t]] * w[t] * dY[t_col[t], c]
 *
 * The conventions are those of mp_engine.h (device pointers, caller-owned buffers, everything enqueued on `stream`,
 * nothing allocates, nothing synchronises, mp_status return codes).  This header is separate from mp_engine.h, and its
 * entries are bound from a table of their own (graphgym_amd/_lib_maxbwd.py), because the closure tests over mp_engine.h
 * name every entry of that header; the closure over this one is tests/test_deterministic_host.py.
 *
 * Every entry name ends in _max_bwd_pull_f32 or _max_bwd_pull_bf16.
 *
 * The operator.  t_rowptr [n_src + 1], t_col [nnz] (the destination of every transposed entry) and t_pos [nnz] (its
 * forward entry) are what mp_csr_transpose writes; plan / counts_host: mp_spmm_plan_build on t_rowptr; ws:
 * mp_spmm_ws_bytes(counts_host, d, MP_SUM, 0).  argmax [N, >= d] int32 (row stride lda) is what the forward wrote: the
 * winning forward entry per destination and column, -1 where the destination is empty (it matches nothing).  Weights in
 * TRANSPOSED order: t_val [nnz] or NULL (ones); the heads form takes t_a [nnz, heads], column c the weight of its head
 * c / (d / heads).  Each term is one fma into an fp32 sum that starts at 0; a source row longer than the plan's hub_deg
 * is summed in pieces of piece_edges entries, the pieces then added in piece order.  Any d >= 1; lda, ldy or ldx below
 * d, d <= 0, n_src < 0, nnz < 0 or a missing array: MP_ERR_INVALID_ARG; n_src or nnz >= 2^31: MP_ERR_UNSUPPORTED; a
 * workspace below mp_spmm_ws_bytes': MP_ERR_WORKSPACE.  n_src = 0 returns MP_OK without a launch; t_col, t_pos, argmax
 * and dY may be NULL for an operator without entries (dX is then all zeros).
 */
#ifndef MP_MAXBWD_H
#define MP_MAXBWD_H

#include "mp_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fp32 dY [N, d] -> fp32 dX [n_src, d] */
int mp_spmm_max_bwd_pull_f32(const int32_t* t_rowptr, const int32_t* t_col, const int32_t* t_pos, const float* t_val,
                             int64_t n_src, int64_t nnz, const int32_t* plan, const int32_t* counts_host,
                             const int32_t* argmax, int64_t lda, const float* dY, int64_t ldy, int32_t d, float* dX,
                             int64_t ldx, void* ws, size_t ws_bytes, mp_stream_t stream);
/* bf16 dY -> bf16 dX: the sum runs in fp32 and is rounded once (no fp32 buffer of dX exists) */
int mp_spmm_max_bwd_pull_bf16(const int32_t* t_rowptr, const int32_t* t_col, const int32_t* t_pos, const float* t_val,
                              int64_t n_src, int64_t nnz, const int32_t* plan, const int32_t* counts_host,
                              const int32_t* argmax, int64_t lda, const void* dY, int64_t ldy, int32_t d, void* dX,
                              int64_t ldx, void* ws, size_t ws_bytes, mp_stream_t stream);
/* t_a [nnz, heads] required; heads 1, 2, 4 or 8 with d % heads == 0 (other counts: MP_ERR_UNSUPPORTED — run
 * mp_spmm_max_bwd_pull_f32 per head on column slices) */
int mp_spmm_heads_max_bwd_pull_f32(const int32_t* t_rowptr, const int32_t* t_col, const int32_t* t_pos,
                                   const float* t_a, int32_t heads, int64_t n_src, int64_t nnz, const int32_t* plan,
                                   const int32_t* counts_host, const int32_t* argmax, int64_t lda, const float* dY,
                                   int64_t ldy, int32_t d, float* dV, int64_t ldv, void* ws, size_t ws_bytes,
                                   mp_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MP_MAXBWD_H */
