/*
 * mp_pair.h — C ABI of the pair decoders of libmpengine.so (csrc/pair.hip).
 *
 * What it replaces: the three lines of GNNEdgeHead.forward (graphgym/models/head.py:62-85) that gather
 * batch.node_feature[batch.edge_label_index] into a [2, K, d] tensor and then take (a * b).sum(-1),
 * F.cosine_similarity(a, b) or cat((a, b), -1) into the MLP.  The score of a pair is one entry of a sampled
 * dense-dense product, its gradient a weighted neighbour sum over "the pairs that touch node v", and the first Linear
 * of the concat decoding distributes over the two halves of the concatenation: nothing of size K x d is gathered.
 *
 * The conventions are those of mp_engine.h (device pointers, caller-owned buffers, everything enqueued on `stream`,
 * nothing allocates, nothing synchronises, mp_status return codes).  This header is separate from mp_engine.h, and its
 * entries are bound from a table of their own (graphgym_amd/_lib_pair.py), because the closure tests over mp_engine.h
 * name every entry of that header; the closures over this one are tests/test_pair_host.py and
 * tests/test_poison_pair_gpu.py.
 *
 * Every entry name starts with mp_pair_ (mp_engine.h has one older entry of that prefix, mp_pair_space_rows of the
 * negative sampler; it is not one of these).
 *
 * The pairs.  a [K], b [K] are int64 device arrays, the two rows of edge_label_index, in no particular order; no
 * int32 copy is made.  An index outside [0, N) is never dereferenced: that pair's result is NaN (score: the score;
 * sum: the whole row) and the int32 device counter `bad` (zeroed by the caller) is incremented once per such pair
 * with an integer atomic.  No float atomics anywhere: the same bits every run.
 *
 * The lane grouping of the score and sum kernels.  A pair is served by G lanes, G the power of two >= ceil(d / 4)
 * capped at 64 (16-byte row loads: the leading dimensions and d multiples of 4, the bases 16-byte aligned) or the
 * power of two >= d capped at 64 (4-byte loads otherwise); a wave serves 64 / G pairs per step and keeps four steps'
 * loads in flight.  Rows wider than one group's span (256 or 64 columns) are walked in column tiles.
 *
 * fp32 only.  A null pointer where one is required, a negative size, d <= 0 or a leading dimension below its row's
 * width: MP_ERR_INVALID_ARG.  N >= 2^31, K >= 2^30 (the inverted index has 2K int32 entries) or d >= 2^30:
 * MP_ERR_UNSUPPORTED.  K == 0 (rnorm: N == 0) returns MP_OK without a launch; the per-pair arrays may then be NULL.
 */
#ifndef MP_PAIR_H
#define MP_PAIR_H

#include "mp_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

/* r[v] = 1 / max(||h_v||_2, eps), one pass over h [N, d] (ldh >= d).  The rule of F.cosine_similarity: each norm is
 * clamped on its own, cos = <a, b> / (max(||a||, eps) * max(||b||, eps)).  eps > 0.
 * q [N], when given: q[v] = 1 / ||h_v||, the reciprocal of the norm itself, and 0 for a zero (or denormal) norm — what
 * the gradient needs beside r, see mp_pair_bwd_weights_f32.  q == r on every row the clamp does not bind. */
int mp_pair_rnorm_f32(const float* h, int64_t ldh, int64_t N, int32_t d, float eps, float* r, float* q_or_null,
                      mp_stream_t stream);

/* score[k] = <h[a_k], h[b_k]>, times r[a_k] * r[b_k] when r [N] is given (the cosine similarity, r from
 * mp_pair_rnorm_f32).  h [N, d] with ldh >= d.  Scores leave a wave as one coalesced store per 64 pairs. */
int mp_pair_score_f32(const float* h, int64_t ldh, int64_t N, int32_t d, const int64_t* a, const int64_t* b, int64_t K,
                      const float* r_or_null, float* score, int32_t* bad, mp_stream_t stream);

/* z[k, :] = U[a_k, :] + V[b_k, :] + bias: the first Linear of the concat decoding after
 * cat(h[a], h[b]) W^T = (h W[:, :d]^T)[a] + (h W[:, d:]^T)[b].  U, V [N, m] with ldu, ldv >= m; z [K, m] with
 * ldz >= m; bias [m] or NULL.  The sum is formed as (U + V) + bias. */
int mp_pair_sum_f32(const float* U, int64_t ldu, const float* V, int64_t ldv, int64_t N, int32_t m, const int64_t* a,
                    const int64_t* b, int64_t K, const float* bias_or_null, float* z, int64_t ldz, int32_t* bad,
                    mp_stream_t stream);

/* The entry weights and the diagonal of the score's input gradient, dh = A_w h + diag (.) h, in one pass over the
 * inverted index of the pair list: rowptr [N + 1] / eid [2K] is the CSR of cat([index, index.flip(0)], 1) by
 * destination (mp_csr_from_coo), row v listing every pair v belongs to, pair k = eid[e] mod K.  g [K] is the gradient
 * of the scores.
 *   w[e]    = g[k]                          (r NULL: dot)
 *   w[e]    = g[k] * r[a_k] * r[b_k]        (r given: cosine)
 *   diag[v] = - r[v] * q[v] * sum_{e in row v} g[k] * score[k]
 *             (diag, score, r and q given together; score is the cosine the forward returned, r and q are those of
 *             mp_pair_rnorm_f32)
 * The diagonal is what torch's F.cosine_similarity differentiates to: it clamps the VALUE of each norm and still
 * differentiates the norm itself, d/dx (1 / max(||x||, eps)) = - x / (||x|| max(||x||, eps)^2), so below eps the term is
 * r q, not r^2 and not 0 ([1e-9] against [2.0]: 9e7 = 1e8 - 1e7); on every other row q == r and it is - r^2.  A zero
 * row has q = 0 and x = 0: no term.
 * A row's sum runs over its entries in a fixed order (16 lanes stride over the row, then a shuffle tree): one writer
 * per element, no atomics.  An entry whose eid or pair ids are out of range gets weight 0. */
int mp_pair_bwd_weights_f32(const int32_t* rowptr, const int32_t* eid, int64_t N, int64_t K, const float* g,
                            const float* score_or_null, const float* r_or_null, const float* q_or_null,
                            const int64_t* a, const int64_t* b, float* w, float* diag_or_null, mp_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MP_PAIR_H */
