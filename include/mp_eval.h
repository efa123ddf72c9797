/*
 * mp_eval.h — C ABI of the loss and evaluation layer of libmpengine.so (csrc/evalmetrics.hip).
 *
 * What it replaces: graphgym/loss.py:41-47 (the BCE-with-logits and MSE branches of compute_loss) and
 * graphgym/logger.py:85-113 (the per-epoch statistics: accuracy, precision, recall, F1, AUC, MAE, MSE, RMSE), which the
 * reference computes with scikit-learn on host copies of every batch.
 *
 * The conventions are those of mp_engine.h (device pointers, caller-owned buffers, everything enqueued on `stream`,
 * nothing synchronises, mp_status return codes).  This header is separate from mp_engine.h, and its entries are bound
 * from a table of their own (graphgym_amd/_lib_eval.py), because the closure tests over mp_engine.h name every entry of
 * that header; the closures over this one are tests/test_eval_host.py and tests/test_poison_eval_gpu.py.
 *
 * Every entry name starts with mp_eval_.
 *
 * State.  An epoch's accumulators live in one caller-owned, zero-initialised device array of MP_EVAL_STATE_WORDS
 * 64-bit words (mp_eval_state_words()).  Words 0 .. 11 are int64 counters, updated with integer atomics: their values do
 * not depend on the order of updates or of workgroups.  Words 12 .. 14 are doubles: each update forms its sum from
 * per-workgroup partials in a fixed order (no float atomics) and one thread adds it to the word, so an epoch of the same
 * updates in the same order reproduces them bit for bit.  An epoch's result is one copy of the array to the host.
 *
 * Bad input.  No label, index or class id is used as an address unchecked: a label outside [0, C) ({0, 1} for the
 * binary statistics) or an index outside [0, n_rows) is counted in MP_EVAL_INVALID and skipped.
 */
#ifndef MP_EVAL_H
#define MP_EVAL_H

#include "mp_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

enum mp_eval_word {
  MP_EVAL_COUNT = 0,   /* examples that entered the statistics (valid label and index) */
  MP_EVAL_HITS = 1,    /* multi-class: rows whose first maximum is the label */
  MP_EVAL_INVALID = 2, /* examples skipped: label or index out of range */
  MP_EVAL_TP = 3,
  MP_EVAL_FP = 4,
  MP_EVAL_TN = 5,
  MP_EVAL_FN = 6,
  MP_EVAL_NAN = 7,   /* AUC: examples whose score is NaN */
  MP_EVAL_TWO_U = 8, /* AUC: 2 U = sum over positives of 2 #(negatives below) + #(negatives equal) */
  MP_EVAL_P = 9,     /* AUC: positives with a score that is not NaN */
  MP_EVAL_N = 10,    /* AUC: negatives with a score that is not NaN */
  MP_EVAL_SIZE = 11, /* sum of batch sizes behind MP_EVAL_LOSS (Logger._size_current, logger.py:129) */
  MP_EVAL_LOSS = 12, /* double: sum of loss * batch_size (logger.py:130) */
  MP_EVAL_ABS = 13,  /* double: sum |pred - true| */
  MP_EVAL_SQ = 14,   /* double: sum (pred - true)^2 */
  MP_EVAL_STATE_WORDS = 16
};

enum mp_eval_loss { MP_EVAL_BCE = 0, MP_EVAL_MSE = 1 };

/* MP_EVAL_STATE_WORDS (host only) */
int mp_eval_state_words(void);

/* bytes of the workspace the entries below take for a problem of n elements (rows): the per-workgroup partial sums.
   Host only.  The workspace's contents on entry do not matter. */
int mp_eval_ws_bytes(int64_t n, size_t* bytes);

/* Element-wise loss, forward (loss.py:41-47).  kind MP_EVAL_BCE: term = max(z, 0) - z y + log1p(exp(-|z|)) and
   score = sigmoid(z) (nn.BCEWithLogitsLoss and the torch.sigmoid next to it; y may be any value in [0, 1]); kind
   MP_EVAL_MSE: term = (z - y)^2 and score = z.  loss[0] = (float)(scale * sum of terms), the sum formed in double
   (scale = 1 / n for reduction 'mean', 1 for 'sum'; n = 0 gives scale * 0).  score [n] and loss [1] are written, not
   accumulated.  z, y, score: contiguous fp32. */
int mp_eval_loss_fwd_f32(int kind, const float* z, const float* y, int64_t n, float scale, float* score, float* loss,
                         void* ws, size_t ws_bytes, mp_stream_t stream);

/* Its backward: dz[k] = (sigmoid(z) - y) g[0] scale (BCE) or 2 (z - y) g[0] scale (MSE), written.  g: one fp32 on the
   device (the incoming gradient of the loss). */
int mp_eval_loss_bwd_f32(int kind, const float* z, const float* y, int64_t n, const float* g, float scale, float* dz,
                         mp_stream_t stream);

/* Multi-class statistics and loss in one pass over raw logits [n_rows, C] (leading dimension ld >= C), one lane per
   selected row k < n_sel: row i = index ? index[k] : k, label labels[k].  best = the lowest index among the row's maxima
   (best = 0; for c in 1 .. C: if z[c] > z[best]: best = c).  Adds to state: COUNT (valid rows), HITS (best == label),
   INVALID, SIZE (n_sel) and LOSS (the softmax cross-entropy of the valid rows, summed in double).  log_softmax is never
   stored.  C > 1024 is MP_ERR_UNSUPPORTED (one lane walks a row three times). */
int mp_eval_multi_logits_f32(const float* logits, int64_t ld, int64_t n_rows, const int64_t* labels,
                             const int64_t* index, int64_t n_sel, int32_t C, int64_t* state, void* ws, size_t ws_bytes,
                             mp_stream_t stream);

/* The same statistics from an already computed score matrix [n, C] (what Logger.update_stats is given,
   logger.py:85-89,102-105), without the loss: COUNT, HITS, INVALID; and SIZE += n, LOSS += loss * n with
   loss = loss_dev ? loss_dev[0] : loss_host (logger.py:128-130). */
int mp_eval_multi_scores_f32(const float* scores, int64_t ld, int64_t n, const int64_t* labels, int32_t C,
                             const float* loss_dev, double loss_host, int64_t* state, mp_stream_t stream);

/* Binary statistics (logger.py:85-100): pred_int = score > thresh; adds TP, FP, TN, FN, COUNT, INVALID (label not in
   {0, 1}), SIZE and LOSS as above.  Exactly one of labels (int64) and labels_f32 is given: the fp32 form takes the
   labels link-prediction batches carry (transform.py:93-98), 1.0f and 0.0f; any other value is invalid.  score_keep [n]
   fp32 and label_keep [n] int8, when both are given, receive a copy of the scores and the labels as 0 / 1 (2 for an
   invalid one): what mp_eval_auc_pairs needs at the end of the epoch. */
int mp_eval_binary_f32(const float* score, const int64_t* labels, const float* labels_f32, int64_t n, float thresh,
                       const float* loss_dev, double loss_host, float* score_keep, int8_t* label_keep, int64_t* state,
                       mp_stream_t stream);

/* Regression statistics (logger.py:107-113): ABS += sum |pred - true|, SQ += sum (pred - true)^2 (differences and sums
   in double), COUNT += n, SIZE and LOSS as above. */
int mp_eval_regression_f32(const float* pred, const float* truth, int64_t n, const float* loss_dev, double loss_host,
                           int64_t* state, void* ws, size_t ws_bytes, mp_stream_t stream);

/* Exact AUC pair count over scores sorted ascending (NaN last, as torch.sort leaves them) with their labels
   (int8: 1 positive, 0 negative, anything else neither) and cn [n + 1], the exclusive prefix count of negatives over
   that order (cn[i] = negatives among the first i).  Per positive i: lb / ub = lower / upper bound of s[i] in s (two
   binary searches, compared with < and <=, so -0.0 and 0.0 are one tie group); TWO_U += cn[lb] + cn[ub].  Also adds P, N
   and NAN.  AUC = TWO_U / (2 P N), all integers: the result does not depend on any summation order.  Every read stays
   inside [0, n) of s / labels and [0, n] of cn whatever the arrays hold. */
int mp_eval_auc_pairs(const float* sorted_score, const int8_t* sorted_label, const int64_t* cn, int64_t n,
                      int64_t* state, mp_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MP_EVAL_H */
