// Loss and evaluation as device passes (include/mp_eval.h): the BCE-with-logits and MSE branches of compute_loss
// (graphgym/loss.py:41-47), forward and backward, and the epoch statistics of graphgym/logger.py:85-113 accumulated into
// a small caller-owned state array, so that a training or evaluation step hands nothing to the host and an epoch's
// metrics cost one copy of MP_EVAL_STATE_WORDS words.
//   counters  int64, one integer atomic per workgroup and counter: order-independent
//   sums      double, per-thread over a fixed assignment of elements -> per-workgroup partial in thread order ->
//             one workgroup adds the partials in a fixed order and ONE thread adds the result to the state word
//             (the bn_block_sum / bn_col_sums pattern of bn_kernels.h; no float atomics)
// Every index is 64-bit, and no label, index or class id reaches an address before it has been range-checked.
#include "common.h"
#include "../../include/mp_eval.h"

namespace mp {

typedef unsigned long long u64;

constexpr int kEvalMaxC = 1024;

// The workgroup's sum of K doubles per thread, in thread order: 16 threads add 16 values each, thread 0 adds the 16
// sums and stores dst[k * stride].  Every thread of the workgroup calls it.
template <int K>
__device__ __forceinline__ void eval_block_sums(const double (&v)[K], double* dst, int64_t stride) {
  __shared__ double sv[K][kBlock];
  __shared__ double sw[K][16];
#pragma unroll
  for (int k = 0; k < K; ++k) sv[k][threadIdx.x] = v[k];
  __syncthreads();
  if (threadIdx.x < 16) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < 16; ++q) s += sv[k][threadIdx.x * 16 + q];
      sw[k][threadIdx.x] = s;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      double s = 0.0;
#pragma unroll
      for (int q = 0; q < 16; ++q) s += sw[k][q];
      dst[k * stride] = s;
    }
  }
  __syncthreads();
}

// The workgroup's K counters -> the state words `slot`: a wave sum by shuffles, one LDS atomic per wave, one global
// integer atomic per workgroup and counter that is not zero.  Every thread of the workgroup calls it.
template <int K>
__device__ __forceinline__ void eval_block_counts(const u64 (&c)[K], const int (&slot)[K], int64_t* __restrict__ state) {
  __shared__ u64 cnt[K];
  if (threadIdx.x < K) cnt[threadIdx.x] = 0;
  __syncthreads();
#pragma unroll
  for (int k = 0; k < K; ++k) {
    u64 v = c[k];
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_down(v, off, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0 && v) atomicAdd(&cnt[k], v);
  }
  __syncthreads();
  if (threadIdx.x < K && cnt[threadIdx.x]) atomicAdd(reinterpret_cast<u64*>(state) + slot[threadIdx.x], cnt[threadIdx.x]);
}

// SIZE += n and LOSS += loss * n (logger.py:128-130) by ONE thread of the launch: no other thread of it touches the two
__device__ __forceinline__ void eval_add_loss(const float* __restrict__ loss_dev, double loss_host, int64_t n,
                                              int64_t* __restrict__ state) {
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    const double l = loss_dev ? (double)loss_dev[0] : loss_host;
    state[MP_EVAL_SIZE] += n;
    reinterpret_cast<double*>(state)[MP_EVAL_LOSS] += l * (double)n;
  }
}

// ---- element-wise losses --------------------------------------------------------------------------------------------
__device__ __forceinline__ float eval_sigmoid(float z, float e) {   // e = exp(-|z|)
  const float r = 1.0f / (1.0f + e);
  return z >= 0.f ? r : e * r;
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void eval_loss_fwd_kernel(const float* __restrict__ z, const float* __restrict__ y,
                                                               int64_t n, float* __restrict__ score,
                                                               double* __restrict__ partial) {
  double acc[1] = {0.0};
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const float a = z[k], t = y[k];
    float term, s;
    if (KIND == MP_EVAL_BCE) {
      const float e = expf(-fabsf(a));
      term = fmaxf(a, 0.f) - a * t + log1pf(e);
      s = eval_sigmoid(a, e);
    } else {
      const float d = a - t;
      term = d * d;
      s = a;
    }
    score[k] = s;
    acc[0] += (double)term;
  }
  eval_block_sums<1>(acc, partial + blockIdx.x, 0);
}

template <int KIND>
__global__ __launch_bounds__(kBlock) void eval_loss_bwd_kernel(const float* __restrict__ z, const float* __restrict__ y,
                                                               int64_t n, const float* __restrict__ g, float scale,
                                                               float* __restrict__ dz) {
  const float coef = g[0] * scale;
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const float a = z[k], t = y[k];
    if (KIND == MP_EVAL_BCE) dz[k] = (eval_sigmoid(a, expf(-fabsf(a))) - t) * coef;
    else dz[k] = 2.0f * (a - t) * coef;
  }
}

// One workgroup: K sums over the nblk per-workgroup partials (partial[k * nblk + b]), each thread every 256th partial,
// then the threads in order.  loss_out: loss_out[0] = (float)(scale * sum 0).  state: word slot[k] += sum k, and
// SIZE += size, by one thread.
template <int K>
__global__ __launch_bounds__(kBlock) void eval_finalize_kernel(const double* __restrict__ partial, int nblk,
                                                               float* __restrict__ loss_out, double scale,
                                                               int64_t* __restrict__ state, int slot0, int slot1,
                                                               int64_t size) {
  __shared__ double res[K];
  double v[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double a = 0.0;
    for (int b = threadIdx.x; b < nblk; b += kBlock) a += partial[(int64_t)k * nblk + b];
    v[k] = a;
  }
  eval_block_sums<K>(v, res, 1);
  if (threadIdx.x == 0) {
    if (loss_out) loss_out[0] = (float)(scale * res[0]);
    if (state) {
      double* sd = reinterpret_cast<double*>(state);
      sd[slot0] += res[0];
      if (K > 1) sd[slot1] += res[K - 1];
      state[MP_EVAL_SIZE] += size;
    }
  }
}

// ---- multi-class --------------------------------------------------------------------------------------------------------
template <bool LOSS>
__global__ __launch_bounds__(kBlock) void eval_multi_kernel(const float* __restrict__ logits, int64_t ld,
                                                            const int64_t* __restrict__ labels,
                                                            const int64_t* __restrict__ index, int64_t n_sel,
                                                            int64_t n_rows, int32_t C, const float* __restrict__ loss_dev,
                                                            double loss_host, int64_t* __restrict__ state,
                                                            double* __restrict__ partial) {
  u64 c[3] = {0, 0, 0};   // COUNT, HITS, INVALID
  double acc[1] = {0.0};
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n_sel; k += (int64_t)gridDim.x * blockDim.x) {
    const int64_t i = index ? index[k] : k;
    const int64_t y = labels[k];
    if ((uint64_t)y >= (uint64_t)C || (uint64_t)i >= (uint64_t)n_rows) { ++c[2]; continue; }
    const float* z = logits + i * ld;
    int best = 0;
    float m = z[0];
    for (int q = 1; q < C; ++q) {
      const float v = z[q];
      if (v > m) { m = v; best = q; }
    }
    ++c[0];
    c[1] += (best == (int)y) ? 1 : 0;
    if (LOSS) {
      float s = 0.f;
      for (int q = 0; q < C; ++q) s += expf(z[q] - m);
      acc[0] += (double)(logf(s) + m - z[y]);
    }
  }
  const int slot[3] = {MP_EVAL_COUNT, MP_EVAL_HITS, MP_EVAL_INVALID};
  eval_block_counts<3>(c, slot, state);
  if (LOSS) eval_block_sums<1>(acc, partial + blockIdx.x, 0);
  else eval_add_loss(loss_dev, loss_host, n_sel, state);
}

// ---- binary ---------------------------------------------------------------------------------------------------------------
// LT: int64 labels, or the fp32 labels link-prediction batches carry (transform.py:93-98): 1.0f and 0.0f are the two
// classes, any other value (0.5, NaN) is invalid
template <typename LT>
__global__ __launch_bounds__(kBlock) void eval_binary_kernel(const float* __restrict__ score,
                                                             const LT* __restrict__ labels, int64_t n, float thresh,
                                                             const float* __restrict__ loss_dev, double loss_host,
                                                             float* __restrict__ score_keep,
                                                             int8_t* __restrict__ label_keep,
                                                             int64_t* __restrict__ state) {
  u64 c[6] = {0, 0, 0, 0, 0, 0};   // TP, FP, TN, FN, COUNT, INVALID
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const float s = score[k];
    const LT y = labels[k];
    const bool pos = s > thresh;
    int8_t y8 = 2;
    if (y == (LT)1) { y8 = 1; ++c[pos ? 0 : 3]; ++c[4]; }
    else if (y == (LT)0) { y8 = 0; ++c[pos ? 1 : 2]; ++c[4]; }
    else ++c[5];
    if (score_keep) { score_keep[k] = s; label_keep[k] = y8; }
  }
  const int slot[6] = {MP_EVAL_TP, MP_EVAL_FP, MP_EVAL_TN, MP_EVAL_FN, MP_EVAL_COUNT, MP_EVAL_INVALID};
  eval_block_counts<6>(c, slot, state);
  eval_add_loss(loss_dev, loss_host, n, state);
}

// ---- regression ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void eval_regression_kernel(const float* __restrict__ pred,
                                                                 const float* __restrict__ truth, int64_t n,
                                                                 const float* __restrict__ loss_dev, double loss_host,
                                                                 int64_t* __restrict__ state,
                                                                 double* __restrict__ partial) {
  double acc[2] = {0.0, 0.0};
  for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (int64_t)gridDim.x * blockDim.x) {
    const double d = (double)pred[k] - (double)truth[k];
    acc[0] += fabs(d);
    acc[1] += d * d;
  }
  eval_block_sums<2>(acc, partial + blockIdx.x, gridDim.x);
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(reinterpret_cast<u64*>(state) + MP_EVAL_COUNT, (u64)n);
  eval_add_loss(loss_dev, loss_host, n, state);
}

// ---- exact AUC ------------------------------------------------------------------------------------------------------------
// s ascending with NaN last: `s[mid] < v` and `s[mid] <= v` are false for a NaN, so both predicates stay monotone over
// the whole array.  lb is searched in [0, i] and ub in [i + 1, n], after a look at the two neighbours (distinct scores:
// lb = i, ub = i + 1 without a search).  Whatever s holds, mid stays in [0, n) and lb, ub in [0, n].
__global__ __launch_bounds__(kBlock) void eval_auc_pairs_kernel(const float* __restrict__ s,
                                                                const int8_t* __restrict__ lab,
                                                                const int64_t* __restrict__ cn, int64_t n,
                                                                int64_t* __restrict__ state) {
  u64 c[4] = {0, 0, 0, 0};   // TWO_U, P, N, NAN
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const float v = s[i];
    const int8_t y = lab[i];
    if (v != v) { ++c[3]; continue; }
    if (y == 0) { ++c[2]; continue; }
    if (y != 1) continue;
    ++c[1];
    int64_t lb = i, ub = i + 1;
    if (i > 0 && !(s[i - 1] < v)) {
      int64_t lo = 0, hi = i;
      while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (s[mid] < v) lo = mid + 1; else hi = mid;
      }
      lb = lo;
    }
    if (i + 1 < n && s[i + 1] <= v) {
      int64_t lo = i + 1, hi = n;
      while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (s[mid] <= v) lo = mid + 1; else hi = mid;
      }
      ub = lo;
    }
    c[0] += (u64)cn[lb] + (u64)cn[ub];
  }
  const int slot[4] = {MP_EVAL_TWO_U, MP_EVAL_P, MP_EVAL_N, MP_EVAL_NAN};
  eval_block_counts<4>(c, slot, state);
}

static inline size_t eval_ws(int64_t n) { return align_up((size_t)flat_grid(n) * 2 * sizeof(double), 256); }

}  // namespace mp

using namespace mp;

extern "C" {

int mp_eval_state_words(void) { return MP_EVAL_STATE_WORDS; }

int mp_eval_ws_bytes(int64_t n, size_t* bytes) {
  if (n < 0 || !bytes) return MP_ERR_INVALID_ARG;
  *bytes = eval_ws(n);
  return MP_OK;
}

int mp_eval_loss_fwd_f32(int kind, const float* z, const float* y, int64_t n, float scale, float* score, float* loss,
                         void* ws, size_t ws_bytes, mp_stream_t stream) {
  if ((kind != MP_EVAL_BCE && kind != MP_EVAL_MSE) || n < 0 || !loss || !ws || (n > 0 && (!z || !y || !score)))
    return MP_ERR_INVALID_ARG;
  if (ws_bytes < eval_ws(n)) return MP_ERR_WORKSPACE;
  double* partial = (double*)ws;
  const int grid = n > 0 ? flat_grid(n) : 0;
  if (n > 0) {
    if (kind == MP_EVAL_BCE)
      hipLaunchKernelGGL(eval_loss_fwd_kernel<MP_EVAL_BCE>, dim3(grid), dim3(kBlock), 0, as_stream(stream), z, y, n, score,
                         partial);
    else
      hipLaunchKernelGGL(eval_loss_fwd_kernel<MP_EVAL_MSE>, dim3(grid), dim3(kBlock), 0, as_stream(stream), z, y, n, score,
                         partial);
    MP_LAUNCH_CHECK();
  }
  hipLaunchKernelGGL(eval_finalize_kernel<1>, dim3(1), dim3(kBlock), 0, as_stream(stream), partial, grid, loss,
                     (double)scale, (int64_t*)nullptr, 0, 0, (int64_t)0);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_eval_loss_bwd_f32(int kind, const float* z, const float* y, int64_t n, const float* g, float scale, float* dz,
                         mp_stream_t stream) {
  if ((kind != MP_EVAL_BCE && kind != MP_EVAL_MSE) || n < 0 || !g || (n > 0 && (!z || !y || !dz)))
    return MP_ERR_INVALID_ARG;
  if (n == 0) return MP_OK;
  if (kind == MP_EVAL_BCE)
    hipLaunchKernelGGL(eval_loss_bwd_kernel<MP_EVAL_BCE>, dim3(flat_grid(n)), dim3(kBlock), 0, as_stream(stream), z, y, n,
                       g, scale, dz);
  else
    hipLaunchKernelGGL(eval_loss_bwd_kernel<MP_EVAL_MSE>, dim3(flat_grid(n)), dim3(kBlock), 0, as_stream(stream), z, y, n,
                       g, scale, dz);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_eval_multi_logits_f32(const float* logits, int64_t ld, int64_t n_rows, const int64_t* labels,
                             const int64_t* index, int64_t n_sel, int32_t C, int64_t* state, void* ws, size_t ws_bytes,
                             mp_stream_t stream) {
  if (n_sel < 0 || n_rows < 0 || C <= 0 || ld < C || !state || !ws || (n_sel > 0 && (!logits || !labels)))
    return MP_ERR_INVALID_ARG;
  if (!index && n_sel > n_rows) return MP_ERR_INVALID_ARG;
  if (C > kEvalMaxC) return MP_ERR_UNSUPPORTED;
  if (ws_bytes < eval_ws(n_sel)) return MP_ERR_WORKSPACE;
  if (n_sel == 0) return MP_OK;
  double* partial = (double*)ws;
  const int grid = flat_grid(n_sel);
  hipLaunchKernelGGL(eval_multi_kernel<true>, dim3(grid), dim3(kBlock), 0, as_stream(stream), logits, ld, labels, index,
                     n_sel, n_rows, C, (const float*)nullptr, 0.0, state, partial);
  MP_LAUNCH_CHECK();
  hipLaunchKernelGGL(eval_finalize_kernel<1>, dim3(1), dim3(kBlock), 0, as_stream(stream), partial, grid,
                     (float*)nullptr, 1.0, state, (int)MP_EVAL_LOSS, (int)MP_EVAL_LOSS, n_sel);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_eval_multi_scores_f32(const float* scores, int64_t ld, int64_t n, const int64_t* labels, int32_t C,
                             const float* loss_dev, double loss_host, int64_t* state, mp_stream_t stream) {
  if (n < 0 || C <= 0 || ld < C || !state || (n > 0 && (!scores || !labels))) return MP_ERR_INVALID_ARG;
  if (C > kEvalMaxC) return MP_ERR_UNSUPPORTED;
  if (n == 0) return MP_OK;
  hipLaunchKernelGGL(eval_multi_kernel<false>, dim3(flat_grid(n)), dim3(kBlock), 0, as_stream(stream), scores, ld, labels,
                     (const int64_t*)nullptr, n, n, C, loss_dev, loss_host, state, (double*)nullptr);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_eval_binary_f32(const float* score, const int64_t* labels, const float* labels_f32, int64_t n, float thresh,
                       const float* loss_dev, double loss_host, float* score_keep, int8_t* label_keep, int64_t* state,
                       mp_stream_t stream) {
  if (n < 0 || !state || (labels && labels_f32) || (n > 0 && (!score || (!labels && !labels_f32))) ||
      ((score_keep == nullptr) != (label_keep == nullptr)))
    return MP_ERR_INVALID_ARG;
  if (n == 0) return MP_OK;
  if (labels)
    hipLaunchKernelGGL(eval_binary_kernel<int64_t>, dim3(flat_grid(n)), dim3(kBlock), 0, as_stream(stream), score, labels,
                       n, thresh, loss_dev, loss_host, score_keep, label_keep, state);
  else
    hipLaunchKernelGGL(eval_binary_kernel<float>, dim3(flat_grid(n)), dim3(kBlock), 0, as_stream(stream), score,
                       labels_f32, n, thresh, loss_dev, loss_host, score_keep, label_keep, state);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_eval_regression_f32(const float* pred, const float* truth, int64_t n, const float* loss_dev, double loss_host,
                           int64_t* state, void* ws, size_t ws_bytes, mp_stream_t stream) {
  if (n < 0 || !state || !ws || (n > 0 && (!pred || !truth))) return MP_ERR_INVALID_ARG;
  if (ws_bytes < eval_ws(n)) return MP_ERR_WORKSPACE;
  if (n == 0) return MP_OK;
  double* partial = (double*)ws;
  const int grid = flat_grid(n);
  hipLaunchKernelGGL(eval_regression_kernel, dim3(grid), dim3(kBlock), 0, as_stream(stream), pred, truth, n, loss_dev,
                     loss_host, state, partial);
  MP_LAUNCH_CHECK();
  hipLaunchKernelGGL(eval_finalize_kernel<2>, dim3(1), dim3(kBlock), 0, as_stream(stream), partial, grid,
                     (float*)nullptr, 1.0, state, (int)MP_EVAL_ABS, (int)MP_EVAL_SQ, (int64_t)0);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_eval_auc_pairs(const float* sorted_score, const int8_t* sorted_label, const int64_t* cn, int64_t n,
                      int64_t* state, mp_stream_t stream) {
  if (n < 0 || !state || !cn || (n > 0 && (!sorted_score || !sorted_label))) return MP_ERR_INVALID_ARG;
  if (n == 0) return MP_OK;
  hipLaunchKernelGGL(eval_auc_pairs_kernel, dim3(flat_grid(n)), dim3(kBlock), 0, as_stream(stream), sorted_score,
                     sorted_label, cn, n, state);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // extern "C"
