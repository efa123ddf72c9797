// BatchNorm1d over the node axis in training mode, with the activation fused — the post-ops GraphGym wraps
// around every conv (graphgym/models/layer.py:26-35: BatchNorm1d(eps, mom) -> act) and the keras
// BatchNormalization inside the TF path's GIN MLPs (main_zd.py:181-186, 214-225).
//
// Why it is here: at the headline size ([10^7, 256] activations) torch's batch_norm_backward_reduce_kernel
// runs one workgroup per feature column and takes 0.52 s per call — 74 % of a GIN training step
// (profiles/r01_gin_step_library_bn.txt).  These are plain HBM-bound passes:
//   forward   stats  : one read of x            -> per-column sum / sum of squares (shifted by the median of three rows)
//             apply  : read x, write y          -> y = act(x * scale + shift)
//   backward  stats  : read dy (, y), x         -> sum(g), sum(g * x)  with g = dy * [y > 0]
//             apply  : read dy (, y), x, write  -> dx = A * g + B * x + C   (per-column constants)
//   skip block  apply  : read x, skip, write out  -> out = act(skip + BN(x)) or [act(skip) | act(BN(x))]  (gnn.py:49-60)
//               bwd    : the statistics pass writes g (= d skip), the apply pass reads it: 7 instead of 8 N d
//   any activation of act.h (the *_act entries): the same passes with act_fwd<ACT> in the apply pass and, backward,
//             g = dy * act'(z) with z recomputed from x (and skip) — the forward's output is never read; PRELU's slope
//             gradient is a third sum of the statistics pass, one partial per workgroup
// Column sums are accumulated per workgroup over a contiguous run of rows (fp32, <= a few thousand terms
// per lane), written as partial slabs and combined in double precision in slab order: deterministic and
// accurate at 10^7 rows.
// The apply pass and the backward's three passes are the kernel templates of bn_kernels.h; this file holds the forward
// statistics, the CONCAT left slab, PRELU's slope finalize and the entries without dropout mask.
#include "bn_kernels.h"

namespace mp {

// The pivot of the forward statistics: per column the median of rows 0, N / 2 and N - 1.  The sums are taken of
// x - pivot, and var = E[v^2] - E[v]^2 loses (pivot - mean)^2 / var of the fp32 partials' precision: a single sample is an
// outlier too often — row 0 of a preferential-attachment graph is its largest hub, ten and more standard deviations
// from the column mean behind an unnormalised add aggregation.  The median of three is exact to select, so the
// statistics kernel and the finalize kernel get the same bits.
template <int W>
__device__ __forceinline__ void bn_pivot(const float* __restrict__ x, int64_t ldx, int64_t N, int c0, float (&pv)[W]) {
  float a[W], b[W], c[W];
  load_vec<W>(x + c0, a);
  load_vec<W>(x + (N / 2) * ldx + c0, b);
  load_vec<W>(x + (N - 1) * ldx + c0, c);
#pragma unroll
  for (int k = 0; k < W; ++k) pv[k] = fmaxf(fminf(a[k], b[k]), fminf(fmaxf(a[k], b[k]), c[k]));
}

// forward statistics: a = sum(x - pivot), b = sum((x - pivot)^2) over the workgroup's run of rows, pivot = bn_pivot(x)
template <int W>
__global__ __launch_bounds__(kBlock) void bn_fwd_stats_kernel(const float* __restrict__ x, int64_t ldx, int64_t N,
                                                              int32_t d, int64_t rows_per_block,
                                                              float* __restrict__ partial) {
  const BnGeom g = bn_geom<W>(d);
  const int cgi = threadIdx.x % g.cg;
  const int rli = threadIdx.x / g.cg;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < N ? r0 + rows_per_block : N;
  for (int t = 0; t < g.tiles; ++t) {
    const int c0 = (t * g.cg + cgi) * W;
    const bool on = c0 < d;
    float a[W], b[W], pv[W];
#pragma unroll
    for (int k = 0; k < W; ++k) { a[k] = 0.f; b[k] = 0.f; pv[k] = 0.f; }
    if (on) {
      bn_pivot<W>(x, ldx, N, c0, pv);
      for (int64_t r = r0 + rli; r < r1; r += g.rl) {
        float xv[W];
        load_vec<W>(x + r * ldx + c0, xv);
#pragma unroll
        for (int k = 0; k < W; ++k) {
          const float v = xv[k] - pv[k];
          a[k] += v;
          b[k] = fmaf(v, v, b[k]);
        }
      }
    }
    bn_colsum_store<W>(a, b, g, cgi, rli, on, c0, d, partial);
  }
}

// forward finalize: mean, invstd, unbiased variance, and the affine of the apply pass
__global__ __launch_bounds__(kBlock) void bn_fwd_finalize_kernel(const float* __restrict__ partial, int nblk,
                                                                 const float* __restrict__ x, int64_t ldx, int64_t N,
                                                                 int32_t d, const float* __restrict__ gamma,
                                                                 const float* __restrict__ beta, float eps,
                                                                 float* mean, float* invstd, float* var_unbiased,
                                                                 float* scale, float* shift) {
  int c;
  double s1, s2;
  if (!bn_col_sums(partial, nblk, d, c, s1, s2)) return;
  const double m_shift = s1 / (double)N;
  double var = s2 / (double)N - m_shift * m_shift;      // biased (training normalisation)
  if (var < 0.0) var = 0.0;
  float pv[1];
  bn_pivot<1>(x, ldx, N, c, pv);
  const double m = (double)pv[0] + m_shift;
  const double istd = 1.0 / sqrt(var + (double)eps);
  mean[c] = (float)m;
  invstd[c] = (float)istd;
  var_unbiased[c] = (float)(N > 1 ? var * (double)N / (double)(N - 1) : var);
  const double gm = gamma ? (double)gamma[c] : 1.0;
  const double bt = beta ? (double)beta[c] : 0.0;
  scale[c] = bn_scale(gamma ? gamma[c] : 1.f, (float)istd);
  shift[c] = (float)bt;                                   // the apply pass computes (x - mean) * scale + beta
}

// the left slab of the CONCAT skip block's backward: dskip = dy * act'(skip) over [N, ds] (dskip NULL: not asked for),
// and for PRELU the workgroup's sum of dy * min(skip, 0) in partial3[block].  A workgroup owns bn_colsum's run of rows.
template <int W, int ACT>
__global__ __launch_bounds__(kBlock) void bn_act_bwd_left_kernel(const float* __restrict__ dy, int64_t lddy,
                                                                 const float* __restrict__ skip, int64_t ldskip,
                                                                 float prm, const float* __restrict__ slope, int64_t N,
                                                                 int32_t ds, int64_t rows_per_block,
                                                                 float* __restrict__ dskip, int64_t lddskip,
                                                                 float* __restrict__ partial3) {
  const float ap = act_param<ACT>(prm, slope);
  const int groups = (ds + W - 1) / W;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < N ? r0 + rows_per_block : N;
  const int64_t total = r1 > r0 ? (r1 - r0) * groups : 0;
  float c3 = 0.f;
  for (int64_t i = threadIdx.x; i < total; i += kBlock) {
    const int64_t r = r0 + i / groups;
    const int c0 = (int)(i % groups) * W;
    float gv[W], sv[W];
    load_vec<W>(dy + r * lddy + c0, gv);
    load_vec<W>(skip + r * ldskip + c0, sv);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      if (ACT == MP_ACT_PRELU) c3 = fmaf(gv[k], act_dslope(sv[k]), c3);
      gv[k] = act_bwd<ACT>(gv[k], sv[k], ap);
    }
    if (dskip != nullptr) store_vec<W>(dskip + r * lddskip + c0, gv);
  }
  if (ACT == MP_ACT_PRELU) bn_block_sum(c3, partial3 + blockIdx.x);
}

// PRELU: the n per-workgroup sums of the statistics pass(es) -> ONE fp32 d slope, in double and in a fixed order
__global__ __launch_bounds__(kBlock) void bn_dslope_finalize_kernel(const float* __restrict__ partial3, int n,
                                                                    float* __restrict__ dslope) {
  __shared__ double v[kBlock];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += kBlock) s += (double)partial3[i];
  v[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int q = 0; q < kBlock; ++q) t += v[q];
    dslope[0] = (float)t;
  }
}

// ---- the launches bn_drop.hip shares (declared in bn_kernels.h) ---------------------------------------------------------
int bn_dslope_finalize(const BnWs& L, int n, float* dslope, hipStream_t st) {
  hipLaunchKernelGGL(bn_dslope_finalize_kernel, dim3(1), dim3(kBlock), 0, st, L.partial3, n, dslope);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int bn_act_bwd_left(int act, const float* dy, int64_t lddy, const float* skip, int64_t ldskip, float prm,
                    const float* slope, int64_t N, int32_t d_skip, float* dskip, int64_t lddskip, const BnWs& L,
                    hipStream_t st) {
  if (act == MP_ACT_NONE) return MP_ERR_INVALID_ARG;
  const int nblk = bn_blocks(N);
  const int64_t rpb = ceil_div(N, nblk);
  const bool vl = bn_vec4(d_skip, {lddy, ldskip, dskip ? lddskip : 0}, {dy, skip, dskip});
  const bool known = with_act(act, [&](auto a) {
    constexpr int A = decltype(a)::value;
    if constexpr (A != MP_ACT_NONE) {
      if (vl)
        hipLaunchKernelGGL((bn_act_bwd_left_kernel<4, A>), dim3(nblk), dim3(kBlock), 0, st, dy, lddy, skip, ldskip, prm,
                           slope, N, d_skip, rpb, dskip, lddskip, L.partial3 + nblk);
      else
        hipLaunchKernelGGL((bn_act_bwd_left_kernel<1, A>), dim3(nblk), dim3(kBlock), 0, st, dy, lddy, skip, ldskip, prm,
                           slope, N, d_skip, rpb, dskip, lddskip, L.partial3 + nblk);
    }
  });
  if (!known) return MP_ERR_INVALID_ARG;
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int bn_fwd_stats(const float* x, int64_t ldx, int64_t N, int32_t d, const float* gamma, const float* beta, float eps,
                 float* mean, float* invstd, float* var_unbiased, const BnWs& L, bool vec, hipStream_t st) {
  const int nblk = bn_blocks(N);
  const int64_t rpb = ceil_div(N, nblk);
  if (vec)       // the sums are shifted by bn_pivot(x), which both kernels take from x themselves
    hipLaunchKernelGGL((bn_fwd_stats_kernel<4>), dim3(nblk), dim3(kBlock), 0, st, x, ldx, N, d, rpb, L.partial);
  else
    hipLaunchKernelGGL((bn_fwd_stats_kernel<1>), dim3(nblk), dim3(kBlock), 0, st, x, ldx, N, d, rpb, L.partial);
  MP_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_fwd_finalize_kernel, dim3((unsigned)ceil_div(d, 16)), dim3(kBlock), 0, st, L.partial, nblk,
                     x, ldx, N, d, gamma, beta, eps, mean, invstd, var_unbiased, L.v[0], L.v[1]);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // namespace mp

using namespace mp;

// The entries without mask: adapters onto bn_fwd_run<false> / bn_bwd_run<false> (bn_kernels.h).  The entries that predate
// the activations carry `relu` (forward) or the forward's output y / out (backward: NULL = no activation).
extern "C" {

int mp_bn_ws_bytes(int64_t N, int32_t d, size_t* bytes_host) { return bn_ws_bytes(N, d, bytes_host, kBnWs); }
int mp_bn_act_ws_bytes(int64_t N, int32_t d, size_t* bytes_host) { return bn_ws_bytes(N, d, bytes_host, kBnWsAct); }

int mp_bn_train_fwd_f32(const float* x, int64_t ldx, int64_t N, int32_t d, const float* gamma, const float* beta,
                        float eps, int relu, float* y, int64_t ldy, float* mean, float* invstd,
                        float* var_unbiased, void* ws, size_t ws_bytes, mp_stream_t stream) {
  return bn_fwd_run<false>({kBnWs, x, ldx, N, d, gamma, beta, mean, invstd, relu ? MP_ACT_RELU : MP_ACT_NONE, 0.f, nullptr,
                            false, nullptr, 0, 0, 0, 0, 0, 0, ws, ws_bytes, stream},
                           eps, y, ldy, mean, invstd, var_unbiased);
}

int mp_bn_train_fwd_skip_f32(const float* x, int64_t ldx, const float* skip, int64_t ldskip, int64_t N, int32_t d,
                             int32_t d_skip, int mode, const float* gamma, const float* beta, float eps, int relu,
                             float* out, int64_t ldo, float* mean, float* invstd, float* var_unbiased, void* ws,
                             size_t ws_bytes, mp_stream_t stream) {
  return bn_fwd_run<false>({kBnWs, x, ldx, N, d, gamma, beta, mean, invstd, relu ? MP_ACT_RELU : MP_ACT_NONE, 0.f, nullptr,
                            true, skip, ldskip, d_skip, mode, 0, 0, 0, ws, ws_bytes, stream},
                           eps, out, ldo, mean, invstd, var_unbiased);
}

int mp_bn_train_fwd_act_f32(const float* x, int64_t ldx, int64_t N, int32_t d, const float* gamma, const float* beta,
                            float eps, int act, float act_param, const float* slope, float* y, int64_t ldy,
                            float* mean, float* invstd, float* var_unbiased, void* ws, size_t ws_bytes,
                            mp_stream_t stream) {
  return bn_fwd_run<false>({kBnWsAct, x, ldx, N, d, gamma, beta, mean, invstd, act, act_param, slope, false, nullptr, 0, 0,
                            0, 0, 0, 0, ws, ws_bytes, stream},
                           eps, y, ldy, mean, invstd, var_unbiased);
}

int mp_bn_train_fwd_skip_act_f32(const float* x, int64_t ldx, const float* skip, int64_t ldskip, int64_t N, int32_t d,
                                 int32_t d_skip, int mode, const float* gamma, const float* beta, float eps, int act,
                                 float act_param, const float* slope, float* out, int64_t ldo, float* mean,
                                 float* invstd, float* var_unbiased, void* ws, size_t ws_bytes, mp_stream_t stream) {
  return bn_fwd_run<false>({kBnWsAct, x, ldx, N, d, gamma, beta, mean, invstd, act, act_param, slope, true, skip, ldskip,
                            d_skip, mode, 0, 0, 0, ws, ws_bytes, stream},
                           eps, out, ldo, mean, invstd, var_unbiased);
}

int mp_bn_train_bwd_f32(const float* dy, int64_t lddy, const float* y, int64_t ldy, const float* x, int64_t ldx,
                        int64_t N, int32_t d, const float* gamma, const float* mean, const float* invstd,
                        float* dx, int64_t lddx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                        mp_stream_t stream) {
  return bn_bwd_run<false>({kBnWs, x, ldx, N, d, gamma, nullptr, mean, invstd, y ? MP_ACT_RELU : MP_ACT_NONE, 0.f, nullptr,
                            false, nullptr, 0, 0, 0, 0, 0, 0, ws, ws_bytes, stream},
                           dy, lddy, y, ldy, dx, lddx, nullptr, 0, dgamma, dbeta, nullptr);
}

int mp_bn_train_bwd_relu_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t N, int32_t d,
                             const float* gamma, const float* beta, const float* mean, const float* invstd,
                             float* dx, int64_t lddx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                             mp_stream_t stream) {
  return bn_bwd_run<false>({kBnWs, x, ldx, N, d, gamma, beta, mean, invstd, MP_ACT_RELU, 0.f, nullptr, false, nullptr, 0, 0,
                            0, 0, 0, 0, ws, ws_bytes, stream},
                           dy, lddy, nullptr, 0, dx, lddx, nullptr, 0, dgamma, dbeta, nullptr);
}

int mp_bn_train_bwd_skip_f32(const float* dy, int64_t lddy, const float* out, int64_t ldo, const float* x, int64_t ldx,
                             int64_t N, int32_t d, const float* gamma, const float* mean, const float* invstd,
                             float* dx, int64_t lddx, float* dskip, int64_t lddskip, float* dgamma, float* dbeta,
                             void* ws, size_t ws_bytes, mp_stream_t stream) {
  if (out && !dskip) return MP_ERR_INVALID_ARG;
  // out NULL = no activation: d(skip) is dy itself and nothing is written for it
  return bn_bwd_run<false>({kBnWs, x, ldx, N, d, gamma, nullptr, mean, invstd, out ? MP_ACT_RELU : MP_ACT_NONE, 0.f,
                            nullptr, false, nullptr, 0, 0, 0, 0, 0, 0, ws, ws_bytes, stream},
                           dy, lddy, out, ldo, dx, lddx, out ? dskip : nullptr, out ? lddskip : 0, dgamma, dbeta, nullptr);
}

int mp_bn_train_bwd_act_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t N, int32_t d,
                            const float* gamma, const float* beta, const float* mean, const float* invstd, int act,
                            float act_param, const float* slope, float* dx, int64_t lddx, float* dgamma, float* dbeta,
                            float* dslope, void* ws, size_t ws_bytes, mp_stream_t stream) {
  return bn_bwd_run<false>({kBnWsAct, x, ldx, N, d, gamma, beta, mean, invstd, act, act_param, slope, false, nullptr, 0, 0,
                            0, 0, 0, 0, ws, ws_bytes, stream},
                           dy, lddy, nullptr, 0, dx, lddx, nullptr, 0, dgamma, dbeta, dslope);
}

int mp_bn_train_bwd_skip_act_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* skip,
                                 int64_t ldskip, int64_t N, int32_t d, int32_t d_skip, int mode, const float* gamma,
                                 const float* beta, const float* mean, const float* invstd, int act, float act_param,
                                 const float* slope, float* dx, int64_t lddx, float* dskip, int64_t lddskip,
                                 float* dgamma, float* dbeta, float* dslope, void* ws, size_t ws_bytes,
                                 mp_stream_t stream) {
  return bn_bwd_run<false>({kBnWsAct, x, ldx, N, d, gamma, beta, mean, invstd, act, act_param, slope, true, skip, ldskip,
                            d_skip, mode, 0, 0, 0, ws, ws_bytes, stream},
                           dy, lddy, nullptr, 0, dx, lddx, dskip, lddskip, dgamma, dbeta, dslope);
}

}  // extern "C"
