// gnn.dropout between the BatchNorm and the activation (graphgym/models/layer.py:26-35: BatchNorm1d -> Dropout -> act;
// in a skip block on the last layer, before the skip operand: gnn.py:49-60), riding the BatchNorm passes with a KEYED
// mask: keep(seed, offset, r, c) of draws.h is a pure function of the call's key and the element's logical index, so
// nothing is stored — the backward recomputes the mask exactly as it recomputes the activation from x.
//   forward   stats  : bn.hip's, unchanged (dropout sits behind the normalisation)
//             apply  : out = act(m * scale * BN(x))            | act(skip + m * scale * BN(x))
//                                                              | [act(skip) | act(m * scale * BN(x))]
//   backward  (ELU, SELU, SILU only) the residue of the fp32 mean: one read of x, see below
//             stats  : z recomputed (masked), g = dy * act'(z); d skip = g (SUM, not masked); the column sums and dx take
//                      m * scale * g; PRELU's slope sum takes dy * min(z, 0) on the masked z
//             apply  : dx = A (m * scale * g) + B (x - mean) + C
//   mp_dropout_keyed_f32: out = m * scale * x, the mask alone (its backward is the same launch on dy)
// One hash per aligned group of four columns: a 4-wide thread draws once per load, a scalar thread once per element.
// The passes are the DROP = true instantiations of bn_kernels.h, which says what the mask adds to the arithmetic; here
// are the entries, the residue of the mean and the mask alone.
#include "bn_kernels.h"

namespace mp {

// The residue of the fp32 mean, pass one: per column the sum of x - mean over the workgroup's rows, in the two-slab form
// of bn_colsum_store2 (the second quantity of a slab is not used)
template <int W>
__global__ __launch_bounds__(kBlock) void bn_drop_mean_lo_kernel(const float* __restrict__ x, int64_t ldx,
                                                                 const float* __restrict__ mean, int64_t N, int32_t d,
                                                                 int64_t rows_per_block, float* __restrict__ partial) {
  const BnGeom g = bn_geom<W>(d);
  const int cgi = threadIdx.x % g.cg;
  const int rli = threadIdx.x / g.cg;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < N ? r0 + rows_per_block : N;
  for (int t = 0; t < g.tiles; ++t) {
    const int c0 = (t * g.cg + cgi) * W;
    const bool on = c0 < d;
    float a[W], al[W], zero[W], pv[W];
#pragma unroll
    for (int k = 0; k < W; ++k) { a[k] = 0.f; al[k] = 0.f; zero[k] = 0.f; pv[k] = 0.f; }
    if (on) {
      load_vec<W>(mean + c0, pv);
      for (int64_t r = r0 + rli; r < r1; r += g.rl) {
        float xv[W];
        load_vec<W>(x + r * ldx + c0, xv);
#pragma unroll
        for (int k = 0; k < W; ++k) two_sum(a[k], al[k], xv[k] - pv[k]);
      }
    }
    bn_colsum_store2<W>(a, al, zero, zero, g, cgi, rli, on, c0, d, (int)gridDim.x, partial);
  }
}

// pass two: mean_lo[c] = (the slabs' sum) / N
__global__ __launch_bounds__(kBlock) void bn_drop_mean_lo_finalize_kernel(const float* __restrict__ partial, int nslab,
                                                                          int64_t N, int32_t d,
                                                                          float* __restrict__ mean_lo) {
  int c;
  double s1, s2;
  if (!bn_col_sums(partial, nslab, d, c, s1, s2)) return;
  mean_lo[c] = (float)(s1 / (double)N);
}

int bn_mean_lo(const float* x, int64_t ldx, const float* mean, int64_t N, int32_t d, const BnWs& L, bool vec,
               hipStream_t st) {
  const int nblk = bn_blocks(N);
  const int64_t rpb = ceil_div(N, nblk);
  if (vec)
    hipLaunchKernelGGL((bn_drop_mean_lo_kernel<4>), dim3(nblk), dim3(kBlock), 0, st, x, ldx, mean, N, d, rpb, L.partial);
  else
    hipLaunchKernelGGL((bn_drop_mean_lo_kernel<1>), dim3(nblk), dim3(kBlock), 0, st, x, ldx, mean, N, d, rpb, L.partial);
  MP_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_drop_mean_lo_finalize_kernel, dim3((unsigned)ceil_div(d, 16)), dim3(kBlock), 0, st, L.partial,
                     2 * nblk, N, d, L.v[4]);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

// out = m * scale * x over an [N, d] view
template <int W>
__global__ __launch_bounds__(kBlock) void dropout_keyed_kernel(const float* __restrict__ x, int64_t ldx, DropKey dk,
                                                               int64_t N, int32_t d, float* __restrict__ out,
                                                               int64_t ldo) {
  const int groups = (d + W - 1) / W;
  const int64_t total = N * groups;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / groups;
    const int c0 = (int)(i - r * groups) * W;
    float v[W];
    bool m[W];
    load_vec<W>(x + r * ldx + c0, v);
    drop_keep<W>(dk, r, c0, m);
    drop_apply<W>(v, m, dk.scale);
    store_vec<W>(out + r * ldo + c0, v);
  }
}

}  // namespace mp

using namespace mp;

// The entries with the mask: adapters onto bn_fwd_run<true> / bn_bwd_run<true> (bn_kernels.h)
extern "C" {

int mp_bn_drop_ws_bytes(int64_t N, int32_t d, size_t* bytes_host) { return bn_ws_bytes(N, d, bytes_host, kBnWsDrop); }

int mp_dropout_keyed_f32(const float* x, int64_t ldx, int64_t N, int32_t d, int32_t T, uint64_t seed, uint64_t offset,
                         float* out, int64_t ldo, mp_stream_t stream) {
  DropKey dk;
  if (N <= 0 || d <= 0 || !x || !out || ldx < d || ldo < d || !drop_make(T, seed, offset, d, &dk))
    return MP_ERR_INVALID_ARG;
  hipStream_t st = as_stream(stream);
  if (bn_vec4(d, {ldx, ldo}, {x, out}))
    hipLaunchKernelGGL((dropout_keyed_kernel<4>), dim3(flat_grid(N * (d / 4))), dim3(kBlock), 0, st, x, ldx, dk, N, d,
                       out, ldo);
  else
    hipLaunchKernelGGL((dropout_keyed_kernel<1>), dim3(flat_grid(N * d)), dim3(kBlock), 0, st, x, ldx, dk, N, d, out,
                       ldo);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_bn_train_fwd_drop_act_f32(const float* x, int64_t ldx, int64_t N, int32_t d, const float* gamma,
                                 const float* beta, float eps, int act, float act_param, const float* slope, int32_t T,
                                 uint64_t seed, uint64_t offset, float* y, int64_t ldy, float* mean, float* invstd,
                                 float* var_unbiased, void* ws, size_t ws_bytes, mp_stream_t stream) {
  return bn_fwd_run<true>({kBnWsDrop, x, ldx, N, d, gamma, beta, mean, invstd, act, act_param, slope, false, nullptr, 0, 0,
                           0, T, seed, offset, ws, ws_bytes, stream},
                          eps, y, ldy, mean, invstd, var_unbiased);
}

int mp_bn_train_bwd_drop_act_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t N, int32_t d,
                                 const float* gamma, const float* beta, const float* mean, const float* invstd,
                                 int act, float act_param, const float* slope, int32_t T, uint64_t seed,
                                 uint64_t offset, float* dx, int64_t lddx, float* dgamma, float* dbeta, float* dslope,
                                 void* ws, size_t ws_bytes, mp_stream_t stream) {
  return bn_bwd_run<true>({kBnWsDrop, x, ldx, N, d, gamma, beta, mean, invstd, act, act_param, slope, false, nullptr, 0, 0,
                           0, T, seed, offset, ws, ws_bytes, stream},
                          dy, lddy, nullptr, 0, dx, lddx, nullptr, 0, dgamma, dbeta, dslope);
}

int mp_bn_train_fwd_drop_skip_act_f32(const float* x, int64_t ldx, const float* skip, int64_t ldskip, int64_t N,
                                      int32_t d, int32_t d_skip, int mode, const float* gamma, const float* beta,
                                      float eps, int act, float act_param, const float* slope, int32_t T,
                                      uint64_t seed, uint64_t offset, float* out, int64_t ldo, float* mean,
                                      float* invstd, float* var_unbiased, void* ws, size_t ws_bytes,
                                      mp_stream_t stream) {
  return bn_fwd_run<true>({kBnWsDrop, x, ldx, N, d, gamma, beta, mean, invstd, act, act_param, slope, true, skip, ldskip,
                           d_skip, mode, T, seed, offset, ws, ws_bytes, stream},
                          eps, out, ldo, mean, invstd, var_unbiased);
}

int mp_bn_train_bwd_drop_skip_act_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* skip,
                                      int64_t ldskip, int64_t N, int32_t d, int32_t d_skip, int mode,
                                      const float* gamma, const float* beta, const float* mean, const float* invstd,
                                      int act, float act_param, const float* slope, int32_t T, uint64_t seed,
                                      uint64_t offset, float* dx, int64_t lddx, float* dskip, int64_t lddskip,
                                      float* dgamma, float* dbeta, float* dslope, void* ws, size_t ws_bytes,
                                      mp_stream_t stream) {
  return bn_bwd_run<true>({kBnWsDrop, x, ldx, N, d, gamma, beta, mean, invstd, act, act_param, slope, true, skip, ldskip,
                           d_skip, mode, T, seed, offset, ws, ws_bytes, stream},
                          dy, lddy, nullptr, 0, dx, lddx, dskip, lddskip, dgamma, dbeta, dslope);
}

}  // extern "C"
