// Pair decoders of the link-prediction head (include/mp_pair.h): the score of K listed pairs of rows of h (dot product or
// cosine similarity), the sum form of the concat decoding, the reciprocal row norms, and the entry weights of the score's
// input gradient over the inverted index of the pair list.  gfx950, wave64.
//
// Lane grouping of the score / sum / rnorm kernels: a row is read by G = 2^lg lanes of W floats each (W = 4: 16-byte
// loads; W = 1: the scalar form for rows that are not 16-byte addressable), so a wave serves P = 64 / G rows or pairs per
// step, and kPairU steps' loads are issued before the first is consumed.  Rows wider than G * W columns are walked in
// column tiles.  A wave owns chunks of 64 pairs: it reads the 64 index pairs with two coalesced int64 loads, checks them
// against [0, N) once, hands them to the groups with shuffles, and stores the 64 scores with one coalesced store.
// sddmm_stream_kernel of attn.hip has the same outline but takes int32 entries it trusts, one pair per wave step and a
// head ladder; its body is not shared, so that kernel stays as it is.
#include <math.h>

#include "common.h"
#include "vecio.h"
#include "../../include/mp_pair.h"

namespace mp {

constexpr int kPairU = 4;            // steps in flight per lane
constexpr int kPairAbsent = -1;      // slot beyond the chunk's pairs: nothing is loaded or stored
constexpr int kPairBad = -2;         // index outside [0, N): nothing is loaded, the result is NaN

// the 64 pairs of a chunk, one per lane: (ia, ib) as int32 (N < 2^31) or the two codes above in ia; counts the bad ones
__device__ __forceinline__ void pair_chunk_indices(const int64_t* __restrict__ a, const int64_t* __restrict__ b, int64_t k0,
                                                   int n, int64_t N, int lane, int32_t* bad, int& ia, int& ib) {
  ia = kPairAbsent;
  ib = 0;
  if (lane < n) {
    const int64_t av = a[k0 + lane], bv = b[k0 + lane];
    if (av < 0 || av >= N || bv < 0 || bv >= N) {
      ia = kPairBad;
      atomicAdd(bad, 1);
    } else {
      ia = (int)av;
      ib = (int)bv;
    }
  }
}

template <int W>
__global__ __launch_bounds__(kBlock) void pair_score_kernel(const float* __restrict__ h, int64_t ldh, int64_t N, int d,
                                                            int lg, const int64_t* __restrict__ a,
                                                            const int64_t* __restrict__ b, int64_t K,
                                                            const float* __restrict__ r, float* __restrict__ score,
                                                            int32_t* bad) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int G = 1 << lg, P = 64 >> lg;
  const int gi = lane >> lg, li = lane & (G - 1);
  const int span = G * W;
  const int64_t chunks = (K + 63) >> 6;
  for (int64_t ch = (int64_t)blockIdx.x * kWavesPerBlock + wave; ch < chunks; ch += (int64_t)gridDim.x * kWavesPerBlock) {
    const int64_t k0 = ch << 6;
    const int n = (int)(K - k0 < 64 ? K - k0 : 64);
    int ia, ib;
    pair_chunk_indices(a, b, k0, n, N, lane, bad, ia, ib);
    float rr = 1.f;
    if (r != nullptr && ia >= 0) rr = r[ia] * r[ib];
    float res = 0.f;
    const int steps = (n + P - 1) >> (6 - lg);
    for (int s0 = 0; s0 < steps; s0 += kPairU) {
      float acc[kPairU];
      int ja[kPairU], jb[kPairU];
#pragma unroll
      for (int j = 0; j < kPairU; ++j) {
        const int slot = ((s0 + j) * P + gi) & 63;
        const int ta = __shfl(ia, slot, kWave);
        jb[j] = __shfl(ib, slot, kWave);
        ja[j] = s0 + j < steps ? ta : kPairAbsent;
        acc[j] = 0.f;
      }
      for (int t0 = 0; t0 < d; t0 += span) {
        const int c = t0 + li * W;
        float x[kPairU][W], y[kPairU][W];
#pragma unroll
        for (int j = 0; j < kPairU; ++j) {
#pragma unroll
          for (int k = 0; k < W; ++k) x[j][k] = y[j][k] = 0.f;
          if (c < d && ja[j] >= 0) {
            load_vec<W>(h + (int64_t)ja[j] * ldh + c, x[j]);
            load_vec<W>(h + (int64_t)jb[j] * ldh + c, y[j]);
          }
        }
#pragma unroll
        for (int j = 0; j < kPairU; ++j)
#pragma unroll
          for (int k = 0; k < W; ++k) acc[j] = fmaf(x[j][k], y[j][k], acc[j]);
      }
#pragma unroll
      for (int j = 0; j < kPairU; ++j) {
        float t = acc[j];
        for (int off = G >> 1; off > 0; off >>= 1) t += __shfl_xor(t, off, kWave);
        // pair `lane` of the chunk was served in step lane / P by group lane % P
        const float got = __shfl(t, (lane & (P - 1)) << lg, kWave);
        if ((lane >> (6 - lg)) == s0 + j) res = got;
      }
    }
    if (lane < n) score[k0 + lane] = ia == kPairBad ? __builtin_nanf("") : res * rr;
  }
}

template <int W>
__global__ __launch_bounds__(kBlock) void pair_sum_kernel(const float* __restrict__ Um, int64_t ldu,
                                                          const float* __restrict__ Vm, int64_t ldv, int64_t N, int m,
                                                          int lg, const int64_t* __restrict__ a,
                                                          const int64_t* __restrict__ b, int64_t K,
                                                          const float* __restrict__ bias, float* __restrict__ z,
                                                          int64_t ldz, int32_t* bad) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int G = 1 << lg, P = 64 >> lg;
  const int gi = lane >> lg, li = lane & (G - 1);
  const int span = G * W;
  const int64_t chunks = (K + 63) >> 6;
  for (int64_t ch = (int64_t)blockIdx.x * kWavesPerBlock + wave; ch < chunks; ch += (int64_t)gridDim.x * kWavesPerBlock) {
    const int64_t k0 = ch << 6;
    const int n = (int)(K - k0 < 64 ? K - k0 : 64);
    int ia, ib;
    pair_chunk_indices(a, b, k0, n, N, lane, bad, ia, ib);
    const int steps = (n + P - 1) >> (6 - lg);
    for (int s0 = 0; s0 < steps; s0 += kPairU) {
      int ja[kPairU], jb[kPairU], slot[kPairU];
#pragma unroll
      for (int j = 0; j < kPairU; ++j) {
        slot[j] = (s0 + j) * P + gi;
        const int ta = __shfl(ia, slot[j] & 63, kWave);
        jb[j] = __shfl(ib, slot[j] & 63, kWave);
        ja[j] = s0 + j < steps ? ta : kPairAbsent;
      }
      for (int t0 = 0; t0 < m; t0 += span) {
        const int c = t0 + li * W;
        float x[kPairU][W], y[kPairU][W], bv[W];
#pragma unroll
        for (int k = 0; k < W; ++k) bv[k] = 0.f;
        if (bias != nullptr && c < m) load_vec<W>(bias + c, bv);
#pragma unroll
        for (int j = 0; j < kPairU; ++j) {
#pragma unroll
          for (int k = 0; k < W; ++k) x[j][k] = y[j][k] = 0.f;
          if (c < m && ja[j] >= 0) {
            load_vec<W>(Um + (int64_t)ja[j] * ldu + c, x[j]);
            load_vec<W>(Vm + (int64_t)jb[j] * ldv + c, y[j]);
          }
        }
#pragma unroll
        for (int j = 0; j < kPairU; ++j) {
          if (c < m && ja[j] != kPairAbsent) {
            float o[W];
#pragma unroll
            for (int k = 0; k < W; ++k) o[k] = ja[j] == kPairBad ? __builtin_nanf("") : (x[j][k] + y[j][k]) + bv[k];
            store_vec<W>(z + (k0 + slot[j]) * ldz + c, o);
          }
        }
      }
    }
  }
}

template <int W>
__global__ __launch_bounds__(kBlock) void pair_rnorm_kernel(const float* __restrict__ h, int64_t ldh, int64_t N, int d,
                                                            int lg, float eps, float* __restrict__ r,
                                                            float* __restrict__ q) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int G = 1 << lg, P = 64 >> lg;
  const int gi = lane >> lg, li = lane & (G - 1);
  const int span = G * W;
  const int64_t per = (int64_t)P * kPairU;     // rows per wave step
  for (int64_t v0 = ((int64_t)blockIdx.x * kWavesPerBlock + wave) * per; v0 < N;
       v0 += (int64_t)gridDim.x * kWavesPerBlock * per) {
    float acc[kPairU];
#pragma unroll
    for (int j = 0; j < kPairU; ++j) acc[j] = 0.f;
    for (int t0 = 0; t0 < d; t0 += span) {
      const int c = t0 + li * W;
      float x[kPairU][W];
#pragma unroll
      for (int j = 0; j < kPairU; ++j) {
        const int64_t v = v0 + j * P + gi;
#pragma unroll
        for (int k = 0; k < W; ++k) x[j][k] = 0.f;
        if (c < d && v < N) load_vec<W>(h + v * ldh + c, x[j]);
      }
#pragma unroll
      for (int j = 0; j < kPairU; ++j)
#pragma unroll
        for (int k = 0; k < W; ++k) acc[j] = fmaf(x[j][k], x[j][k], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < kPairU; ++j) {
      float t = acc[j];
      for (int off = G >> 1; off > 0; off >>= 1) t += __shfl_xor(t, off, kWave);
      const int64_t v = v0 + j * P + gi;
      if (li == 0 && v < N) {
        const float nrm = sqrtf(t);
        r[v] = 1.0f / fmaxf(nrm, eps);
        if (q != nullptr) q[v] = nrm >= 1.17549435e-38f ? 1.0f / nrm : 0.f;      // no reciprocal of a zero or denormal norm
      }
    }
  }
}

// 16 lanes per row of the inverted index, four rows per wave step
__global__ __launch_bounds__(kBlock) void pair_bwd_weights_kernel(const int32_t* __restrict__ rowptr,
                                                                  const int32_t* __restrict__ eid, int64_t N, int64_t K,
                                                                  const float* __restrict__ g,
                                                                  const float* __restrict__ score,
                                                                  const float* __restrict__ r,
                                                                  const float* __restrict__ q,
                                                                  const int64_t* __restrict__ a,
                                                                  const int64_t* __restrict__ b, float* __restrict__ w,
                                                                  float* __restrict__ diag) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int gi = lane >> 4, li = lane & 15;
  for (int64_t v0 = ((int64_t)blockIdx.x * kWavesPerBlock + wave) * 4; v0 < N;
       v0 += (int64_t)gridDim.x * kWavesPerBlock * 4) {
    const int64_t v = v0 + gi;
    int e0 = 0, e1 = 0;
    if (v < N) {
      e0 = rowptr[v];
      e1 = rowptr[v + 1];
    }
    float sum = 0.f;
    for (int e = e0 + li; e < e1; e += 16) {
      const int64_t id = eid[e];
      float we = 0.f, gs = 0.f;
      if (id >= 0 && id < 2 * K) {
        const int64_t k = id >= K ? id - K : id;
        const float gk = g[k];
        if (r != nullptr) {
          const int64_t av = a[k], bv = b[k];
          if (av >= 0 && av < N && bv >= 0 && bv < N) we = gk * (r[av] * r[bv]);
        } else {
          we = gk;
        }
        if (diag != nullptr) gs = gk * score[k];
      }
      w[e] = we;
      sum += gs;
    }
    if (diag != nullptr) {
      for (int off = 8; off > 0; off >>= 1) sum += __shfl_xor(sum, off, kWave);
      // (sum * q first: the scores of row v carry a factor ||h_v||, so the product stays finite where q is large)
      if (li == 0 && v < N) diag[v] = -r[v] * (sum * q[v]);
    }
  }
}

static bool al16(const void* p) { return ((uintptr_t)p % 16) == 0; }

// log2 of the lanes that read one row of `width` columns at W floats per lane: the power of two >= ceil(width / W), <= 64
static int group_log2(int width, int W) {
  const int need = (width + W - 1) / W;
  int lg = 0;
  while ((1 << lg) < need && lg < 6) ++lg;
  return lg;
}

static int chunk_grid(int64_t K) {
  int64_t blocks = ceil_div(ceil_div(K, 64), kWavesPerBlock);
  if (blocks > kNumCU * 8) blocks = kNumCU * 8;
  return (int)(blocks < 1 ? 1 : blocks);
}

}  // namespace mp

using namespace mp;

extern "C" {

int mp_pair_rnorm_f32(const float* h, int64_t ldh, int64_t N, int32_t d, float eps, float* r, float* q_or_null,
                      mp_stream_t stream) {
  if (N < 0 || d <= 0 || ldh < d || !(eps > 0.f)) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || d >= (1 << 30)) return MP_ERR_UNSUPPORTED;
  if (N == 0) return MP_OK;
  if (!h || !r) return MP_ERR_INVALID_ARG;
  const bool vec = d % 4 == 0 && ldh % 4 == 0 && al16(h);
  const int lg = group_log2(d, vec ? 4 : 1);
  const int64_t per = (int64_t)(64 >> lg) * kPairU * kWavesPerBlock;
  int64_t blocks = ceil_div(N, per);
  if (blocks > kNumCU * 8) blocks = kNumCU * 8;
  if (vec)
    hipLaunchKernelGGL(pair_rnorm_kernel<4>, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), h, ldh, N, d, lg,
                       eps, r, q_or_null);
  else
    hipLaunchKernelGGL(pair_rnorm_kernel<1>, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), h, ldh, N, d, lg,
                       eps, r, q_or_null);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_pair_score_f32(const float* h, int64_t ldh, int64_t N, int32_t d, const int64_t* a, const int64_t* b, int64_t K,
                      const float* r_or_null, float* score, int32_t* bad, mp_stream_t stream) {
  if (N < 0 || K < 0 || d <= 0 || ldh < d) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || K >= (1 << 30) || d >= (1 << 30)) return MP_ERR_UNSUPPORTED;
  if (K == 0) return MP_OK;
  if (!a || !b || !score || !bad || (N > 0 && !h)) return MP_ERR_INVALID_ARG;
  const bool vec = d % 4 == 0 && ldh % 4 == 0 && al16(h);
  const int lg = group_log2(d, vec ? 4 : 1);
  if (vec)
    hipLaunchKernelGGL(pair_score_kernel<4>, dim3(chunk_grid(K)), dim3(kBlock), 0, as_stream(stream), h, ldh, N, d, lg, a,
                       b, K, r_or_null, score, bad);
  else
    hipLaunchKernelGGL(pair_score_kernel<1>, dim3(chunk_grid(K)), dim3(kBlock), 0, as_stream(stream), h, ldh, N, d, lg, a,
                       b, K, r_or_null, score, bad);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_pair_sum_f32(const float* U, int64_t ldu, const float* V, int64_t ldv, int64_t N, int32_t m, const int64_t* a,
                    const int64_t* b, int64_t K, const float* bias_or_null, float* z, int64_t ldz, int32_t* bad,
                    mp_stream_t stream) {
  if (N < 0 || K < 0 || m <= 0 || ldu < m || ldv < m || ldz < m) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || K >= (1 << 30) || m >= (1 << 30)) return MP_ERR_UNSUPPORTED;
  if (K == 0) return MP_OK;
  if (!a || !b || !z || !bad || (N > 0 && (!U || !V))) return MP_ERR_INVALID_ARG;
  const bool vec = m % 4 == 0 && ldu % 4 == 0 && ldv % 4 == 0 && ldz % 4 == 0 && al16(U) && al16(V) && al16(z) &&
                   al16(bias_or_null);
  const int lg = group_log2(m, vec ? 4 : 1);
  if (vec)
    hipLaunchKernelGGL(pair_sum_kernel<4>, dim3(chunk_grid(K)), dim3(kBlock), 0, as_stream(stream), U, ldu, V, ldv, N, m,
                       lg, a, b, K, bias_or_null, z, ldz, bad);
  else
    hipLaunchKernelGGL(pair_sum_kernel<1>, dim3(chunk_grid(K)), dim3(kBlock), 0, as_stream(stream), U, ldu, V, ldv, N, m,
                       lg, a, b, K, bias_or_null, z, ldz, bad);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_pair_bwd_weights_f32(const int32_t* rowptr, const int32_t* eid, int64_t N, int64_t K, const float* g,
                            const float* score_or_null, const float* r_or_null, const float* q_or_null,
                            const int64_t* a, const int64_t* b, float* w, float* diag_or_null, mp_stream_t stream) {
  if (N < 0 || K < 0) return MP_ERR_INVALID_ARG;
  if (diag_or_null && (!score_or_null || !r_or_null || !q_or_null)) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || K >= (1 << 30)) return MP_ERR_UNSUPPORTED;
  if (K == 0 || N == 0) return MP_OK;
  if (!rowptr || !eid || !g || !w || (r_or_null && (!a || !b))) return MP_ERR_INVALID_ARG;
  int64_t blocks = ceil_div(N, 4 * kWavesPerBlock);
  if (blocks > kNumCU * 8) blocks = kNumCU * 8;
  hipLaunchKernelGGL(pair_bwd_weights_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), rowptr, eid, N, K,
                     g, score_or_null, r_or_null, q_or_null, a, b, w, diag_or_null);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // extern "C"
