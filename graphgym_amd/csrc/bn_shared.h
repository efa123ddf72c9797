// What bn.hip (the BatchNorm passes) and bn_drop.hip (the same passes with a keyed dropout mask) both use: the geometry
// of a statistics workgroup, the tail of a statistics kernel, the workspace layouts, and the launches that stay in
// bn.hip — the forward statistics, the two finalize kernels and the CONCAT left slab — as host functions.
#pragma once
#include "common.h"
#include "vecio.h"
#include "act.h"

namespace mp {

constexpr int kBnMaxBlocks = kNumCU * 8;

struct BnGeom {
  int cg;        // column groups (threads along the feature axis), each owns W consecutive columns
  int rl;        // rows processed in parallel by one workgroup
  int tiles;     // column tiles when d > cg * W
};

template <int W>
__host__ __device__ inline BnGeom bn_geom(int d) {
  BnGeom g;
  const int groups = (d + W - 1) / W;
  g.cg = groups < kBlock ? groups : kBlock;
  int p = 1;
  while (p < g.cg) p <<= 1;             // power of two so that rl = 256 / cg is exact
  g.cg = p > kBlock ? kBlock : p;
  g.rl = kBlock / g.cg;
  g.tiles = (groups + g.cg - 1) / g.cg;
  return g;
}

// the affine scale of the apply pass, from the ROUNDED invstd the forward hands out: the forward and a backward that
// recomputes the activation from x get the same bits
__host__ __device__ __forceinline__ float bn_scale(float gamma, float invstd) {
  return (float)((double)gamma * (double)invstd);
}

// The tail of a statistics kernel's column tile: the workgroup's rl row lanes of the two running sums a / b -> one
// partial per column, added in row-lane order, in slab blockIdx.x of `partial` ([blocks][2][d]).  Every thread of the
// workgroup calls it (two barriers); `on`: this thread's columns c0 .. c0 + W exist.
template <int W>
__device__ __forceinline__ void bn_colsum_store(const float (&a)[W], const float (&b)[W], const BnGeom& g, int cgi,
                                                int rli, bool on, int c0, int32_t d, float* __restrict__ partial) {
  __shared__ float red[2][kBlock][W];
#pragma unroll
  for (int k = 0; k < W; ++k) { red[0][threadIdx.x][k] = a[k]; red[1][threadIdx.x][k] = b[k]; }
  __syncthreads();
  if (rli == 0 && on) {
#pragma unroll
    for (int k = 0; k < W; ++k) {
      float sa = 0.f, sb = 0.f;
      for (int q = 0; q < g.rl; ++q) { sa += red[0][q * g.cg + cgi][k]; sb += red[1][q * g.cg + cgi][k]; }
      if (c0 + k < d) {
        partial[((int64_t)blockIdx.x * 2 + 0) * d + c0 + k] = sa;
        partial[((int64_t)blockIdx.x * 2 + 1) * d + c0 + k] = sb;
      }
    }
  }
  __syncthreads();
}

// The two column sums of a finalize kernel over the nblk per-block partials, in double and in a fixed order: a
// workgroup owns 16 columns, its 16 block lanes each add every 16th partial through two independent running sums per
// quantity, and lane 0 adds the 16 lane sums in lane order.  (One thread per column walking all partials in a dependent
// chain of double adds took 0.8 ms per call at 2 048 partials.)  Returns true in the threads that hold a result.
__device__ __forceinline__ bool bn_col_sums(const float* __restrict__ partial, int nblk, int32_t d, int& c, double& s1,
                                            double& s2) {
  __shared__ double part[2][16][16];
  const int e = threadIdx.x & 15, sl = threadIdx.x >> 4;
  c = blockIdx.x * 16 + e;
  double a1 = 0.0, b1 = 0.0, a2 = 0.0, b2 = 0.0;
  if (c < d) {
    int b = sl;
    for (; b + 16 < nblk; b += 32) {
      a1 += (double)partial[((int64_t)b * 2 + 0) * d + c];
      a2 += (double)partial[((int64_t)b * 2 + 1) * d + c];
      b1 += (double)partial[((int64_t)(b + 16) * 2 + 0) * d + c];
      b2 += (double)partial[((int64_t)(b + 16) * 2 + 1) * d + c];
    }
    if (b < nblk) {
      a1 += (double)partial[((int64_t)b * 2 + 0) * d + c];
      a2 += (double)partial[((int64_t)b * 2 + 1) * d + c];
    }
  }
  part[0][sl][e] = a1 + b1;
  part[1][sl][e] = a2 + b2;
  __syncthreads();
  s1 = 0.0; s2 = 0.0;
  if (sl == 0 && c < d) {
#pragma unroll
    for (int r = 0; r < 16; ++r) { s1 += part[0][r][e]; s2 += part[1][r][e]; }
    return true;
  }
  return false;
}

// ACT is a template parameter; `prm` is the kind's host parameter (LRELU's slope, ELU's alpha) and `slope` the device
// pointer to PRELU's one learnable slope, read here and never on the host.
template <int ACT>
__device__ __forceinline__ float act_param(float prm, const float* __restrict__ slope) {
  if constexpr (ACT == MP_ACT_PRELU) return slope[0];
  else return prm;
}

// the sum of one value per thread over the workgroup, in double and in thread order: 16 threads add 16 values each,
// thread 0 adds the 16 sums and stores
__device__ __forceinline__ void bn_block_sum(float c, float* __restrict__ dst) {
  __shared__ float v[kBlock];
  __shared__ double w[16];
  v[threadIdx.x] = c;
  __syncthreads();
  if (threadIdx.x < 16) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) s += (double)v[threadIdx.x * 16 + q];
    w[threadIdx.x] = s;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = 0.0;
#pragma unroll
    for (int q = 0; q < 16; ++q) s += w[q];
    *dst = (float)s;
  }
}

static inline int bn_blocks(int64_t N) {
  int64_t b = ceil_div(N, 64);
  if (b < 1) b = 1;
  if (b > kBnMaxBlocks) b = kBnMaxBlocks;
  return (int)b;
}

static inline bool bn_al(const void* p, size_t a) { return p == nullptr || ((uintptr_t)p % a) == 0; }

struct BnWs { float* partial; float* v[5]; size_t total; };
// slabs: partial slabs per statistics workgroup (bn_drop.hip keeps a low-order slab beside each sum: 2)
static inline void bn_ws_layout(int64_t N, int32_t d, void* base, BnWs* w, int slabs = 1) {
  char* p = (char*)base;
  size_t off = 0;
  auto take = [&](size_t bytes) { void* r = p ? p + off : nullptr; off += align_up(bytes, 256); return r; };
  w->partial = (float*)take((size_t)bn_blocks(N) * slabs * 2 * d * 4);
  for (int i = 0; i < 5; ++i) w->v[i] = (float*)take((size_t)d * 4);
  w->total = off;
}

// the workspace of the *_act entries: mp_bn_ws_bytes' layout, then PRELU's per-workgroup sums (the BN slab's, then the
// CONCAT left slab's)
struct BnActWs { BnWs bn; float* partial3; size_t total; };
static inline void bn_act_ws_layout(int64_t N, int32_t d, void* base, BnActWs* w, int slabs = 1) {
  bn_ws_layout(N, d, base, &w->bn, slabs);
  w->partial3 = base ? (float*)((char*)base + w->bn.total) : nullptr;
  w->total = w->bn.total + align_up((size_t)2 * kBnMaxBlocks * 4, 256);
}

static inline bool act_known(int act) { return act >= MP_ACT_NONE && act <= MP_ACT_SILU; }

// ---- launches of bn.hip's kernels (defined there) ---------------------------------------------------------------------
// the statistics and finalize launches of the forward: mean / invstd / var_unbiased, and the affine of the apply pass in
// L.v[0] (scale) and L.v[1] (shift)
int bn_fwd_stats(const float* x, int64_t ldx, int64_t N, int32_t d, const float* gamma, const float* beta, float eps,
                 float* mean, float* invstd, float* var_unbiased, const BnWs& L, bool vec, hipStream_t st);
// backward finalize over the first nslab slabs of L.partial: dgamma, dbeta, the constants of dx = A g + B (x - mean) + C
// in L.v[0 .. 2] and, with fwd_scale, the forward's scale vector in L.v[3]
int bn_bwd_finalize(int64_t N, int32_t d, const float* gamma, const float* mean, const float* invstd, float* dgamma,
                    float* dbeta, const BnWs& L, int nslab, bool fwd_scale, hipStream_t st);
// PRELU: the first n per-workgroup sums of L.partial3 -> dslope[0]
int bn_dslope_finalize(const BnActWs& L, int n, float* dslope, hipStream_t st);
// the left slab of a CONCAT skip block's backward: dskip = dy[:, :d_skip] * act'(skip) (dskip NULL: not asked for) and,
// for PRELU, bn_blocks(N) per-workgroup sums at L.partial3 + bn_blocks(N).  act: one of the six activations.
int bn_act_bwd_left(int act, const float* dy, int64_t lddy, const float* skip, int64_t ldskip, float prm,
                    const float* slope, int64_t N, int32_t d_skip, float* dskip, int64_t lddskip, const BnActWs& L,
                    hipStream_t st);

}  // namespace mp
