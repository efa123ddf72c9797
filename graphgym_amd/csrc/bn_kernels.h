// The BatchNorm passes, written once: bn.hip (the entries without dropout) and bn_drop.hip (the entries with the keyed
// mask) instantiate the same three kernel templates and the same two host routines.
//   forward   apply  bn_apply_fwd_kernel<WS, WX, FORM, ACT, DROP>  out = act([skip +] [drop] BN(x)) | [act(skip) | ...]
//   backward  stats  bn_bwd_stats_kernel<W, ACT, ZSRC, DROP>        sum(g), sum(g (x - mean)), g = dy * act'(z) [masked]
//             final  bn_bwd_finalize_kernel<T>                      dgamma, dbeta, A, B, C (T: float, double under DROP)
//             apply  bn_bwd_apply_kernel<W, ACT, ZSRC, DROP>        dx = A g + B (x - mean) + C
// ACT is MP_ACT_NONE .. MP_ACT_SILU, DROP the keyed mask of draws.h between the normalisation and the skip operand.
// ZSRC: where the backward takes the pre-activation from — x (recomputed, the forward's own expression on the forward's
// own operands, kZX; kZXS: plus the skip operand of a SUM block when given) or, for the ReLU entries that are handed the
// forward's output, that output (kZY).
// The forward statistics, their finalize kernel and the CONCAT left slab are kernels of bn.hip behind host functions.
#pragma once
#include <initializer_list>
#include "common.h"
#include "vecio.h"
#include "act.h"
#include "draws.h"

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

// bn_colsum_store for sums that carry a low-order part: the rl row lanes' (hi + lo) are added in double in row-lane
// order; slab blockIdx.x receives the sum rounded to fp32, slab nblk + blockIdx.x what the rounding lost
template <int W>
__device__ __forceinline__ void bn_colsum_store2(const float (&a)[W], const float (&al)[W], const float (&b)[W],
                                                 const float (&bl)[W], const BnGeom& g, int cgi, int rli, bool on, int c0,
                                                 int32_t d, int nblk, float* __restrict__ partial) {
  __shared__ double red[2][kBlock][W];
#pragma unroll
  for (int k = 0; k < W; ++k) {
    red[0][threadIdx.x][k] = (double)a[k] + (double)al[k];
    red[1][threadIdx.x][k] = (double)b[k] + (double)bl[k];
  }
  __syncthreads();
  if (rli == 0 && on) {
#pragma unroll
    for (int k = 0; k < W; ++k) {
      double sa = 0.0, sb = 0.0;
      for (int q = 0; q < g.rl; ++q) { sa += red[0][q * g.cg + cgi][k]; sb += red[1][q * g.cg + cgi][k]; }
      if (c0 + k < d) {
        const float ha = (float)sa, hb = (float)sb;
        partial[((int64_t)blockIdx.x * 2 + 0) * d + c0 + k] = ha;
        partial[((int64_t)blockIdx.x * 2 + 1) * d + c0 + k] = hb;
        partial[((int64_t)(nblk + blockIdx.x) * 2 + 0) * d + c0 + k] = (float)(sa - (double)ha);
        partial[((int64_t)(nblk + blockIdx.x) * 2 + 1) * d + c0 + k] = (float)(sb - (double)hb);
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

// ---- the keyed mask (DROP) ----------------------------------------------------------------------------------------------
// Products with `scale` are __fmul_rn: never contracted into the skip add, so every form has the bits of the composition
// act([skip +] dropout_keyed(BN(x))).
template <int W>
__device__ __forceinline__ void drop_apply(float (&z)[W], const bool (&m)[W], float scale) {
#pragma unroll
  for (int k = 0; k < W; ++k) z[k] = m[k] ? __fmul_rn(z[k], scale) : 0.f;
}

// What the masked backward adds to the unmasked arithmetic, and why:
// (1) m * scale * g as an unrounded pair: hi = rn(g * scale), lo = the product's rounding residue (one fmaf).  The
//     scale is one more rounding than the undropped backward has; in a batch of two, where dx is the residue of terms
//     that cancel, that rounding alone is the size of the whole result's allowance.
// (2) column sums with their low-order parts: a thread adds by TwoSum, the workgroup reduces in double, and each
//     statistics workgroup writes TWO slabs, the sum rounded to fp32 and what that rounding lost (slab nblk + block),
//     which the finalize kernel adds like any other slab.  An fp32 slab alone rounds g0 + g1 of a batch of two.
// (3) for the kinds whose derivative is a smooth function of z (ELU, SELU, SILU), the derivative is taken at z with the
//     residue of the fp32 mean folded in: mean_lo[c] = sum_r (x[r, c] - mean[c]) / N, one more read of x ahead of the
//     statistics pass (bn_drop.hip).  mean[c] is the correctly rounded fp32 mean, but half an ulp of a mean of 12 is 4e-6
//     of a column deviation of 0.12, and act'' carries that into dx (times the dropout scale once more than the row
//     itself).  The BRANCH of a kinked kind (ELU's and SELU's z > 0) stays on the forward's own z, whose sign the output
//     has.  The kinds whose derivative is piecewise constant skip the pass.
// (4) dx = A g + B (x - mean) + C in double with A, B, C left in double by the finalize kernel (drop_dx below).
template <int ACT>
constexpr bool act_smooth() { return ACT == MP_ACT_ELU || ACT == MP_ACT_SELU || ACT == MP_ACT_SILU; }

// g = dy * act'(.): the branch on z (the forward's bits), the smooth part at zs
template <int ACT>
__device__ __forceinline__ float act_bwd_at(float dy, float z, float zs, float p) {
  if constexpr (ACT == MP_ACT_ELU) return z > 0.f ? dy : dy * (p * expf(zs));
  else if constexpr (ACT == MP_ACT_SELU) return dy * (kSeluScale * (z > 0.f ? 1.f : kSeluAlpha * expf(zs)));
  else if constexpr (ACT == MP_ACT_SILU) return dy * act_grad<ACT>(zs, p);
  else return act_bwd<ACT>(dy, z, p);
}

// (hi, lo) = m * scale * g without rounding; a dropped element is (0, 0)
__device__ __forceinline__ void drop_pair(float g, bool m, float scale, float& hi, float& lo) {
  const float h = __fmul_rn(g, scale);
  hi = m ? h : 0.f;
  lo = m ? fmaf(g, scale, -h) : 0.f;
}

// s + v -> s, with the rounding error added to e (Knuth's TwoSum)
__device__ __forceinline__ void two_sum(float& s, float& e, float v) {
  const float t = s + v;
  const float bb = t - s;
  e += (s - (t - bb)) + (v - bb);
  s = t;
}

// dx = A (hi + lo) + B xc + C in double, rounded once: in a batch of two the three terms are of size 2 and cancel to 1e-4,
// and the fp32 roundings of A, B, C and of the fmaf chain are each the size of the result's allowance
__device__ __forceinline__ float drop_dx(double A, double B, double C, float hi, float lo, float xc) {
  return (float)fma(A, (double)hi + (double)lo, fma(B, (double)xc, C));
}

// ---- forward apply -------------------------------------------------------------------------------------------------------
// FORM  kBnPlain : out = act(drop(BN(x)))
//       kBnSum   : out = act(skip + drop(BN(x)))                          (d_skip == d)
//       kBnConcat: out[:, :d_skip] = act(skip), out[:, d_skip:] = act(drop(BN(x)))
// with BN(x) = fmaf(x - ctr, p0, p1) and drop the identity unless DROP (then dk is not read and no draw is made).  WS /
// WX: vector widths of the skip slab and of the BN slab (equal unless CONCAT); a row is d_skip / WS (CONCAT) + d / WX
// work items.  The mask is indexed by x's own row and column, whatever the form.
enum { kBnPlain = 0, kBnSum = 1, kBnConcat = 2 };

template <int WS, int WX, int FORM, int ACT, bool DROP>
__global__ __launch_bounds__(kBlock) void bn_apply_fwd_kernel(const float* __restrict__ x, int64_t ldx,
                                                              const float* __restrict__ skip, int64_t ldskip,
                                                              const float* __restrict__ p0,
                                                              const float* __restrict__ p1,
                                                              const float* __restrict__ ctr, float prm,
                                                              const float* __restrict__ slope, DropKey dk, int64_t N,
                                                              int32_t d, int32_t d_skip, float* __restrict__ out,
                                                              int64_t ldo) {
  constexpr bool CONCAT = FORM == kBnConcat;
  const float ap = act_param<ACT>(prm, slope);
  const int gs = CONCAT ? (d_skip + WS - 1) / WS : 0;
  const int groups = gs + (d + WX - 1) / WX;
  const int64_t total = N * groups;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / groups;
    const int j = (int)(i - r * groups);
    if (CONCAT && j < gs) {
      const int c0 = j * WS;
      float sv[WS];
      load_vec<WS>(skip + r * ldskip + c0, sv);
#pragma unroll
      for (int k = 0; k < WS; ++k) sv[k] = act_fwd<ACT>(sv[k], ap);
      store_vec<WS>(out + r * ldo + c0, sv);
    } else {
      const int c0 = (j - gs) * WX;
      float xv[WX], a[WX], b[WX], o[WX], mv[WX];
      load_vec<WX>(x + r * ldx + c0, xv);
      load_vec<WX>(p0 + c0, a);
      load_vec<WX>(p1 + c0, b);
      load_vec<WX>(ctr + c0, mv);
#pragma unroll
      for (int k = 0; k < WX; ++k) o[k] = fmaf(xv[k] - mv[k], a[k], b[k]);
      if constexpr (DROP) {
        bool m[WX];
        drop_keep<WX>(dk, r, c0, m);
        drop_apply<WX>(o, m, dk.scale);
      }
      if constexpr (FORM == kBnSum) {
        float sv[WX];
        load_vec<WX>(skip + r * ldskip + c0, sv);
#pragma unroll
        for (int k = 0; k < WX; ++k) o[k] = sv[k] + o[k];
      }
#pragma unroll
      for (int k = 0; k < WX; ++k) o[k] = act_fwd<ACT>(o[k], ap);
      store_vec<WX>(out + r * ldo + (CONCAT ? d_skip : 0) + c0, o);
    }
  }
}

// ---- backward ------------------------------------------------------------------------------------------------------------
enum { kZX = 0, kZXS = 1, kZY = 2 };

// The pre-activation of one row's W columns for both backward kernels.  xc = x - mean.
//   ZSRC = kZY (RELU, no mask): z is the forward's output, read from s + soff
//   ZSRC = kZX, kZXS          : z = drop(fmaf(xc, sc, bt)) [+ skip, read from s + soff unless s is NULL: kZXS], the forward's
//                               own expression; under DROP the smooth kinds get zs, the same with xc - ml (see (3) above)
//   ACT = NONE                : nothing is read or formed
template <int W, int ACT, int ZSRC, bool DROP>
__device__ __forceinline__ void bn_bwd_z(float (&z)[W], float (&zs)[W], const float (&xc)[W], const float (&sc)[W],
                                         const float (&bt)[W], const float (&ml)[W], const bool (&m)[W], float dscale,
                                         const float* __restrict__ s, int64_t soff) {
  constexpr bool SMOOTH = DROP && act_smooth<ACT>();
#pragma unroll
  for (int k = 0; k < W; ++k) { z[k] = 0.f; zs[k] = 0.f; }
  if constexpr (ACT == MP_ACT_NONE) {
    return;
  } else if constexpr (ZSRC == kZY) {
    load_vec<W>(s + soff, z);
  } else {
#pragma unroll
    for (int k = 0; k < W; ++k) {
      z[k] = fmaf(xc[k], sc[k], bt[k]);
      zs[k] = SMOOTH ? fmaf(xc[k] - ml[k], sc[k], bt[k]) : 0.f;
    }
    if constexpr (DROP) drop_apply<W>(z, m, dscale);
    if constexpr (SMOOTH) drop_apply<W>(zs, m, dscale);
    if (ZSRC == kZXS && s != nullptr) {
      float sv[W];
      load_vec<W>(s + soff, sv);
#pragma unroll
      for (int k = 0; k < W; ++k) { z[k] = sv[k] + z[k]; zs[k] = sv[k] + zs[k]; }
    }
  }
}

// g = dy * act'(z): NONE hands dy on; under DROP the smooth kinds branch on z and take the derivative at zs
template <int ACT, bool DROP>
__device__ __forceinline__ float bn_bwd_g(float dy, float z, float zs, float ap) {
  if constexpr (ACT == MP_ACT_NONE) return dy;
  else if constexpr (DROP && act_smooth<ACT>()) return act_bwd_at<ACT>(dy, z, zs, ap);
  else return act_bwd<ACT>(dy, z, ap);
}

// backward statistics: per column a = sum(g'), b = sum(g' (x - mean)) over the workgroup's run of rows, with g as in
// bn_bwd_g and g' = g (fp32 sums, bn_colsum_store) or, under DROP, g' = m * scale * g as an unrounded pair added by TwoSum
// (bn_colsum_store2: two slabs per workgroup), z as in bn_bwd_z.  `s`: skip (ZSRC = kZXS, NULL: none) or the forward's output (kZY); there g
// goes to gout when given: d skip of the SUM block, NOT masked.  With kZX neither operand exists, at compile time: the
// NONE / RELU statistics of a layer without mask and without skip operand, the default layer's, then fit the 64 registers
// of 8 waves per SIMD (the other kinds take no fewer registers that way and run as kZXS without the operands).  PRELU carries a third sum, dy * min(z, 0), over the workgroup's
// rows AND columns: one value per workgroup in partial3, added in thread order.
template <int W, int ACT, int ZSRC, bool DROP>
__global__ __launch_bounds__(kBlock) void bn_bwd_stats_kernel(const float* __restrict__ x, int64_t ldx,
                                                              const float* __restrict__ dy, int64_t lddy,
                                                              const float* __restrict__ s, int64_t lds,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ gamma,
                                                              const float* __restrict__ beta,
                                                              const float* __restrict__ invstd, float prm,
                                                              const float* __restrict__ slope,
                                                              const float* __restrict__ mean_lo, DropKey dk, int64_t N,
                                                              int32_t d, int64_t rows_per_block,
                                                              float* __restrict__ partial, float* __restrict__ partial3,
                                                              float* __restrict__ gout, int64_t ldg) {
  constexpr bool NEEDZ = ACT != MP_ACT_NONE && ZSRC != kZY;
  const float ap = act_param<ACT>(prm, slope);
  const BnGeom g = bn_geom<W>(d);
  const int cgi = threadIdx.x % g.cg;
  const int rli = threadIdx.x / g.cg;
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
  const int64_t r1 = r0 + rows_per_block < N ? r0 + rows_per_block : N;
  float c3 = 0.f;
  for (int t = 0; t < g.tiles; ++t) {
    const int c0 = (t * g.cg + cgi) * W;
    const bool on = c0 < d;
    float a[W], al[W], b[W], bl[W], pv[W], sc[W], bt[W], ml[W];
#pragma unroll
    for (int k = 0; k < W; ++k) {
      a[k] = 0.f; al[k] = 0.f; b[k] = 0.f; bl[k] = 0.f; pv[k] = 0.f; sc[k] = 0.f; bt[k] = 0.f; ml[k] = 0.f;
    }
    if (on) {
      load_vec<W>(mean + c0, pv);
      if constexpr (DROP && act_smooth<ACT>()) load_vec<W>(mean_lo + c0, ml);
      if constexpr (NEEDZ) {
#pragma unroll
        for (int k = 0; k < W; ++k)
          if (c0 + k < d) {
            sc[k] = bn_scale(gamma ? gamma[c0 + k] : 1.f, invstd[c0 + k]);
            bt[k] = beta ? beta[c0 + k] : 0.f;
          }
      }
      for (int64_t r = r0 + rli; r < r1; r += g.rl) {
        float xv[W], gv[W];
        bool m[W] = {};
        load_vec<W>(x + r * ldx + c0, xv);
        load_vec<W>(dy + r * lddy + c0, gv);
        if constexpr (DROP) drop_keep<W>(dk, r, c0, m);
#pragma unroll
        for (int k = 0; k < W; ++k) xv[k] -= pv[k];
        float z[W], zs[W];
        bn_bwd_z<W, ACT, ZSRC, DROP>(z, zs, xv, sc, bt, ml, m, dk.scale, s, r * lds + c0);
#pragma unroll
        for (int k = 0; k < W; ++k) {
          if constexpr (ACT == MP_ACT_PRELU) c3 = fmaf(gv[k], act_dslope(z[k]), c3);      // dy * min(z, 0): d out / d slope
          gv[k] = bn_bwd_g<ACT, DROP>(gv[k], z[k], zs[k], ap);
        }
        if (ZSRC != kZX && gout != nullptr) store_vec<W>(gout + r * ldg + c0, gv);
#pragma unroll
        for (int k = 0; k < W; ++k) {
          if constexpr (DROP) {
            float hi, lo;
            drop_pair(gv[k], m[k], dk.scale, hi, lo);
            two_sum(a[k], al[k], hi);
            al[k] += lo;
            const float pr = __fmul_rn(hi, xv[k]);
            two_sum(b[k], bl[k], pr);
            bl[k] += fmaf(hi, xv[k], -pr) + lo * xv[k];
          } else {
            a[k] += gv[k];
            b[k] = fmaf(gv[k], xv[k], b[k]);
          }
        }
      }
    }
    if constexpr (DROP) bn_colsum_store2<W>(a, al, b, bl, g, cgi, rli, on, c0, d, (int)gridDim.x, partial);
    else bn_colsum_store<W>(a, b, g, cgi, rli, on, c0, d, partial);
  }
  if constexpr (ACT == MP_ACT_PRELU) bn_block_sum(c3, partial3 + blockIdx.x);
}

// backward finalize over nslab slabs: dgamma, dbeta, the constants of dx = A g + B (x - mean) + C (T: fp32, or double for
// the masked backward) and, fwd_scale given, the forward's scale vector for the recomputed pre-activation
template <class T>
__global__ __launch_bounds__(kBlock) void bn_bwd_finalize_kernel(const float* __restrict__ partial, int nslab, int64_t N,
                                                                 int32_t d, const float* __restrict__ gamma,
                                                                 const float* __restrict__ invstd, float* dgamma,
                                                                 float* dbeta, T* A, T* B, T* Cc, float* fwd_scale) {
  int c;
  double sg, sgx;
  if (!bn_col_sums(partial, nslab, d, c, sg, sgx)) return;
  const double istd = invstd[c];
  const double gm = gamma ? (double)gamma[c] : 1.0;
  const double dgam = sgx * istd;                       // sum g * xhat (the sums were taken against the mean)
  if (dgamma) dgamma[c] = (float)dgam;
  if (dbeta) dbeta[c] = (float)sg;
  const double a = gm * istd;
  const double bb = -gm * istd * istd * dgam / (double)N;
  A[c] = (T)a;
  B[c] = (T)bb;
  Cc[c] = (T)(-a * sg / (double)N);
  if (fwd_scale != nullptr) fwd_scale[c] = bn_scale(gamma ? gamma[c] : 1.f, invstd[c]);
}

template <bool DROP> using BnCoef = std::conditional_t<DROP, double, float>;

// backward apply: dx = A g' + B (x - mean) + C with g / g' as in the statistics kernel; "g on hand" (the statistics pass
// wrote it) is ACT = NONE on that g, which loads neither fwd_scale, beta nor mean_lo.  fp32: two fmaf; DROP: drop_dx.
template <int W, int ACT, int ZSRC, bool DROP>
__global__ __launch_bounds__(kBlock) void bn_bwd_apply_kernel(const float* __restrict__ x, int64_t ldx,
                                                              const float* __restrict__ dy, int64_t lddy,
                                                              const float* __restrict__ s, int64_t lds,
                                                              const BnCoef<DROP>* __restrict__ A,
                                                              const BnCoef<DROP>* __restrict__ B,
                                                              const BnCoef<DROP>* __restrict__ Cc,
                                                              const float* __restrict__ mean,
                                                              const float* __restrict__ fwd_scale,
                                                              const float* __restrict__ beta, float prm,
                                                              const float* __restrict__ slope,
                                                              const float* __restrict__ mean_lo, DropKey dk, int64_t N,
                                                              int32_t d, float* __restrict__ out, int64_t ldo) {
  constexpr bool NEEDZ = ACT != MP_ACT_NONE && ZSRC != kZY;
  const float ap = act_param<ACT>(prm, slope);
  const int groups = (d + W - 1) / W;
  const int64_t total = N * groups;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / groups;
    const int c0 = (int)(i - r * groups) * W;
    float xv[W], o[W], mv[W], gv[W], sck[W], btk[W], ml[W];
    bool m[W] = {};
#pragma unroll
    for (int k = 0; k < W; ++k) { sck[k] = 0.f; btk[k] = 0.f; ml[k] = 0.f; }
    if constexpr (DROP && act_smooth<ACT>()) load_vec<W>(mean_lo + c0, ml);
    load_vec<W>(x + r * ldx + c0, xv);
    load_vec<W>(dy + r * lddy + c0, gv);
    float a[W], b[W], cv[W];
    if constexpr (!DROP) {
      load_vec<W>(A + c0, a);
      load_vec<W>(B + c0, b);
      load_vec<W>(Cc + c0, cv);
    }
    load_vec<W>(mean + c0, mv);
    if constexpr (NEEDZ) {
      load_vec<W>(fwd_scale + c0, sck);
      if (beta != nullptr) load_vec<W>(beta + c0, btk);
    }
    if constexpr (DROP) drop_keep<W>(dk, r, c0, m);
#pragma unroll
    for (int k = 0; k < W; ++k) xv[k] -= mv[k];
    float z[W], zs[W];
    bn_bwd_z<W, ACT, ZSRC, DROP>(z, zs, xv, sck, btk, ml, m, dk.scale, s, r * lds + c0);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      const float g = bn_bwd_g<ACT, DROP>(gv[k], z[k], zs[k], ap);
      if constexpr (DROP) {
        float hi, lo;
        drop_pair(g, m[k], dk.scale, hi, lo);
        o[k] = drop_dx(A[c0 + k], B[c0 + k], Cc[c0 + k], hi, lo, xv[k]);
      } else {
        o[k] = fmaf(a[k], g, fmaf(b[k], xv[k], cv[k]));
      }
    }
    store_vec<W>(out + r * ldo + c0, o);
  }
}

// ---- host side -----------------------------------------------------------------------------------------------------------
static inline int bn_blocks(int64_t N) {
  int64_t b = ceil_div(N, 64);
  if (b < 1) b = 1;
  if (b > kBnMaxBlocks) b = kBnMaxBlocks;
  return (int)b;
}

// The 4-wide form of a launch: the width, every leading dimension and every pointer its kernel loads or stores 4-wide
// (NULL: operand absent, with a leading dimension of 0) fit a 16-byte access.
static inline bool bn_vec4(int32_t d, std::initializer_list<int64_t> lds, std::initializer_list<const void*> ptrs) {
  bool ok = d % 4 == 0;
  for (int64_t ld : lds) ok = ok && ld % 4 == 0;
  for (const void* p : ptrs) ok = ok && (uintptr_t)p % 16 == 0;
  return ok;
}

// One view of the three workspace layouts: mp_bn_ws_bytes' (kBnWs: the partial slabs and five [d] vectors),
// mp_bn_act_ws_bytes' (kBnWsAct: then PRELU's per-workgroup sums, the BN slab's and the CONCAT left slab's) and
// mp_bn_drop_ws_bytes' (kBnWsDrop: a low-order slab beside each partial slab, and A, B, C in double at the end).
enum { kBnWs = 0, kBnWsAct = 1, kBnWsDrop = 2 };
struct BnWs { float* partial; float* v[5]; float* partial3; double* c[3]; size_t total; };
static inline void bn_ws_layout(int64_t N, int32_t d, void* base, BnWs* w, int kind) {
  char* p = (char*)base;
  size_t off = 0;
  auto take = [&](size_t bytes) { void* r = p ? p + off : nullptr; off += align_up(bytes, 256); return r; };
  w->partial = (float*)take((size_t)bn_blocks(N) * (kind == kBnWsDrop ? 2 : 1) * 2 * d * 4);
  for (int i = 0; i < 5; ++i) w->v[i] = (float*)take((size_t)d * 4);
  w->partial3 = kind >= kBnWsAct ? (float*)take((size_t)2 * kBnMaxBlocks * 4) : nullptr;
  for (int i = 0; i < 3; ++i) w->c[i] = kind == kBnWsDrop ? (double*)take((size_t)d * 8) : nullptr;
  w->total = off;
}
static inline int bn_ws_bytes(int64_t N, int32_t d, size_t* bytes_host, int kind) {
  if (!bytes_host || N < 0 || d <= 0) return MP_ERR_INVALID_ARG;
  BnWs w;
  bn_ws_layout(N, d, nullptr, &w, kind);
  *bytes_host = w.total;
  return MP_OK;
}

static inline bool act_known(int act) { return act >= MP_ACT_NONE && act <= MP_ACT_SILU; }

// T in [0, 65536] -> the call's key, threshold and scale; false for a T outside the range
static inline bool drop_make(int32_t T, uint64_t seed, uint64_t offset, int32_t d, DropKey* k) {
  if (T < 0 || T > 65536) return false;
  k->key = drop_key(seed, offset);
  k->T = (uint32_t)T;
  k->scale = T == 65536 ? 0.f : (float)(65536.0 / (double)(65536 - T));
  k->q = (d + 3) / 4;
  return true;
}

// ---- launches of bn.hip's kernels (defined there) ---------------------------------------------------------------------
// the statistics and finalize launches of the forward: mean / invstd / var_unbiased, and the affine of the apply pass in
// L.v[0] (scale) and L.v[1] (shift)
int bn_fwd_stats(const float* x, int64_t ldx, int64_t N, int32_t d, const float* gamma, const float* beta, float eps,
                 float* mean, float* invstd, float* var_unbiased, const BnWs& L, bool vec, hipStream_t st);
// PRELU: the first n per-workgroup sums of L.partial3 -> dslope[0]
int bn_dslope_finalize(const BnWs& L, int n, float* dslope, hipStream_t st);
// the left slab of a CONCAT skip block's backward: dskip = dy[:, :d_skip] * act'(skip) (dskip NULL: not asked for) and,
// for PRELU, bn_blocks(N) per-workgroup sums at L.partial3 + bn_blocks(N).  act: one of the six activations.
int bn_act_bwd_left(int act, const float* dy, int64_t lddy, const float* skip, int64_t ldskip, float prm,
                    const float* slope, int64_t N, int32_t d_skip, float* dskip, int64_t lddskip, const BnWs& L,
                    hipStream_t st);
// the residue of the fp32 mean into L.v[4] (bn_drop.hip; uses L.partial)
int bn_mean_lo(const float* x, int64_t ldx, const float* mean, int64_t N, int32_t d, const BnWs& L, bool vec,
               hipStream_t st);

// The operands of a forward or backward entry, as its adapter hands them to bn_fwd_run / bn_bwd_run.  skipped: the entry
// has a skip operand (skip, d_skip, mode: MP_BN_SKIP_*).  T, seed, offset: the mask's key (DROP).  wskind: the workspace
// the entry demands.
struct BnCall {
  int wskind;
  const float* x; int64_t ldx;
  int64_t N; int32_t d;
  const float *gamma, *beta;
  const float *mean, *invstd;           // the forward's own outputs, handed in again beside
  int act; float prm; const float* slope;
  bool skipped; const float* skip; int64_t ldskip; int32_t d_skip; int mode;
  int32_t T; uint64_t seed, offset;
  void* ws; size_t ws_bytes; mp_stream_t stream;
};

// what every entry checks before anything is launched, the workspace last: its view in *L, the mask's key in *dk
template <bool DROP>
static int bn_check(const BnCall& c, bool others_ok, BnWs* L, DropKey* dk) {
  if (!act_known(c.act) || (c.act == MP_ACT_PRELU && !c.slope)) return MP_ERR_INVALID_ARG;
  if (c.N <= 0 || c.d <= 0 || !c.x || !c.mean || !c.invstd || c.ldx < c.d || !others_ok) return MP_ERR_INVALID_ARG;
  if (c.skipped) {
    if (c.mode != MP_BN_SKIP_SUM && c.mode != MP_BN_SKIP_CONCAT) return MP_ERR_INVALID_ARG;
    if (c.d_skip <= 0 || !c.skip || c.ldskip < c.d_skip || (c.mode == MP_BN_SKIP_SUM && c.d_skip != c.d))
      return MP_ERR_INVALID_ARG;
  }
  if (DROP && !drop_make(c.T, c.seed, c.offset, c.d, dk)) return MP_ERR_INVALID_ARG;
  bn_ws_layout(c.N, c.d, c.ws, L, c.wskind);
  if (!c.ws || c.ws_bytes < L->total) return MP_ERR_WORKSPACE;
  return MP_OK;
}

// the BN slab plus, in a CONCAT block, the skip slab
static inline int64_t bn_row_width(const BnCall& c) {
  return c.skipped && c.mode == MP_BN_SKIP_CONCAT ? (int64_t)c.d_skip + c.d : (int64_t)c.d;
}

// Every forward entry: the statistics, then ONE apply launch of the entry's form, widths and activation.
template <bool DROP>
static int bn_fwd_run(BnCall c, float eps, float* out, int64_t ldo, float* mean, float* invstd, float* var_unbiased) {
  c.mean = mean;
  c.invstd = invstd;
  BnWs L;
  DropKey dk{};
  const int rc = bn_check<DROP>(c, out && var_unbiased && ldo >= bn_row_width(c), &L, &dk);
  if (rc != MP_OK) return rc;
  hipStream_t st = as_stream(c.stream);
  const bool cat = c.skipped && c.mode == MP_BN_SKIP_CONCAT;
  // a launch takes its vector form when every pointer it forms is 16-byte aligned: the apply pass writes the BN slab at
  // out (out + d_skip: CONCAT) and the skip slab at out.  The statistics read x alone; those of a layer without skip
  // operand share the apply pass's form.
  const bool vx = bn_vec4(c.d, {c.ldx}, {c.x, c.mean});
  const bool vo = bn_vec4(4, {ldo}, {out});
  const bool vs = c.skipped && bn_vec4(c.d_skip, {c.ldskip}, {c.skip}) && vo;
  const bool vr = vx && vo && (!cat || c.d_skip % 4 == 0);      // CONCAT: the right slab starts at out + d_skip
  const int frc = bn_fwd_stats(c.x, c.ldx, c.N, c.d, c.gamma, c.beta, eps, mean, invstd, var_unbiased, L,
                               c.skipped ? vx : vr, st);
  if (frc != MP_OK) return frc;
#define MP_BN_FWD_LAUNCH(WS, WX, FORM)                                                                                  \
  hipLaunchKernelGGL((bn_apply_fwd_kernel<WS, WX, FORM, A, DROP>),                                                      \
                     dim3(flat_grid(c.N * ((FORM == kBnConcat ? (int64_t)c.d_skip / WS : 0) + (int64_t)c.d / WX))),     \
                     dim3(kBlock), 0, st, c.x, c.ldx, c.skip, c.ldskip, L.v[0], L.v[1], c.mean, c.prm, c.slope, dk,     \
                     c.N, c.d, c.d_skip, out, ldo)
  with_act(c.act, [&](auto a) {
    constexpr int A = decltype(a)::value;
    if (!c.skipped) {
      if (vr) MP_BN_FWD_LAUNCH(4, 4, kBnPlain);
      else MP_BN_FWD_LAUNCH(1, 1, kBnPlain);
    } else if (!cat) {
      if (vx && vs) MP_BN_FWD_LAUNCH(4, 4, kBnSum);
      else MP_BN_FWD_LAUNCH(1, 1, kBnSum);
    } else {
      if (vs && vr) MP_BN_FWD_LAUNCH(4, 4, kBnConcat);
      else if (vs) MP_BN_FWD_LAUNCH(4, 1, kBnConcat);
      else if (vr) MP_BN_FWD_LAUNCH(1, 4, kBnConcat);
      else MP_BN_FWD_LAUNCH(1, 1, kBnConcat);
    }
  });
#undef MP_BN_FWD_LAUNCH
  MP_LAUNCH_CHECK();
  return MP_OK;
}

// statistics, finalize and apply of one backward.  s: the skip operand inside the pre-activation (ZSRC = kZXS) or the
// forward's output (kZY).  gout != NULL: the statistics pass writes g there and the apply pass reads it in place of dy, the
// pre-activation and s — same terms, same order, one [N, d] read fewer.  PRELU leaves its per-workgroup sums in
// L.partial3[0 .. bn_blocks(N)).
template <int ACT, int ZSRC, bool DROP>
static int bn_bwd_launch(const BnCall& c, const float* dy, int64_t lddy, const float* s, int64_t lds, const DropKey& dk,
                         float* dx, int64_t lddx, float* gout, int64_t ldg, float* dgamma, float* dbeta, const BnWs& L,
                         hipStream_t st) {
  constexpr bool NEEDZ = ACT != MP_ACT_NONE && ZSRC != kZY;
  const int nblk = bn_blocks(c.N);
  const int64_t rpb = ceil_div(c.N, nblk);
  const dim3 blk(kBlock);
  const bool vec = bn_vec4(c.d, {c.ldx, lddy, lddx, lds, ldg}, {c.x, dy, dx, s, gout, NEEDZ ? c.beta : nullptr, c.mean});
  const dim3 flat(flat_grid(c.N * (vec ? c.d / 4 : c.d)));
  const float* mean_lo = nullptr;
  if constexpr (DROP && act_smooth<ACT>()) {      // into L.v[4]; the slabs are reused below
    const int rc = bn_mean_lo(c.x, c.ldx, c.mean, c.N, c.d, L, vec, st);
    if (rc != MP_OK) return rc;
    mean_lo = L.v[4];
  }
#define MP_BN_BWD_STATS(W)                                                                                              \
  hipLaunchKernelGGL((bn_bwd_stats_kernel<W, ACT, ZSRC, DROP>), dim3(nblk), blk, 0, st, c.x, c.ldx, dy, lddy, s, lds,  \
                     c.mean, c.gamma, c.beta, c.invstd, c.prm, c.slope, mean_lo, dk, c.N, c.d, rpb, L.partial,         \
                     L.partial3, gout, ldg)
  if (vec) MP_BN_BWD_STATS(4);
  else MP_BN_BWD_STATS(1);
#undef MP_BN_BWD_STATS
  MP_LAUNCH_CHECK();
  BnCoef<DROP>*A, *B, *Cc;
  if constexpr (DROP) { A = L.c[0]; B = L.c[1]; Cc = L.c[2]; }
  else { A = L.v[0]; B = L.v[1]; Cc = L.v[2]; }
  hipLaunchKernelGGL(bn_bwd_finalize_kernel<BnCoef<DROP>>, dim3((unsigned)ceil_div(c.d, 16)), blk, 0, st, L.partial,
                     DROP ? 2 * nblk : nblk, c.N, c.d, c.gamma, c.invstd, dgamma, dbeta, A, B, Cc,
                     NEEDZ || DROP ? L.v[3] : nullptr);
  MP_LAUNCH_CHECK();
#define MP_BN_BWD_APPLY(W, A_, Z_, DY, LDDY, S, LDS)                                                                    \
  hipLaunchKernelGGL((bn_bwd_apply_kernel<W, A_, Z_, DROP>), flat, blk, 0, st, c.x, c.ldx, DY, LDDY, S, LDS, A, B, Cc, \
                     c.mean, L.v[3], c.beta, c.prm, c.slope, mean_lo, dk, c.N, c.d, dx, lddx)
  if (gout != nullptr) {      // g is on hand
    if (vec) MP_BN_BWD_APPLY(4, MP_ACT_NONE, kZX, gout, ldg, nullptr, 0);
    else MP_BN_BWD_APPLY(1, MP_ACT_NONE, kZX, gout, ldg, nullptr, 0);
  } else {
    if (vec) MP_BN_BWD_APPLY(4, ACT, ZSRC, dy, lddy, s, lds);
    else MP_BN_BWD_APPLY(1, ACT, ZSRC, dy, lddy, s, lds);
  }
#undef MP_BN_BWD_APPLY
  MP_LAUNCH_CHECK();
  return MP_OK;
}

// Every backward entry.  dy: [N, d], or [N, d_skip + d] in a CONCAT block.  y (RELU without mask only): the forward's
// output stands in for the pre-activation.  dskip: where d skip goes — g itself in a SUM block with an activation and in
// the entries handed y, dy's left slab times act'(skip) in a CONCAT block (one more launch); without activation d skip is
// dy (its left slab) itself and nothing is written.
template <bool DROP>
static int bn_bwd_run(const BnCall& c, const float* dy, int64_t lddy, const float* y, int64_t ldy, float* dx,
                      int64_t lddx, float* dskip, int64_t lddskip, float* dgamma, float* dbeta, float* dslope) {
  BnWs L;
  DropKey dk{};
  const int crc = bn_check<DROP>(c, dy && dx && lddy >= bn_row_width(c) && lddx >= c.d && (!y || ldy >= c.d) &&
                                        (!dskip || lddskip >= (c.skipped ? c.d_skip : c.d)), &L, &dk);
  if (crc != MP_OK) return crc;
  hipStream_t st = as_stream(c.stream);
  const bool cat = c.skipped && c.mode == MP_BN_SKIP_CONCAT;
  const bool none = c.act == MP_ACT_NONE;
  const bool sum = c.skipped && !cat && !none;      // the pre-activation holds skip
  const float* dyr = cat ? dy + c.d_skip : dy;      // the BN slab of dy
  const float* s = y ? y : sum ? c.skip : nullptr;
  const int64_t lds = y ? ldy : sum ? c.ldskip : 0;
  float* gout = y || sum ? dskip : nullptr;
  int rc = MP_OK;
  with_act(c.act, [&](auto a) {
    constexpr int A = decltype(a)::value;
#define MP_BN_BWD(ZSRC)                                                                                                 \
  rc = bn_bwd_launch<A, ZSRC, DROP>(c, dyr, lddy, s, lds, dk, dx, lddx, gout, gout ? lddskip : 0, dgamma, dbeta, L, st)
    if constexpr (DROP || A > MP_ACT_RELU) {
      MP_BN_BWD(kZXS);
    } else if constexpr (A == MP_ACT_RELU) {
      if (y) MP_BN_BWD(kZY);
      else if (sum) MP_BN_BWD(kZXS);
      else MP_BN_BWD(kZX);
    } else {
      MP_BN_BWD(kZX);
    }
#undef MP_BN_BWD
  });
  if (rc != MP_OK) return rc;
  const bool prelu = c.act == MP_ACT_PRELU && dslope;
  if (cat && !none && (dskip || prelu)) {      // the left slab never sees the mask
    rc = bn_act_bwd_left(c.act, dy, lddy, c.skip, c.ldskip, c.prm, c.slope, c.N, c.d_skip, dskip, lddskip, L, st);
    if (rc != MP_OK) return rc;
  }
  if (prelu) return bn_dslope_finalize(L, cat ? 2 * bn_blocks(c.N) : bn_blocks(c.N), dslope, st);
  return MP_OK;
}

}  // namespace mp
