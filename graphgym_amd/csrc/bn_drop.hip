// gnn.dropout between the BatchNorm and the activation (graphgym/models/layer.py:26-35: BatchNorm1d -> Dropout -> act;
// in a skip block on the last layer, before the skip operand: gnn.py:49-60), riding bn.hip's passes with a KEYED mask:
// keep(seed, offset, r, c) of draws.h is a pure function of the call's key and the element's logical index, so nothing
// is stored — the backward recomputes the mask exactly as it recomputes the activation from x.
//   forward   stats  : bn.hip's, unchanged (dropout sits behind the normalisation)
//             apply  : out = act(m * scale * BN(x))            | act(skip + m * scale * BN(x))
//                                                              | [act(skip) | act(m * scale * BN(x))]
//   backward  (ELU, SELU, SILU only) the residue of the fp32 mean: one read of x, see below
//             stats  : z recomputed (masked), g = dy * act'(z); d skip = g (SUM, not masked); the column sums and dx take
//                      m * scale * g; PRELU's slope sum takes dy * min(z, 0) on the masked z
//             apply  : dx = A (m * scale * g) + B (x - mean) + C
//   mp_dropout_keyed_f32: out = m * scale * x, the mask alone (its backward is the same launch on dy)
// One hash per aligned group of four columns: a 4-wide thread draws once per load, a scalar thread once per element.
// Products with `scale` are __fmul_rn: never contracted into the skip add, so every form has the bits of the composition
// act([skip +] dropout_keyed(BN(x))).
#include "bn_shared.h"
#include "draws.h"

namespace mp {

template <int W>
__device__ __forceinline__ void drop_apply(float (&z)[W], const bool (&m)[W], float scale) {
#pragma unroll
  for (int k = 0; k < W; ++k) z[k] = m[k] ? __fmul_rn(z[k], scale) : 0.f;
}

// ---- what the backward adds to bn.hip's arithmetic, and why -----------------------------------------------------------
// (1) m * scale * g as an unrounded pair: hi = rn(g * scale), lo = the product's rounding residue (one fmaf).  The
//     scale is one more rounding than the undropped backward has; in a batch of two, where dx is the residue of terms
//     that cancel, that rounding alone is the size of the whole result's allowance.
// (2) column sums with their low-order parts: a thread adds by TwoSum, the workgroup reduces in double, and each
//     statistics workgroup writes TWO slabs, the sum rounded to fp32 and what that rounding lost (slab nblk + block),
//     which the finalize kernel adds like any other slab.  An fp32 slab alone rounds g0 + g1 of a batch of two.
// (3) for the kinds whose derivative is a smooth function of z (ELU, SELU, SILU), the derivative is taken at z with the
//     residue of the fp32 mean folded in: mean_lo[c] = sum_r (x[r, c] - mean[c]) / N, one more read of x ahead of the
//     statistics pass.  mean[c] is the correctly rounded fp32 mean, but half an ulp of a mean of 12 is 4e-6 of a
//     column deviation of 0.12, and act'' carries that into dx (times the dropout scale once more than the row itself).
//     The BRANCH of a kinked kind (ELU's and SELU's z > 0) stays on the forward's own z, whose sign the output has.
//     The kinds whose derivative is piecewise constant skip the pass.
// (4) dx = A g + B (x - mean) + C in double with A, B, C left in double by a finalize kernel of its own (drop_dx below).
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

// dx = A (hi + lo) + B xc + C in double, rounded once: in a batch of two the three terms are of size 2 and cancel to 1e-4,
// and the fp32 roundings of A, B, C and of the fmaf chain are each the size of the result's allowance
__device__ __forceinline__ float drop_dx(double A, double B, double C, float hi, float lo, float xc) {
  return (float)fma(A, (double)hi + (double)lo, fma(B, (double)xc, C));
}

// bn_bwd_finalize_kernel with the constants of dx = A g + B (x - mean) + C left in double
__global__ __launch_bounds__(kBlock) void bn_drop_bwd_finalize_kernel(const float* __restrict__ partial, int nslab,
                                                                      int64_t N, int32_t d,
                                                                      const float* __restrict__ gamma,
                                                                      const float* __restrict__ invstd, float* dgamma,
                                                                      float* dbeta, double* A, double* B, double* Cc,
                                                                      float* fwd_scale) {
  int c;
  double sg, sgx;
  if (!bn_col_sums(partial, nslab, d, c, sg, sgx)) return;
  const double istd = invstd[c];
  const double gm = gamma ? (double)gamma[c] : 1.0;
  const double dgam = sgx * istd;                       // sum g * xhat (the sums were taken against the mean)
  if (dgamma) dgamma[c] = (float)dgam;
  if (dbeta) dbeta[c] = (float)sg;
  const double a = gm * istd;
  A[c] = a;
  B[c] = -gm * istd * istd * dgam / (double)N;
  Cc[c] = -a * sg / (double)N;
  fwd_scale[c] = bn_scale(gamma ? gamma[c] : 1.f, invstd[c]);
}

// the workspace of the entries below: bn_act_ws_layout with two partial slabs per statistics workgroup, then A, B, C
struct DropWs { BnActWs act; double* c[3]; size_t total; };
static void drop_ws_layout(int64_t N, int32_t d, void* base, DropWs* w) {
  bn_act_ws_layout(N, d, base, &w->act, 2);
  size_t off = w->act.total;
  for (int i = 0; i < 3; ++i) {
    w->c[i] = base ? (double*)((char*)base + off) : nullptr;
    off += align_up((size_t)d * 8, 256);
  }
  w->total = off;
}

// FORM 0: out = act(drop(BN(x)))   1 (SUM): out = act(skip + drop(BN(x)))   2 (CONCAT): out = [act(skip) | act(drop(BN(x)))]
// The BN term is bn_apply_kernel<W, 0>'s own fmaf.  WS / WX: vector widths of the skip slab and of the BN slab; a row
// is d_skip / WS (CONCAT) + d / WX work items.  The mask is indexed by x's own row and column, whatever the form.
template <int WS, int WX, int FORM, int ACT>
__global__ __launch_bounds__(kBlock) void bn_drop_apply_kernel(const float* __restrict__ x, int64_t ldx,
                                                               const float* __restrict__ skip, int64_t ldskip,
                                                               const float* __restrict__ p0,
                                                               const float* __restrict__ p1,
                                                               const float* __restrict__ ctr, float prm,
                                                               const float* __restrict__ slope, DropKey dk, int64_t N,
                                                               int32_t d, int32_t d_skip, float* __restrict__ out,
                                                               int64_t ldo) {
  constexpr bool CONCAT = FORM == 2;
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
      bool m[WX];
      load_vec<WX>(x + r * ldx + c0, xv);
      load_vec<WX>(p0 + c0, a);
      load_vec<WX>(p1 + c0, b);
      load_vec<WX>(ctr + c0, mv);
      drop_keep<WX>(dk, r, c0, m);
#pragma unroll
      for (int k = 0; k < WX; ++k) o[k] = fmaf(xv[k] - mv[k], a[k], b[k]);
      drop_apply<WX>(o, m, dk.scale);
      if (FORM == 1) {
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

// backward statistics: bn_colsum_act_kernel with the mask — z = drop(fmaf(x - mean, float(gamma * invstd), beta)), plus
// `skip` when given (SUM); g = dy * act'(z) goes to gout when given (SUM: d skip, NOT masked); the two column sums take
// drop(g), the gradient into the BatchNorm.  PRELU's third sum, dy * min(z, 0), is over the masked z.
template <int W, int ACT>
__global__ __launch_bounds__(kBlock) void bn_drop_colsum_kernel(const float* __restrict__ x, int64_t ldx,
                                                                const float* __restrict__ dy, int64_t lddy,
                                                                const float* __restrict__ skip, int64_t ldskip,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ gamma,
                                                                const float* __restrict__ beta,
                                                                const float* __restrict__ invstd, float prm,
                                                                const float* __restrict__ slope,
                                                                const float* __restrict__ mean_lo, DropKey dk,
                                                                int64_t N, int32_t d, int64_t rows_per_block,
                                                                float* __restrict__ partial,
                                                                float* __restrict__ partial3, float* __restrict__ gout,
                                                                int64_t ldg) {
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
      if constexpr (act_smooth<ACT>()) load_vec<W>(mean_lo + c0, ml);
#pragma unroll
      for (int k = 0; k < W; ++k)
        if (c0 + k < d) {
          sc[k] = bn_scale(gamma ? gamma[c0 + k] : 1.f, invstd[c0 + k]);
          bt[k] = beta ? beta[c0 + k] : 0.f;
        }
      for (int64_t r = r0 + rli; r < r1; r += g.rl) {
        float xv[W], gv[W], z[W], zs[W];
        bool m[W];
        load_vec<W>(x + r * ldx + c0, xv);
        load_vec<W>(dy + r * lddy + c0, gv);
        drop_keep<W>(dk, r, c0, m);
#pragma unroll
        for (int k = 0; k < W; ++k) {
          xv[k] -= pv[k];
          z[k] = fmaf(xv[k], sc[k], bt[k]);
          zs[k] = act_smooth<ACT>() ? fmaf(xv[k] - ml[k], sc[k], bt[k]) : 0.f;
        }
        drop_apply<W>(z, m, dk.scale);
        if constexpr (act_smooth<ACT>()) drop_apply<W>(zs, m, dk.scale);
        if (skip != nullptr) {
          float sv[W];
          load_vec<W>(skip + r * ldskip + c0, sv);
#pragma unroll
          for (int k = 0; k < W; ++k) { z[k] = sv[k] + z[k]; zs[k] = sv[k] + zs[k]; }
        }
#pragma unroll
        for (int k = 0; k < W; ++k) {
          if (ACT == MP_ACT_PRELU) c3 = fmaf(gv[k], act_dslope(z[k]), c3);
          gv[k] = act_bwd_at<ACT>(gv[k], z[k], zs[k], ap);
        }
        if (gout != nullptr) store_vec<W>(gout + r * ldg + c0, gv);
#pragma unroll
        for (int k = 0; k < W; ++k) {
          float hi, lo;
          drop_pair(gv[k], m[k], dk.scale, hi, lo);
          two_sum(a[k], al[k], hi);
          al[k] += lo;
          const float pr = __fmul_rn(hi, xv[k]);
          two_sum(b[k], bl[k], pr);
          bl[k] += fmaf(hi, xv[k], -pr) + lo * xv[k];
        }
      }
    }
    bn_colsum_store2<W>(a, al, b, bl, g, cgi, rli, on, c0, d, (int)gridDim.x, partial);
  }
  if (ACT == MP_ACT_PRELU) bn_block_sum(c3, partial3 + blockIdx.x);
}

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

// backward apply: dx = A drop(g) + B (x - mean) + C with g = dy * act'(z) recomputed as in bn_drop_colsum_kernel
template <int W, int ACT>
__global__ __launch_bounds__(kBlock) void bn_drop_apply_bwd_kernel(const float* __restrict__ x, int64_t ldx,
                                                                   const float* __restrict__ dy, int64_t lddy,
                                                                   const float* __restrict__ skip, int64_t ldskip,
                                                                   const double* __restrict__ A,
                                                                   const double* __restrict__ B,
                                                                   const double* __restrict__ Cc,
                                                                   const float* __restrict__ mean,
                                                                   const float* __restrict__ fwd_scale,
                                                                   const float* __restrict__ beta, float prm,
                                                                   const float* __restrict__ slope,
                                                                   const float* __restrict__ mean_lo, DropKey dk,
                                                                   int64_t N, int32_t d, float* __restrict__ out,
                                                                   int64_t ldo) {
  const float ap = act_param<ACT>(prm, slope);
  const int groups = (d + W - 1) / W;
  const int64_t total = N * groups;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / groups;
    const int c0 = (int)(i - r * groups) * W;
    float xv[W], o[W], mv[W], gv[W], sck[W], btk[W], z[W], zs[W], ml[W];
    bool m[W];
#pragma unroll
    for (int k = 0; k < W; ++k) ml[k] = 0.f;
    if constexpr (act_smooth<ACT>()) load_vec<W>(mean_lo + c0, ml);
    load_vec<W>(x + r * ldx + c0, xv);
    load_vec<W>(dy + r * lddy + c0, gv);
    load_vec<W>(mean + c0, mv);
    load_vec<W>(fwd_scale + c0, sck);
#pragma unroll
    for (int k = 0; k < W; ++k) btk[k] = 0.f;
    if (beta != nullptr) load_vec<W>(beta + c0, btk);
    drop_keep<W>(dk, r, c0, m);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      xv[k] -= mv[k];
      z[k] = fmaf(xv[k], sck[k], btk[k]);
      zs[k] = act_smooth<ACT>() ? fmaf(xv[k] - ml[k], sck[k], btk[k]) : 0.f;
    }
    drop_apply<W>(z, m, dk.scale);
    if constexpr (act_smooth<ACT>()) drop_apply<W>(zs, m, dk.scale);
    if (skip != nullptr) {
      float sv[W];
      load_vec<W>(skip + r * ldskip + c0, sv);
#pragma unroll
      for (int k = 0; k < W; ++k) { z[k] = sv[k] + z[k]; zs[k] = sv[k] + zs[k]; }
    }
#pragma unroll
    for (int k = 0; k < W; ++k) {
      float hi, lo;
      drop_pair(act_bwd_at<ACT>(gv[k], z[k], zs[k], ap), m[k], dk.scale, hi, lo);
      o[k] = drop_dx(A[c0 + k], B[c0 + k], Cc[c0 + k], hi, lo, xv[k]);
    }
    store_vec<W>(out + r * ldo + c0, o);
  }
}

// the same with g on hand (SUM: the statistics pass wrote d skip = g): dx = A drop(g) + B (x - mean) + C
template <int W>
__global__ __launch_bounds__(kBlock) void bn_drop_apply_bwd_g_kernel(const float* __restrict__ x, int64_t ldx,
                                                                     const float* __restrict__ g, int64_t ldg,
                                                                     const double* __restrict__ A,
                                                                     const double* __restrict__ B,
                                                                     const double* __restrict__ Cc,
                                                                     const float* __restrict__ mean, DropKey dk,
                                                                     int64_t N, int32_t d, float* __restrict__ out,
                                                                     int64_t ldo) {
  const int groups = (d + W - 1) / W;
  const int64_t total = N * groups;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / groups;
    const int c0 = (int)(i - r * groups) * W;
    float xv[W], o[W], mv[W], gv[W];
    bool m[W];
    load_vec<W>(x + r * ldx + c0, xv);
    load_vec<W>(g + r * ldg + c0, gv);
    load_vec<W>(mean + c0, mv);
    drop_keep<W>(dk, r, c0, m);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      float hi, lo;
      drop_pair(gv[k], m[k], dk.scale, hi, lo);
      o[k] = drop_dx(A[c0 + k], B[c0 + k], Cc[c0 + k], hi, lo, xv[k] - mv[k]);
    }
    store_vec<W>(out + r * ldo + c0, o);
  }
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

// T in [0, 65536] -> the call's key, threshold and scale; false for a T outside the range
static bool drop_make(int32_t T, uint64_t seed, uint64_t offset, int32_t d, DropKey* k) {
  if (T < 0 || T > 65536) return false;
  k->key = drop_key(seed, offset);
  k->T = (uint32_t)T;
  k->scale = T == 65536 ? 0.f : (float)(65536.0 / (double)(65536 - T));
  k->q = (d + 3) / 4;
  return true;
}

// with_act plus MP_ACT_NONE: here a layer without activation has kernels of its own (the mask is still applied)
template <class Fn>
static inline void with_act_or_none(int act, Fn&& f) {
  if (act == MP_ACT_NONE) f(std::integral_constant<int, MP_ACT_NONE>{});
  else with_act(act, f);
}

// statistics, finalize and apply of the masked backward; gout != NULL: the statistics pass writes g there and the apply
// pass reads it back (7 N d).  PRELU leaves its per-workgroup sums in L.partial3[0 .. bn_blocks(N)).
template <int ACT>
static int bn_drop_bwd_launch(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* skip,
                              int64_t ldskip, int64_t N, int32_t d, const float* gamma, const float* beta,
                              const float* mean, const float* invstd, float prm, const float* slope, const DropKey& dk,
                              float* dx, int64_t lddx, float* gout, int64_t ldg, float* dgamma, float* dbeta,
                              const DropWs& Wk, hipStream_t st) {
  const BnActWs& L = Wk.act;
  const int nblk = bn_blocks(N);
  const int64_t rpb = ceil_div(N, nblk);
  const bool vec = d % 4 == 0 && ldx % 4 == 0 && lddy % 4 == 0 && lddx % 4 == 0 && bn_al(x, 16) && bn_al(dy, 16) &&
                   bn_al(dx, 16) && bn_al(beta, 16) && bn_al(mean, 16) && ldskip % 4 == 0 && bn_al(skip, 16) &&
                   ldg % 4 == 0 && bn_al(gout, 16);
  const BnWs& B = L.bn;
  const float* mean_lo = nullptr;
  if constexpr (act_smooth<ACT>()) {      // the residue of the fp32 mean, into B.v[4] (the slabs are reused below)
    if (vec)
      hipLaunchKernelGGL((bn_drop_mean_lo_kernel<4>), dim3(nblk), dim3(kBlock), 0, st, x, ldx, mean, N, d, rpb, B.partial);
    else
      hipLaunchKernelGGL((bn_drop_mean_lo_kernel<1>), dim3(nblk), dim3(kBlock), 0, st, x, ldx, mean, N, d, rpb, B.partial);
    MP_LAUNCH_CHECK();
    hipLaunchKernelGGL(bn_drop_mean_lo_finalize_kernel, dim3((unsigned)ceil_div(d, 16)), dim3(kBlock), 0, st, B.partial,
                       2 * nblk, N, d, B.v[4]);
    MP_LAUNCH_CHECK();
    mean_lo = B.v[4];
  }
  if (vec)
    hipLaunchKernelGGL((bn_drop_colsum_kernel<4, ACT>), dim3(nblk), dim3(kBlock), 0, st, x, ldx, dy, lddy, skip, ldskip,
                       mean, gamma, beta, invstd, prm, slope, mean_lo, dk, N, d, rpb, B.partial, L.partial3, gout, ldg);
  else
    hipLaunchKernelGGL((bn_drop_colsum_kernel<1, ACT>), dim3(nblk), dim3(kBlock), 0, st, x, ldx, dy, lddy, skip, ldskip,
                       mean, gamma, beta, invstd, prm, slope, mean_lo, dk, N, d, rpb, B.partial, L.partial3, gout, ldg);
  MP_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_drop_bwd_finalize_kernel, dim3((unsigned)ceil_div(d, 16)), dim3(kBlock), 0, st, B.partial,
                     2 * nblk, N, d, gamma, invstd, dgamma, dbeta, Wk.c[0], Wk.c[1], Wk.c[2], B.v[3]);      // sums and residues
  MP_LAUNCH_CHECK();
  if (gout != nullptr) {      // g is on hand
    if (vec)
      hipLaunchKernelGGL((bn_drop_apply_bwd_g_kernel<4>), dim3(flat_grid(N * (d / 4))), dim3(kBlock), 0, st, x, ldx, gout,
                         ldg, Wk.c[0], Wk.c[1], Wk.c[2], mean, dk, N, d, dx, lddx);
    else
      hipLaunchKernelGGL((bn_drop_apply_bwd_g_kernel<1>), dim3(flat_grid(N * d)), dim3(kBlock), 0, st, x, ldx, gout, ldg,
                         Wk.c[0], Wk.c[1], Wk.c[2], mean, dk, N, d, dx, lddx);
  } else if (vec) {
    hipLaunchKernelGGL((bn_drop_apply_bwd_kernel<4, ACT>), dim3(flat_grid(N * (d / 4))), dim3(kBlock), 0, st, x, ldx, dy,
                       lddy, skip, ldskip, Wk.c[0], Wk.c[1], Wk.c[2], mean, B.v[3], beta, prm, slope, mean_lo, dk, N, d, dx, lddx);
  } else {
    hipLaunchKernelGGL((bn_drop_apply_bwd_kernel<1, ACT>), dim3(flat_grid(N * d)), dim3(kBlock), 0, st, x, ldx, dy, lddy,
                       skip, ldskip, Wk.c[0], Wk.c[1], Wk.c[2], mean, B.v[3], beta, prm, slope, mean_lo, dk, N, d, dx, lddx);
  }
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // namespace mp

using namespace mp;

extern "C" {

int mp_bn_drop_ws_bytes(int64_t N, int32_t d, size_t* bytes_host) {
  if (!bytes_host || N < 0 || d <= 0) return MP_ERR_INVALID_ARG;
  DropWs w;
  drop_ws_layout(N, d, nullptr, &w);
  *bytes_host = w.total;
  return MP_OK;
}

int mp_dropout_keyed_f32(const float* x, int64_t ldx, int64_t N, int32_t d, int32_t T, uint64_t seed, uint64_t offset,
                         float* out, int64_t ldo, mp_stream_t stream) {
  DropKey dk;
  if (N <= 0 || d <= 0 || !x || !out || ldx < d || ldo < d || !drop_make(T, seed, offset, d, &dk))
    return MP_ERR_INVALID_ARG;
  hipStream_t st = as_stream(stream);
  const bool vec = d % 4 == 0 && ldx % 4 == 0 && ldo % 4 == 0 && bn_al(x, 16) && bn_al(out, 16);
  if (vec)
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
  DropKey dk;
  if (!act_known(act) || (act == MP_ACT_PRELU && !slope)) return MP_ERR_INVALID_ARG;
  if (N <= 0 || d <= 0 || !x || !y || !mean || !invstd || !var_unbiased || ldx < d || ldy < d) return MP_ERR_INVALID_ARG;
  if (!drop_make(T, seed, offset, d, &dk)) return MP_ERR_INVALID_ARG;
  DropWs Wk;
  drop_ws_layout(N, d, ws, &Wk);
  if (!ws || ws_bytes < Wk.total) return MP_ERR_WORKSPACE;
  const BnActWs& L = Wk.act;
  hipStream_t st = as_stream(stream);
  const bool vec = d % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && bn_al(x, 16) && bn_al(y, 16) && bn_al(mean, 16);
  const int rc = bn_fwd_stats(x, ldx, N, d, gamma, beta, eps, mean, invstd, var_unbiased, L.bn, vec, st);
  if (rc != MP_OK) return rc;
  with_act_or_none(act, [&](auto a) {
    constexpr int A = decltype(a)::value;
    if (vec)
      hipLaunchKernelGGL((bn_drop_apply_kernel<4, 4, 0, A>), dim3(flat_grid(N * (d / 4))), dim3(kBlock), 0, st, x, ldx,
                         nullptr, 0, L.bn.v[0], L.bn.v[1], mean, act_param, slope, dk, N, d, 0, y, ldy);
    else
      hipLaunchKernelGGL((bn_drop_apply_kernel<1, 1, 0, A>), dim3(flat_grid(N * d)), dim3(kBlock), 0, st, x, ldx,
                         nullptr, 0, L.bn.v[0], L.bn.v[1], mean, act_param, slope, dk, N, d, 0, y, ldy);
  });
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_bn_train_bwd_drop_act_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t N, int32_t d,
                                 const float* gamma, const float* beta, const float* mean, const float* invstd,
                                 int act, float act_param, const float* slope, int32_t T, uint64_t seed,
                                 uint64_t offset, float* dx, int64_t lddx, float* dgamma, float* dbeta, float* dslope,
                                 void* ws, size_t ws_bytes, mp_stream_t stream) {
  DropKey dk;
  if (!act_known(act) || (act == MP_ACT_PRELU && !slope)) return MP_ERR_INVALID_ARG;
  if (N <= 0 || d <= 0 || !dy || !x || !mean || !invstd || !dx || lddy < d || ldx < d || lddx < d)
    return MP_ERR_INVALID_ARG;
  if (!drop_make(T, seed, offset, d, &dk)) return MP_ERR_INVALID_ARG;
  DropWs Wk;
  drop_ws_layout(N, d, ws, &Wk);
  if (!ws || ws_bytes < Wk.total) return MP_ERR_WORKSPACE;
  const BnActWs& L = Wk.act;
  hipStream_t st = as_stream(stream);
  int rc = MP_OK;
  with_act_or_none(act, [&](auto a) {
    rc = bn_drop_bwd_launch<decltype(a)::value>(dy, lddy, x, ldx, nullptr, 0, N, d, gamma, beta, mean, invstd,
                                                act_param, slope, dk, dx, lddx, nullptr, 0, dgamma, dbeta, Wk, st);
  });
  if (rc != MP_OK) return rc;
  if (act == MP_ACT_PRELU && dslope) return bn_dslope_finalize(L, bn_blocks(N), dslope, st);
  return MP_OK;
}

int mp_bn_train_fwd_drop_skip_act_f32(const float* x, int64_t ldx, const float* skip, int64_t ldskip, int64_t N,
                                      int32_t d, int32_t d_skip, int mode, const float* gamma, const float* beta,
                                      float eps, int act, float act_param, const float* slope, int32_t T,
                                      uint64_t seed, uint64_t offset, float* out, int64_t ldo, float* mean,
                                      float* invstd, float* var_unbiased, void* ws, size_t ws_bytes,
                                      mp_stream_t stream) {
  DropKey dk;
  if (!act_known(act) || (act == MP_ACT_PRELU && !slope)) return MP_ERR_INVALID_ARG;
  if (N <= 0 || d <= 0 || d_skip <= 0 || !x || !skip || !out || !mean || !invstd || !var_unbiased || ldx < d ||
      ldskip < d_skip)
    return MP_ERR_INVALID_ARG;
  if (mode != MP_BN_SKIP_SUM && mode != MP_BN_SKIP_CONCAT) return MP_ERR_INVALID_ARG;
  if (mode == MP_BN_SKIP_SUM && d_skip != d) return MP_ERR_INVALID_ARG;
  const bool cat = mode == MP_BN_SKIP_CONCAT;
  if (ldo < (cat ? (int64_t)d_skip + d : (int64_t)d)) return MP_ERR_INVALID_ARG;
  if (!drop_make(T, seed, offset, d, &dk)) return MP_ERR_INVALID_ARG;
  DropWs Wk;
  drop_ws_layout(N, d, ws, &Wk);
  if (!ws || ws_bytes < Wk.total) return MP_ERR_WORKSPACE;
  const BnActWs& L = Wk.act;
  hipStream_t st = as_stream(stream);
  // the vector forms of mp_bn_train_fwd_skip_f32
  const bool vx = d % 4 == 0 && ldx % 4 == 0 && bn_al(x, 16) && bn_al(mean, 16);
  const bool vo = ldo % 4 == 0 && bn_al(out, 16);
  const bool vs = d_skip % 4 == 0 && ldskip % 4 == 0 && bn_al(skip, 16) && vo;
  const int rc = bn_fwd_stats(x, ldx, N, d, gamma, beta, eps, mean, invstd, var_unbiased, L.bn, vx, st);
  if (rc != MP_OK) return rc;
#define MP_BN_DROP_LAUNCH(WS, WX, FORM)                                                                                \
  hipLaunchKernelGGL((bn_drop_apply_kernel<WS, WX, FORM, A>),                                                          \
                     dim3(flat_grid(N * ((FORM == 2 ? (int64_t)d_skip / WS : 0) + (int64_t)d / WX))), dim3(kBlock), 0, \
                     st, x, ldx, skip, ldskip, L.bn.v[0], L.bn.v[1], mean, act_param, slope, dk, N, d, d_skip, out, ldo)
  with_act_or_none(act, [&](auto a) {
    constexpr int A = decltype(a)::value;
    if (!cat) {
      if (vx && vs) MP_BN_DROP_LAUNCH(4, 4, 1);
      else MP_BN_DROP_LAUNCH(1, 1, 1);
    } else {
      const bool vr = vx && vo && d_skip % 4 == 0;      // the right slab starts at out + d_skip
      if (vs && vr) MP_BN_DROP_LAUNCH(4, 4, 2);
      else if (vs) MP_BN_DROP_LAUNCH(4, 1, 2);
      else if (vr) MP_BN_DROP_LAUNCH(1, 4, 2);
      else MP_BN_DROP_LAUNCH(1, 1, 2);
    }
  });
#undef MP_BN_DROP_LAUNCH
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_bn_train_bwd_drop_skip_act_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* skip,
                                      int64_t ldskip, int64_t N, int32_t d, int32_t d_skip, int mode,
                                      const float* gamma, const float* beta, const float* mean, const float* invstd,
                                      int act, float act_param, const float* slope, int32_t T, uint64_t seed,
                                      uint64_t offset, float* dx, int64_t lddx, float* dskip, int64_t lddskip,
                                      float* dgamma, float* dbeta, float* dslope, void* ws, size_t ws_bytes,
                                      mp_stream_t stream) {
  DropKey dk;
  if (!act_known(act) || (act == MP_ACT_PRELU && !slope)) return MP_ERR_INVALID_ARG;
  if (mode != MP_BN_SKIP_SUM && mode != MP_BN_SKIP_CONCAT) return MP_ERR_INVALID_ARG;
  const bool cat = mode == MP_BN_SKIP_CONCAT;
  if (N <= 0 || d <= 0 || d_skip <= 0 || (!cat && d_skip != d) || !dy || !x || !skip || !mean || !invstd || !dx ||
      lddy < (cat ? (int64_t)d_skip + d : (int64_t)d) || ldx < d || ldskip < d_skip || lddx < d ||
      (dskip && lddskip < d_skip))
    return MP_ERR_INVALID_ARG;
  if (!drop_make(T, seed, offset, d, &dk)) return MP_ERR_INVALID_ARG;
  DropWs Wk;
  drop_ws_layout(N, d, ws, &Wk);
  if (!ws || ws_bytes < Wk.total) return MP_ERR_WORKSPACE;
  const BnActWs& L = Wk.act;
  hipStream_t st = as_stream(stream);
  const float* dyr = cat ? dy + d_skip : dy;      // the BN slab of dy
  const bool none = act == MP_ACT_NONE;           // d(skip) is dy (its left slab) itself: dskip is not written
  const bool sum = !cat && !none;                 // the pre-activation holds skip
  float* gout = sum ? dskip : nullptr;
  int rc = MP_OK;
  with_act_or_none(act, [&](auto a) {
    rc = bn_drop_bwd_launch<decltype(a)::value>(dyr, lddy, x, ldx, sum ? skip : nullptr, sum ? ldskip : 0, N, d, gamma,
                                                beta, mean, invstd, act_param, slope, dk, dx, lddx, gout,
                                                gout ? lddskip : 0, dgamma, dbeta, Wk, st);
  });
  if (rc != MP_OK) return rc;
  const int nblk = bn_blocks(N);
  if (cat && !none && (dskip || (act == MP_ACT_PRELU && dslope))) {      // the left slab never sees the mask
    rc = bn_act_bwd_left(act, dy, lddy, skip, ldskip, act_param, slope, N, d_skip, dskip, lddskip, L, st);
    if (rc != MP_OK) return rc;
  }
  if (act == MP_ACT_PRELU && dslope) return bn_dslope_finalize(L, cat ? 2 * nblk : nblk, dslope, st);
  return MP_OK;
}

}  // extern "C"
