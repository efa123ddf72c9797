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
#include "bn_shared.h"

namespace mp {

// MODE 0: a = sum(x - pivot), b = sum((x - pivot)^2)          (forward statistics; pivot = bn_pivot(x))
// MODE 1: a = sum(g),         b = sum(g * (x - pivot)),  g = dy * [y > 0] when y != nullptr, pivot = mean
// MODE 2: MODE 1 with y given, and g written to gout on the way: the skip block's d(skip), which its apply pass then
//         reads in place of dy and y
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

template <int W, int MODE>
__global__ __launch_bounds__(kBlock) void bn_colsum_kernel(const float* __restrict__ x, int64_t ldx,
                                                           const float* __restrict__ dy, int64_t lddy,
                                                           const float* __restrict__ y, int64_t ldy,
                                                           const float* __restrict__ pivot, int64_t N, int32_t d,
                                                           int64_t rows_per_block, float* __restrict__ partial,
                                                           const float* __restrict__ mx_gamma = nullptr,
                                                           const float* __restrict__ mx_beta = nullptr,
                                                           const float* __restrict__ mx_invstd = nullptr,
                                                           float* __restrict__ gout = nullptr, int64_t ldg = 0) {
  // mx_invstd != NULL (MODE 1): the ReLU mask [y > 0] is recomputed from x — y = relu(fmaf(x - mean, scale, beta))
  // with scale = float(gamma * invstd), the forward's own expression on the forward's own operands, bit for bit —
  // instead of reading y
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
      if (MODE == 0) bn_pivot<W>(x, ldx, N, c0, pv);      // `pivot` is not read
      else load_vec<W>(pivot + c0, pv);
    }
    float sc[W], bt[W];
#pragma unroll
    for (int k = 0; k < W; ++k) { sc[k] = 0.f; bt[k] = 0.f; }
    if (MODE != 0 && mx_invstd != nullptr && on) {
#pragma unroll
      for (int k = 0; k < W; ++k)
        if (c0 + k < d) {
          sc[k] = bn_scale(mx_gamma ? mx_gamma[c0 + k] : 1.f, mx_invstd[c0 + k]);
          bt[k] = mx_beta ? mx_beta[c0 + k] : 0.f;
        }
    }
    if (on) {
      for (int64_t r = r0 + rli; r < r1; r += g.rl) {
        float xv[W];
        load_vec<W>(x + r * ldx + c0, xv);
        if (MODE == 0) {
#pragma unroll
          for (int k = 0; k < W; ++k) {
            const float v = xv[k] - pv[k];
            a[k] += v;
            b[k] = fmaf(v, v, b[k]);
          }
        } else {
          float gv[W];
          load_vec<W>(dy + r * lddy + c0, gv);
          if (mx_invstd != nullptr) {
#pragma unroll
            for (int k = 0; k < W; ++k) gv[k] = fmaf(xv[k] - pv[k], sc[k], bt[k]) > 0.f ? gv[k] : 0.f;
          } else if (y != nullptr) {
            float yv[W];
            load_vec<W>(y + r * ldy + c0, yv);
#pragma unroll
            for (int k = 0; k < W; ++k) gv[k] = yv[k] > 0.f ? gv[k] : 0.f;
          }
          if (MODE == 2) store_vec<W>(gout + r * ldg + c0, gv);
#pragma unroll
          for (int k = 0; k < W; ++k) {
            a[k] += gv[k];
            b[k] = fmaf(gv[k], xv[k] - pv[k], b[k]);
          }
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

// backward finalize: dgamma, dbeta and the constants of dx = A g + B x + C
__global__ __launch_bounds__(kBlock) void bn_bwd_finalize_kernel(const float* __restrict__ partial, int nblk,
                                                                 int64_t N, int32_t d,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ mean,
                                                                 const float* __restrict__ invstd, float* dgamma,
                                                                 float* dbeta, float* A, float* B, float* Cc,
                                                                 float* fwd_scale) {
  int c;
  double sg, sgx;
  if (!bn_col_sums(partial, nblk, d, c, sg, sgx)) return;
  const double m = mean[c], istd = invstd[c];
  const double gm = gamma ? (double)gamma[c] : 1.0;
  const double dgam = sgx * istd;                       // sum g * xhat (the sums were taken against the mean)
  (void)m;
  if (dgamma) dgamma[c] = (float)dgam;
  if (dbeta) dbeta[c] = (float)sg;
  const double a = gm * istd;
  const double bb = -gm * istd * istd * dgam / (double)N;
  A[c] = (float)a;
  B[c] = (float)bb;
  Cc[c] = (float)(-a * sg / (double)N);                 // dx = A g + B (x - mean) + C
  if (fwd_scale != nullptr) fwd_scale[c] = bn_scale(gamma ? gamma[c] : 1.f, invstd[c]);   // for the recomputed ReLU mask
}

// MODE 0: out = act((x - ctr) * p0 + p1)        MODE 1: out = p0 * g + p1 * (x - ctr) + p2,  g = dy * [y > 0]
template <int W, int MODE>
__global__ __launch_bounds__(kBlock) void bn_apply_kernel(const float* __restrict__ x, int64_t ldx,
                                                          const float* __restrict__ dy, int64_t lddy,
                                                          const float* __restrict__ y, int64_t ldy,
                                                          const float* __restrict__ p0, const float* __restrict__ p1,
                                                          const float* __restrict__ p2,
                                                          const float* __restrict__ ctr, int relu, int64_t N,
                                                          int32_t d, float* __restrict__ out, int64_t ldo,
                                                          const float* __restrict__ mx_scale = nullptr,
                                                          const float* __restrict__ mx_beta = nullptr) {
  const int groups = (d + W - 1) / W;
  const int64_t total = N * groups;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / groups;
    const int c0 = (int)(i - r * groups) * W;
    float xv[W], a[W], b[W], o[W], mv[W];
    load_vec<W>(x + r * ldx + c0, xv);
    load_vec<W>(p0 + c0, a);
    load_vec<W>(p1 + c0, b);
    load_vec<W>(ctr + c0, mv);
#pragma unroll
    for (int k = 0; k < W; ++k) xv[k] -= mv[k];
    if (MODE == 0) {
#pragma unroll
      for (int k = 0; k < W; ++k) {
        o[k] = fmaf(xv[k], a[k], b[k]);
        if (relu) o[k] = fmaxf(o[k], 0.f);
      }
    } else {
      float gv[W], cv[W];
      load_vec<W>(dy + r * lddy + c0, gv);
      load_vec<W>(p2 + c0, cv);
      if (mx_scale != nullptr) {      // the forward's activation, recomputed (see bn_colsum_kernel); the scale
        float sck[W], btk[W];         // vector was rebuilt by the finalize kernel
        load_vec<W>(mx_scale + c0, sck);
#pragma unroll
        for (int k = 0; k < W; ++k) btk[k] = 0.f;
        if (mx_beta != nullptr) load_vec<W>(mx_beta + c0, btk);
#pragma unroll
        for (int k = 0; k < W; ++k) gv[k] = fmaf(xv[k], sck[k], btk[k]) > 0.f ? gv[k] : 0.f;
      } else if (y != nullptr) {
        float yv[W];
        load_vec<W>(y + r * ldy + c0, yv);
#pragma unroll
        for (int k = 0; k < W; ++k) gv[k] = yv[k] > 0.f ? gv[k] : 0.f;
      }
#pragma unroll
      for (int k = 0; k < W; ++k) o[k] = fmaf(a[k], gv[k], fmaf(b[k], xv[k], cv[k]));
    }
    store_vec<W>(out + r * ldo + c0, o);
  }
}

// The skip block's apply pass (graphgym/models/gnn.py:49-60 behind a last layer without activation), one launch:
//   SUM    (CONCAT = false, d_skip == d): out = act(skip + ((x - ctr) * p0 + p1))
//   CONCAT                              : out[:, :d_skip] = act(skip), out[:, d_skip:] = act((x - ctr) * p0 + p1)
// The BN term is bn_apply_kernel<W, 0>'s own fmaf.  WS / WX: vector widths of the skip slab and of the BN slab (equal in
// SUM); a row is d_skip / WS + d / WX work items.
template <int WS, int WX, bool CONCAT>
__global__ __launch_bounds__(kBlock) void bn_apply_skip_kernel(const float* __restrict__ x, int64_t ldx,
                                                               const float* __restrict__ skip, int64_t ldskip,
                                                               const float* __restrict__ p0,
                                                               const float* __restrict__ p1,
                                                               const float* __restrict__ ctr, int relu, int64_t N,
                                                               int32_t d, int32_t d_skip, float* __restrict__ out,
                                                               int64_t ldo) {
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
      if (relu) {
#pragma unroll
        for (int k = 0; k < WS; ++k) sv[k] = fmaxf(sv[k], 0.f);
      }
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
      if (!CONCAT) {
        float sv[WX];
        load_vec<WX>(skip + r * ldskip + c0, sv);
#pragma unroll
        for (int k = 0; k < WX; ++k) o[k] = sv[k] + o[k];
      }
      if (relu) {
#pragma unroll
        for (int k = 0; k < WX; ++k) o[k] = fmaxf(o[k], 0.f);
      }
      store_vec<WX>(out + r * ldo + (CONCAT ? d_skip : 0) + c0, o);
    }
  }
}

// ---- the same passes with any activation of act.h ----------------------------------------------------------------------
// (act_param<ACT>: bn_shared.h)
// forward apply: out = act((x - ctr) * p0 + p1), bn_apply_kernel<W, 0>'s fmaf
template <int W, int ACT>
__global__ __launch_bounds__(kBlock) void bn_apply_act_kernel(const float* __restrict__ x, int64_t ldx,
                                                              const float* __restrict__ p0,
                                                              const float* __restrict__ p1,
                                                              const float* __restrict__ ctr, float prm,
                                                              const float* __restrict__ slope, int64_t N, int32_t d,
                                                              float* __restrict__ out, int64_t ldo) {
  const float ap = act_param<ACT>(prm, slope);
  const int groups = (d + W - 1) / W;
  const int64_t total = N * groups;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / groups;
    const int c0 = (int)(i - r * groups) * W;
    float xv[W], a[W], b[W], o[W], mv[W];
    load_vec<W>(x + r * ldx + c0, xv);
    load_vec<W>(p0 + c0, a);
    load_vec<W>(p1 + c0, b);
    load_vec<W>(ctr + c0, mv);
#pragma unroll
    for (int k = 0; k < W; ++k) o[k] = act_fwd<ACT>(fmaf(xv[k] - mv[k], a[k], b[k]), ap);
    store_vec<W>(out + r * ldo + c0, o);
  }
}

// bn_apply_skip_kernel with act_fwd<ACT> in place of the ReLU
template <int WS, int WX, bool CONCAT, int ACT>
__global__ __launch_bounds__(kBlock) void bn_apply_skip_act_kernel(const float* __restrict__ x, int64_t ldx,
                                                                   const float* __restrict__ skip, int64_t ldskip,
                                                                   const float* __restrict__ p0,
                                                                   const float* __restrict__ p1,
                                                                   const float* __restrict__ ctr, float prm,
                                                                   const float* __restrict__ slope, int64_t N,
                                                                   int32_t d, int32_t d_skip, float* __restrict__ out,
                                                                   int64_t ldo) {
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
      if (!CONCAT) {
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

// backward statistics: bn_colsum_kernel's MODE 1 / 2 with the pre-activation recomputed from x — z = fmaf(x - mean,
// float(gamma * invstd), beta), the forward's own expression, plus `skip` when given (the SUM skip block) — and
// g = dy * act'(z); g goes to gout when given (SUM: d skip).  The two column sums and their partial slabs are
// bn_colsum_kernel's.  PRELU carries a third sum, dy * min(z, 0) (d out / d slope), over the workgroup's rows AND
// columns: one value per workgroup in partial3, added in thread order.
template <int W, int ACT>
__global__ __launch_bounds__(kBlock) void bn_colsum_act_kernel(const float* __restrict__ x, int64_t ldx,
                                                               const float* __restrict__ dy, int64_t lddy,
                                                               const float* __restrict__ skip, int64_t ldskip,
                                                               const float* __restrict__ mean,
                                                               const float* __restrict__ gamma,
                                                               const float* __restrict__ beta,
                                                               const float* __restrict__ invstd, float prm,
                                                               const float* __restrict__ slope, int64_t N, int32_t d,
                                                               int64_t rows_per_block, float* __restrict__ partial,
                                                               float* __restrict__ partial3,
                                                               float* __restrict__ gout, int64_t ldg) {
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
    float a[W], b[W], pv[W], sc[W], bt[W];
#pragma unroll
    for (int k = 0; k < W; ++k) { a[k] = 0.f; b[k] = 0.f; pv[k] = 0.f; sc[k] = 0.f; bt[k] = 0.f; }
    if (on) {
      load_vec<W>(mean + c0, pv);
#pragma unroll
      for (int k = 0; k < W; ++k)
        if (c0 + k < d) {
          sc[k] = bn_scale(gamma ? gamma[c0 + k] : 1.f, invstd[c0 + k]);
          bt[k] = beta ? beta[c0 + k] : 0.f;
        }
      for (int64_t r = r0 + rli; r < r1; r += g.rl) {
        float xv[W], gv[W], z[W];
        load_vec<W>(x + r * ldx + c0, xv);
        load_vec<W>(dy + r * lddy + c0, gv);
#pragma unroll
        for (int k = 0; k < W; ++k) z[k] = fmaf(xv[k] - pv[k], sc[k], bt[k]);
        if (skip != nullptr) {
          float sv[W];
          load_vec<W>(skip + r * ldskip + c0, sv);
#pragma unroll
          for (int k = 0; k < W; ++k) z[k] = sv[k] + z[k];
        }
#pragma unroll
        for (int k = 0; k < W; ++k) {
          if (ACT == MP_ACT_PRELU) c3 = fmaf(gv[k], act_dslope(z[k]), c3);
          gv[k] = act_bwd<ACT>(gv[k], z[k], ap);
        }
        if (gout != nullptr) store_vec<W>(gout + r * ldg + c0, gv);
#pragma unroll
        for (int k = 0; k < W; ++k) {
          a[k] += gv[k];
          b[k] = fmaf(gv[k], xv[k] - pv[k], b[k]);
        }
      }
    }
    bn_colsum_store<W>(a, b, g, cgi, rli, on, c0, d, partial);
  }
  if (ACT == MP_ACT_PRELU) bn_block_sum(c3, partial3 + blockIdx.x);
}

// backward apply: dx = A g + B (x - mean) + C with g = dy * act'(z) recomputed as in bn_colsum_act_kernel
template <int W, int ACT>
__global__ __launch_bounds__(kBlock) void bn_apply_bwd_act_kernel(const float* __restrict__ x, int64_t ldx,
                                                                  const float* __restrict__ dy, int64_t lddy,
                                                                  const float* __restrict__ skip, int64_t ldskip,
                                                                  const float* __restrict__ A,
                                                                  const float* __restrict__ B,
                                                                  const float* __restrict__ Cc,
                                                                  const float* __restrict__ mean,
                                                                  const float* __restrict__ fwd_scale,
                                                                  const float* __restrict__ beta, float prm,
                                                                  const float* __restrict__ slope, int64_t N,
                                                                  int32_t d, float* __restrict__ out, int64_t ldo) {
  const float ap = act_param<ACT>(prm, slope);
  const int groups = (d + W - 1) / W;
  const int64_t total = N * groups;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / groups;
    const int c0 = (int)(i - r * groups) * W;
    float xv[W], a[W], b[W], cv[W], o[W], mv[W], gv[W], sck[W], btk[W], z[W];
    load_vec<W>(x + r * ldx + c0, xv);
    load_vec<W>(dy + r * lddy + c0, gv);
    load_vec<W>(A + c0, a);
    load_vec<W>(B + c0, b);
    load_vec<W>(Cc + c0, cv);
    load_vec<W>(mean + c0, mv);
    load_vec<W>(fwd_scale + c0, sck);
#pragma unroll
    for (int k = 0; k < W; ++k) btk[k] = 0.f;
    if (beta != nullptr) load_vec<W>(beta + c0, btk);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      xv[k] -= mv[k];
      z[k] = fmaf(xv[k], sck[k], btk[k]);
    }
    if (skip != nullptr) {
      float sv[W];
      load_vec<W>(skip + r * ldskip + c0, sv);
#pragma unroll
      for (int k = 0; k < W; ++k) z[k] = sv[k] + z[k];
    }
#pragma unroll
    for (int k = 0; k < W; ++k) o[k] = fmaf(a[k], act_bwd<ACT>(gv[k], z[k], ap), fmaf(b[k], xv[k], cv[k]));
    store_vec<W>(out + r * ldo + c0, o);
  }
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

// ---- the launches bn_drop.hip shares (declared in bn_shared.h) ----------------------------------------------------------
int bn_bwd_finalize(int64_t N, int32_t d, const float* gamma, const float* mean, const float* invstd, float* dgamma,
                    float* dbeta, const BnWs& L, int nslab, bool fwd_scale, hipStream_t st) {
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((unsigned)ceil_div(d, 16)), dim3(kBlock), 0, st, L.partial,
                     nslab, N, d, gamma, mean, invstd, dgamma, dbeta, L.v[0], L.v[1], L.v[2],
                     fwd_scale ? L.v[3] : nullptr);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int bn_dslope_finalize(const BnActWs& L, int n, float* dslope, hipStream_t st) {
  hipLaunchKernelGGL(bn_dslope_finalize_kernel, dim3(1), dim3(kBlock), 0, st, L.partial3, n, dslope);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int bn_act_bwd_left(int act, const float* dy, int64_t lddy, const float* skip, int64_t ldskip, float prm,
                    const float* slope, int64_t N, int32_t d_skip, float* dskip, int64_t lddskip, const BnActWs& L,
                    hipStream_t st) {
  const int nblk = bn_blocks(N);
  const int64_t rpb = ceil_div(N, nblk);
  const bool vl = d_skip % 4 == 0 && lddy % 4 == 0 && ldskip % 4 == 0 && bn_al(dy, 16) && bn_al(skip, 16) &&
                  (!dskip || (lddskip % 4 == 0 && bn_al(dskip, 16)));
  const bool known = with_act(act, [&](auto a) {
    constexpr int A = decltype(a)::value;
    if (vl)
      hipLaunchKernelGGL((bn_act_bwd_left_kernel<4, A>), dim3(nblk), dim3(kBlock), 0, st, dy, lddy, skip, ldskip, prm,
                         slope, N, d_skip, rpb, dskip, lddskip, L.partial3 + nblk);
    else
      hipLaunchKernelGGL((bn_act_bwd_left_kernel<1, A>), dim3(nblk), dim3(kBlock), 0, st, dy, lddy, skip, ldskip, prm,
                         slope, N, d_skip, rpb, dskip, lddskip, L.partial3 + nblk);
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
    hipLaunchKernelGGL((bn_colsum_kernel<4, 0>), dim3(nblk), dim3(kBlock), 0, st, x, ldx, nullptr, 0, nullptr, 0, nullptr,
                       N, d, rpb, L.partial);
  else
    hipLaunchKernelGGL((bn_colsum_kernel<1, 0>), dim3(nblk), dim3(kBlock), 0, st, x, ldx, nullptr, 0, nullptr, 0, nullptr,
                       N, d, rpb, L.partial);
  MP_LAUNCH_CHECK();
  hipLaunchKernelGGL(bn_fwd_finalize_kernel, dim3((unsigned)ceil_div(d, 16)), dim3(kBlock), 0, st, L.partial, nblk,
                     x, ldx, N, d, gamma, beta, eps, mean, invstd, var_unbiased, L.v[0], L.v[1]);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // namespace mp

using namespace mp;

extern "C" {

int mp_bn_ws_bytes(int64_t N, int32_t d, size_t* bytes_host) {
  if (!bytes_host || N < 0 || d <= 0) return MP_ERR_INVALID_ARG;
  BnWs w;
  bn_ws_layout(N, d, nullptr, &w);
  *bytes_host = w.total;
  return MP_OK;
}

int mp_bn_train_fwd_f32(const float* x, int64_t ldx, int64_t N, int32_t d, const float* gamma, const float* beta,
                        float eps, int relu, float* y, int64_t ldy, float* mean, float* invstd,
                        float* var_unbiased, void* ws, size_t ws_bytes, mp_stream_t stream) {
  if (N <= 0 || d <= 0 || !x || !y || !mean || !invstd || !var_unbiased || ldx < d || ldy < d) return MP_ERR_INVALID_ARG;
  BnWs L;
  bn_ws_layout(N, d, ws, &L);
  if (!ws || ws_bytes < L.total) return MP_ERR_WORKSPACE;
  hipStream_t st = as_stream(stream);
  const bool vec = d % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && bn_al(x, 16) && bn_al(y, 16);
  const int rc = bn_fwd_stats(x, ldx, N, d, gamma, beta, eps, mean, invstd, var_unbiased, L, vec, st);
  if (rc != MP_OK) return rc;
  if (vec)
    hipLaunchKernelGGL((bn_apply_kernel<4, 0>), dim3(flat_grid(N * (d / 4))), dim3(kBlock), 0, st, x, ldx, nullptr, 0,
                       nullptr, 0, L.v[0], L.v[1], nullptr, mean, relu, N, d, y, ldy);
  else
    hipLaunchKernelGGL((bn_apply_kernel<1, 0>), dim3(flat_grid(N * d)), dim3(kBlock), 0, st, x, ldx, nullptr, 0,
                       nullptr, 0, L.v[0], L.v[1], nullptr, mean, relu, N, d, y, ldy);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_bn_train_fwd_skip_f32(const float* x, int64_t ldx, const float* skip, int64_t ldskip, int64_t N, int32_t d,
                             int32_t d_skip, int mode, const float* gamma, const float* beta, float eps, int relu,
                             float* out, int64_t ldo, float* mean, float* invstd, float* var_unbiased, void* ws,
                             size_t ws_bytes, mp_stream_t stream) {
  if (N <= 0 || d <= 0 || d_skip <= 0 || !x || !skip || !out || !mean || !invstd || !var_unbiased || ldx < d ||
      ldskip < d_skip)
    return MP_ERR_INVALID_ARG;
  if (mode != MP_BN_SKIP_SUM && mode != MP_BN_SKIP_CONCAT) return MP_ERR_INVALID_ARG;
  if (mode == MP_BN_SKIP_SUM && d_skip != d) return MP_ERR_INVALID_ARG;
  const bool cat = mode == MP_BN_SKIP_CONCAT;
  if (ldo < (cat ? (int64_t)d_skip + d : (int64_t)d)) return MP_ERR_INVALID_ARG;
  BnWs L;
  bn_ws_layout(N, d, ws, &L);
  if (!ws || ws_bytes < L.total) return MP_ERR_WORKSPACE;
  hipStream_t st = as_stream(stream);
  // a launch takes its vector form when every pointer it forms is 16-byte aligned: the statistics read x alone; the
  // apply pass writes the BN slab at out (SUM) or out + d_skip (CONCAT) and the skip slab at out
  const bool vx = d % 4 == 0 && ldx % 4 == 0 && bn_al(x, 16);
  const bool vo = ldo % 4 == 0 && bn_al(out, 16);
  const bool vs = d_skip % 4 == 0 && ldskip % 4 == 0 && bn_al(skip, 16) && vo;
  const int rc = bn_fwd_stats(x, ldx, N, d, gamma, beta, eps, mean, invstd, var_unbiased, L, vx, st);
  if (rc != MP_OK) return rc;
#define MP_BN_SKIP_LAUNCH(WS, WX, CAT)                                                                              \
  hipLaunchKernelGGL((bn_apply_skip_kernel<WS, WX, CAT>),                                                           \
                     dim3(flat_grid(N * ((CAT ? (int64_t)d_skip / WS : 0) + (int64_t)d / WX))), dim3(kBlock), 0, st, \
                     x, ldx, skip, ldskip, L.v[0], L.v[1], mean, relu, N, d, d_skip, out, ldo)
  if (!cat) {
    if (vx && vs) MP_BN_SKIP_LAUNCH(4, 4, false);
    else MP_BN_SKIP_LAUNCH(1, 1, false);
  } else {
    const bool vr = vx && vo && d_skip % 4 == 0;      // the right slab starts at out + d_skip
    if (vs && vr) MP_BN_SKIP_LAUNCH(4, 4, true);
    else if (vs) MP_BN_SKIP_LAUNCH(4, 1, true);
    else if (vr) MP_BN_SKIP_LAUNCH(1, 4, true);
    else MP_BN_SKIP_LAUNCH(1, 1, true);
  }
#undef MP_BN_SKIP_LAUNCH
  MP_LAUNCH_CHECK();
  return MP_OK;
}

static int bn_bwd_common(const float* dy, int64_t lddy, const float* y, int64_t ldy, const float* x, int64_t ldx,
                         int64_t N, int32_t d, const float* gamma, const float* beta, int mask_from_x,
                         const float* mean, const float* invstd, float* dx, int64_t lddx, float* dgamma, float* dbeta,
                         void* ws, size_t ws_bytes, hipStream_t st, float* dskip = nullptr, int64_t lddskip = 0) {
  // dskip != NULL (with y): the statistics pass also writes g = dy * [y > 0] there and the apply pass reads it in
  // place of dy and y — same terms, same order, one [N, d] read fewer than masking dy twice and writing g apart
  if (N <= 0 || d <= 0 || !dy || !x || !mean || !invstd || !dx || lddy < d || ldx < d || lddx < d || (y && ldy < d) ||
      (dskip && (!y || mask_from_x || lddskip < d)))
    return MP_ERR_INVALID_ARG;
  BnWs L;
  bn_ws_layout(N, d, ws, &L);
  if (!ws || ws_bytes < L.total) return MP_ERR_WORKSPACE;
  const int nblk = bn_blocks(N);
  const int64_t rpb = ceil_div(N, nblk);
  const bool vec = d % 4 == 0 && ldx % 4 == 0 && lddy % 4 == 0 && lddx % 4 == 0 && (!y || ldy % 4 == 0) &&
                   bn_al(x, 16) && bn_al(dy, 16) && bn_al(y, 16) && bn_al(dx, 16) && (!mask_from_x || bn_al(beta, 16)) &&
                   lddskip % 4 == 0 && bn_al(dskip, 16);
  const float* mg = mask_from_x ? gamma : nullptr;
  const float* mb = mask_from_x ? beta : nullptr;
  const float* mi = mask_from_x ? invstd : nullptr;
  if (dskip && vec)
    hipLaunchKernelGGL((bn_colsum_kernel<4, 2>), dim3(nblk), dim3(kBlock), 0, st, x, ldx, dy, lddy, y, ldy, mean, N,
                       d, rpb, L.partial, nullptr, nullptr, nullptr, dskip, lddskip);
  else if (dskip)
    hipLaunchKernelGGL((bn_colsum_kernel<1, 2>), dim3(nblk), dim3(kBlock), 0, st, x, ldx, dy, lddy, y, ldy, mean, N,
                       d, rpb, L.partial, nullptr, nullptr, nullptr, dskip, lddskip);
  else if (vec)
    hipLaunchKernelGGL((bn_colsum_kernel<4, 1>), dim3(nblk), dim3(kBlock), 0, st, x, ldx, dy, lddy, y, ldy, mean, N,
                       d, rpb, L.partial, mg, mb, mi);
  else
    hipLaunchKernelGGL((bn_colsum_kernel<1, 1>), dim3(nblk), dim3(kBlock), 0, st, x, ldx, dy, lddy, y, ldy, mean, N,
                       d, rpb, L.partial, mg, mb, mi);
  MP_LAUNCH_CHECK();
  const int rc = bn_bwd_finalize(N, d, gamma, mean, invstd, dgamma, dbeta, L, nblk, mask_from_x != 0, st);
  if (rc != MP_OK) return rc;
  const float* msc = mask_from_x ? L.v[3] : nullptr;
  if (dskip) { dy = dskip; lddy = lddskip; y = nullptr; }     // g is on hand: the mask is already applied
  if (vec)
    hipLaunchKernelGGL((bn_apply_kernel<4, 1>), dim3(flat_grid(N * (d / 4))), dim3(kBlock), 0, st, x, ldx, dy, lddy, y,
                       ldy, L.v[0], L.v[1], L.v[2], mean, 0, N, d, dx, lddx, msc, mb);
  else
    hipLaunchKernelGGL((bn_apply_kernel<1, 1>), dim3(flat_grid(N * d)), dim3(kBlock), 0, st, x, ldx, dy, lddy, y, ldy,
                       L.v[0], L.v[1], L.v[2], mean, 0, N, d, dx, lddx, msc, mb);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_bn_train_bwd_f32(const float* dy, int64_t lddy, const float* y, int64_t ldy, const float* x, int64_t ldx,
                        int64_t N, int32_t d, const float* gamma, const float* mean, const float* invstd,
                        float* dx, int64_t lddx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                        mp_stream_t stream) {
  return bn_bwd_common(dy, lddy, y, ldy, x, ldx, N, d, gamma, nullptr, 0, mean, invstd, dx, lddx, dgamma, dbeta, ws,
                       ws_bytes, as_stream(stream));
}

int mp_bn_train_bwd_relu_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t N, int32_t d,
                             const float* gamma, const float* beta, const float* mean, const float* invstd,
                             float* dx, int64_t lddx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                             mp_stream_t stream) {
  return bn_bwd_common(dy, lddy, nullptr, 0, x, ldx, N, d, gamma, beta, 1, mean, invstd, dx, lddx, dgamma, dbeta, ws,
                       ws_bytes, as_stream(stream));
}

int mp_bn_train_bwd_skip_f32(const float* dy, int64_t lddy, const float* out, int64_t ldo, const float* x, int64_t ldx,
                             int64_t N, int32_t d, const float* gamma, const float* mean, const float* invstd,
                             float* dx, int64_t lddx, float* dskip, int64_t lddskip, float* dgamma, float* dbeta,
                             void* ws, size_t ws_bytes, mp_stream_t stream) {
  if (out && !dskip) return MP_ERR_INVALID_ARG;
  // out NULL = no activation: d(skip) is dy itself and nothing is written for it
  return bn_bwd_common(dy, lddy, out, ldo, x, ldx, N, d, gamma, nullptr, 0, mean, invstd, dx, lddx, dgamma, dbeta, ws,
                       ws_bytes, as_stream(stream), out ? dskip : nullptr, out ? lddskip : 0);
}

// ---- any activation of act.h: MP_ACT_NONE and MP_ACT_RELU go to the entries above where those compute the same ------
int mp_bn_act_ws_bytes(int64_t N, int32_t d, size_t* bytes_host) {
  if (!bytes_host || N < 0 || d <= 0) return MP_ERR_INVALID_ARG;
  BnActWs w;
  bn_act_ws_layout(N, d, nullptr, &w);
  *bytes_host = w.total;
  return MP_OK;
}

int mp_bn_train_fwd_act_f32(const float* x, int64_t ldx, int64_t N, int32_t d, const float* gamma, const float* beta,
                            float eps, int act, float act_param, const float* slope, float* y, int64_t ldy,
                            float* mean, float* invstd, float* var_unbiased, void* ws, size_t ws_bytes,
                            mp_stream_t stream) {
  if (!act_known(act) || (act == MP_ACT_PRELU && !slope)) return MP_ERR_INVALID_ARG;
  if (N <= 0 || d <= 0 || !x || !y || !mean || !invstd || !var_unbiased || ldx < d || ldy < d) return MP_ERR_INVALID_ARG;
  BnActWs L;
  bn_act_ws_layout(N, d, ws, &L);
  if (!ws || ws_bytes < L.total) return MP_ERR_WORKSPACE;
  if (act == MP_ACT_NONE || act == MP_ACT_RELU)
    return mp_bn_train_fwd_f32(x, ldx, N, d, gamma, beta, eps, act == MP_ACT_RELU, y, ldy, mean, invstd, var_unbiased,
                               ws, ws_bytes, stream);
  hipStream_t st = as_stream(stream);
  const bool vec = d % 4 == 0 && ldx % 4 == 0 && ldy % 4 == 0 && bn_al(x, 16) && bn_al(y, 16);
  const int rc = bn_fwd_stats(x, ldx, N, d, gamma, beta, eps, mean, invstd, var_unbiased, L.bn, vec, st);
  if (rc != MP_OK) return rc;
  with_act(act, [&](auto a) {
    constexpr int A = decltype(a)::value;
    if constexpr (A != MP_ACT_RELU) {      // RELU went to mp_bn_train_fwd_f32 above
      if (vec)
        hipLaunchKernelGGL((bn_apply_act_kernel<4, A>), dim3(flat_grid(N * (d / 4))), dim3(kBlock), 0, st, x, ldx,
                           L.bn.v[0], L.bn.v[1], mean, act_param, slope, N, d, y, ldy);
      else
        hipLaunchKernelGGL((bn_apply_act_kernel<1, A>), dim3(flat_grid(N * d)), dim3(kBlock), 0, st, x, ldx, L.bn.v[0],
                           L.bn.v[1], mean, act_param, slope, N, d, y, ldy);
    }
  });
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_bn_train_fwd_skip_act_f32(const float* x, int64_t ldx, const float* skip, int64_t ldskip, int64_t N, int32_t d,
                                 int32_t d_skip, int mode, const float* gamma, const float* beta, float eps, int act,
                                 float act_param, const float* slope, float* out, int64_t ldo, float* mean,
                                 float* invstd, float* var_unbiased, void* ws, size_t ws_bytes, mp_stream_t stream) {
  if (!act_known(act) || (act == MP_ACT_PRELU && !slope)) return MP_ERR_INVALID_ARG;
  if (N <= 0 || d <= 0 || d_skip <= 0 || !x || !skip || !out || !mean || !invstd || !var_unbiased || ldx < d ||
      ldskip < d_skip)
    return MP_ERR_INVALID_ARG;
  if (mode != MP_BN_SKIP_SUM && mode != MP_BN_SKIP_CONCAT) return MP_ERR_INVALID_ARG;
  if (mode == MP_BN_SKIP_SUM && d_skip != d) return MP_ERR_INVALID_ARG;
  const bool cat = mode == MP_BN_SKIP_CONCAT;
  if (ldo < (cat ? (int64_t)d_skip + d : (int64_t)d)) return MP_ERR_INVALID_ARG;
  BnActWs L;
  bn_act_ws_layout(N, d, ws, &L);
  if (!ws || ws_bytes < L.total) return MP_ERR_WORKSPACE;
  if (act == MP_ACT_NONE || act == MP_ACT_RELU)
    return mp_bn_train_fwd_skip_f32(x, ldx, skip, ldskip, N, d, d_skip, mode, gamma, beta, eps, act == MP_ACT_RELU, out,
                                    ldo, mean, invstd, var_unbiased, ws, ws_bytes, stream);
  hipStream_t st = as_stream(stream);
  // the vector forms of mp_bn_train_fwd_skip_f32
  const bool vx = d % 4 == 0 && ldx % 4 == 0 && bn_al(x, 16);
  const bool vo = ldo % 4 == 0 && bn_al(out, 16);
  const bool vs = d_skip % 4 == 0 && ldskip % 4 == 0 && bn_al(skip, 16) && vo;
  const int rc = bn_fwd_stats(x, ldx, N, d, gamma, beta, eps, mean, invstd, var_unbiased, L.bn, vx, st);
  if (rc != MP_OK) return rc;
#define MP_BN_SKIP_LAUNCH(WS, WX, CAT)                                                                              \
  hipLaunchKernelGGL((bn_apply_skip_act_kernel<WS, WX, CAT, A>),                                                    \
                     dim3(flat_grid(N * ((CAT ? (int64_t)d_skip / WS : 0) + (int64_t)d / WX))), dim3(kBlock), 0, st, \
                     x, ldx, skip, ldskip, L.bn.v[0], L.bn.v[1], mean, act_param, slope, N, d, d_skip, out, ldo)
  with_act(act, [&](auto a) {
    constexpr int A = decltype(a)::value;
    if constexpr (A != MP_ACT_RELU) {      // RELU went to mp_bn_train_fwd_skip_f32 above
      if (!cat) {
        if (vx && vs) MP_BN_SKIP_LAUNCH(4, 4, false);
        else MP_BN_SKIP_LAUNCH(1, 1, false);
      } else {
        const bool vr = vx && vo && d_skip % 4 == 0;      // the right slab starts at out + d_skip
        if (vs && vr) MP_BN_SKIP_LAUNCH(4, 4, true);
        else if (vs) MP_BN_SKIP_LAUNCH(4, 1, true);
        else if (vr) MP_BN_SKIP_LAUNCH(1, 4, true);
        else MP_BN_SKIP_LAUNCH(1, 1, true);
      }
    }
  });
#undef MP_BN_SKIP_LAUNCH
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // extern "C"

// statistics, finalize and apply of a backward whose g = dy * act'(z) is recomputed from x (and skip: SUM).  gout != NULL:
// the statistics pass writes g there and the apply pass reads it in place of dy, x's affine and skip (the 7 N d scheme
// of mp_bn_train_bwd_skip_f32).  PRELU leaves its per-workgroup sums in L.partial3[0 .. bn_blocks(N)).
template <int ACT>
static int bn_bwd_act_launch(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* skip,
                             int64_t ldskip, int64_t N, int32_t d, const float* gamma, const float* beta,
                             const float* mean, const float* invstd, float prm, const float* slope, float* dx,
                             int64_t lddx, float* gout, int64_t ldg, float* dgamma, float* dbeta, const BnActWs& L,
                             hipStream_t st) {
  const int nblk = bn_blocks(N);
  const int64_t rpb = ceil_div(N, nblk);
  const bool vec = d % 4 == 0 && ldx % 4 == 0 && lddy % 4 == 0 && lddx % 4 == 0 && bn_al(x, 16) && bn_al(dy, 16) &&
                   bn_al(dx, 16) && bn_al(beta, 16) && ldskip % 4 == 0 && bn_al(skip, 16) && ldg % 4 == 0 &&
                   bn_al(gout, 16);
  const BnWs& B = L.bn;
  if (vec)
    hipLaunchKernelGGL((bn_colsum_act_kernel<4, ACT>), dim3(nblk), dim3(kBlock), 0, st, x, ldx, dy, lddy, skip, ldskip,
                       mean, gamma, beta, invstd, prm, slope, N, d, rpb, B.partial, L.partial3, gout, ldg);
  else
    hipLaunchKernelGGL((bn_colsum_act_kernel<1, ACT>), dim3(nblk), dim3(kBlock), 0, st, x, ldx, dy, lddy, skip, ldskip,
                       mean, gamma, beta, invstd, prm, slope, N, d, rpb, B.partial, L.partial3, gout, ldg);
  MP_LAUNCH_CHECK();
  const int rc = bn_bwd_finalize(N, d, gamma, mean, invstd, dgamma, dbeta, B, nblk, true, st);
  if (rc != MP_OK) return rc;
  if (gout != nullptr) {      // g is on hand
    if (vec)
      hipLaunchKernelGGL((bn_apply_kernel<4, 1>), dim3(flat_grid(N * (d / 4))), dim3(kBlock), 0, st, x, ldx, gout, ldg,
                         nullptr, 0, B.v[0], B.v[1], B.v[2], mean, 0, N, d, dx, lddx, nullptr, nullptr);
    else
      hipLaunchKernelGGL((bn_apply_kernel<1, 1>), dim3(flat_grid(N * d)), dim3(kBlock), 0, st, x, ldx, gout, ldg,
                         nullptr, 0, B.v[0], B.v[1], B.v[2], mean, 0, N, d, dx, lddx, nullptr, nullptr);
  } else if (vec) {
    hipLaunchKernelGGL((bn_apply_bwd_act_kernel<4, ACT>), dim3(flat_grid(N * (d / 4))), dim3(kBlock), 0, st, x, ldx, dy,
                       lddy, skip, ldskip, B.v[0], B.v[1], B.v[2], mean, B.v[3], beta, prm, slope, N, d, dx, lddx);
  } else {
    hipLaunchKernelGGL((bn_apply_bwd_act_kernel<1, ACT>), dim3(flat_grid(N * d)), dim3(kBlock), 0, st, x, ldx, dy, lddy,
                       skip, ldskip, B.v[0], B.v[1], B.v[2], mean, B.v[3], beta, prm, slope, N, d, dx, lddx);
  }
  MP_LAUNCH_CHECK();
  return MP_OK;
}

extern "C" {

int mp_bn_train_bwd_act_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t N, int32_t d,
                            const float* gamma, const float* beta, const float* mean, const float* invstd, int act,
                            float act_param, const float* slope, float* dx, int64_t lddx, float* dgamma, float* dbeta,
                            float* dslope, void* ws, size_t ws_bytes, mp_stream_t stream) {
  if (!act_known(act) || (act == MP_ACT_PRELU && !slope)) return MP_ERR_INVALID_ARG;
  if (N <= 0 || d <= 0 || !dy || !x || !mean || !invstd || !dx || lddy < d || ldx < d || lddx < d)
    return MP_ERR_INVALID_ARG;
  BnActWs L;
  bn_act_ws_layout(N, d, ws, &L);
  if (!ws || ws_bytes < L.total) return MP_ERR_WORKSPACE;
  hipStream_t st = as_stream(stream);
  if (act == MP_ACT_NONE || act == MP_ACT_RELU)
    return bn_bwd_common(dy, lddy, nullptr, 0, x, ldx, N, d, gamma, beta, act == MP_ACT_RELU, mean, invstd, dx, lddx,
                         dgamma, dbeta, ws, ws_bytes, st);
  int rc = MP_OK;
  with_act(act, [&](auto a) {
    rc = bn_bwd_act_launch<decltype(a)::value>(dy, lddy, x, ldx, nullptr, 0, N, d, gamma, beta, mean, invstd, act_param,
                                               slope, dx, lddx, nullptr, 0, dgamma, dbeta, L, st);
  });
  if (rc != MP_OK) return rc;
  if (act == MP_ACT_PRELU && dslope) return bn_dslope_finalize(L, bn_blocks(N), dslope, st);
  return MP_OK;
}

int mp_bn_train_bwd_skip_act_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* skip,
                                 int64_t ldskip, int64_t N, int32_t d, int32_t d_skip, int mode, const float* gamma,
                                 const float* beta, const float* mean, const float* invstd, int act, float act_param,
                                 const float* slope, float* dx, int64_t lddx, float* dskip, int64_t lddskip,
                                 float* dgamma, float* dbeta, float* dslope, void* ws, size_t ws_bytes,
                                 mp_stream_t stream) {
  if (!act_known(act) || (act == MP_ACT_PRELU && !slope)) return MP_ERR_INVALID_ARG;
  if (mode != MP_BN_SKIP_SUM && mode != MP_BN_SKIP_CONCAT) return MP_ERR_INVALID_ARG;
  const bool cat = mode == MP_BN_SKIP_CONCAT;
  if (N <= 0 || d <= 0 || d_skip <= 0 || (!cat && d_skip != d) || !dy || !x || !skip || !mean || !invstd || !dx ||
      lddy < (cat ? (int64_t)d_skip + d : (int64_t)d) || ldx < d || ldskip < d_skip || lddx < d ||
      (dskip && lddskip < d_skip))
    return MP_ERR_INVALID_ARG;
  BnActWs L;
  bn_act_ws_layout(N, d, ws, &L);
  if (!ws || ws_bytes < L.total) return MP_ERR_WORKSPACE;
  hipStream_t st = as_stream(stream);
  const float* dyr = cat ? dy + d_skip : dy;      // the BN slab of dy
  if (act == MP_ACT_NONE)      // d(skip) is dy (its left slab) itself: dskip is not written
    return bn_bwd_common(dyr, lddy, nullptr, 0, x, ldx, N, d, gamma, nullptr, 0, mean, invstd, dx, lddx, dgamma, dbeta,
                         ws, ws_bytes, st);
  const int nblk = bn_blocks(N);
  const bool left = cat && (dskip || (act == MP_ACT_PRELU && dslope));
  int rc = MP_OK;
  with_act(act, [&](auto a) {
    constexpr int A = decltype(a)::value;
    rc = bn_bwd_act_launch<A>(dyr, lddy, x, ldx, cat ? nullptr : skip, cat ? 0 : ldskip, N, d, gamma, beta, mean, invstd,
                              act_param, slope, dx, lddx, cat ? nullptr : dskip, cat ? 0 : lddskip, dgamma, dbeta, L,
                              st);
  });
  if (rc != MP_OK) return rc;
  if (left) {
    rc = bn_act_bwd_left(act, dy, lddy, skip, ldskip, act_param, slope, N, d_skip, dskip, lddskip, L, st);
    if (rc != MP_OK) return rc;
  }
  if (act == MP_ACT_PRELU && dslope) return bn_dslope_finalize(L, cat ? 2 * nblk : nblk, dslope, st);
  return MP_OK;
}

}  // extern "C"
