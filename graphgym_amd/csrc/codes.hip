// codes.hip — integer-coded features: rows of small tables summed per item, and the reduction of a gradient into those
// few table rows (graphgym/models/feature_encoder.py:13-103; the bond term of generalconv_ogb.py:30-35,115-118).
//
//   mp_embed_sum_f32     out[r] = ((0 + T[off_0 + codes[r,0]]) + T[off_1 + codes[r,1]]) + ...   a store stream of R*d floats
//   mp_code_reduce_f32   dT[c]  = sum over the items i with code_i = c of w_i * dY[row_i]       no float atomics
//
// The reduce has C destinations (173 atom rows, 60 combined bond codes) of up to millions of items each: a destination
// is not a unit of work.  A workgroup is ONE wave that owns a contiguous range of rows and a 64-column panel; lane l owns
// column panel*64 + l and accumulates into its own LDS word acc[c][l], so no two lanes ever touch one word and there is
// neither an atomic nor a barrier.  The wave stores its [C, 64] partial as one slab; code_slabs_sum_kernel adds the
// slabs of a column in slab order.  Items are walked in row order inside a slab and slabs are added in index order: the
// grid is a function of (R, C, d) alone, so two runs give the same bits.
//
// Cap on C: kCodeMaxC = 208.  208 * 64 * 4 B = 52 KiB of LDS per wave, three resident waves on the 160 KiB of a CU
// (Atom: 173 rows -> 44 KiB, also three; Bond: 60 rows -> 15 KiB, ten).  At that occupancy a wave hides latency
// itself: it keeps the dY row loads of a block of rows in flight while it adds the block before, and updates its
// accumulators several at a time (rmw_batch: one LDS round trip for a batch of items, not one per item).
//
// Workspace: n_slabs * C * d floats with n_slabs = clamp(R / (16 C), 1, 1024), i.e. at most max(C d, R d / 16) floats —
// a sixteenth of dY or less (Atom at R = 10^6, d = 300: 361 slabs, 75 MB against 1.2 GB).
//
// Measured (profiles/ogb_bench.json, N = 10^6, d = 256): the Bond reduce over 2.2 * 10^6 entries takes 1.15 ms, the Atom
// reduce 5.45 ms — against 0.41 and 2.20 ms for the plan-based aggregation on the transposed one-hot operator, which reads
// dY up to nine times but at full occupancy.  ops.code_reduce_path therefore sends reductions whose items are known ahead
// of the call to that operator and keeps this kernel for the per-column winners of max (and MP_CODE_REDUCE=kernel).
#include "common.h"

namespace mp {
namespace {

constexpr int kCodeMaxK = 64;       // the codes of one row are read by one wave, one lane each
constexpr int kCodePanel = 64;      // columns per workgroup of the reduce: one per lane
constexpr int kCodeMaxC = 208;
constexpr int kCodeMaxSlabs = 1024;
constexpr int kCodeRowsPerSlabPerCode = 16;

// ---- forward ---------------------------------------------------------------------------------------------------------
// a wave takes a row: lanes 0..K-1 read its K code words once, every lane gets them by broadcast; the K table-row loads
// of a column chunk are issued before the first is added.  W columns per lane (4: 16-byte loads and stores).
// The broadcasts run in wave-uniform control flow ONLY: a cross-lane read from a lane that is masked off returns 0, so
// the column loop below is uniform (every lane takes every chunk) and only the loads and the store are predicated — a
// last chunk with fewer live lanes than K still sees all K codes.
template <int W>
struct RowVec { float v[W]; };

template <int W>
__device__ __forceinline__ RowVec<W> load_cols(const float* p, bool live) {
  RowVec<W> r;
#pragma unroll
  for (int j = 0; j < W; ++j) r.v[j] = 0.f;
  if (live) {
    if constexpr (W == 4) {
      const float4 q = *reinterpret_cast<const float4*>(p);
      r.v[0] = q.x; r.v[1] = q.y; r.v[2] = q.z; r.v[3] = q.w;
    } else {
      r.v[0] = *p;
    }
  }
  return r;
}

template <int W>
__device__ __forceinline__ void store_cols(float* p, const RowVec<W>& r) {
  if constexpr (W == 4) *reinterpret_cast<float4*>(p) = make_float4(r.v[0], r.v[1], r.v[2], r.v[3]);
  else *p = r.v[0];
}

// KT: K at compile time (1, 3, 9: the reference's encoders), 0: any K <= kCodeMaxK in chunks of eight loads
template <int W, int KT>
__global__ __launch_bounds__(kBlock) void embed_sum_kernel(const int32_t* __restrict__ codes, int32_t K,
                                                           const int32_t* __restrict__ off,
                                                           const float* __restrict__ T, int64_t ldt, int64_t R,
                                                           int32_t d, float* __restrict__ out, int64_t ldo) {
  const int lane = threadIdx.x & (kWave - 1);
  const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
  const int64_t n_waves = (int64_t)gridDim.x * kWavesPerBlock;
  const int32_t my_off = (off != nullptr && lane < K) ? off[lane] : 0;
  for (int64_t r = wave; r < R; r += n_waves) {             // wave-uniform: r depends on the wave alone
    const int32_t mine = lane < K ? codes[r * K + lane] + my_off : 0;
    int32_t row[KT > 0 ? KT : 1];
    if constexpr (KT > 0) {
#pragma unroll
      for (int k = 0; k < KT; ++k) row[k] = __shfl(mine, k);   // every lane active here
    }
    for (int cb = 0; cb < d; cb += kWave * W) {                // wave-uniform: cb is the same in every lane
      const int c0 = cb + lane * W;
      const bool live = c0 < d;
      RowVec<W> acc;
#pragma unroll
      for (int j = 0; j < W; ++j) acc.v[j] = 0.f;
      if constexpr (KT > 0) {
        RowVec<W> t[KT];
#pragma unroll
        for (int k = 0; k < KT; ++k) t[k] = load_cols<W>(T + (int64_t)row[k] * ldt + c0, live);
#pragma unroll
        for (int k = 0; k < KT; ++k)
#pragma unroll
          for (int j = 0; j < W; ++j) acc.v[j] = acc.v[j] + t[k].v[j];
      } else {
        for (int k0 = 0; k0 < K; k0 += 8) {                    // wave-uniform
          RowVec<W> t[8];
#pragma unroll
          for (int k = 0; k < 8; ++k) {
            const int32_t rk = __shfl(mine, k0 + k < K ? k0 + k : 0);     // outside every lane-dependent branch
            t[k] = load_cols<W>(T + (int64_t)rk * ldt + c0, live && k0 + k < K);
          }
#pragma unroll
          for (int k = 0; k < 8; ++k)
            if (k0 + k < K)
#pragma unroll
              for (int j = 0; j < W; ++j) acc.v[j] = acc.v[j] + t[k].v[j];
        }
      }
      if (live) store_cols<W>(out + r * ldo + c0, acc);
    }
  }
}

// ---- backward --------------------------------------------------------------------------------------------------------
enum CodeMode { kFixedK = 0, kRowptr = 1, kPerColumn = 2 };

#pragma clang fp contract(off)

// B read-modify-writes of lane-private accumulators as ONE round trip to LDS: B reads in flight, the sums in registers,
// B writes.  Items of a batch may share a code (DISTINCT false): each then takes the batch's whole contribution to its
// code, t_0 .. t_{B-1} added in item order with exact zeros for the others — the bits of the one-by-one sequence — and
// equal codes write equal words.  A code outside [0, C) is skipped.  Every product w * dY is rounded on its own
// (fp contract off below: no fused multiply-add), so every batching of the same items gives the same bits.
template <int B, bool DISTINCT>
__device__ __forceinline__ void rmw_batch(float* acc, int lane, const int32_t (&c)[B], const float (&t)[B], int32_t C) {
  float v[B];
#pragma unroll
  for (int i = 0; i < B; ++i) v[i] = (uint32_t)c[i] < (uint32_t)C ? acc[c[i] * kCodePanel + lane] : 0.f;
  float tot[B];
#pragma unroll
  for (int i = 0; i < B; ++i) {
    tot[i] = v[i];
    if constexpr (DISTINCT) {
      tot[i] += t[i];
    } else {
#pragma unroll
      for (int j = 0; j < B; ++j) tot[i] += (c[j] == c[i]) ? t[j] : 0.f;
    }
  }
#pragma unroll
  for (int i = 0; i < B; ++i)
    if ((uint32_t)c[i] < (uint32_t)C) acc[c[i] * kCodePanel + lane] = tot[i];
}

constexpr int kCodeRowBlock = 8;    // rows whose loads are issued together

// one block of kCodeRowBlock rows of the fixed-K form: lane k < K holds the row's k-th code (+ offset) and weight, every
// lane its column of dY
struct RowBlock {
  int32_t mine[kCodeRowBlock];
  float wv[kCodeRowBlock];
  float g[kCodeRowBlock];
};

__device__ __forceinline__ RowBlock load_row_block(int64_t rb, int64_t r1, int lane, int32_t K, int32_t my_off,
                                                   const int32_t* __restrict__ codes, const float* __restrict__ w,
                                                   const float* __restrict__ dY, int64_t ldy, int col, bool on) {
  RowBlock b;
#pragma unroll
  for (int j = 0; j < kCodeRowBlock; ++j) {
    const int64_t r = rb + j;
    const bool live = r < r1;
    b.mine[j] = (live && lane < K) ? codes[r * K + lane] + my_off : -1;
    b.wv[j] = (live && lane < K && w != nullptr) ? w[r * K + lane] : 1.f;
    b.g[j] = (live && on) ? dY[r * ldy + col] : 0.f;
  }
  return b;
}

// grid (panels, slabs), one wave per workgroup; dynamic LDS acc[C][64].  Lane l reads and writes acc[c * 64 + l] only.
//   kFixedK     row r holds K items, item k has code off[k] + codes[r*K + k] and weight w[r*K + k].  KT: K at compile
//               time with the K codes of a row known to differ (stacked tables: 3, 9), 1: one item per row (batches of
//               four rows), 0: any K
//   kRowptr     row r holds the entries rowptr[r] .. rowptr[r+1]; entry i has code codes[i] (< 0: no term), weight w[i]
//               and row rows[i].  The slab walks its entries, not its rows: 64 at a time, one per lane
//   kPerColumn  row r, column c holds the one item sel[r*lds + c] (< 0: none) with code codes[item] and weight w[item]
// w NULL = ones.  A code outside [0, C) adds nothing (the host has checked them; this keeps the LDS index in range).
template <int MODE, int KT>
__global__ __launch_bounds__(kWave) void code_reduce_kernel(const int32_t* __restrict__ rowptr,
                                                            const int32_t* __restrict__ rows, int32_t K,
                                                            const int32_t* __restrict__ codes,
                                                            const int32_t* __restrict__ off,
                                                            const float* __restrict__ w,
                                                            const int32_t* __restrict__ sel, int64_t lds,
                                                            int64_t R, int64_t rows_per_slab, int32_t C,
                                                            const float* __restrict__ dY, int64_t ldy, int32_t d,
                                                            float* __restrict__ slabs) {
  extern __shared__ float acc[];
  const int lane = threadIdx.x;
  const int col = blockIdx.x * kCodePanel + lane;
  const bool on = col < d;
  for (int c = 0; c < C; ++c) acc[c * kCodePanel + lane] = 0.f;
  const int64_t r0 = (int64_t)blockIdx.y * rows_per_slab;
  const int64_t r1 = r0 + rows_per_slab < R ? r0 + rows_per_slab : R;

  if constexpr (MODE == kFixedK) {
    const int32_t my_off = (off != nullptr && lane < K) ? off[lane] : 0;
    if (r0 < r1) {
      RowBlock cur = load_row_block(r0, r1, lane, K, my_off, codes, w, dY, ldy, col, on);
      for (int64_t rb = r0; rb < r1; rb += kCodeRowBlock) {
        RowBlock nxt;
        if (rb + kCodeRowBlock < r1)      // the next block's loads fly while this one is added
          nxt = load_row_block(rb + kCodeRowBlock, r1, lane, K, my_off, codes, w, dY, ldy, col, on);
        if constexpr (KT == 1) {
#pragma unroll
          for (int j0 = 0; j0 < kCodeRowBlock; j0 += 4) {
            int32_t c[4];
            float t[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
              c[i] = __shfl(cur.mine[j0 + i], 0);
              t[i] = __shfl(cur.wv[j0 + i], 0) * cur.g[j0 + i];
            }
            rmw_batch<4, false>(acc, lane, c, t, C);
          }
        } else if constexpr (KT > 1) {
#pragma unroll
          for (int j = 0; j < kCodeRowBlock; ++j) {
            int32_t c[KT];
            float t[KT];
#pragma unroll
            for (int k = 0; k < KT; ++k) {
              c[k] = __shfl(cur.mine[j], k);
              t[k] = __shfl(cur.wv[j], k) * cur.g[j];
            }
            rmw_batch<KT, true>(acc, lane, c, t, C);
          }
        } else {
#pragma unroll
          for (int j = 0; j < kCodeRowBlock; ++j) {
            for (int k0 = 0; k0 < K; k0 += 4) {
              int32_t c[4];
              float t[4];
#pragma unroll
              for (int i = 0; i < 4; ++i) {
                const int k = k0 + i < K ? k0 + i : 0;
                c[i] = k0 + i < K ? __shfl(cur.mine[j], k) : -1;
                t[i] = __shfl(cur.wv[j], k) * cur.g[j];
              }
              rmw_batch<4, false>(acc, lane, c, t, C);
            }
          }
        }
        if (rb + kCodeRowBlock < r1) cur = nxt;
      }
    }
  } else if constexpr (MODE == kRowptr) {
    const int32_t e0 = r0 < r1 ? rowptr[r0] : 0, e1 = r0 < r1 ? rowptr[r1] : 0;
    for (int32_t i0 = e0; i0 < e1; i0 += kWave) {
      const int32_t n = e1 - i0 < kWave ? e1 - i0 : kWave;
      const int32_t my_c = lane < n ? codes[i0 + lane] : -1;
      const int32_t my_r = lane < n ? rows[i0 + lane] : 0;
      const float my_w = (lane < n && w != nullptr) ? w[i0 + lane] : 1.f;
      for (int k0 = 0; k0 < n; k0 += 16) {
        int32_t c[16];
        float t[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {       // sixteen row loads in flight (neighbouring entries share rows: cache hits)
          const int k = (k0 + i) & (kWave - 1);
          c[i] = k0 + i < n ? __shfl(my_c, k) : -1;
          const int64_t r = __shfl(my_r, k);
          t[i] = (on && c[i] >= 0) ? dY[r * ldy + col] : 0.f;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) t[i] = __shfl(my_w, (k0 + i) & (kWave - 1)) * t[i];
#pragma unroll
        for (int b = 0; b < 16; b += 4) {
          const int32_t cb[4] = {c[b], c[b + 1], c[b + 2], c[b + 3]};
          const float tb[4] = {t[b], t[b + 1], t[b + 2], t[b + 3]};
          rmw_batch<4, false>(acc, lane, cb, tb, C);
        }
      }
    }
  } else {
    for (int64_t rb = r0; rb < r1; rb += kCodeRowBlock) {
      int32_t item[kCodeRowBlock], c[kCodeRowBlock];
      float t[kCodeRowBlock];
#pragma unroll
      for (int j = 0; j < kCodeRowBlock; ++j) item[j] = (on && rb + j < r1) ? sel[(rb + j) * lds + col] : -1;
#pragma unroll
      for (int j = 0; j < kCodeRowBlock; ++j) {
        c[j] = item[j] >= 0 ? codes[item[j]] : -1;
        const float wk = (item[j] >= 0 && w != nullptr) ? w[item[j]] : 1.f;
        t[j] = item[j] >= 0 ? wk * dY[(rb + j) * ldy + col] : 0.f;
      }
#pragma unroll
      for (int b = 0; b < kCodeRowBlock; b += 4) {
        const int32_t cb[4] = {c[b], c[b + 1], c[b + 2], c[b + 3]};
        const float tb[4] = {t[b], t[b + 1], t[b + 2], t[b + 3]};
        rmw_batch<4, false>(acc, lane, cb, tb, C);
      }
    }
  }

  if (on) {
    float* slab = slabs + (int64_t)blockIdx.y * C * d + col;
    for (int c = 0; c < C; ++c) slab[(int64_t)c * d] = acc[c * kCodePanel + lane];
  }
}

// dT[c, col] = slab_0[c, col] + slab_1[c, col] + ... in slab order
__global__ __launch_bounds__(kBlock) void code_slabs_sum_kernel(const float* __restrict__ slabs, int32_t n_slabs,
                                                                int32_t C, int32_t d, float* __restrict__ dT,
                                                                int64_t ldt) {
  const int64_t n = (int64_t)C * d;
  for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
    float s = slabs[i];
    for (int32_t k = 1; k < n_slabs; ++k) s += slabs[(int64_t)k * n + i];
    dT[(i / d) * ldt + (i % d)] = s;
  }
}

int32_t code_slabs(int64_t R, int32_t C) {
  int64_t s = R / ((int64_t)kCodeRowsPerSlabPerCode * C);
  if (s < 1) s = 1;
  if (s > kCodeMaxSlabs) s = kCodeMaxSlabs;
  return (int32_t)s;
}

template <int W>
void launch_embed_sum(int grid, hipStream_t st, const int32_t* codes, int32_t K, const int32_t* off, const float* T,
                      int64_t ldt, int64_t R, int32_t d, float* out, int64_t ldo) {
  switch (K) {
    case 1: hipLaunchKernelGGL((embed_sum_kernel<W, 1>), dim3(grid), dim3(kBlock), 0, st, codes, K, off, T, ldt, R, d, out, ldo); break;
    case 3: hipLaunchKernelGGL((embed_sum_kernel<W, 3>), dim3(grid), dim3(kBlock), 0, st, codes, K, off, T, ldt, R, d, out, ldo); break;
    case 9: hipLaunchKernelGGL((embed_sum_kernel<W, 9>), dim3(grid), dim3(kBlock), 0, st, codes, K, off, T, ldt, R, d, out, ldo); break;
    default: hipLaunchKernelGGL((embed_sum_kernel<W, 0>), dim3(grid), dim3(kBlock), 0, st, codes, K, off, T, ldt, R, d, out, ldo); break;
  }
}

}  // namespace
}  // namespace mp

using namespace mp;

extern "C" {

int mp_embed_sum_f32(const int32_t* codes, int32_t K, const int32_t* offsets, const float* table, int64_t ldt,
                     int64_t R, int32_t d, float* out, int64_t ldo, mp_stream_t stream) {
  if (R < 0 || d <= 0 || K <= 0 || ldt < d || ldo < d || (R > 0 && (!codes || !table || !out)))
    return MP_ERR_INVALID_ARG;
  if (K > kCodeMaxK) return MP_ERR_UNSUPPORTED;
  if (R == 0) return MP_OK;
  const bool vec = d % 4 == 0 && ldt % 4 == 0 && ldo % 4 == 0 && (uintptr_t)table % 16 == 0 && (uintptr_t)out % 16 == 0;
  const int grid = row_grid(R);
  if (vec) launch_embed_sum<4>(grid, as_stream(stream), codes, K, offsets, table, ldt, R, d, out, ldo);
  else launch_embed_sum<1>(grid, as_stream(stream), codes, K, offsets, table, ldt, R, d, out, ldo);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_code_reduce_max_codes(void) { return kCodeMaxC; }

int mp_code_reduce_ws_bytes(int64_t R, int32_t C, int32_t d, int32_t* n_slabs, size_t* bytes) {
  if (R < 0 || C <= 0 || d <= 0 || !bytes) return MP_ERR_INVALID_ARG;
  if (C > kCodeMaxC) return MP_ERR_UNSUPPORTED;
  const int32_t s = code_slabs(R, C);
  if (n_slabs) *n_slabs = s;
  *bytes = (size_t)s * C * d * sizeof(float);
  return MP_OK;
}

int mp_code_reduce_f32(const int32_t* rowptr, const int32_t* rows, int32_t K, const int32_t* codes,
                       const int32_t* offsets, int tables_disjoint, const float* w, const int32_t* sel, int64_t lds,
                       int64_t R, int32_t C, const float* dY, int64_t ldy, int32_t d, float* dT, int64_t ldt, void* ws,
                       size_t ws_bytes, mp_stream_t stream) {
  if (R < 0 || C <= 0 || d <= 0 || ldy < d || ldt < d || !dT || !ws || (R > 0 && (!codes || !dY)))
    return MP_ERR_INVALID_ARG;
  if (sel != nullptr && (rowptr != nullptr || lds < d)) return MP_ERR_INVALID_ARG;
  if (rowptr != nullptr && R > 0 && !rows) return MP_ERR_INVALID_ARG;
  if (sel == nullptr && rowptr == nullptr && K <= 0) return MP_ERR_INVALID_ARG;
  if (C > kCodeMaxC || R >= ((int64_t)1 << 31)) return MP_ERR_UNSUPPORTED;
  if (sel == nullptr && rowptr == nullptr && K > kCodeMaxK) return MP_ERR_UNSUPPORTED;
  const int32_t n_slabs = code_slabs(R, C);
  if (ws_bytes < (size_t)n_slabs * C * d * sizeof(float)) return MP_ERR_INVALID_ARG;
  hipStream_t st = as_stream(stream);
  float* slabs = static_cast<float*>(ws);
  const int64_t rows_per_slab = ceil_div(R > 0 ? R : 1, n_slabs);
  const dim3 grid((unsigned)ceil_div(d, kCodePanel), (unsigned)n_slabs);
  const size_t lds_bytes = (size_t)C * kCodePanel * sizeof(float);
#define MP_CODE_REDUCE(MODE, KT)                                                                                       \
  hipLaunchKernelGGL((code_reduce_kernel<MODE, KT>), grid, dim3(kWave), lds_bytes, st, rowptr, rows, K, codes, offsets, \
                     w, sel, lds, R, rows_per_slab, C, dY, ldy, d, slabs)
  if (sel != nullptr) MP_CODE_REDUCE(kPerColumn, 0);
  else if (rowptr != nullptr) MP_CODE_REDUCE(kRowptr, 0);
  else if (K == 1) MP_CODE_REDUCE(kFixedK, 1);
  else if (K == 3 && tables_disjoint) MP_CODE_REDUCE(kFixedK, 3);
  else if (K == 9 && tables_disjoint) MP_CODE_REDUCE(kFixedK, 9);
  else MP_CODE_REDUCE(kFixedK, 0);
#undef MP_CODE_REDUCE
  MP_LAUNCH_CHECK();
  hipLaunchKernelGGL(code_slabs_sum_kernel, dim3(flat_grid((int64_t)C * d)), dim3(kBlock), 0, st, slabs, n_slabs, C, d,
                     dT, ldt);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // extern "C"
