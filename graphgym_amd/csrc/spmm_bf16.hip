// bf16 form of the plan-based aggregation of spmm.hip: X, S and Y are stored as bf16, every
// reduction and epilogue step runs in fp32.
//
// The structure is spmm.hip's: one wave per nnz-balanced segment of whole rows (g.plan()), rows longer than hub_deg
// cut into pieces whose fp32 partials a finalize pass sums in piece order, one store per output row, no atomics.
// A gathered row is kept as packed bf16 words until it is used and then widened (a 16-bit shift, exact), so the
// terms, their order and every fp32 operation on them are those of mp_spmm_csr_f32 on the widened X: each output is
// that kernel's fp32 value rounded once to bf16 (round to nearest even, v_cvt_pk_bf16_f32).
//
// A lane reads W bf16 (2W bytes, up to 16 B); a 512-byte row (d = 256, W = 4) is half the bytes of spmm.hip's
// 1 KiB row per load instruction, so these kernels keep twice the rows in flight per wave below W = 8.
#include "common.h"
#include "vecio.h"
#include <limits.h>

namespace mp {

struct Bf16AggArgs {
  const int32_t* rowptr;
  const int32_t* col;
  const float* val;
  const int32_t* seg_row;
  int32_t n_seg;
  int32_t hub_deg;
  const uint16_t* X; int64_t ldx;
  uint16_t* Y; int64_t ldy;
  uint16_t* Q; int64_t ldq;
  const uint16_t* S; int64_t lds; float self_scale;
  const float* bias;
  int32_t act;
  int32_t* argmax;
  int32_t d;
  // hub path
  const int32_t* header;
  const int32_t* hub_row;
  const int32_t* hub_base;
  const int32_t* hub_np;
  const int32_t* piece_hub;
  const int32_t* piece_k;
  int32_t piece_edges;
  float* part;
  float* part2;
  int32_t* part_arg;
};

// rows in flight per wave: the same bytes outstanding per lane (128) at W = 8 and W = 4
template <int W> constexpr int bf16_rows_in_flight() { return W == 8 ? 8 : 16; }

// ---- per-lane bf16 and fp32 vectors ------------------------------------------------------

template <int W> constexpr int bf16_words() { return W == 1 ? 1 : W / 2; }

// W bf16 as packed 32-bit words (element 2i in the low half of word i); W = 1: the low half
template <int W> __device__ __forceinline__ void load_bf16_raw(const uint16_t* p, uint32_t (&r)[bf16_words<W>()]) {
  if constexpr (W == 8) {
    const i32x4 t = *reinterpret_cast<const i32x4*>(p);
    r[0] = t[0]; r[1] = t[1]; r[2] = t[2]; r[3] = t[3];
  } else if constexpr (W == 4) {
    const i32x2 t = *reinterpret_cast<const i32x2*>(p);
    r[0] = t[0]; r[1] = t[1];
  } else if constexpr (W == 2) {
    r[0] = *reinterpret_cast<const uint32_t*>(p);
  } else {
    r[0] = *p;
  }
}

template <int W> __device__ __forceinline__ void widen_bf16(const uint32_t (&r)[bf16_words<W>()], float (&v)[W]) {
#pragma unroll
  for (int k = 0; k < W; ++k)
    v[k] = __builtin_bit_cast(float, (k & 1) ? (r[k >> 1] & 0xffff0000u) : (r[k >> 1] << 16));
}

template <int W> __device__ __forceinline__ void load_bf16(const uint16_t* p, float (&v)[W]) {
  uint32_t r[bf16_words<W>()];
  load_bf16_raw<W>(p, r);
  widen_bf16<W>(r, v);
}

typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

// round to nearest even, two values per v_cvt_pk_bf16_f32
template <int W, bool NT> __device__ __forceinline__ void store_bf16(uint16_t* p, const float (&v)[W]) {
  if constexpr (W == 1) {
    const uint16_t h = __builtin_bit_cast(uint16_t, (__bf16)v[0]);
    if constexpr (NT) __builtin_nontemporal_store(h, p); else *p = h;
  } else {
    uint32_t w[W / 2];
#pragma unroll
    for (int i = 0; i < W / 2; ++i) {
      const f32x2 f = {v[2 * i], v[2 * i + 1]};
      w[i] = __builtin_bit_cast(uint32_t, __builtin_convertvector(f, bf16x2_t));
    }
    if constexpr (W == 8) {
      const i32x4 t = {(int)w[0], (int)w[1], (int)w[2], (int)w[3]};
      if constexpr (NT) __builtin_nontemporal_store(t, reinterpret_cast<i32x4*>(p));
      else *reinterpret_cast<i32x4*>(p) = t;
    } else if constexpr (W == 4) {
      const i32x2 t = {(int)w[0], (int)w[1]};
      if constexpr (NT) __builtin_nontemporal_store(t, reinterpret_cast<i32x2*>(p));
      else *reinterpret_cast<i32x2*>(p) = t;
    } else {
      if constexpr (NT) __builtin_nontemporal_store(w[0], reinterpret_cast<uint32_t*>(p));
      else *reinterpret_cast<uint32_t*>(p) = w[0];
    }
  }
}

// fp32 / int32 operands (bias, partials, argmax) of W per lane, as vecio.h vectors of at most 4
template <int W> __device__ __forceinline__ void load_f32(const float* p, float (&v)[W]) {
  if constexpr (W == 8) {
    float lo[4], hi[4];
    load_vec<4>(p, lo); load_vec<4>(p + 4, hi);
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = lo[k]; v[k + 4] = hi[k]; }
  } else {
    load_vec<W>(p, v);
  }
}
template <int W> __device__ __forceinline__ void store_f32(float* p, const float (&v)[W]) {
  if constexpr (W == 8) {
    const float lo[4] = {v[0], v[1], v[2], v[3]}, hi[4] = {v[4], v[5], v[6], v[7]};
    store_vec<4>(p, lo); store_vec<4>(p + 4, hi);
  } else {
    store_vec<W>(p, v);
  }
}
template <int W> __device__ __forceinline__ void load_i32(const int32_t* p, int (&v)[W]) {
  if constexpr (W == 8) {
    int lo[4], hi[4];
    load_ivec<4>(p, lo); load_ivec<4>(p + 4, hi);
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = lo[k]; v[k + 4] = hi[k]; }
  } else {
    load_ivec<W>(p, v);
  }
}
template <int W> __device__ __forceinline__ void store_i32(int32_t* p, const int (&v)[W]) {
  if constexpr (W == 8) {
    const int lo[4] = {v[0], v[1], v[2], v[3]}, hi[4] = {v[4], v[5], v[6], v[7]};
    store_ivec<4>(p, lo); store_ivec<4>(p + 4, hi);
  } else {
    store_ivec<W>(p, v);
  }
}

// ---- row reduction: spmm.hip's RowAcc and finish_row on widened values ---------------------

template <int W, int REDUCE, bool BRANCH2>
struct Bf16RowAcc {
  float a[W];
  float b[BRANCH2 ? W : 1];
  int arg[REDUCE == MP_MAX ? W : 1];

  __device__ __forceinline__ void reset() {
#pragma unroll
    for (int k = 0; k < W; ++k) {
      a[k] = (REDUCE == MP_MAX) ? -INFINITY : 0.f;
      if constexpr (BRANCH2) b[k] = 0.f;
      if constexpr (REDUCE == MP_MAX) arg[k] = -1;
    }
  }
  __device__ __forceinline__ void add(const uint32_t (&r)[bf16_words<W>()], float w, bool marked, int e) {
    float v[W];
    widen_bf16<W>(r, v);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      if constexpr (REDUCE == MP_MAX) {
        float m = w * v[k];
        if (m > a[k]) { a[k] = m; arg[k] = e; }
      } else {
        a[k] = fmaf(w, v[k], a[k]);
      }
    }
    if constexpr (BRANCH2) {
      if (marked) {   // wave-uniform
#pragma unroll
        for (int k = 0; k < W; ++k) b[k] = fmaf(w, v[k], b[k]);
      }
    }
  }
};

template <int W, int REDUCE, bool BRANCH2, bool NT>
__device__ __forceinline__ void bf16_finish_row(const Bf16AggArgs& a, int row, int deg,
                                                Bf16RowAcc<W, REDUCE, BRANCH2>& acc, int c0, int c0ld,
                                                bool lane_on) {
  float out[W];
#pragma unroll
  for (int k = 0; k < W; ++k) {
    if (REDUCE == MP_MEAN) out[k] = deg > 0 ? acc.a[k] / (float)deg : 0.f;
    else if (REDUCE == MP_MAX) out[k] = deg > 0 ? acc.a[k] : 0.f;
    else out[k] = acc.a[k];
  }
  if (a.S != nullptr) {
    float s[W];
    load_bf16<W>(a.S + (int64_t)row * a.lds + c0ld, s);
#pragma unroll
    for (int k = 0; k < W; ++k) out[k] = fmaf(a.self_scale, s[k], out[k]);
  }
  if (a.bias != nullptr) {
    float bv[W];
    load_f32<W>(a.bias + c0ld, bv);
#pragma unroll
    for (int k = 0; k < W; ++k) out[k] += bv[k];
  }
  if (a.act == MP_ACT_RELU) {
#pragma unroll
    for (int k = 0; k < W; ++k) out[k] = fmaxf(out[k], 0.f);
  }
  if (lane_on) {
    store_bf16<W, NT>(a.Y + (int64_t)row * a.ldy + c0, out);
    if constexpr (BRANCH2) store_bf16<W, false>(a.Q + (int64_t)row * a.ldq + c0, acc.b);
    if constexpr (REDUCE == MP_MAX) {
      if (a.argmax != nullptr) store_i32<W>(a.argmax + (int64_t)row * a.d + c0, acc.arg);
    }
  }
  acc.reset();
}

// ---- kernels -------------------------------------------------------------------------------

// one wave per segment of whole rows (agg_rows_kernel of spmm.hip)
template <int W, int REDUCE, bool WEIGHTED, bool BRANCH2, int U>
__global__ __launch_bounds__(kBlock) void agg_bf16_rows_kernel(Bf16AggArgs a) {
  constexpr int NW = bf16_words<W>();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int seg = blockIdx.x * kWavesPerBlock + wave;
  if (seg >= a.n_seg) return;
  const int c0 = (blockIdx.y * kWave + lane) * W;
  const bool lane_on = c0 < a.d;
  const int c0ld = lane_on ? c0 : 0;  // idle lanes re-read column 0, never store

  const int r0 = a.seg_row[seg];
  int r1 = a.seg_row[seg + 1];
  if (r0 >= r1) return;
  const int e0 = a.rowptr[r0];
  int e1 = a.rowptr[r1];
  {
    // a hub row can only be the last row that starts in a segment; the hub path owns it
    const int last_start = a.rowptr[r1 - 1];
    if (e1 - last_start > a.hub_deg) { r1 -= 1; e1 = last_start; }
  }
  if (r0 >= r1) return;

  const uint16_t* __restrict__ xlane = a.X + c0ld;

  int rbase = r0;
  int rendv = (rbase + lane < r1) ? a.rowptr[rbase + 1 + lane] : INT_MAX;
  int r = r0;
  int rstart = e0;
  int rend = bcast_i(rendv, 0);

  Bf16RowAcc<W, REDUCE, BRANCH2> acc;
  acc.reset();

  auto advance = [&]() {
    r += 1;
    rstart = rend;
    if (r - rbase == kWave) {
      rbase = r;
      rendv = (rbase + lane < r1) ? a.rowptr[rbase + 1 + lane] : INT_MAX;
    }
    rend = (r < r1) ? bcast_i(rendv, r - rbase) : INT_MAX;
  };

  for (int ec = e0; ec < e1; ec += kWave) {
    const int me = min(ec + lane, e1 - 1);
    const int cv = a.col[me];
    const float wv = WEIGHTED ? a.val[me] : 1.f;
    const int n = min(kWave, e1 - ec);
    for (int jb = 0; jb < n; jb += U) {
      uint32_t v[U][NW];
      int cj[U];
#pragma unroll
      for (int j = 0; j < U; ++j) {
        cj[j] = bcast_i(cv, jb + j);
        const int c = BRANCH2 ? (cj[j] & 0x7fffffff) : cj[j];
        load_bf16_raw<W>(xlane + (int64_t)c * a.ldx, v[j]);
      }
#pragma unroll
      for (int j = 0; j < U; ++j) {
        const int e = ec + jb + j;
        if (e < e1) {
          while (e >= rend) {
            bf16_finish_row<W, REDUCE, BRANCH2, true>(a, r, rend - rstart, acc, c0, c0ld, lane_on);
            advance();
          }
          const float w = WEIGHTED ? bcast_f(wv, jb + j) : 1.f;
          acc.add(v[j], w, BRANCH2 && cj[j] < 0, e);
        }
      }
    }
  }
  while (r < r1) {
    bf16_finish_row<W, REDUCE, BRANCH2, true>(a, r, rend - rstart, acc, c0, c0ld, lane_on);
    advance();
  }
}

// hub path 1/2: one wave reduces one piece (<= piece_edges entries) of a hub row into fp32 partials
template <int W, int REDUCE, bool WEIGHTED, bool BRANCH2, int U>
__global__ __launch_bounds__(kBlock) void agg_bf16_hub_pieces_kernel(Bf16AggArgs a) {
  constexpr int NW = bf16_words<W>();
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int c0 = (blockIdx.y * kWave + lane) * W;
  const bool lane_on = c0 < a.d;
  const int c0ld = lane_on ? c0 : 0;
  const uint16_t* __restrict__ xlane = a.X + c0ld;
  const int n_piece = a.header[PW_NPIECE];

  for (int p = blockIdx.x * kWavesPerBlock + wave; p < n_piece; p += gridDim.x * kWavesPerBlock) {
    const int h = a.piece_hub[p];
    const int k = a.piece_k[p];
    const int row = a.hub_row[h];
    const int rs = a.rowptr[row];
    const int re = a.rowptr[row + 1];
    const int e0 = rs + k * a.piece_edges;
    const int e1 = min(e0 + a.piece_edges, re);

    Bf16RowAcc<W, REDUCE, BRANCH2> acc;
    acc.reset();
    for (int ec = e0; ec < e1; ec += kWave) {
      const int me = min(ec + lane, e1 - 1);
      const int cv = a.col[me];
      const float wv = WEIGHTED ? a.val[me] : 1.f;
      const int n = min(kWave, e1 - ec);
      for (int jb = 0; jb < n; jb += U) {
        uint32_t v[U][NW];
        int cj[U];
#pragma unroll
        for (int j = 0; j < U; ++j) {
          cj[j] = bcast_i(cv, jb + j);
          const int c = BRANCH2 ? (cj[j] & 0x7fffffff) : cj[j];
          load_bf16_raw<W>(xlane + (int64_t)c * a.ldx, v[j]);
        }
#pragma unroll
        for (int j = 0; j < U; ++j) {
          const int e = ec + jb + j;
          if (e < e1) acc.add(v[j], WEIGHTED ? bcast_f(wv, jb + j) : 1.f, BRANCH2 && cj[j] < 0, e);
        }
      }
    }
    if (lane_on) {
      store_f32<W>(a.part + (int64_t)p * a.d + c0, acc.a);
      if constexpr (BRANCH2) store_f32<W>(a.part2 + (int64_t)p * a.d + c0, acc.b);
      if constexpr (REDUCE == MP_MAX) store_i32<W>(a.part_arg + (int64_t)p * a.d + c0, acc.arg);
    }
  }
}

// hub path 2/2: combine a hub row's pieces in piece order, run the epilogue, store
template <int W, int REDUCE, bool BRANCH2>
__global__ __launch_bounds__(kBlock) void agg_bf16_hub_finalize_kernel(Bf16AggArgs a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int c0 = (blockIdx.y * kWave + lane) * W;
  const bool lane_on = c0 < a.d;
  const int c0ld = lane_on ? c0 : 0;
  const int n_hub = a.header[PW_NHUB];

  for (int h = blockIdx.x * kWavesPerBlock + wave; h < n_hub; h += gridDim.x * kWavesPerBlock) {
    const int row = a.hub_row[h];
    const int base = a.hub_base[h];
    const int np = a.hub_np[h];
    const int deg = a.rowptr[row + 1] - a.rowptr[row];
    Bf16RowAcc<W, REDUCE, BRANCH2> acc;
    acc.reset();
    for (int p = base; p < base + np; ++p) {
      float v[W];
      load_f32<W>(a.part + (int64_t)p * a.d + c0ld, v);
      if constexpr (REDUCE == MP_MAX) {
        int ai[W];
        load_i32<W>(a.part_arg + (int64_t)p * a.d + c0ld, ai);
#pragma unroll
        for (int k = 0; k < W; ++k)
          if (v[k] > acc.a[k]) { acc.a[k] = v[k]; acc.arg[k] = ai[k]; }
      } else {
#pragma unroll
        for (int k = 0; k < W; ++k) acc.a[k] += v[k];
      }
      if constexpr (BRANCH2) {
        float v2[W];
        load_f32<W>(a.part2 + (int64_t)p * a.d + c0ld, v2);
#pragma unroll
        for (int k = 0; k < W; ++k) acc.b[k] += v2[k];
      }
    }
    bf16_finish_row<W, REDUCE, BRANCH2, false>(a, row, deg, acc, c0, c0ld, lane_on);
  }
}

__global__ __launch_bounds__(kBlock) void max_bwd_bf16_kernel(const int32_t* __restrict__ col,
                                                              const float* __restrict__ val,
                                                              const int32_t* __restrict__ argmax,
                                                              const uint16_t* __restrict__ dY, int64_t ldy,
                                                              int64_t N, int32_t d, float* dX, int64_t ldx) {
  const int64_t total = N * d;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / d;
    const int c = (int)(i - r * d);
    const int e = argmax[i];
    if (e >= 0) {
      const float g = __builtin_bit_cast(float, (uint32_t)dY[r * ldy + c] << 16);
      atomicAdd(&dX[(int64_t)col[e] * ldx + c], (val ? val[e] : 1.f) * g);
    }
  }
}

// ---- dispatch ------------------------------------------------------------------------------

template <int W, int REDUCE, bool WEIGHTED, bool BRANCH2>
static int launch_bf16(const Bf16AggArgs& a, const int32_t* counts, hipStream_t st) {
  constexpr int U = bf16_rows_in_flight<W>();
  const int tiles = (int)ceil_div(a.d, kWave * W);
  dim3 grid((unsigned)ceil_div(a.n_seg, kWavesPerBlock), (unsigned)tiles);
  hipLaunchKernelGGL((agg_bf16_rows_kernel<W, REDUCE, WEIGHTED, BRANCH2, U>), grid, dim3(kBlock), 0, st, a);
  MP_LAUNCH_CHECK();
  const int n_hub = counts[1], n_piece = counts[2];
  if (n_hub > 0) {
    int pb = (int)ceil_div(n_piece, kWavesPerBlock);
    if (pb > kNumCU * 8) pb = kNumCU * 8;
    hipLaunchKernelGGL((agg_bf16_hub_pieces_kernel<W, REDUCE, WEIGHTED, BRANCH2, U>), dim3(pb, tiles),
                       dim3(kBlock), 0, st, a);
    MP_LAUNCH_CHECK();
    int hb = (int)ceil_div(n_hub, kWavesPerBlock);
    if (hb > kNumCU * 8) hb = kNumCU * 8;
    hipLaunchKernelGGL((agg_bf16_hub_finalize_kernel<W, REDUCE, BRANCH2>), dim3(hb, tiles), dim3(kBlock), 0, st, a);
    MP_LAUNCH_CHECK();
  }
  return MP_OK;
}

template <int W>
static int dispatch_bf16(const Bf16AggArgs& a, const int32_t* counts, int reduce, hipStream_t st) {
  const bool weighted = a.val != nullptr;
  if (a.Q != nullptr) {
    return weighted ? launch_bf16<W, MP_SUM, true, true>(a, counts, st)
                    : launch_bf16<W, MP_SUM, false, true>(a, counts, st);
  }
  switch (reduce) {
    case MP_SUM:
      return weighted ? launch_bf16<W, MP_SUM, true, false>(a, counts, st)
                      : launch_bf16<W, MP_SUM, false, false>(a, counts, st);
    case MP_MEAN:
      return weighted ? launch_bf16<W, MP_MEAN, true, false>(a, counts, st)
                      : launch_bf16<W, MP_MEAN, false, false>(a, counts, st);
    case MP_MAX:
      return weighted ? launch_bf16<W, MP_MAX, true, false>(a, counts, st)
                      : launch_bf16<W, MP_MAX, false, false>(a, counts, st);
  }
  return MP_ERR_INVALID_ARG;
}

static bool aligned_to(const void* p, size_t a) { return p == nullptr || ((uintptr_t)p % a) == 0; }

// widest per-lane vector (W bf16, 2W bytes, W <= 8) every operand allows, then no wider than the row needs
static int pick_width_bf16(const Bf16AggArgs& a) {
  auto ok = [&](int w) {
    const size_t hb = 2u * w;                   // bf16 operands: one 2W-byte access per lane
    const size_t fb = 4u * (w < 4 ? w : 4);     // fp32 / int32 operands: vectors of at most 4
    if (a.d % w) return false;
    if (a.ldx % w || a.ldy % w) return false;
    if (a.Q && a.ldq % w) return false;
    if (a.S && a.lds % w) return false;
    return aligned_to(a.X, hb) && aligned_to(a.Y, hb) && aligned_to(a.Q, hb) && aligned_to(a.S, hb) &&
           aligned_to(a.bias, fb) && aligned_to(a.argmax, fb) &&
           aligned_to(a.part, fb) && aligned_to(a.part2, fb) && aligned_to(a.part_arg, fb);
  };
  int w = 8;
  while (w > 1 && !ok(w)) w >>= 1;
  while (w > 1 && kWave * (w / 2) >= a.d) w >>= 1;  // d = 256 -> 4, d = 128 -> 2, d = 64 -> 1: keep all lanes busy
  return w;
}

static int agg_bf16_common(const int32_t* rowptr, const int32_t* col, const float* val, int64_t N,
                           const int32_t* plan, const int32_t* counts, const void* X, int64_t ldx, void* Y,
                           int64_t ldy, void* Q, int64_t ldq, int32_t d, int reduce, const void* S, int64_t lds,
                           float self_scale, const float* bias, int act, int32_t* argmax, void* ws, size_t ws_bytes,
                           hipStream_t st) {
  if (!rowptr || !plan || !counts || !X || !Y) return MP_ERR_INVALID_ARG;
  if (N < 0 || d <= 0 || ldx < d || ldy < d) return MP_ERR_INVALID_ARG;
  if (reduce < MP_SUM || reduce > MP_MAX) return MP_ERR_INVALID_ARG;
  if (act != MP_ACT_NONE && act != MP_ACT_RELU) return MP_ERR_INVALID_ARG;
  if (Q && ldq < d) return MP_ERR_INVALID_ARG;
  if (S && lds < d) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX) return MP_ERR_UNSUPPORTED;
  if (N == 0) return MP_OK;
  const int32_t n_seg = counts[0], n_piece = counts[2];
  if (n_seg < 1) return MP_ERR_INVALID_ARG;
  if (!col && n_piece > 0) return MP_ERR_INVALID_ARG;

  size_t need = 0;   // the partials are fp32: the fp32 kernel's workspace
  mp_spmm_ws_bytes(counts, d, reduce, Q != nullptr, &need);
  if (need > 0 && (!ws || ws_bytes < need)) return MP_ERR_WORKSPACE;

  Bf16AggArgs a;
  a.rowptr = rowptr; a.col = col; a.val = val;
  a.header = plan;
  a.seg_row = plan + PW_HEADER_WORDS;
  a.n_seg = n_seg;
  a.hub_deg = counts[6];       // the config the plan was built under
  a.piece_edges = counts[7];
  a.X = (const uint16_t*)X; a.ldx = ldx; a.Y = (uint16_t*)Y; a.ldy = ldy; a.Q = (uint16_t*)Q; a.ldq = ldq;
  a.S = (const uint16_t*)S; a.lds = lds; a.self_scale = self_scale; a.bias = bias; a.act = act;
  a.argmax = argmax; a.d = d;
  a.hub_row = a.hub_base = a.hub_np = a.piece_hub = a.piece_k = nullptr;
  a.part = a.part2 = nullptr; a.part_arg = nullptr;
  if (n_piece > 0) {
    // the hub arrays sit behind seg_row; counts[3], counts[4] = their capacities (spmm.hip, agg_common)
    const int32_t cap_hub = counts[3], cap_piece = counts[4];
    a.hub_row = a.seg_row + (n_seg + 1);
    a.hub_base = a.hub_row + cap_hub;
    a.hub_np = a.hub_base + cap_hub;
    a.piece_hub = a.hub_np + cap_hub;
    a.piece_k = a.piece_hub + cap_piece;
    char* w = (char*)ws;
    const size_t slab = align_up((size_t)n_piece * d * 4, 256);
    a.part = (float*)w; w += slab;
    if (Q) { a.part2 = (float*)w; w += slab; }
    if (reduce == MP_MAX) { a.part_arg = (int32_t*)w; w += slab; }
  }

  switch (pick_width_bf16(a)) {
    case 8: return dispatch_bf16<8>(a, counts, reduce, st);
    case 4: return dispatch_bf16<4>(a, counts, reduce, st);
    case 2: return dispatch_bf16<2>(a, counts, reduce, st);
    default: return dispatch_bf16<1>(a, counts, reduce, st);
  }
}

}  // namespace mp

using namespace mp;

extern "C" {

int mp_spmm_csr_bf16(const int32_t* rowptr, const int32_t* col, const float* val, int64_t N,
                     const int32_t* plan, const int32_t* counts_host, const void* X, int64_t ldx,
                     void* Y, int64_t ldy, int32_t d, int reduce, const void* S, int64_t lds,
                     float self_scale, const float* bias, int act, int32_t* argmax, void* ws,
                     size_t ws_bytes, mp_stream_t stream) {
  return agg_bf16_common(rowptr, col, val, N, plan, counts_host, X, ldx, Y, ldy, nullptr, 0, d, reduce, S, lds,
                         self_scale, bias, act, argmax, ws, ws_bytes, as_stream(stream));
}

int mp_idgnn_agg_bf16(const int32_t* rowptr, const int32_t* col_marked, const float* val, int64_t N,
                      const int32_t* plan, const int32_t* counts_host, const void* X, int64_t ldx,
                      void* P, int64_t ldp, void* Q, int64_t ldq, int32_t d, void* ws,
                      size_t ws_bytes, mp_stream_t stream) {
  if (!Q) return MP_ERR_INVALID_ARG;
  return agg_bf16_common(rowptr, col_marked, val, N, plan, counts_host, X, ldx, P, ldp, Q, ldq, d, MP_SUM,
                         nullptr, 0, 0.f, nullptr, MP_ACT_NONE, nullptr, ws, ws_bytes, as_stream(stream));
}

int mp_spmm_max_bwd_bf16(const int32_t* col, const float* val, const int32_t* argmax, const void* dY,
                         int64_t ldy, int64_t N, int32_t d, float* dX, int64_t ldx, mp_stream_t stream) {
  if (!col || !argmax || !dY || !dX || N < 0 || d <= 0) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX) return MP_ERR_UNSUPPORTED;
  if (N == 0) return MP_OK;
  hipLaunchKernelGGL(max_bwd_bf16_kernel, dim3(flat_grid(N * d)), dim3(kBlock), 0, as_stream(stream), col,
                     val, argmax, (const uint16_t*)dY, ldy, N, d, dX, ldx);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // extern "C"
