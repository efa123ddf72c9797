// Per-lane vector load/store helpers and wave broadcasts shared by the aggregation and
// attention kernels (gfx950, wave64).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mp {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef int i32x2 __attribute__((ext_vector_type(2)));

template <int W> __device__ __forceinline__ void load_vec(const float* p, float (&v)[W]);
template <> __device__ __forceinline__ void load_vec<4>(const float* p, float (&v)[4]) {
  f32x4 t = *reinterpret_cast<const f32x4*>(p);
  v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
}
template <> __device__ __forceinline__ void load_vec<2>(const float* p, float (&v)[2]) {
  f32x2 t = *reinterpret_cast<const f32x2*>(p);
  v[0] = t[0]; v[1] = t[1];
}
template <> __device__ __forceinline__ void load_vec<1>(const float* p, float (&v)[1]) { v[0] = *p; }

// streaming (non-temporal) load of a row that this kernel reads once: it should not push resident data (the transform's
// weights) out of the L2
template <int W> __device__ __forceinline__ void load_vec_nt(const float* p, float (&v)[W]) {
  if constexpr (W == 4) {
    f32x4 t = __builtin_nontemporal_load(reinterpret_cast<const f32x4*>(p));
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  } else if constexpr (W == 2) {
    f32x2 t = __builtin_nontemporal_load(reinterpret_cast<const f32x2*>(p));
    v[0] = t[0]; v[1] = t[1];
  } else {
    v[0] = __builtin_nontemporal_load(p);
  }
}

// v[W] at byte offset `off` (< bytes) of the wave-uniform row `base`, as a buffer load with cache policy POL (0: default,
// 2: nt on gfx950).  The policy is an operand of the instruction: the compiler merges a plain load and a
// __builtin_nontemporal_load of the same address in the two arms of a branch into one plain load (the hint dropped),
// but not two buffer loads of different policies.
template <int W, int POL> __device__ __forceinline__ void load_vec_row_buf(const float* base, int off, int bytes, float (&v)[W]) {
  const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), (short)0, bytes, 0x00020000);
  if constexpr (W == 4) {
    const f32x4 t = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, POL));
    v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
  } else if constexpr (W == 2) {
    const f32x2 t = __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, POL));
    v[0] = t[0]; v[1] = t[1];
  } else {
    v[0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, POL));
  }
}

template <int W> __device__ __forceinline__ void store_vec(float* p, const float (&v)[W]);
template <> __device__ __forceinline__ void store_vec<4>(float* p, const float (&v)[4]) {
  f32x4 t = {v[0], v[1], v[2], v[3]};
  *reinterpret_cast<f32x4*>(p) = t;
}
template <> __device__ __forceinline__ void store_vec<2>(float* p, const float (&v)[2]) {
  f32x2 t = {v[0], v[1]};
  *reinterpret_cast<f32x2*>(p) = t;
}
template <> __device__ __forceinline__ void store_vec<1>(float* p, const float (&v)[1]) { *p = v[0]; }

// streaming (non-temporal) store of an output row: written once, never re-read by this kernel
template <int W> __device__ __forceinline__ void store_vec_nt(float* p, const float (&v)[W]) {
  if constexpr (W == 4) {
    f32x4 t = {v[0], v[1], v[2], v[3]};
    __builtin_nontemporal_store(t, reinterpret_cast<f32x4*>(p));
  } else if constexpr (W == 2) {
    f32x2 t = {v[0], v[1]};
    __builtin_nontemporal_store(t, reinterpret_cast<f32x2*>(p));
  } else {
    __builtin_nontemporal_store(v[0], p);
  }
}

template <int W> __device__ __forceinline__ void store_ivec(int32_t* p, const int (&v)[W]);
template <> __device__ __forceinline__ void store_ivec<4>(int32_t* p, const int (&v)[4]) {
  i32x4 t = {v[0], v[1], v[2], v[3]};
  *reinterpret_cast<i32x4*>(p) = t;
}
template <> __device__ __forceinline__ void store_ivec<2>(int32_t* p, const int (&v)[2]) {
  i32x2 t = {v[0], v[1]};
  *reinterpret_cast<i32x2*>(p) = t;
}
template <> __device__ __forceinline__ void store_ivec<1>(int32_t* p, const int (&v)[1]) { *p = v[0]; }

template <int W> __device__ __forceinline__ void load_ivec(const int32_t* p, int (&v)[W]);
template <> __device__ __forceinline__ void load_ivec<4>(const int32_t* p, int (&v)[4]) {
  i32x4 t = *reinterpret_cast<const i32x4*>(p);
  v[0] = t[0]; v[1] = t[1]; v[2] = t[2]; v[3] = t[3];
}
template <> __device__ __forceinline__ void load_ivec<2>(const int32_t* p, int (&v)[2]) {
  i32x2 t = *reinterpret_cast<const i32x2*>(p);
  v[0] = t[0]; v[1] = t[1];
}
template <> __device__ __forceinline__ void load_ivec<1>(const int32_t* p, int (&v)[1]) { v[0] = *p; }

// fp32 / int32 operands of up to 8 per lane, as the vectors above (at most 4 wide); W <= 4: exactly load_vec / store_vec
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

// ---- W bf16 per lane (2W bytes, W <= 8), widened to fp32 exactly (a 16-bit shift) --------------

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

__device__ __forceinline__ int bcast_i(int v, int lane) {
  return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(lane));
}
__device__ __forceinline__ float bcast_f(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v),
                                                             __builtin_amdgcn_readfirstlane(lane)));
}


}  // namespace mp
