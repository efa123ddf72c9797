// Integer helpers shared by the keyed samplers (link.hip: negative sampling; sample.hip: mini-batch subgraph samplers)
// and the keyed dropout mask (bn_drop.hip).
// Integer mixing only: a draw is a pure function of its key, never of the launch geometry.
#pragma once
#include "common.h"

namespace mp {

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

__host__ __device__ __forceinline__ uint64_t mix64(uint64_t z) {       // (the splitmix64 finaliser)
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// ---- the keyed dropout mask (bn_drop.hip; graphgym_amd.nn.dropout_keep_host restates it in NumPy integers) ------------
// keep(seed, offset, r, c) over an [N, d] operand is a pure function of the 64-bit seed, the 64-bit call offset and the
// LOGICAL row r and column c — not of addresses, leading dimensions, vector width, grid size or the kernel that asks:
//   q    = ceil(d / 4)
//   key  = mix64((mix64(seed + kGolden) ^ offset) + kGolden)          once per call (drop_key, on the host)
//   h    = mix64((key ^ (r * q + c / 4)) + kGolden)                   uint64 arithmetic; one hash per aligned group of
//                                                                     four columns: its 16-bit lanes are their draws
//   keep = ((h >> 16 * (c % 4)) & 0xffff) >= T                        T = round(p * 65536) in [0, 65536]
// A kept element is multiplied by scale = float(65536 / (65536 - T)), an fp32 constant of the host (0 when T = 65536:
// nothing is kept); a dropped one is +0.
struct DropKey {
  uint64_t key;
  uint32_t T;
  float scale;
  int32_t q;         // ceil(d / 4)
};

__host__ __device__ __forceinline__ uint64_t drop_key(uint64_t seed, uint64_t offset) {
  return mix64((mix64(seed + kGolden) ^ offset) + kGolden);
}

// the mask of columns c0 .. c0 + W of row r.  W = 4: c0 is a multiple of 4, one hash for the four; W = 1: a hash per
// element, lane c0 % 4
template <int W>
__device__ __forceinline__ void drop_keep(const DropKey& k, int64_t r, int c0, bool (&m)[W]) {
  static_assert(W == 1 || W == 4, "a thread owns one column or one aligned group of four");
  const uint64_t h = mix64((k.key ^ ((uint64_t)r * (uint64_t)k.q + (uint64_t)(c0 >> 2))) + kGolden);
  if constexpr (W == 4) {
#pragma unroll
    for (int j = 0; j < 4; ++j) m[j] = ((uint32_t)(h >> (16 * j)) & 0xffffu) >= k.T;
  } else {
    m[0] = ((uint32_t)(h >> (16 * (c0 & 3))) & 0xffffu) >= k.T;
  }
}

// first index in [lo, hi) whose value is above key
template <class T>
__device__ __forceinline__ int64_t upper_bound(const T* __restrict__ a, int64_t lo, int64_t hi, int64_t key) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)a[mid] <= key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

}  // namespace mp
