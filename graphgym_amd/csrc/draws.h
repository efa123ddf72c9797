// Integer helpers shared by the keyed samplers (link.hip: negative sampling; sample.hip: mini-batch subgraph samplers).
// Integer mixing only: a draw is a pure function of its key, never of the launch geometry.
#pragma once
#include "common.h"

namespace mp {

constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ uint64_t mix64(uint64_t z) {       // (the splitmix64 finaliser)
  z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
  z ^= z >> 27; z *= 0x94D049BB133111EBull;
  return z ^ (z >> 31);
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
