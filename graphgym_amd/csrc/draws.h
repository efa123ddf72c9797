// Integer helpers shared by the keyed samplers (link.hip: negative sampling; sample.hip: mini-batch subgraph samplers;
// neighbor.hip: the neighbour sampler; centrality.hip: one-hot ids) and the keyed dropout mask (bn_drop.hip).
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

// ---- the keyed bijection (link.hip: ranks of non-edges; centrality.hip: one-hot ids; neighbor.hip: row positions) ---------
// perm(i) on [0, C): a balanced Feistel network on 2b bits, b = max(1, ceil(bits(C - 1) / 2)), walked until the value is
// below C (cycle walking: the domain is below 4 C, fewer than 4 encryptions on average, and the walk from a start below
// C always returns below C because the network is a bijection).  The round keys come from (seed, offset, g).  The caller
// guarantees 0 <= i < C: a walk from a start outside the domain need not end.
constexpr int kFeistelRounds = 6;

__device__ __forceinline__ uint32_t feistel_round(uint32_t half, uint32_t key) {      // (the murmur3 finaliser)
  uint32_t x = half + key;
  x ^= x >> 16; x *= 0x85EBCA6Bu;
  x ^= x >> 13; x *= 0xC2B2AE35u;
  return x ^ (x >> 16);
}

// the round keys of (seed, offset, g): a caller that permutes several i under one g (neighbor.hip: the positions of one
// row) computes them once
__device__ __forceinline__ void perm_keys(uint64_t seed, uint64_t offset, uint64_t g, uint32_t (&key)[kFeistelRounds]) {
  uint64_t h = mix64(seed + kGolden);
  h = mix64((h ^ offset) + kGolden);
  h = mix64((h ^ g) + kGolden);
#pragma unroll
  for (int k = 0; k < kFeistelRounds; ++k) key[k] = (uint32_t)(mix64(h + (uint64_t)(k + 1) * kGolden) >> 32);
}

__device__ __forceinline__ uint64_t perm_walk(const uint32_t (&key)[kFeistelRounds], uint64_t i, int64_t C) {
  const int bits = C > 1 ? 64 - __builtin_clzll((uint64_t)(C - 1)) : 0;
  const int b = bits > 1 ? (bits + 1) >> 1 : 1;
  const uint32_t mask = b >= 32 ? 0xFFFFFFFFu : ((1u << b) - 1u);
  uint64_t x = i;
  do {
    uint32_t L = (uint32_t)(x >> b), R = (uint32_t)x & mask;
#pragma unroll
    for (int k = 0; k < kFeistelRounds; ++k) {
      const uint32_t t = L ^ (feistel_round(R, key[k]) & mask);
      L = R;
      R = t;
    }
    x = ((uint64_t)L << b) | R;
  } while (x >= (uint64_t)C);
  return x;
}

__device__ __forceinline__ uint64_t keyed_perm(uint64_t seed, uint64_t offset, uint64_t g, uint64_t i, int64_t C) {
  uint32_t key[kFeistelRounds];
  perm_keys(seed, offset, g, key);
  return perm_walk(key, i, C);
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

// the graph (or the slot range) that holds x: the last g in [0, G) with ptr[g] <= x
__device__ __forceinline__ int64_t range_of(const int64_t* __restrict__ ptr, int64_t G, int64_t x) {
  int64_t g = upper_bound(ptr, 0, G + 1, x) - 1;
  return g < 0 ? 0 : (g >= G ? G - 1 : g);
}

}  // namespace mp
