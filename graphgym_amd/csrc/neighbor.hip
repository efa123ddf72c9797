// The neighbour sampler on the device (include/mp_neighbor.h): the sampled computation tree of a batch of seed nodes as
// one subgraph — seeds plus sampled in-neighbours per hop.  graphgym_amd/neighbor.py drives the hops and restates every
// kernel in NumPy integers.
//
// One hop is three launches over the hop's frontier (the nodes that entered the batch at that hop), each with the hop's
// fanout s as a scalar:
//   mp_nbr_mark   the sampled columns of every frontier node into the batch's bitmap (atomicOr).  The next frontier is
//                 the new bitmap minus the old one, listed by sample.hip's mp_bitmap_word_counts / mp_bitmap_nodes.
//   mp_nbr_count  cnt[new id] = min(deg, s), one thread per frontier node: the row is not walked.
//   mp_nbr_fill   the row's entries in ascending base position, relabelled through the final bitmap's ranks.
// A frontier node v of hop h takes positions perm(j), j < s, of its row, perm the keyed bijection of [0, deg v) of
// draws.h under the group (h << 32) | v: s distinct positions and no rejection loop.  The round keys belong to the row:
// perm_keys once per lane, perm_walk per position.
//
// A row belongs to a group of kGroup = 16 lanes, as in sample.hip: the cycle walk of perm diverges per lane and a hub
// row takes up to 256 / 16 = 16 walks per lane, which a whole wave would otherwise wait for.  Every loop below runs
// over quantities the whole group shares.
//
// The in-group sort of mp_nbr_fill.  The k <= MP_NBR_MAX_FANOUT positions of a row are distinct, so the slot of a
// position is the number of positions below it.  The group writes its positions to its own 1 KiB of LDS (16 groups:
// 16 KiB a block), every lane then counts, for each position it owns, the positions below it: k reads per position,
// the same address across the group (a broadcast, no bank conflict), k * k / 16 compares per lane — 25 at k = 20,
// 4096 at k = 256.  The writers and the readers are lanes of one wave under one control flow, so the exchange needs
// no s_barrier: an LDS fence on either side of a scheduling barrier orders the group's writes before its reads, and the
// reads before the next row's writes.
#include "common.h"
#include "draws.h"
#include "../../include/mp_neighbor.h"

namespace mp {

constexpr int kGroup = 16;                          // lanes that own one row
constexpr int kGroupsPerBlock = kBlock / kGroup;
constexpr uint64_t kStream = (uint64_t)MP_NBR_STREAM;
constexpr uint64_t kSeedGroup = 1ull << 63;         // the group of the seed permutation: no (h << 32) | v reaches it

__device__ __forceinline__ int32_t row_take(int32_t deg, int32_t fanout) {
  return (fanout < 0 || deg <= fanout) ? deg : fanout;
}

__device__ __forceinline__ uint64_t hop_group(int32_t hop, int32_t v) {
  return ((uint64_t)(uint32_t)hop << 32) | (uint64_t)(uint32_t)v;
}

__device__ __forceinline__ int32_t new_id(const uint32_t* __restrict__ bitmap, const int32_t* __restrict__ word_rank,
                                          int32_t c) {
  return word_rank[c >> 5] + __popc(bitmap[c >> 5] & ((1u << (c & 31)) - 1u));
}

// the lanes of a group exchange through LDS (see the head of the file)
__device__ __forceinline__ void group_exchange() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

__global__ __launch_bounds__(kBlock) void nbr_seeds_kernel(const int32_t* __restrict__ pool, int64_t n_pool,
                                                           int64_t first, int64_t count, uint64_t seed, uint64_t epoch,
                                                           int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= count) return;
  const int64_t at = (int64_t)keyed_perm(seed ^ kStream, epoch, kSeedGroup, (uint64_t)(first + i), n_pool);
  out[i] = pool ? pool[at] : (int32_t)at;
}

__global__ __launch_bounds__(kBlock) void nbr_mark_kernel(const int32_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ col, int64_t N,
                                                          const int32_t* __restrict__ frontier, int64_t n, int32_t hop,
                                                          int32_t fanout, uint64_t seed, uint64_t step,
                                                          uint32_t* bitmap) {
  const int gl = threadIdx.x & (kGroup - 1);
  const int64_t stride = (int64_t)gridDim.x * kGroupsPerBlock;
  auto mark = [&](int32_t c) {
    const uint32_t bit = 1u << (c & 31);
    if (!(bitmap[c >> 5] & bit)) atomicOr(&bitmap[c >> 5], bit);      // (a bit is only ever set: a stale read costs one atomic)
  };
  for (int64_t i = (int64_t)blockIdx.x * kGroupsPerBlock + threadIdx.x / kGroup; i < n; i += stride) {
    const int32_t v = frontier[i];
    if (v < 0 || v >= N) continue;
    const int32_t rs = rowptr[v], deg = rowptr[v + 1] - rs, k = row_take(deg, fanout);
    if (k == deg) {
      for (int32_t j = gl; j < deg; j += kGroup) mark(col[rs + j]);
      continue;
    }
    uint32_t key[kFeistelRounds];
    perm_keys(seed ^ kStream, step, hop_group(hop, v), key);
    for (int32_t j = gl; j < k; j += kGroup) mark(col[rs + (int32_t)perm_walk(key, (uint64_t)j, deg)]);
  }
}

__global__ __launch_bounds__(kBlock) void nbr_count_kernel(const int32_t* __restrict__ rowptr, int64_t N,
                                                           const int32_t* __restrict__ frontier, int64_t n, int32_t hop,
                                                           int32_t fanout, const uint32_t* __restrict__ bitmap,
                                                           const int32_t* __restrict__ word_rank,
                                                           int32_t* __restrict__ cnt, int32_t* __restrict__ hop_out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int32_t v = frontier[i];
  if (v < 0 || v >= N) return;
  const int32_t k = new_id(bitmap, word_rank, v);
  cnt[k] = row_take(rowptr[v + 1] - rowptr[v], fanout);
  hop_out[k] = hop;
}

__global__ __launch_bounds__(kBlock) void nbr_fill_kernel(const int32_t* __restrict__ rowptr,
                                                          const int32_t* __restrict__ col, int64_t N,
                                                          const int32_t* __restrict__ frontier, int64_t n, int32_t hop,
                                                          int32_t fanout, uint64_t seed, uint64_t step,
                                                          const uint32_t* __restrict__ bitmap,
                                                          const int32_t* __restrict__ word_rank,
                                                          const int32_t* __restrict__ rowptr_sub,
                                                          int32_t* __restrict__ col_sub,
                                                          int32_t* __restrict__ base_entry) {
  __shared__ int32_t drawn[kGroupsPerBlock][MP_NBR_MAX_FANOUT];
  const int gl = threadIdx.x & (kGroup - 1);
  int32_t* mine = drawn[threadIdx.x / kGroup];
  const int64_t stride = (int64_t)gridDim.x * kGroupsPerBlock;
  for (int64_t i = (int64_t)blockIdx.x * kGroupsPerBlock + threadIdx.x / kGroup; i < n; i += stride) {
    const int32_t v = frontier[i];
    if (v < 0 || v >= N) continue;
    const int32_t rs = rowptr[v], deg = rowptr[v + 1] - rs, k = row_take(deg, fanout);
    const int32_t at = rowptr_sub[new_id(bitmap, word_rank, v)];
    if (k == deg) {                                   // the whole row, in order
      for (int32_t j = gl; j < deg; j += kGroup) {
        col_sub[at + j] = new_id(bitmap, word_rank, col[rs + j]);
        base_entry[at + j] = rs + j;
      }
      continue;
    }
    uint32_t key[kFeistelRounds];                     // (k < deg, so k = fanout <= MP_NBR_MAX_FANOUT)
    perm_keys(seed ^ kStream, step, hop_group(hop, v), key);
    for (int32_t j = gl; j < k; j += kGroup) mine[j] = (int32_t)perm_walk(key, (uint64_t)j, deg);
    group_exchange();
    for (int32_t j = gl; j < k; j += kGroup) {
      const int32_t p = mine[j];
      int32_t slot = 0;
      for (int32_t t = 0; t < k; ++t) slot += mine[t] < p;
      col_sub[at + slot] = new_id(bitmap, word_rank, col[rs + p]);
      base_entry[at + slot] = rs + p;
    }
    group_exchange();                                 // (the next row's positions overwrite these)
  }
}

constexpr int64_t kMaxEntries = (int64_t)INT32_MAX - kGroup;     // (rs + j steps up to kGroup past the row's end in int32)

static inline int group_grid(int64_t n) {
  int64_t b = ceil_div(n, kGroupsPerBlock);
  if (b > kNumCU * 32) b = kNumCU * 32;
  return (int)(b < 1 ? 1 : b);
}

static inline int fanout_status(int32_t fanout) {
  if (fanout == 0 || fanout < -1) return MP_ERR_INVALID_ARG;
  return fanout > MP_NBR_MAX_FANOUT ? MP_ERR_UNSUPPORTED : MP_OK;
}

}  // namespace mp

using namespace mp;

extern "C" int mp_nbr_seeds(const int32_t* pool, int64_t n_pool, int64_t first, int64_t count, uint64_t seed,
                            uint64_t epoch, int32_t* out, mp_stream_t stream) {
  if (n_pool < 0 || first < 0 || count < 0 || count > n_pool || first > n_pool - count) return MP_ERR_INVALID_ARG;
  if (count > 0 && !out) return MP_ERR_INVALID_ARG;
  if (n_pool > INT32_MAX) return MP_ERR_UNSUPPORTED;
  if (count == 0) return MP_OK;
  hipLaunchKernelGGL(nbr_seeds_kernel, dim3((unsigned)ceil_div(count, kBlock)), dim3(kBlock), 0, as_stream(stream), pool,
                     n_pool, first, count, seed, epoch, out);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

extern "C" int mp_nbr_mark(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, const int32_t* frontier,
                           int64_t n_frontier, int32_t hop, int32_t fanout, uint64_t seed, uint64_t step,
                           uint32_t* bitmap, mp_stream_t stream) {
  if (N < 0 || nnz < 0 || n_frontier < 0 || hop < 0) return MP_ERR_INVALID_ARG;
  if (const int st = fanout_status(fanout)) return st;
  if (!rowptr || (nnz > 0 && !col)) return MP_ERR_INVALID_ARG;
  if (n_frontier > 0 && (!frontier || !bitmap || N == 0)) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || nnz > kMaxEntries) return MP_ERR_UNSUPPORTED;
  if (n_frontier == 0) return MP_OK;
  hipLaunchKernelGGL(nbr_mark_kernel, dim3((unsigned)group_grid(n_frontier)), dim3(kBlock), 0, as_stream(stream), rowptr,
                     col, N, frontier, n_frontier, hop, fanout, seed, step, bitmap);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

extern "C" int mp_nbr_count(const int32_t* rowptr, int64_t N, const int32_t* frontier, int64_t n_frontier, int32_t hop,
                            int32_t fanout, const uint32_t* bitmap, const int32_t* word_rank, int32_t* cnt,
                            int32_t* hop_out, mp_stream_t stream) {
  if (N < 0 || n_frontier < 0 || hop < 0) return MP_ERR_INVALID_ARG;
  if (const int st = fanout_status(fanout)) return st;
  if (!rowptr) return MP_ERR_INVALID_ARG;
  if (n_frontier > 0 && (!frontier || !bitmap || !word_rank || !cnt || !hop_out || N == 0)) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || ceil_div(n_frontier, kBlock) > INT32_MAX) return MP_ERR_UNSUPPORTED;
  if (n_frontier == 0) return MP_OK;
  hipLaunchKernelGGL(nbr_count_kernel, dim3((unsigned)ceil_div(n_frontier, kBlock)), dim3(kBlock), 0, as_stream(stream),
                     rowptr, N, frontier, n_frontier, hop, fanout, bitmap, word_rank, cnt, hop_out);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

extern "C" int mp_nbr_fill(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, const int32_t* frontier,
                           int64_t n_frontier, int32_t hop, int32_t fanout, uint64_t seed, uint64_t step,
                           const uint32_t* bitmap, const int32_t* word_rank, const int32_t* rowptr_sub, int32_t* col_sub,
                           int32_t* base_entry, mp_stream_t stream) {
  if (N < 0 || nnz < 0 || n_frontier < 0 || hop < 0) return MP_ERR_INVALID_ARG;
  if (const int st = fanout_status(fanout)) return st;
  if (!rowptr || (nnz > 0 && !col)) return MP_ERR_INVALID_ARG;
  if (n_frontier > 0 && (!frontier || !bitmap || !word_rank || !rowptr_sub || !col_sub || !base_entry || N == 0))
    return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || nnz > kMaxEntries) return MP_ERR_UNSUPPORTED;
  if (n_frontier == 0) return MP_OK;
  hipLaunchKernelGGL(nbr_fill_kernel, dim3((unsigned)group_grid(n_frontier)), dim3(kBlock), 0, as_stream(stream), rowptr,
                     col, N, frontier, n_frontier, hop, fanout, seed, step, bitmap, word_rank, rowptr_sub, col_sub,
                     base_entry);
  MP_LAUNCH_CHECK();
  return MP_OK;
}
