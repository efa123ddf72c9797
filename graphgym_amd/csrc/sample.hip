// Mini-batch subgraph samplers on the device (GraphGym's train.sampler = random_node | saint_node | saint_edge | saint_rw,
// graphgym/config.py:215,242-248, graphgym/loader_pyg.py:204-255): the four are one operation with different draws — pick
// a node set, then take the induced subgraph of the base CSR (row r = in-edges of r, columns ascending inside a row).
//
// The key of a draw, in integers only (mix64 and kGolden of draws.h; graphgym_amd/samplers.py restates it):
//   key(seed, offset, i, t) = mix64((mix64((mix64((mix64(seed + kGolden) ^ offset) + kGolden) ^ i) + kGolden) ^ t) + kGolden)
// and a bounded draw is mulhi(key, n) = the high 64 bits of key * n, a value of [0, n).  Draw i of step `offset` depends
// on (seed, offset, i, t) and the graph alone, never on the launch geometry.
//
// Draws (one thread per draw, nothing but reads and the stores of its own outputs):
//   mp_sample_parts       part[v] = mulhi(key(seed, epoch, v, 0), P) for every node v: the P parts of an epoch
//                         partition the nodes (random_node)
//   mp_sample_entry_rows  draw i: e = mulhi(key(seed, offset, i, 0), nnz), out[i] = the row that holds entry e
//                         (upper_bound in rowptr): P(node) proportional to its stored in-degree (saint_node)
//   mp_sample_walks       out [K, L + 1]: out[i, 0] = pool[mulhi(key(.., i, 0), n_pool)] (pool = NULL: all of [0, N)),
//                         out[i, t] = col[rowptr[cur] + mulhi(key(.., i, t), deg(cur))], cur = out[i, t - 1]; a node
//                         with an empty row stays where it is (saint_rw: L = walk_length; saint_edge: L = 1 over the
//                         pool of non-empty rows)
//
// Node set -> ascending list: a bitmap of N bits (uint32 words, bit c & 31 of word c >> 5).
//   mp_bitmap_mark         atomicOr of the drawn nodes (an entry below 0 is no draw and is skipped; one at or above N
//                          sets flags[0] and is skipped); the caller zeroes bitmap and flags
//   mp_bitmap_word_counts  popcount per word; the caller's inclusive prefix sum behind a leading 0 is word_rank [W + 1]
//   mp_bitmap_nodes        orig [n_sub] ascending: word w writes its set bits from word_rank[w] on
// The new id of a member c is word_rank[c >> 5] + popc(word[c >> 5] & ((1u << (c & 31)) - 1)): two tables of N / 8 bytes
// each (1.25 MB at N = 1e7, together inside one XCD's 4 MiB L2) instead of an int32 [N] table.
//
// Induced subgraph: two passes over the selected rows only, a row walked by a group of kGroup = 16 lanes in chunks of 16
// (16 chunks per step while that many are left, then four, then the last one alone: walk_row).
//   mp_induced_count  cnt[k] = entries of row orig[k] whose column is a member
//   mp_induced_fill   col_sub (new ids) and base_entry (the entry's position in the base CSR) from rowptr_sub[k] on; inside
//                     a chunk an entry's slot is the prefix popcount of the group's ballot, across chunks a running offset:
//                     order is kept, and since the relabelling is monotone col_sub ascends inside a row and equal entries
//                     keep the base's order.  Self entries and repeated entries of the base are kept as stored.
#include "common.h"
#include "draws.h"

namespace mp {

constexpr int kGroup = 16;                          // lanes that walk one row
constexpr int kGroupsPerBlock = kBlock / kGroup;

__device__ __forceinline__ uint64_t draw_key(uint64_t seed, uint64_t offset, uint64_t i, uint64_t t) {
  uint64_t h = mix64(seed + kGolden);
  h = mix64((h ^ offset) + kGolden);
  h = mix64((h ^ i) + kGolden);
  return mix64((h ^ t) + kGolden);
}

__device__ __forceinline__ int64_t bounded(uint64_t key, int64_t n) { return (int64_t)__umul64hi(key, (uint64_t)n); }

__global__ __launch_bounds__(kBlock) void sample_parts_kernel(int64_t N, int64_t P, uint64_t seed, uint64_t epoch,
                                                              int32_t* __restrict__ part) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= N) return;
  part[v] = (int32_t)bounded(draw_key(seed, epoch, (uint64_t)v, 0), P);
}

__global__ __launch_bounds__(kBlock) void sample_entry_rows_kernel(const int32_t* __restrict__ rowptr, int64_t N,
                                                                   int64_t nnz, int64_t K, uint64_t seed, uint64_t offset,
                                                                   int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= K) return;
  const int64_t e = bounded(draw_key(seed, offset, (uint64_t)i, 0), nnz);
  int64_t r = upper_bound(rowptr, 0, N + 1, e) - 1;           // the last row that starts at or before e: it is not empty
  out[i] = (int32_t)(r < 0 ? 0 : (r >= N ? N - 1 : r));
}

__global__ __launch_bounds__(kBlock) void sample_walks_kernel(const int32_t* __restrict__ rowptr,
                                                              const int32_t* __restrict__ col, int64_t N,
                                                              const int32_t* __restrict__ pool, int64_t n_pool, int64_t K,
                                                              int32_t L, uint64_t seed, uint64_t offset,
                                                              int32_t* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= K) return;
  const int64_t slot = bounded(draw_key(seed, offset, (uint64_t)i, 0), pool ? n_pool : N);
  int32_t cur = pool ? pool[slot] : (int32_t)slot;
  int32_t* __restrict__ mine = out + i * ((int64_t)L + 1);
  mine[0] = cur;
  for (int32_t t = 1; t <= L; ++t) {
    const int32_t rs = rowptr[cur], deg = rowptr[cur + 1] - rs;
    if (deg > 0) cur = col[rs + bounded(draw_key(seed, offset, (uint64_t)i, (uint64_t)t), deg)];
    mine[t] = cur;
  }
}

__global__ __launch_bounds__(kBlock) void bitmap_mark_kernel(const int32_t* __restrict__ nodes, int64_t n, int64_t N,
                                                             uint32_t* __restrict__ bitmap, int32_t* __restrict__ flags) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const int32_t v = nodes[i];
  if (v < 0) return;
  if (v >= N) {
    flags[0] = 1;
    return;
  }
  atomicOr(&bitmap[v >> 5], 1u << (v & 31));
}

__global__ __launch_bounds__(kBlock) void bitmap_word_counts_kernel(const uint32_t* __restrict__ bitmap, int64_t W,
                                                                    int32_t* __restrict__ counts) {
  const int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (w < W) counts[w] = __popc(bitmap[w]);
}

__global__ __launch_bounds__(kBlock) void bitmap_nodes_kernel(const uint32_t* __restrict__ bitmap,
                                                              const int32_t* __restrict__ word_rank, int64_t W,
                                                              int32_t* __restrict__ orig) {
  const int64_t w = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (w >= W) return;
  uint32_t bits = bitmap[w];
  int32_t at = word_rank[w];
  while (bits) {
    orig[at++] = (int32_t)(w << 5) + (__ffs(bits) - 1);
    bits &= bits - 1;
  }
}

// the 16 ballot bits of this lane's group (every lane of the group is active: the callers' loops are group-uniform)
__device__ __forceinline__ uint32_t group_ballot(bool p) {
  const int lane = threadIdx.x & (kWave - 1);
  return (uint32_t)(__ballot(p) >> (lane & ~(kGroup - 1))) & ((1u << kGroup) - 1u);
}

// U chunks of a row from entry b on: lane gl of the group takes entries b + j * kGroup + gl.  All U column loads are
// issued before the U bitmap loads they feed (a lane beyond the row's end re-reads the row's first entry, so every load
// is unconditional), then m[j] = the group's ballot of "entry j is a member".
template <int U>
__device__ __forceinline__ void member_chunks(const int32_t* __restrict__ col, const uint32_t* __restrict__ bitmap,
                                              int32_t b, int gl, int32_t rs, int32_t re, int32_t (&e)[U],
                                              int32_t (&c)[U], uint32_t (&word)[U], uint32_t (&m)[U]) {
#pragma unroll
  for (int j = 0; j < U; ++j) {
    e[j] = b + j * kGroup + gl;
    c[j] = col[e[j] < re ? e[j] : rs];
  }
#pragma unroll
  for (int j = 0; j < U; ++j) word[j] = bitmap[c[j] >> 5];
#pragma unroll
  for (int j = 0; j < U; ++j) m[j] = group_ballot(e[j] < re && ((word[j] >> (c[j] & 31)) & 1u));
}

// A row's walk is a chain of dependent gathers (column, then bitmap word), so its length in steps decides how long a
// hub holds its group: while kLong = 16 whole chunks are left a step takes all 16 (256 entries, every load of the step
// in flight together), then kUnroll = 4 chunks per step while more than one is left, the last chunk — the only one of a
// short row — alone.  each(e, c, word, m) receives the step's chunks as arrays, in entry order.
constexpr int kUnroll = 4, kLong = 16;

template <int U, class Fn>
__device__ __forceinline__ void walk_chunks(const int32_t* __restrict__ col, const uint32_t* __restrict__ bitmap,
                                            int32_t b, int gl, int32_t rs, int32_t re, Fn&& each) {
  int32_t e[U], c[U];
  uint32_t word[U], m[U];
  member_chunks<U>(col, bitmap, b, gl, rs, re, e, c, word, m);
  each(e, c, word, m);
}

template <class Fn>
__device__ __forceinline__ void walk_row(const int32_t* __restrict__ col, const uint32_t* __restrict__ bitmap, int gl,
                                         int32_t rs, int32_t re, Fn&& each) {
  int32_t b = rs;
  for (; re - b >= kGroup * kLong; b += kGroup * kLong) walk_chunks<kLong>(col, bitmap, b, gl, rs, re, each);
  for (; re - b > kGroup; b += kGroup * kUnroll) walk_chunks<kUnroll>(col, bitmap, b, gl, rs, re, each);
  if (b < re) walk_chunks<1>(col, bitmap, b, gl, rs, re, each);
}

__global__ __launch_bounds__(kBlock) void induced_count_kernel(const int32_t* __restrict__ rowptr,
                                                               const int32_t* __restrict__ col,
                                                               const int32_t* __restrict__ orig, int64_t n_sub,
                                                               const uint32_t* __restrict__ bitmap,
                                                               int32_t* __restrict__ cnt) {
  const int gl = threadIdx.x & (kGroup - 1);
  const int64_t stride = (int64_t)gridDim.x * kGroupsPerBlock;
  for (int64_t k = (int64_t)blockIdx.x * kGroupsPerBlock + threadIdx.x / kGroup; k < n_sub; k += stride) {
    const int32_t r = orig[k];
    int32_t total = 0;
    walk_row(col, bitmap, gl, rowptr[r], rowptr[r + 1], [&](auto& e, auto& c, auto& word, auto& m) {
#pragma unroll
      for (int j = 0; j < (int)(sizeof(m) / sizeof(m[0])); ++j) total += __popc(m[j]);
    });
    if (gl == 0) cnt[k] = total;
  }
}

__global__ __launch_bounds__(kBlock) void induced_fill_kernel(const int32_t* __restrict__ rowptr,
                                                              const int32_t* __restrict__ col,
                                                              const int32_t* __restrict__ orig, int64_t n_sub,
                                                              const uint32_t* __restrict__ bitmap,
                                                              const int32_t* __restrict__ word_rank,
                                                              const int32_t* __restrict__ rowptr_sub,
                                                              int32_t* __restrict__ col_sub,
                                                              int32_t* __restrict__ base_entry) {
  const int gl = threadIdx.x & (kGroup - 1);
  const int64_t stride = (int64_t)gridDim.x * kGroupsPerBlock;
  for (int64_t k = (int64_t)blockIdx.x * kGroupsPerBlock + threadIdx.x / kGroup; k < n_sub; k += stride) {
    const int32_t r = orig[k];
    int32_t at = rowptr_sub[k];
    const int32_t end = rowptr_sub[k + 1];
    walk_row(col, bitmap, gl, rowptr[r], rowptr[r + 1], [&](auto& e, auto& c, auto& word, auto& m) {
      constexpr int U = (int)(sizeof(m) / sizeof(m[0]));
      int32_t rank[U];
#pragma unroll
      for (int j = 0; j < U; ++j) rank[j] = ((m[j] >> gl) & 1u) ? word_rank[c[j] >> 5] : 0;   // the members' rank gathers: together
#pragma unroll
      for (int j = 0; j < U; ++j) {
        const int32_t pos = at + __popc(m[j] & ((1u << gl) - 1u));
        if (((m[j] >> gl) & 1u) && pos < end) {    // (pos < end always holds for the counts of mp_induced_count)
          col_sub[pos] = rank[j] + __popc(word[j] & ((1u << (c[j] & 31)) - 1u));
          base_entry[pos] = e[j];
        }
        at += __popc(m[j]);
      }
    });
  }
}

// (a row walk steps up to kGroup * kUnroll entries past the row's end in int32)
constexpr int64_t kMaxEntries = (int64_t)INT32_MAX - kGroup * kUnroll;

static inline bool flat_ok(int64_t n) { return ceil_div(n, kBlock) <= INT32_MAX; }

}  // namespace mp

using namespace mp;

extern "C" int mp_sample_parts(int64_t N, int64_t num_parts, uint64_t seed, uint64_t epoch, int32_t* part,
                               mp_stream_t stream) {
  if (N < 0 || num_parts < 1) return MP_ERR_INVALID_ARG;
  if (N > 0 && !part) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || num_parts > INT32_MAX) return MP_ERR_UNSUPPORTED;
  if (N == 0) return MP_OK;
  hipLaunchKernelGGL(sample_parts_kernel, dim3((unsigned)ceil_div(N, kBlock)), dim3(kBlock), 0, as_stream(stream), N,
                     num_parts, seed, epoch, part);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

extern "C" int mp_sample_entry_rows(const int32_t* rowptr, int64_t N, int64_t nnz, int64_t K, uint64_t seed,
                                    uint64_t offset, int32_t* out, mp_stream_t stream) {
  if (N < 0 || nnz < 0 || K < 0) return MP_ERR_INVALID_ARG;
  if (!rowptr) return MP_ERR_INVALID_ARG;
  if (K > 0 && (!out || N == 0 || nnz == 0)) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || nnz > INT32_MAX || !flat_ok(K)) return MP_ERR_UNSUPPORTED;
  if (K == 0) return MP_OK;
  hipLaunchKernelGGL(sample_entry_rows_kernel, dim3((unsigned)ceil_div(K, kBlock)), dim3(kBlock), 0, as_stream(stream),
                     rowptr, N, nnz, K, seed, offset, out);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

extern "C" int mp_sample_walks(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, const int32_t* pool,
                               int64_t n_pool, int64_t K, int32_t walk_length, uint64_t seed, uint64_t offset,
                               int32_t* out, mp_stream_t stream) {
  if (N < 0 || nnz < 0 || K < 0 || n_pool < 0 || walk_length < 0) return MP_ERR_INVALID_ARG;
  if (!rowptr) return MP_ERR_INVALID_ARG;
  if (nnz > 0 && !col) return MP_ERR_INVALID_ARG;
  if (K > 0 && (!out || N == 0 || (pool && n_pool == 0))) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || nnz > INT32_MAX || n_pool > INT32_MAX || !flat_ok(K)) return MP_ERR_UNSUPPORTED;
  if (K == 0) return MP_OK;
  hipLaunchKernelGGL(sample_walks_kernel, dim3((unsigned)ceil_div(K, kBlock)), dim3(kBlock), 0, as_stream(stream), rowptr,
                     col, N, pool, n_pool, K, walk_length, seed, offset, out);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

extern "C" int mp_bitmap_mark(const int32_t* nodes, int64_t n, int64_t N, uint32_t* bitmap, int32_t* flags,
                              mp_stream_t stream) {
  if (n < 0 || N < 0) return MP_ERR_INVALID_ARG;
  if (n > 0 && (!nodes || !bitmap || !flags)) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || !flat_ok(n)) return MP_ERR_UNSUPPORTED;
  if (n == 0) return MP_OK;
  hipLaunchKernelGGL(bitmap_mark_kernel, dim3((unsigned)ceil_div(n, kBlock)), dim3(kBlock), 0, as_stream(stream), nodes, n,
                     N, bitmap, flags);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

extern "C" int mp_bitmap_word_counts(const uint32_t* bitmap, int64_t n_words, int32_t* counts, mp_stream_t stream) {
  if (n_words < 0) return MP_ERR_INVALID_ARG;
  if (n_words > 0 && (!bitmap || !counts)) return MP_ERR_INVALID_ARG;
  if (n_words > INT32_MAX) return MP_ERR_UNSUPPORTED;
  if (n_words == 0) return MP_OK;
  hipLaunchKernelGGL(bitmap_word_counts_kernel, dim3((unsigned)ceil_div(n_words, kBlock)), dim3(kBlock), 0,
                     as_stream(stream), bitmap, n_words, counts);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

extern "C" int mp_bitmap_nodes(const uint32_t* bitmap, const int32_t* word_rank, int64_t n_words, int32_t* orig,
                               mp_stream_t stream) {
  if (n_words < 0) return MP_ERR_INVALID_ARG;
  if (n_words > 0 && (!bitmap || !word_rank || !orig)) return MP_ERR_INVALID_ARG;
  if (n_words > INT32_MAX) return MP_ERR_UNSUPPORTED;
  if (n_words == 0) return MP_OK;
  hipLaunchKernelGGL(bitmap_nodes_kernel, dim3((unsigned)ceil_div(n_words, kBlock)), dim3(kBlock), 0, as_stream(stream),
                     bitmap, word_rank, n_words, orig);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

static inline int group_grid(int64_t n_sub) {
  int64_t b = ceil_div(n_sub, kGroupsPerBlock);
  if (b > kNumCU * 32) b = kNumCU * 32;
  return (int)(b < 1 ? 1 : b);
}

extern "C" int mp_induced_count(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, const int32_t* orig,
                                int64_t n_sub, const uint32_t* bitmap, int32_t* cnt, mp_stream_t stream) {
  if (N < 0 || nnz < 0 || n_sub < 0 || n_sub > N) return MP_ERR_INVALID_ARG;
  if (!rowptr) return MP_ERR_INVALID_ARG;
  if (nnz > 0 && !col) return MP_ERR_INVALID_ARG;
  if (n_sub > 0 && (!orig || !bitmap || !cnt)) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || nnz > kMaxEntries) return MP_ERR_UNSUPPORTED;
  if (n_sub == 0) return MP_OK;
  hipLaunchKernelGGL(induced_count_kernel, dim3((unsigned)group_grid(n_sub)), dim3(kBlock), 0, as_stream(stream), rowptr,
                     col, orig, n_sub, bitmap, cnt);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

extern "C" int mp_induced_fill(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, const int32_t* orig,
                               int64_t n_sub, const uint32_t* bitmap, const int32_t* word_rank, const int32_t* rowptr_sub,
                               int32_t* col_sub, int32_t* base_entry, mp_stream_t stream) {
  if (N < 0 || nnz < 0 || n_sub < 0 || n_sub > N) return MP_ERR_INVALID_ARG;
  if (!rowptr) return MP_ERR_INVALID_ARG;
  if (nnz > 0 && !col) return MP_ERR_INVALID_ARG;
  if (n_sub > 0 && (!orig || !bitmap || !word_rank || !rowptr_sub || !col_sub || !base_entry)) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || nnz > kMaxEntries) return MP_ERR_UNSUPPORTED;
  if (n_sub == 0) return MP_OK;
  hipLaunchKernelGGL(induced_fill_kernel, dim3((unsigned)group_grid(n_sub)), dim3(kBlock), 0, as_stream(stream), rowptr,
                     col, orig, n_sub, bitmap, word_rank, rowptr_sub, col_sub, base_entry);
  MP_LAUNCH_CHECK();
  return MP_OK;
}
