// Structural labels and features of graphgym/models/feature_augment.py:51-107 on the device: the integers behind
// nx.clustering / nx.average_clustering (mp_csr_triangles) and behind the shortest-path means of path_len_fun and
// nx.average_shortest_path_length (mp_hop_sums).  Both write integers only: no float atomics, bit-reproducible.
//
// Triangles (mp_csr_triangles).  The unit of work is a stored entry (u, v) of a symmetric CSR without repeated entries
// (columns ascending inside a row): its share of tri2[u] is |{w in row u and row v : w != u, w != v}|.  The SHORTER of
// the two rows is spread over the kTriGroup lanes of a group and every element is binary-searched in the LONGER one:
//   probes = sum over entries of min(d_u, d_v) * ceil(log2 max(d_u, d_v))
// (the cost model DESIGN 4.11 prices).  Entries are handed out in contiguous, entry-balanced chunks — kTriChunk per
// wave, kTriRun consecutive ones per group — with the row read from row_of (mp_csr_row_ids): a hub row of 1e4 entries
// is shared by ~40 waves and no thread walks a row on its own.  A group sums its lanes' counts per row; the rows a
// group owns alone inside its wave (neither its first nor its last) go out with one 64-bit integer atomicAdd each, the
// first and last rows of the eight groups are merged across the wave first: one atomicAdd per (wave, row).
//
// Hop sums (mp_hop_sums).  One workgroup per source runs the breadth-first search of hop_bfs_kernel (edge.hip) inside
// the source's graph, visited / frontier / next bitmaps in LDS (3 x 8 KiB for up to 2^16 nodes).  It closes no pairs:
// level l adds l * popcount(new frontier) to the source's sum and the popcount to its count, until nothing new is
// reached.
#include "common.h"

namespace mp {

// ---- triangles ---------------------------------------------------------------------------------------------------

constexpr int kTriGroup = 8;                       // lanes that share one stored entry
constexpr int kTriGroups = kWave / kTriGroup;      // entries a wave works on at a time
constexpr int kTriRun = 32;                        // consecutive entries of one group
constexpr int kTriChunk = kTriGroups * kTriRun;    // consecutive entries of one wave

__device__ __forceinline__ int row_holds(const int32_t* __restrict__ col, int32_t lo, int32_t hi, int32_t key) {
  while (lo < hi) {
    const int32_t mid = lo + ((hi - lo) >> 1);
    const int32_t c = col[mid];
    if (c == key) return 1;
    if (c < key) lo = mid + 1; else hi = mid;
  }
  return 0;
}

__device__ __forceinline__ int64_t group_sum(int64_t v) {
#pragma unroll
  for (int o = kTriGroup >> 1; o > 0; o >>= 1) v += __shfl_xor(v, o, kTriGroup);
  return v;
}

// deg[u] = entries of row u besides its self entry (at most one: no entry is stored twice)
__global__ __launch_bounds__(kBlock) void csr_loopless_degree_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t N, int32_t* __restrict__ deg) {
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  for (int64_t u = (int64_t)blockIdx.x * kBlock + threadIdx.x; u < N; u += stride) {
    const int32_t lo = rowptr[u], hi = rowptr[u + 1];
    deg[u] = hi - lo - row_holds(col, lo, hi, (int32_t)u);
  }
}

__global__ __launch_bounds__(kBlock) void csr_triangles_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ row_of,
    int64_t N, int64_t nnz, unsigned long long* __restrict__ tri2) {
  const int lane = threadIdx.x & (kWave - 1);
  const int sub = lane & (kTriGroup - 1), grp = lane / kTriGroup;
  const int64_t wave = (int64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave;
  const int64_t e0 = wave * kTriChunk + (int64_t)grp * kTriRun;
  const int64_t e1 = e0 + kTriRun < nnz ? e0 + kTriRun : nnz;
  // the group's open row and this lane's count for it; the group's first row is kept back for the merge below
  int32_t cur = -1, first_row = -1;
  int64_t acc = 0, first_cnt = 0;
  bool interior = false;                                   // the open row is not the group's first
  for (int64_t e = e0; e < e1; ++e) {                      // (group-uniform: e, u, v and the branches on them)
    const int32_t u = row_of[e], v = col[e];
    if (u != cur) {
      if (cur >= 0) {
        const int64_t total = group_sum(acc);
        if (!interior) { first_row = cur; first_cnt = total; interior = true; }
        else if (sub == 0 && total) atomicAdd(&tri2[cur], (unsigned long long)total);
      }
      cur = u;
      acc = 0;
    }
    if (v == u || (uint32_t)v >= (uint32_t)N || (uint32_t)u >= (uint32_t)N) continue;
    int32_t ss = rowptr[u], se = rowptr[u + 1], ls = rowptr[v], le = rowptr[v + 1];
    if (se - ss > le - ls) {
      int32_t t = ss; ss = ls; ls = t;
      t = se; se = le; le = t;
    }
    for (int32_t i = ss + sub; i < se; i += kTriGroup) {
      const int32_t w = col[i];
      if (w != u && w != v) acc += row_holds(col, ls, le, w);
    }
  }
  const int64_t last_cnt = group_sum(acc);                 // (every lane of the wave is back here)
  // the groups' first and last rows in entry order: equal rows are neighbours, one add per run
  int32_t run_row = -1;
  int64_t run_cnt = 0;
#pragma unroll
  for (int g = 0; g < kTriGroups; ++g) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int32_t r = __shfl(k ? cur : first_row, g * kTriGroup);
      const int64_t c = __shfl(k ? last_cnt : first_cnt, g * kTriGroup);
      if (r < 0) continue;                                 // (wave-uniform)
      if (r != run_row) {
        if (lane == 0 && run_row >= 0 && run_cnt) atomicAdd(&tri2[run_row], (unsigned long long)run_cnt);
        run_row = r;
        run_cnt = 0;
      }
      run_cnt += c;
    }
  }
  if (lane == 0 && run_row >= 0 && run_cnt) atomicAdd(&tri2[run_row], (unsigned long long)run_cnt);
}

// ---- hop sums ----------------------------------------------------------------------------------------------------

constexpr int kHopMaxNodes = 1 << 16;
constexpr int kHopWords = kHopMaxNodes / 32;

// workgroup s: breadth-first search from sources[s] inside its graph [graph_ptr[g], graph_ptr[g + 1]) along the rows of
// the CSR; dist_sum[s] = sum of the levels of the nodes it reaches, reached[s] = their number, the source (level 0)
// included.  s_new holds the size of the frontier about to be expanded.
__global__ __launch_bounds__(kBlock) void hop_sums_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int64_t* __restrict__ graph_ptr,
    const int64_t* __restrict__ sources, const int32_t* __restrict__ source_graph, int64_t* __restrict__ dist_sum,
    int32_t* __restrict__ reached) {
  __shared__ uint32_t vis[kHopWords], fr[kHopWords], nx[kHopWords];
  __shared__ int s_new;
  const int64_t s = blockIdx.x;
  const int t = threadIdx.x;
  const int32_t g = source_graph[s];
  const int64_t lo = graph_ptr[g], n = graph_ptr[g + 1] - lo;
  const int64_t src = sources[s] - lo;
  // (the caller checks both; the guard keeps the bitmaps in bounds whatever the data say)
  const bool ok = n > 0 && n <= kHopMaxNodes && src >= 0 && src < n;
  const int words = ok ? (int)((n + 31) >> 5) : 0;
  for (int w = t; w < words; w += kBlock) { vis[w] = 0u; fr[w] = 0u; nx[w] = 0u; }
  if (t == 0) s_new = ok ? 1 : 0;
  __syncthreads();
  if (t == 0 && ok) {
    vis[src >> 5] = 1u << (src & 31);
    fr[src >> 5] = 1u << (src & 31);
  }
  int64_t sum = 0;
  int32_t count = 0;
  for (int level = 0;; ++level) {
    __syncthreads();                                   // the frontier of this level and its size
    const int fresh = s_new;
    if (fresh == 0) break;                             // (uniform)
    sum += (int64_t)level * fresh;
    count += fresh;
    __syncthreads();                                   // s_new read by every thread before it is reset
    if (t == 0) s_new = 0;
    for (int w = t; w < words; w += kBlock) {
      uint32_t bits = fr[w];
      while (bits) {
        const int b = __builtin_ctz(bits);
        bits &= bits - 1;
        const int64_t u = lo + ((int64_t)w << 5) + b;
        const int32_t e1 = rowptr[u + 1];
        for (int32_t e = rowptr[u]; e < e1; ++e) {
          const int64_t v = (int64_t)col[e] - lo;
          if (v < 0 || v >= n) continue;               // (an edge that leaves the graph: not followed)
          const uint32_t m = 1u << (v & 31);
          if (vis[v >> 5] & m) continue;
          const uint32_t old = atomicOr(&vis[v >> 5], m);
          if (!(old & m)) atomicOr(&nx[v >> 5], m);
        }
      }
    }
    __syncthreads();                                   // this level's discoveries are complete, s_new is 0
    int mine = 0;
    for (int w = t; w < words; w += kBlock) {
      const uint32_t x = nx[w];
      mine += __builtin_popcount(x);
      fr[w] = x;
      nx[w] = 0u;
    }
#pragma unroll
    for (int o = kWave >> 1; o > 0; o >>= 1) mine += __shfl_xor(mine, o);
    if ((t & (kWave - 1)) == 0 && mine) atomicAdd(&s_new, mine);
  }
  if (t == 0) {
    dist_sum[s] = sum;
    reached[s] = count;
  }
}

}  // namespace mp

using namespace mp;

extern "C" int mp_csr_triangles(const int32_t* rowptr, const int32_t* col, const int32_t* row_of, int64_t N, int64_t nnz,
                                int64_t* tri2, int32_t* deg, mp_stream_t stream) {
  if (N < 0 || nnz < 0) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || nnz > INT32_MAX) return MP_ERR_UNSUPPORTED;
  if (N == 0) return MP_OK;
  if (!rowptr || !tri2 || !deg) return MP_ERR_INVALID_ARG;
  if (nnz > 0 && (!col || !row_of)) return MP_ERR_INVALID_ARG;
  hipStream_t st = as_stream(stream);
  MP_HIP(hipMemsetAsync(tri2, 0, (size_t)N * sizeof(int64_t), st));
  if (nnz == 0) {
    MP_HIP(hipMemsetAsync(deg, 0, (size_t)N * sizeof(int32_t), st));
    return MP_OK;
  }
  hipLaunchKernelGGL(csr_loopless_degree_kernel, dim3(flat_grid(N)), dim3(kBlock), 0, st, rowptr, col, N, deg);
  MP_LAUNCH_CHECK();
  const int64_t blocks = ceil_div(nnz, (int64_t)kTriChunk * kWavesPerBlock);     // <= 2^31 / 1024
  hipLaunchKernelGGL(csr_triangles_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, st, rowptr, col, row_of, N, nnz,
                     reinterpret_cast<unsigned long long*>(tri2));
  MP_LAUNCH_CHECK();
  return MP_OK;
}

extern "C" int mp_hop_sums(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, const int64_t* graph_ptr,
                           int64_t n_graphs, int64_t max_graph_nodes, const int64_t* sources,
                           const int32_t* source_graph, int64_t n_sources, int64_t* dist_sum, int32_t* reached,
                           mp_stream_t stream) {
  if (N < 0 || nnz < 0 || n_graphs < 0 || max_graph_nodes < 0 || n_sources < 0) return MP_ERR_INVALID_ARG;
  if (!rowptr || !graph_ptr) return MP_ERR_INVALID_ARG;
  if (nnz > 0 && !col) return MP_ERR_INVALID_ARG;
  if (n_sources > 0 && (!sources || !source_graph || !dist_sum || !reached || n_graphs == 0)) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || nnz > INT32_MAX || n_sources > INT32_MAX || n_graphs >= INT32_MAX) return MP_ERR_UNSUPPORTED;
  if (max_graph_nodes > kHopMaxNodes) return MP_ERR_UNSUPPORTED;     // the bitmaps live in LDS
  if (n_sources == 0) return MP_OK;
  hipLaunchKernelGGL(hop_sums_kernel, dim3((unsigned)n_sources), dim3(kBlock), 0, as_stream(stream), rowptr, col,
                     graph_ptr, sources, source_graph, dist_sum, reached);
  MP_LAUNCH_CHECK();
  return MP_OK;
}
