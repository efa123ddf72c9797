// Link-prediction labels on the device: the pair space of a batch (how many non-stored partners every row has) and a
// sampler that draws K_g distinct non-edges per graph without rejection (GraphGym's edge_negative_sampling_ratio /
// resample_negative, graphgym/config.py:147-163; the reference leaves the draw to DeepSNAP's host rejection loop).
//
// The base CSR is the engine's (row = destination, columns ascending inside a row, no column twice in a row), the
// disjoint union of the graphs graph_ptr [G+1] delimits.  A candidate pair lies inside one graph:
//   MP_PAIRS_UNDIRECTED  (r, c) with c > r: every unordered pair once, a stored diagonal never matters;
//   MP_PAIRS_DIRECTED    (src = c, dst = r) with c != r: a stored diagonal entry is no candidate and is stepped over once.
// free[r] counts the candidates of row r that are not stored (mp_pair_space_rows).  The non-edges of graph g, ordered by
// (row, column), are then numbered 0 .. C_g - 1 with C_g the sum of free over the graph, and the caller's exclusive
// prefix sum of free turns a number (a rank) back into its row.
//
// Sampling (mp_sample_non_edges), one thread per sample, nothing but reads and one store pair:
//   1. rank = perm_g(i): a balanced Feistel network on 2b bits, b = max(1, ceil(bits(C_g - 1) / 2)), walked until the
//      value is below C_g (cycle walking: the domain is below 4 C_g, fewer than 4 encryptions on average, and the walk
//      from a start below C_g always returns below C_g because the network is a bijection).  perm_g is a bijection on
//      [0, C_g): K_g samples are K_g distinct non-edges, K_g = C_g the whole complement.  Integer mixing only.
//   2. rank -> row: binary search in the graph's slice of the prefix.
//   3. rank inside the row -> column: with the stored candidate columns a_0 < a_1 < ..., (a_j - first) - j candidates
//      below a_j are free; the first j where that exceeds t says how many stored columns to step over.
//   4. undirected: (r, c), r < c; directed: (c, r) as (src, dst).
// Sample i of graph g depends on (seed, offset, g, i) and the graph alone, never on the launch geometry.
#include "common.h"
#include "draws.h"       // keyed_perm, upper_bound

namespace mp {

// is r stored in its own row [rs, re)?
__device__ __forceinline__ bool has_diagonal(const int32_t* __restrict__ col, int64_t rs, int64_t re, int64_t r) {
  const int64_t d = upper_bound(col, rs, re, r - 1);
  return d < re && col[d] == r;
}

// flags[0]: a row stores a column twice; flags[1]: a row stores a column outside its graph
template <bool DIRECTED>
__global__ __launch_bounds__(kBlock) void pair_space_rows_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t N,
    const int64_t* __restrict__ graph_ptr, int64_t G, int64_t* __restrict__ free_out, int32_t* __restrict__ flags) {
  const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (r >= N) return;
  const int64_t g = range_of(graph_ptr, G, r);
  const int64_t lo = graph_ptr[g], hi = graph_ptr[g + 1];
  const int64_t rs = rowptr[r], re = rowptr[r + 1];
  bool twice = false;
  for (int64_t e = rs + 1; e < re; ++e) twice |= col[e] == col[e - 1];
  if (twice) flags[0] = 1;
  if (re > rs && (col[rs] < lo || col[re - 1] >= hi)) flags[1] = 1;
  int64_t f;
  if (DIRECTED) f = (hi - lo - 1) - ((re - rs) - (has_diagonal(col, rs, re, r) ? 1 : 0));
  else f = (hi - 1 - r) - (re - upper_bound(col, rs, re, r));
  free_out[r] = f < 0 ? 0 : f;               // (below zero only in a flagged row)
}

template <bool DIRECTED>
__global__ __launch_bounds__(kBlock) void sample_non_edges_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int64_t* __restrict__ graph_ptr, int64_t G,
    const int64_t* __restrict__ prefix, const int64_t* __restrict__ slot_base, int64_t K, uint64_t seed, uint64_t offset,
    int64_t* __restrict__ out) {
  const int64_t slot = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (slot >= K) return;
  const int64_t g = range_of(slot_base, G, slot);
  const uint64_t i = (uint64_t)(slot - slot_base[g]);
  const int64_t lo = graph_ptr[g], hi = graph_ptr[g + 1];
  const int64_t p0 = prefix[lo];
  const int64_t C = prefix[hi] - p0;
  if (C <= 0 || i >= (uint64_t)C) {          // (the caller checks K_g <= C_g; the guard keeps the walk finite)
    out[slot] = -1;
    out[K + slot] = -1;
    return;
  }
  // 1. the keyed bijection (draws.h)
  const uint64_t x = keyed_perm(seed, offset, (uint64_t)g, i, C);
  // 2. rank -> row: the first r of [lo, hi) with prefix[r + 1] above the rank
  const int64_t target = p0 + (int64_t)x;
  int64_t r = upper_bound(prefix, lo + 1, hi + 1, target) - 1;
  if (r >= hi) r = hi - 1;
  const int64_t t = target - prefix[r];
  // 3. rank inside the row -> column
  const int64_t rs = rowptr[r], re = rowptr[r + 1];
  int64_t c;
  if (DIRECTED) {
    // candidates lo .. hi - 1 without r: r counts as stored, once (where the row stores it, it is among the entries)
    const bool diag = has_diagonal(col, rs, re, r);
    int64_t a = rs, z = re;
    while (a < z) {
      const int64_t mid = (a + z) >> 1, cm = col[mid];
      const int64_t below = (cm - lo) - (mid - rs) - ((cm > r && !diag) ? 1 : 0);
      if (below <= t) a = mid + 1; else z = mid;
    }
    c = lo + t + (a - rs);
    if (!diag && c >= r) ++c;
    out[slot] = c;
    out[K + slot] = r;
  } else {
    const int64_t s0 = upper_bound(col, rs, re, r);
    int64_t a = s0, z = re;
    while (a < z) {
      const int64_t mid = (a + z) >> 1;
      const int64_t below = ((int64_t)col[mid] - (r + 1)) - (mid - s0);
      if (below <= t) a = mid + 1; else z = mid;
    }
    c = r + 1 + t + (a - s0);
    out[slot] = r;
    out[K + slot] = c;
  }
}

}  // namespace mp

using namespace mp;

extern "C" int mp_pair_space_rows(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz,
                                  const int64_t* graph_ptr, int64_t n_graphs, int32_t mode, int64_t* free_out,
                                  int32_t* flags, mp_stream_t stream) {
  if (N < 0 || nnz < 0 || n_graphs < 0) return MP_ERR_INVALID_ARG;
  if (mode != MP_PAIRS_UNDIRECTED && mode != MP_PAIRS_DIRECTED) return MP_ERR_INVALID_ARG;
  if (!rowptr || !graph_ptr || !flags) return MP_ERR_INVALID_ARG;
  if (nnz > 0 && !col) return MP_ERR_INVALID_ARG;
  if (N > 0 && (!free_out || n_graphs == 0)) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || nnz > INT32_MAX || n_graphs >= INT32_MAX) return MP_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  MP_HIP(hipMemsetAsync(flags, 0, 2 * sizeof(int32_t), st));
  if (N == 0) return MP_OK;
  const dim3 grid((unsigned)ceil_div(N, kBlock));
  if (mode == MP_PAIRS_DIRECTED)
    hipLaunchKernelGGL(pair_space_rows_kernel<true>, grid, dim3(kBlock), 0, st, rowptr, col, N, graph_ptr, n_graphs,
                       free_out, flags);
  else
    hipLaunchKernelGGL(pair_space_rows_kernel<false>, grid, dim3(kBlock), 0, st, rowptr, col, N, graph_ptr, n_graphs,
                       free_out, flags);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

extern "C" int mp_sample_non_edges(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz,
                                   const int64_t* graph_ptr, int64_t n_graphs, const int64_t* prefix,
                                   const int64_t* slot_base, int64_t K, int32_t mode, uint64_t seed, uint64_t offset,
                                   int64_t* out, mp_stream_t stream) {
  if (N < 0 || nnz < 0 || n_graphs < 0 || K < 0) return MP_ERR_INVALID_ARG;
  if (mode != MP_PAIRS_UNDIRECTED && mode != MP_PAIRS_DIRECTED) return MP_ERR_INVALID_ARG;
  if (!rowptr || !graph_ptr || !prefix || !slot_base) return MP_ERR_INVALID_ARG;
  if (nnz > 0 && !col) return MP_ERR_INVALID_ARG;
  if (K > 0 && (!out || n_graphs == 0 || N == 0)) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || nnz > INT32_MAX || n_graphs >= INT32_MAX) return MP_ERR_UNSUPPORTED;
  if (ceil_div(K, kBlock) > INT32_MAX) return MP_ERR_UNSUPPORTED;
  if (K == 0) return MP_OK;
  const dim3 grid((unsigned)ceil_div(K, kBlock));
  hipStream_t st = as_stream(stream);
  if (mode == MP_PAIRS_DIRECTED)
    hipLaunchKernelGGL(sample_non_edges_kernel<true>, grid, dim3(kBlock), 0, st, rowptr, col, graph_ptr, n_graphs,
                       prefix, slot_base, K, seed, offset, out);
  else
    hipLaunchKernelGGL(sample_non_edges_kernel<false>, grid, dim3(kBlock), 0, st, rowptr, col, graph_ptr, n_graphs,
                       prefix, slot_base, K, seed, offset, out);
  MP_LAUNCH_CHECK();
  return MP_OK;
}
