// Centralities and one-hot ids of graphgym/models/feature_augment.py:55-58,70-73,88-91 on the device
// (include/mp_structure.h): nx.pagerank's power iteration, Brandes' betweenness from every source, and a keyed
// permutation per graph.  All float64, no float atomics, and every sum in an order the graph alone decides: a graph's
// values are the same bits alone, inside any batch and on every run.
//
// PageRank (mp_struct_pagerank).  Which form a graph takes depends on its own n:
//   n <= kPrLds   one workgroup runs the whole loop in one launch, x, x' and 1/deg in LDS; thread t owns the rows
//                 t, t + kBlock, ... and walks each in stored order; dsum and err are its rows' sums in that order,
//                 then the fixed tree of block_sum2 over the kBlock threads.  The barrier structure is
//                 hop_sums_kernel's: the stop test is uniform because every thread reads the same reduced err.
//   n >  kPrLds   per step one workgroup per chunk of kPrChunk rows (the same thread-to-row map and tree inside the
//                 chunk) writes x' and the chunk's partial dsum / err, then one thread per graph adds the chunks'
//                 partials in chunk order, tests err and keeps the stop state in iters[g] (0 while running): the host
//                 enqueues max_iter steps without reading anything, and the steps of a finished graph return at once.
//   cost: steps x (nnz gathers of x and 1/deg + n stores); the LDS form pays 2 log2(kBlock) + 3 barriers a step.
//
// Betweenness (mp_struct_betweenness).  One workgroup per (graph, slice of kBcSlice sources).  Per source a
// level-synchronous pull search — every node not yet reached reads its row for neighbours of the previous level and adds
// their sigma, one barrier a level — then the dependencies from the deepest level up, again one pull and one barrier a
// level; the source's delta is added, by the thread that owns the node, into the slice's vector.
//   cost per source: (levels + 1) passes over the rows of the nodes not yet reached + levels passes over the level
//   array and the rows of one level each: O(levels x nnz) reads, no queue, no atomic.
// level / sigma / delta / the slice's sum live in LDS up to kBcLds nodes (28 bytes a node) and in the workspace above.
#include "common.h"
#include "draws.h"       // keyed_perm, range_of
#include "../../include/mp_structure.h"

namespace mp {

constexpr int kPrLds = MP_STRUCT_PAGERANK_LDS_NODES;
constexpr int kPrChunk = MP_STRUCT_PAGERANK_CHUNK;
constexpr int kBcSlice = MP_STRUCT_BETWEENNESS_SLICE;
constexpr int kBcLds = MP_STRUCT_BETWEENNESS_LDS_NODES;
constexpr int kBcMax = MP_STRUCT_BETWEENNESS_MAX_NODES;
static_assert(kPrChunk % kBlock == 0 && kPrChunk <= kPrLds, "a chunk is whole rounds of the workgroup; a large graph has more than one");

// the workgroup's sums of a and b in a fixed order: red[t] = thread t's value, then the halving tree.  red holds
// 2 kBlock doubles; every thread of the block calls it, and gets both sums.
__device__ __forceinline__ void block_sum2(double& a, double& b, double* red) {
  const int t = threadIdx.x;
  __syncthreads();                                     // the sums of the call before are read
  red[t] = a;
  red[kBlock + t] = b;
  __syncthreads();
  for (int o = kBlock >> 1; o > 0; o >>= 1) {
    if (t < o) {
      red[t] += red[t + o];
      red[kBlock + t] += red[kBlock + t + o];
    }
    __syncthreads();
  }
  a = red[0];
  b = red[kBlock];
}

// y[j] of one row: the entries in stored order (an entry that leaves the graph is not followed)
template <class X>
__device__ __forceinline__ double pr_row(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t lo,
                                         int64_t n, int64_t j, const X* x, const X* inv) {
  double y = 0.0;
  const int32_t e1 = rowptr[lo + j + 1];
  for (int32_t e = rowptr[lo + j]; e < e1; ++e) {
    const int64_t i = (int64_t)col[e] - lo;
    if (i < 0 || i >= n) continue;
    y += x[i] * inv[i];
  }
  return y;
}

// ---- PageRank, LDS form: workgroup g iterates graph g ---------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void pagerank_lds_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int64_t* __restrict__ graph_ptr,
    int64_t N, double alpha, double tol, int max_iter, double* __restrict__ out, int32_t* __restrict__ iters) {
  __shared__ double xa[kPrLds], xb[kPrLds], inv[kPrLds];
  __shared__ double red[2 * kBlock];
  const int64_t g = blockIdx.x;
  const int64_t lo = graph_ptr[g], n = graph_ptr[g + 1] - lo;
  // (uniform.  A larger graph takes the other form; the caller checks graph_ptr, the guard keeps every index in bounds)
  if (n <= 0 || n > kPrLds || lo < 0 || lo + n > N) return;
  const int t = threadIdx.x, ni = (int)n;
  const double p = 1.0 / (double)n;
  double dsum = 0.0, err = 0.0;
  for (int j = t; j < ni; j += kBlock) {
    const int32_t deg = rowptr[lo + j + 1] - rowptr[lo + j];
    xa[j] = p;
    inv[j] = deg > 0 ? 1.0 / (double)deg : 0.0;
    if (deg <= 0) dsum += p;
  }
  block_sum2(dsum, err, red);
  double* x = xa;
  double* xn = xb;
  int stopped = -1;
  for (int it = 1; it <= max_iter; ++it) {
    double dnext = 0.0;
    err = 0.0;
    for (int j = t; j < ni; j += kBlock) {
      const double y = pr_row(rowptr, col, lo, n, j, x, inv);
      const double v = alpha * (y + dsum * p) + (1.0 - alpha) * p;
      xn[j] = v;
      err += fabs(v - x[j]);
      if (inv[j] == 0.0) dnext += v;
    }
    block_sum2(dnext, err, red);                       // (its barriers: x' is complete, x is read by no one any more)
    dsum = dnext;
    double* s = x; x = xn; xn = s;
    if (err < (double)n * tol) { stopped = it; break; }     // (uniform: every thread holds the same err)
  }
  for (int j = t; j < ni; j += kBlock) out[lo + j] = x[j];
  if (t == 0) iters[g] = stopped;
}

// ---- PageRank, large form ---------------------------------------------------------------------------------------
// workspace: xa [N], xb [N], inv [N], perr [n_chunks], pds [n_chunks], ds [G] (doubles)
struct PrWs {
  double *xa, *xb, *inv, *perr, *pds, *ds;
};

// workgroup b -> (graph, first row of its chunk); false where b names no chunk
__device__ __forceinline__ bool pr_chunk(const int64_t* __restrict__ graph_ptr, const int64_t* __restrict__ chunk_ptr,
                                         int64_t G, int64_t N, int64_t b, int64_t& g, int64_t& lo, int64_t& n, int64_t& j0) {
  g = range_of(chunk_ptr, G, b);
  lo = graph_ptr[g];
  n = graph_ptr[g + 1] - lo;
  j0 = (b - chunk_ptr[g]) * kPrChunk;
  return b < chunk_ptr[g + 1] && n > kPrLds && lo >= 0 && lo + n <= N && j0 >= 0 && j0 < n;
}

// x = p, inv = 1 / deg, and the chunk's share of the first dsum
__global__ __launch_bounds__(kBlock) void pagerank_init_kernel(
    const int32_t* __restrict__ rowptr, const int64_t* __restrict__ graph_ptr, const int64_t* __restrict__ chunk_ptr,
    int64_t G, int64_t N, PrWs w) {
  __shared__ double red[2 * kBlock];
  int64_t g, lo, n, j0;
  if (!pr_chunk(graph_ptr, chunk_ptr, G, N, blockIdx.x, g, lo, n, j0)) return;       // (uniform)
  const double p = 1.0 / (double)n;
  double dsum = 0.0, none = 0.0;
  for (int64_t j = j0 + threadIdx.x; j < j0 + kPrChunk && j < n; j += kBlock) {
    const int32_t deg = rowptr[lo + j + 1] - rowptr[lo + j];
    w.xa[lo + j] = p;
    w.inv[lo + j] = deg > 0 ? 1.0 / (double)deg : 0.0;
    if (deg <= 0) dsum += p;
  }
  block_sum2(dsum, none, red);
  if (threadIdx.x == 0) w.pds[blockIdx.x] = dsum;
}

// step `it` of one chunk: reads xa on odd steps and xb on even ones, writes the other and out
__global__ __launch_bounds__(kBlock) void pagerank_step_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int64_t* __restrict__ graph_ptr,
    const int64_t* __restrict__ chunk_ptr, int64_t G, int64_t N, double alpha, int it, PrWs w, double* __restrict__ out,
    const int32_t* __restrict__ iters) {
  __shared__ double red[2 * kBlock];
  int64_t g, lo, n, j0;
  if (!pr_chunk(graph_ptr, chunk_ptr, G, N, blockIdx.x, g, lo, n, j0)) return;       // (uniform)
  if (iters[g] != 0) return;                                                       // (uniform: the graph has stopped)
  const double* x = ((it & 1) ? w.xa : w.xb) + lo;
  double* xn = ((it & 1) ? w.xb : w.xa) + lo;
  const double* inv = w.inv + lo;
  const double p = 1.0 / (double)n, dsum = w.ds[g];
  double dnext = 0.0, err = 0.0;
  for (int64_t j = j0 + threadIdx.x; j < j0 + kPrChunk && j < n; j += kBlock) {
    const double y = pr_row(rowptr, col, lo, n, j, x, inv);
    const double v = alpha * (y + dsum * p) + (1.0 - alpha) * p;
    xn[j] = v;
    out[lo + j] = v;
    err += fabs(v - x[j]);
    if (inv[j] == 0.0) dnext += v;
  }
  block_sum2(dnext, err, red);
  if (threadIdx.x == 0) {
    w.pds[blockIdx.x] = dnext;
    w.perr[blockIdx.x] = err;
  }
}

// thread g closes step `it` of graph g: its chunks' partials in chunk order, the stop test, the state.  it = 0 closes
// the initialisation: the first dsum, and iters[g] = 0 (running).
__global__ __launch_bounds__(kBlock) void pagerank_close_kernel(
    const int64_t* __restrict__ graph_ptr, const int64_t* __restrict__ chunk_ptr, int64_t G, double tol, int it,
    int max_iter, PrWs w, int32_t* __restrict__ iters) {
  const int64_t g = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= G) return;
  const int64_t c0 = chunk_ptr[g], c1 = chunk_ptr[g + 1];
  const int64_t n = graph_ptr[g + 1] - graph_ptr[g];
  if (c1 <= c0 || n <= kPrLds) return;                 // (an LDS-form graph: pagerank_lds_kernel writes its iters)
  if (it > 0 && iters[g] != 0) return;
  double dsum = 0.0, err = 0.0;
  for (int64_t c = c0; c < c1; ++c) {
    dsum += w.pds[c];
    if (it > 0) err += w.perr[c];
  }
  w.ds[g] = dsum;
  int32_t state = 0;
  if (it > 0 && err < (double)n * tol) state = it;
  else if (it >= max_iter) state = -1;
  iters[g] = state;
}

// ---- betweenness ---------------------------------------------------------------------------------------------------
// workspace: partial [S N] doubles, then (S N each, only when a graph is above kBcLds) sigma, delta doubles, level int32
template <bool LDS>
__global__ __launch_bounds__(kBlock) void betweenness_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int64_t* __restrict__ graph_ptr, int64_t G,
    const int64_t* __restrict__ slice_ptr, int64_t N, int64_t max_nodes, double* __restrict__ partial,
    double* __restrict__ ws_sigma, double* __restrict__ ws_delta, int32_t* __restrict__ ws_level) {
  constexpr int kCap = LDS ? kBcLds : 1;
  __shared__ double s_sigma[kCap], s_delta[kCap], s_acc[kCap];
  __shared__ int32_t s_level[kCap];
  const int64_t b = blockIdx.x;
  const int64_t g = range_of(slice_ptr, G, b);
  const int64_t lo = graph_ptr[g], n = graph_ptr[g + 1] - lo;
  const int64_t s = b - slice_ptr[g];
  // (uniform.  The caller checks the sizes; the guards keep every index in bounds whatever the data say)
  if (n <= 0 || n > max_nodes || n > kBcMax || lo < 0 || lo + n > N || (n <= kBcLds) != LDS) return;
  if (s < 0 || s * kBcSlice >= n) return;
  const int t = threadIdx.x, ni = (int)n;
  const int64_t slab = s * N + lo;
  double *sigma, *delta, *acc;
  int32_t* level;
  if constexpr (LDS) {
    sigma = s_sigma; delta = s_delta; acc = s_acc; level = s_level;
  } else {
    sigma = ws_sigma + slab; delta = ws_delta + slab; acc = partial + slab; level = ws_level + slab;
  }
  for (int v = t; v < ni; v += kBlock) acc[v] = 0.0;
  const int src1 = (int)((s + 1) * kBcSlice < n ? (s + 1) * kBcSlice : n);
  for (int src = (int)(s * kBcSlice); src < src1; ++src) {
    for (int v = t; v < ni; v += kBlock) {
      level[v] = v == src ? 0 : -1;
      sigma[v] = v == src ? 1.0 : 0.0;
      delta[v] = 0.0;
    }
    __syncthreads();
    // forward: level L is every node not yet reached with a neighbour of level L - 1.  A neighbour reached in this very
    // pass holds -1 or L, never L - 1: the pass reads only what the barrier before it completed.
    int depth = 0;
    for (int L = 1;; ++L) {
      int found = 0;
      for (int v = t; v < ni; v += kBlock) {
        if (level[v] >= 0) continue;
        double paths = 0.0;
        bool hit = false;
        const int32_t e1 = rowptr[lo + v + 1];
        for (int32_t e = rowptr[lo + v]; e < e1; ++e) {
          const int64_t u = (int64_t)col[e] - lo;
          if (u < 0 || u >= n) continue;
          if (level[u] == L - 1) { paths += sigma[u]; hit = true; }
        }
        if (hit) { level[v] = L; sigma[v] = paths; found = 1; }
      }
      if (!__syncthreads_or(found)) break;             // (uniform)
      depth = L;
    }
    // backward: the dependencies, from the level above the deepest down to the source
    for (int L = depth - 1; L >= 0; --L) {
      for (int v = t; v < ni; v += kBlock) {
        if (level[v] != L) continue;
        const double sv = sigma[v];
        double d = 0.0;
        const int32_t e1 = rowptr[lo + v + 1];
        for (int32_t e = rowptr[lo + v]; e < e1; ++e) {
          const int64_t u = (int64_t)col[e] - lo;
          if (u < 0 || u >= n) continue;
          if (level[u] == L + 1) d += sv * ((1.0 + delta[u]) / sigma[u]);
        }
        delta[v] = d;
      }
      __syncthreads();
    }
    for (int v = t; v < ni; v += kBlock)               // (a thread's own nodes: nobody else touches acc[v])
      if (level[v] > 0) acc[v] += delta[v];
    __syncthreads();                                   // level / delta are read before the next source resets them
  }
  if constexpr (LDS)
    for (int v = t; v < ni; v += kBlock) partial[slab + v] = acc[v];
}

// out[v] = (the partials of v in slice order) / ((n - 1) (n - 2))
__global__ __launch_bounds__(kBlock) void betweenness_sum_kernel(
    const int64_t* __restrict__ graph_ptr, int64_t G, int64_t N, int64_t max_nodes, const double* __restrict__ partial,
    double* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= N) return;
  const int64_t g = range_of(graph_ptr, G, v);
  const int64_t n = graph_ptr[g + 1] - graph_ptr[g];
  if (n <= 0 || n > max_nodes || n > kBcMax) return;
  const int64_t slices = (n + kBcSlice - 1) / kBcSlice;
  double sum = 0.0;
  for (int64_t s = 0; s < slices; ++s) sum += partial[s * N + v];
  const double scale = n > 2 ? 1.0 / ((double)(n - 1) * (double)(n - 2)) : 0.0;
  out[v] = sum * scale;
}

// ---- one-hot ids ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void onehot_kernel(const int64_t* __restrict__ graph_ptr, int64_t G, int64_t N,
                                                        uint64_t seed, int64_t* __restrict__ out) {
  const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (v >= N) return;
  const int64_t g = range_of(graph_ptr, G, v);
  const int64_t i = v - graph_ptr[g], n = graph_ptr[g + 1] - graph_ptr[g];
  if (i < 0 || i >= n) {                               // (the caller checks graph_ptr; the guard keeps the walk finite)
    out[v] = -1;
    return;
  }
  out[v] = (int64_t)keyed_perm(seed, (uint64_t)MP_STRUCT_ONEHOT_STREAM, (uint64_t)g, (uint64_t)i, n);
}

static inline bool bad_graph_args(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz,
                                  const int64_t* graph_ptr, int64_t n_graphs) {
  return N < 0 || nnz < 0 || n_graphs < 0 || !rowptr || !graph_ptr || (nnz > 0 && !col) || (N > 0 && n_graphs == 0);
}

}  // namespace mp

using namespace mp;

extern "C" int mp_struct_pagerank_ws_bytes(int64_t N, int64_t n_graphs, int64_t n_chunks, size_t* bytes) {
  if (!bytes || N < 0 || n_graphs < 0 || n_chunks < 0) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || n_graphs >= INT32_MAX || n_chunks >= INT32_MAX) return MP_ERR_UNSUPPORTED;
  *bytes = n_chunks == 0 ? 16 : sizeof(double) * (size_t)(3 * N + 2 * n_chunks + n_graphs);
  return MP_OK;
}

extern "C" int mp_struct_pagerank(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz,
                                  const int64_t* graph_ptr, int64_t n_graphs, const int64_t* chunk_ptr, int64_t n_chunks,
                                  double alpha, double tol, int32_t max_iter, double* out, int32_t* iters, void* ws,
                                  size_t ws_bytes, mp_stream_t stream) {
  if (bad_graph_args(rowptr, col, N, nnz, graph_ptr, n_graphs) || n_chunks < 0) return MP_ERR_INVALID_ARG;
  if (!(alpha >= 0.0 && alpha <= 1.0) || !(tol >= 0.0) || max_iter < 1) return MP_ERR_INVALID_ARG;
  if (N > 0 && (!out || !iters)) return MP_ERR_INVALID_ARG;
  if (n_chunks > 0 && (!chunk_ptr || !ws)) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || nnz > INT32_MAX || n_graphs >= INT32_MAX || n_chunks >= INT32_MAX) return MP_ERR_UNSUPPORTED;
  size_t need = 0;
  if (mp_struct_pagerank_ws_bytes(N, n_graphs, n_chunks, &need) != MP_OK) return MP_ERR_INVALID_ARG;
  if (n_chunks > 0 && ws_bytes < need) return MP_ERR_WORKSPACE;
  if (N == 0) return MP_OK;
  hipStream_t st = as_stream(stream);
  hipLaunchKernelGGL(pagerank_lds_kernel, dim3((unsigned)n_graphs), dim3(kBlock), 0, st, rowptr, col, graph_ptr, N, alpha,
                     tol, (int)max_iter, out, iters);
  MP_LAUNCH_CHECK();
  if (n_chunks == 0) return MP_OK;
  PrWs w;
  w.xa = static_cast<double*>(ws);
  w.xb = w.xa + N;
  w.inv = w.xb + N;
  w.perr = w.inv + N;
  w.pds = w.perr + n_chunks;
  w.ds = w.pds + n_chunks;
  const dim3 chunks((unsigned)n_chunks), graphs((unsigned)ceil_div(n_graphs, kBlock));
  hipLaunchKernelGGL(pagerank_init_kernel, chunks, dim3(kBlock), 0, st, rowptr, graph_ptr, chunk_ptr, n_graphs, N,
                     w);
  MP_LAUNCH_CHECK();
  for (int it = 0; it <= max_iter; ++it) {
    if (it > 0) {
      hipLaunchKernelGGL(pagerank_step_kernel, chunks, dim3(kBlock), 0, st, rowptr, col, graph_ptr, chunk_ptr, n_graphs,
                         N, alpha, it, w, out, iters);
      MP_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(pagerank_close_kernel, graphs, dim3(kBlock), 0, st, graph_ptr, chunk_ptr, n_graphs, tol, it,
                       (int)max_iter, w, iters);
    MP_LAUNCH_CHECK();
  }
  return MP_OK;
}

static inline int64_t bc_slices(int64_t max_graph_nodes) { return ceil_div(max_graph_nodes, (int64_t)kBcSlice); }

extern "C" int mp_struct_betweenness_ws_bytes(int64_t N, int64_t max_graph_nodes, size_t* bytes) {
  if (!bytes || N < 0 || max_graph_nodes < 0 || max_graph_nodes > N) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || max_graph_nodes > kBcMax) return MP_ERR_UNSUPPORTED;
  const size_t slots = (size_t)bc_slices(max_graph_nodes) * (size_t)N;
  const size_t per_slot = max_graph_nodes > kBcLds ? 3 * sizeof(double) + sizeof(int32_t) : sizeof(double);
  *bytes = slots * per_slot + 16;
  return MP_OK;
}

extern "C" int mp_struct_betweenness(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz,
                                     const int64_t* graph_ptr, int64_t n_graphs, int64_t max_graph_nodes,
                                     const int64_t* slice_ptr, int64_t n_slices, double* out, void* ws, size_t ws_bytes,
                                     mp_stream_t stream) {
  if (bad_graph_args(rowptr, col, N, nnz, graph_ptr, n_graphs)) return MP_ERR_INVALID_ARG;
  if (max_graph_nodes < 0 || max_graph_nodes > N || n_slices < 0) return MP_ERR_INVALID_ARG;
  if (N > 0 && (!out || !slice_ptr || !ws)) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || nnz > INT32_MAX || n_graphs >= INT32_MAX || n_slices >= INT32_MAX) return MP_ERR_UNSUPPORTED;
  if (max_graph_nodes > kBcMax) return MP_ERR_UNSUPPORTED;
  size_t need = 0;
  if (mp_struct_betweenness_ws_bytes(N, max_graph_nodes, &need) != MP_OK) return MP_ERR_INVALID_ARG;
  if (N > 0 && ws_bytes < need) return MP_ERR_WORKSPACE;
  if (N == 0) return MP_OK;
  hipStream_t st = as_stream(stream);
  const size_t slots = (size_t)bc_slices(max_graph_nodes) * (size_t)N;
  double* partial = static_cast<double*>(ws);
  double* sigma = partial + slots;
  double* delta = sigma + slots;
  int32_t* level = reinterpret_cast<int32_t*>(delta + slots);
  if (n_slices > 0) {
    hipLaunchKernelGGL(betweenness_kernel<true>, dim3((unsigned)n_slices), dim3(kBlock), 0, st, rowptr, col, graph_ptr,
                       n_graphs, slice_ptr, N, max_graph_nodes, partial, (double*)nullptr, (double*)nullptr,
                       (int32_t*)nullptr);
    MP_LAUNCH_CHECK();
    if (max_graph_nodes > kBcLds) {
      hipLaunchKernelGGL(betweenness_kernel<false>, dim3((unsigned)n_slices), dim3(kBlock), 0, st, rowptr, col,
                         graph_ptr, n_graphs, slice_ptr, N, max_graph_nodes, partial, sigma, delta, level);
      MP_LAUNCH_CHECK();
    }
  }
  hipLaunchKernelGGL(betweenness_sum_kernel, dim3((unsigned)ceil_div(N, kBlock)), dim3(kBlock), 0, st, graph_ptr,
                     n_graphs, N, max_graph_nodes, partial, out);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

extern "C" int mp_struct_onehot(const int64_t* graph_ptr, int64_t n_graphs, int64_t N, uint64_t seed, int64_t* out,
                                mp_stream_t stream) {
  if (N < 0 || n_graphs < 0 || !graph_ptr || (N > 0 && (!out || n_graphs == 0))) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || n_graphs >= INT32_MAX) return MP_ERR_UNSUPPORTED;
  if (N == 0) return MP_OK;
  hipLaunchKernelGGL(onehot_kernel, dim3((unsigned)ceil_div(N, kBlock)), dim3(kBlock), 0, as_stream(stream), graph_ptr,
                     n_graphs, N, seed, out);
  MP_LAUNCH_CHECK();
  return MP_OK;
}
