// Edge-level ID-GNN tasks on the device: the edge-net expansion of graphgym/models/transform.py:41-65 and the hop
// distances behind the path-length labels of transform.py:68-90.
//
// Expansion (mp_edge_expand).  The reference makes one relabelled copy of the whole graph per node (a networkx loop,
// O(n^2) Python per graph).  Here a copy is a row of a table (its graph, its source node), and node j of copy c gets the
// new id node_base[c] + j; with every node of every graph a source, in batch order and source order, that is the
// reference's i*n + j inside a graph, graphs one after another.  The caller prefix-sums the per-copy sizes (nodes n_g,
// stored entries e_g of the copy's graph) and preallocates every output, so the work is one launch that only writes:
//   * a workgroup per (copy, slice of its graph): the slice's nodes write orig_node / copy_of_node (and, with the CSR,
//     their row starts and self entries), the slice's base entries write one edge each;
//   * the base CSR is walked in its own order (rows ascending, columns ascending inside a row) and the relabelling is
//     monotone inside a copy, copies ascending: the edge list comes out in the engine's CSR order (dst, src in new ids)
//     without a sort, and the batch's CSR is the base CSR shifted copy by copy — entry for entry what mp_csr_from_coo
//     builds from that edge list (parallel entries keep their base order, which is their edge-list order).
//
// Hop distances (mp_hop_distances).  One workgroup per distinct source runs a breadth-first search over the source's own
// graph with the visited / frontier / next bitmaps in LDS (3 x 8 KiB for up to 2^16 nodes: six workgroups per CU); the
// pairs that share the source are resolved level by level and the search stops when they all are (or nothing new is
// reached).  Exact at any depth: -1 only for a destination the search never reached.
#include "common.h"

namespace mp {

// ---- expansion ---------------------------------------------------------------------------------------------------

constexpr int kEdgeSlice = 1024;   // base entries (and nodes) of one copy per workgroup

__device__ __forceinline__ int64_t upper_bound_col(const int32_t* __restrict__ col, int64_t lo, int64_t hi, int32_t key) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (col[mid] <= key) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// grid (copies, slices): workgroup (c, y) takes nodes [y * kEdgeSlice, ...) and entries [y * kEdgeSlice, ...) of copy
// c's graph, striding by gridDim.y * kEdgeSlice.  CSR: with LOOPS every row gains one self entry; the rows of copy c
// start behind the copies before it (entry_base[c] + node_base[c] entries with LOOPS) and an entry of local row j with
// local column cl lands behind the j self entries of the rows in front of it, and behind its own row's one if cl > j
// (columns ascending: the self entry sits behind every column <= j, as mp_csr_from_coo places an inserted loop
// behind an existing one).
template <bool CSR, bool LOOPS>
__global__ __launch_bounds__(kBlock) void edge_expand_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int32_t* __restrict__ row,
    const int32_t* __restrict__ eid, const int64_t* __restrict__ graph_ptr, const int32_t* __restrict__ copy_graph,
    const int32_t* __restrict__ copy_src, const int64_t* __restrict__ node_base, const int64_t* __restrict__ entry_base,
    int64_t n_out_edges, int64_t* __restrict__ src_out, int64_t* __restrict__ dst_out, int64_t* __restrict__ orig_node,
    int32_t* __restrict__ copy_of_node, int64_t* __restrict__ orig_edge, int64_t* __restrict__ id_index,
    int32_t* __restrict__ csr_col, int32_t* __restrict__ csr_eid, int32_t* __restrict__ csr_rowptr) {
  const int64_t c = blockIdx.x;
  const int32_t g = copy_graph[c];
  const int64_t lo = graph_ptr[g], n = graph_ptr[g + 1] - lo;
  const int64_t elo = rowptr[lo], ne = (int64_t)rowptr[lo + n] - elo;
  const int64_t nb = node_base[c], kb = entry_base[c];
  const int64_t stride = (int64_t)gridDim.y * kEdgeSlice;
  if (blockIdx.y == 0 && threadIdx.x == 0) id_index[c] = nb + copy_src[c];
  for (int64_t j = (int64_t)blockIdx.y * kEdgeSlice + threadIdx.x; j < n; j += stride) {
    for (int64_t jj = j; jj < n && jj < j + kEdgeSlice; jj += kBlock) {
      orig_node[nb + jj] = lo + jj;
      copy_of_node[nb + jj] = (int32_t)c;
      if (CSR) {
        const int64_t rs = rowptr[lo + jj];
        const int64_t start = kb + (rs - elo) + (LOOPS ? nb + jj : 0);
        csr_rowptr[nb + jj] = (int32_t)start;
        if (LOOPS) {
          const int64_t before = upper_bound_col(col, rs, rowptr[lo + jj + 1], (int32_t)(lo + jj)) - rs;
          csr_col[start + before] = (int32_t)(nb + jj);
          csr_eid[start + before] = (int32_t)(-1 - (nb + jj));
        }
      }
    }
  }
  for (int64_t i = (int64_t)blockIdx.y * kEdgeSlice + threadIdx.x; i < ne; i += stride) {
    for (int64_t ii = i; ii < ne && ii < i + kEdgeSlice; ii += kBlock) {
      const int64_t e = elo + ii, k = kb + ii;
      const int64_t j = (int64_t)row[e] - lo, cl = (int64_t)col[e] - lo;
      src_out[k] = nb + cl;
      dst_out[k] = nb + j;
      orig_edge[k] = eid ? (int64_t)eid[e] : e;
      if (CSR) {
        const int64_t pos = k + (LOOPS ? nb + j + (cl > j ? 1 : 0) : 0);
        csr_col[pos] = (int32_t)(nb + cl);
        csr_eid[pos] = (int32_t)k;
      }
    }
  }
  if (CSR && c == 0 && blockIdx.y == 0 && threadIdx.x == 0)
    csr_rowptr[node_base[gridDim.x]] = (int32_t)(n_out_edges + (LOOPS ? node_base[gridDim.x] : 0));
}

__global__ void edge_empty_rowptr_kernel(int32_t* rowptr) { rowptr[0] = 0; }

// ---- hop distances -----------------------------------------------------------------------------------------------

constexpr int kBfsMaxNodes = 1 << 16;
constexpr int kBfsWords = kBfsMaxNodes / 32;

// workgroup s: breadth-first search from sources[s] inside its graph [graph_ptr[g], graph_ptr[g + 1]) along the rows of
// the CSR (row u = the nodes u reaches in one hop); the pairs pair_off[s] .. pair_off[s + 1] (destinations pair_dst,
// output slots pair_pos) get the level at which their destination is first reached, 0 for the source itself, -1 if the
// search ends without it.  A pair's slot is written and re-read by one thread only (pairs stride by the block).
__global__ __launch_bounds__(kBlock) void hop_bfs_kernel(
    const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, const int64_t* __restrict__ graph_ptr,
    const int64_t* __restrict__ sources, const int32_t* __restrict__ source_graph,
    const int64_t* __restrict__ pair_off, const int64_t* __restrict__ pair_dst, const int64_t* __restrict__ pair_pos,
    int32_t* __restrict__ dist) {
  __shared__ uint32_t vis[kBfsWords], fr[kBfsWords], nx[kBfsWords];
  __shared__ int s_left, s_new;
  const int64_t s = blockIdx.x;
  const int t = threadIdx.x;
  const int32_t g = source_graph[s];
  const int64_t lo = graph_ptr[g], n = graph_ptr[g + 1] - lo;
  const int64_t src = sources[s] - lo;
  const int64_t p0 = pair_off[s], p1 = pair_off[s + 1];
  // (the caller checks both; the guard keeps the bitmaps in bounds whatever the data say)
  const bool ok = n > 0 && n <= kBfsMaxNodes && src >= 0 && src < n;
  const int words = ok ? (int)((n + 31) >> 5) : 0;
  for (int w = t; w < words; w += kBlock) { vis[w] = 0u; fr[w] = 0u; nx[w] = 0u; }
  if (t == 0) s_left = 0;
  __syncthreads();
  if (t == 0 && ok) {
    vis[src >> 5] = 1u << (src & 31);
    fr[src >> 5] = 1u << (src & 31);
  }
  int mine = 0;
  for (int64_t p = p0 + t; p < p1; p += kBlock) {
    const int64_t d = pair_dst[p] - lo;
    const bool open = ok && d >= 0 && d < n && d != src;
    dist[pair_pos[p]] = (ok && d == src) ? 0 : -1;
    mine += open ? 1 : 0;
  }
  if (mine) atomicAdd(&s_left, mine);
  for (int level = 1;; ++level) {
    __syncthreads();                                   // frontier, pair states and s_left of the previous level
    if (s_left == 0) break;                            // (uniform: every pair resolved, or none open)
    if (t == 0) s_new = 0;
    __syncthreads();
    int found = 0;
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
          if (!(old & m)) { atomicOr(&nx[v >> 5], m); found = 1; }
        }
      }
    }
    if (found) atomicOr(&s_new, 1);
    __syncthreads();                                   // this level's discoveries are complete
    if (s_new == 0) break;                             // (uniform) nothing new: the open pairs stay -1
    int closed = 0;
    for (int64_t p = p0 + t; p < p1; p += kBlock) {
      const int64_t d = pair_dst[p] - lo;
      if (d < 0 || d >= n || d == src) continue;
      const int64_t q = pair_pos[p];
      // open until now and reached: reached at this level (every earlier level closed what it reached)
      if (dist[q] < 0 && (nx[d >> 5] & (1u << (d & 31)))) { dist[q] = level; ++closed; }
    }
    if (closed) atomicSub(&s_left, closed);
    __syncthreads();                                   // nx read by the pair pass before it is cleared
    for (int w = t; w < words; w += kBlock) { fr[w] = nx[w]; nx[w] = 0u; }
  }
}

}  // namespace mp

using namespace mp;

extern "C" int mp_edge_expand(const int32_t* rowptr, const int32_t* col, const int32_t* row, const int32_t* eid,
                              int64_t N, int64_t nnz, const int64_t* graph_ptr, int64_t n_graphs,
                              const int32_t* copy_graph, const int32_t* copy_src, const int64_t* node_base,
                              const int64_t* entry_base, int64_t n_copies, int64_t n_out_nodes, int64_t n_out_edges,
                              int64_t max_graph_size, int32_t flags, int64_t* edge_index, int64_t* orig_node,
                              int32_t* copy_of_node, int64_t* orig_edge, int64_t* id_index, int32_t* csr_rowptr,
                              int32_t* csr_col, int32_t* csr_eid, mp_stream_t stream) {
  if (N < 0 || nnz < 0 || n_graphs < 0 || n_copies < 0 || n_out_nodes < 0 || n_out_edges < 0 || max_graph_size < 0)
    return MP_ERR_INVALID_ARG;
  if (flags & ~(MP_EGO_CSR | MP_EGO_CSR_SELF_LOOPS)) return MP_ERR_INVALID_ARG;
  if ((flags & MP_EGO_CSR_SELF_LOOPS) && !(flags & MP_EGO_CSR)) return MP_ERR_INVALID_ARG;
  const bool want_csr = (flags & MP_EGO_CSR) != 0, loops = (flags & MP_EGO_CSR_SELF_LOOPS) != 0;
  if (!rowptr || !graph_ptr) return MP_ERR_INVALID_ARG;
  if (nnz > 0 && (!col || !row)) return MP_ERR_INVALID_ARG;
  if (n_copies > 0 && (!copy_graph || !copy_src || !node_base || !entry_base || !id_index)) return MP_ERR_INVALID_ARG;
  if (n_out_nodes > 0 && (!orig_node || !copy_of_node)) return MP_ERR_INVALID_ARG;
  if (n_out_edges > 0 && (!edge_index || !orig_edge)) return MP_ERR_INVALID_ARG;
  if (want_csr && (!csr_rowptr || ((n_out_edges > 0 || loops) && n_out_nodes > 0 && (!csr_col || !csr_eid))))
    return MP_ERR_INVALID_ARG;
  if (n_copies > 0 && n_graphs == 0) return MP_ERR_INVALID_ARG;
  // int32 ids and positions: the CSR (row starts up to nnz + N', node ids), copy_of_node, the base CSR
  const int64_t kMax = INT32_MAX;
  if (N >= kMax || nnz > kMax || n_copies > kMax || n_graphs >= kMax) return MP_ERR_UNSUPPORTED;
  if (n_out_nodes >= kMax || n_out_edges > kMax || n_out_edges + (loops ? n_out_nodes : 0) > kMax)
    return MP_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  if (n_copies == 0) {
    if (want_csr) {
      hipLaunchKernelGGL(edge_empty_rowptr_kernel, dim3(1), dim3(1), 0, st, csr_rowptr);
      MP_LAUNCH_CHECK();
    }
    return MP_OK;
  }
  int64_t slices = ceil_div(max_graph_size > 0 ? max_graph_size : 1, kEdgeSlice);
  if (slices > 65535) slices = 65535;
  const dim3 grid((unsigned)n_copies, (unsigned)slices);
  int64_t* src_out = edge_index;
  int64_t* dst_out = edge_index ? edge_index + n_out_edges : nullptr;
#define EDGE_LAUNCH(C_, L_)                                                                                        \
  hipLaunchKernelGGL((edge_expand_kernel<C_, L_>), grid, dim3(kBlock), 0, st, rowptr, col, row, eid, graph_ptr,     \
                     copy_graph, copy_src, node_base, entry_base, n_out_edges, src_out, dst_out, orig_node,          \
                     copy_of_node, orig_edge, id_index, csr_col, csr_eid, csr_rowptr)
  if (!want_csr) EDGE_LAUNCH(false, false);
  else if (!loops) EDGE_LAUNCH(true, false);
  else EDGE_LAUNCH(true, true);
#undef EDGE_LAUNCH
  MP_LAUNCH_CHECK();
  return MP_OK;
}

extern "C" int mp_hop_distances(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz,
                                const int64_t* graph_ptr, int64_t n_graphs, int64_t max_graph_nodes,
                                const int64_t* sources, const int32_t* source_graph, int64_t n_sources,
                                const int64_t* pair_off, const int64_t* pair_dst, const int64_t* pair_pos,
                                int64_t n_pairs, int32_t* dist, mp_stream_t stream) {
  if (N < 0 || nnz < 0 || n_graphs < 0 || max_graph_nodes < 0 || n_sources < 0 || n_pairs < 0)
    return MP_ERR_INVALID_ARG;
  if (!rowptr || !graph_ptr) return MP_ERR_INVALID_ARG;
  if (nnz > 0 && !col) return MP_ERR_INVALID_ARG;
  if (n_sources > 0 && (!sources || !source_graph || !pair_off || n_graphs == 0)) return MP_ERR_INVALID_ARG;
  if (n_pairs > 0 && (!pair_dst || !pair_pos || !dist || n_sources == 0)) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || nnz > INT32_MAX || n_sources > INT32_MAX || n_graphs >= INT32_MAX) return MP_ERR_UNSUPPORTED;
  if (max_graph_nodes > kBfsMaxNodes) return MP_ERR_UNSUPPORTED;     // the bitmaps live in LDS
  if (n_sources == 0) return MP_OK;
  hipLaunchKernelGGL(hop_bfs_kernel, dim3((unsigned)n_sources), dim3(kBlock), 0, as_stream(stream), rowptr, col,
                     graph_ptr, sources, source_graph, pair_off, pair_dst, pair_pos, dist);
  MP_LAUNCH_CHECK();
  return MP_OK;
}
