// Graph-task batches on the device (GraphGym's dataset.task = graph: DataLoader(dataset, collate_fn=Batch.collate(),
// batch_size=cfg.train.batch_size, shuffle=True), graphgym/loader.py:247-260).  A dataset is ONE base CSR (row r =
// in-edges of r, columns ascending inside a row) that holds the disjoint union of G graphs; graph g is the node range
// graph_ptr[g] .. graph_ptr[g + 1] and so the entry range rowptr[graph_ptr[g]] .. rowptr[graph_ptr[g + 1]].  A batch is a
// list ids [B] of graph ids in batch order (any order, repeats allowed) with the exclusive prefix sums node_off [B + 1] and
// entry_off [B + 1] of the listed graphs' node and entry counts, which the caller computes from its host mirrors of
// graph_ptr and the entry pointer: n = node_off[B] and nnz = entry_off[B] are known before the launch, nothing is read
// back.  Collation is then a segmented copy with rebasing, one thread per output element:
//   batch node k   of batch graph j (node_off[j] <= k < node_off[j + 1]): base node v = graph_ptr[ids[j]] + k - node_off[j]
//                  rowptr_out[k] = rowptr[v] - rowptr[graph_ptr[ids[j]]] + entry_off[j], owner[k] = j, orig_node[k] = v;
//                  thread n writes rowptr_out[n] = nnz
//   batch entry e  of batch graph j (entry_off[j] <= e < entry_off[j + 1]): base entry s = rowptr[graph_ptr[ids[j]]] + e -
//                  entry_off[j]; col_out[e] = col[s] - graph_ptr[ids[j]] + node_off[j], base_entry[e] = s, val_out[e] =
//                  val[s]; row_out[e] = the batch row that holds e (an upper bound over the graph's rows of rowptr), and
//                  edge_index [2, nnz] = (col_out, row_out) as int64: the batch's COO list in CSR order
// The owner j is an upper bound (draws.h) over the B + 1 offsets, staged in LDS when they fit kStageCap words and read
// from global memory above it.  One launch: the first ceil((n + 1) / 256) workgroups take the nodes, the rest the entries.
// Work and memory follow the batch; nothing is sized by the dataset.
//
// mp_collate_check_entries is the dataset's one construction-time pass: the first stored entry that joins two graphs.
#include "common.h"
#include "draws.h"

namespace mp {

constexpr int kStageCap = 1024;      // offsets (B + 1) a workgroup stages in LDS: 4 KiB

struct CollateArgs {
  const int32_t* rowptr;
  const int32_t* col;
  const float* val;
  const int64_t* graph_ptr;
  const int32_t* ids;
  const int32_t* node_off;
  const int32_t* entry_off;
  int64_t N, nnz_base, G, B, n, nnz, row_blocks;
  int32_t* rowptr_out;
  int64_t* owner;
  int32_t* owner32;
  int64_t* orig_node;
  int32_t* col_out;
  int32_t* row_out;
  int32_t* base_entry;
  int64_t* edge_index;
  float* val_out;
};

__device__ __forceinline__ int64_t clamp_to(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the batch graph that holds element i of the prefix array `off` [B + 1] (off[j] <= i < off[j + 1]; empty graphs are
// stepped over), and the first base node of that graph.  The clamps keep every read of a caller whose offsets do not
// describe its ids inside the arrays; for a consistent caller they change nothing.
template <class Off>
__device__ __forceinline__ int64_t owner_of(Off off, const CollateArgs& a, int64_t i, int64_t& first_node) {
  const int64_t j = clamp_to(upper_bound(off, 0, a.B + 1, i) - 1, 0, a.B - 1);
  first_node = clamp_to(a.graph_ptr[clamp_to(a.ids[j], 0, a.G - 1)], 0, a.N);
  return j;
}

template <class Off>
__device__ __forceinline__ void collate_node(Off off, const CollateArgs& a, int64_t k) {
  if (k == a.n) {
    a.rowptr_out[k] = (int32_t)a.nnz;
    return;
  }
  int64_t g0;
  const int64_t j = owner_of(off, a, k, g0);
  const int64_t v = clamp_to(g0 + (k - (int64_t)off[j]), 0, a.N);
  a.rowptr_out[k] = (int32_t)((int64_t)a.rowptr[v] - (int64_t)a.rowptr[g0] + (int64_t)a.entry_off[j]);
  a.owner[k] = j;
  a.owner32[k] = (int32_t)j;
  a.orig_node[k] = v;
}

template <class Off>
__device__ __forceinline__ void collate_entry(Off off, const CollateArgs& a, int64_t e) {
  int64_t g0;
  const int64_t j = owner_of(off, a, e, g0);
  const int64_t s = clamp_to((int64_t)a.rowptr[g0] + (e - (int64_t)off[j]), 0, a.nnz_base - 1);
  const int64_t shift = (int64_t)a.node_off[j] - g0;
  const int64_t g1 = clamp_to(g0 + ((int64_t)a.node_off[j + 1] - (int64_t)a.node_off[j]), g0, a.N);
  const int64_t c = (int64_t)a.col[s] + shift;
  const int64_t r = upper_bound(a.rowptr, g0, g1 + 1, s) - 1 + shift;     // the last row that starts at or before s
  a.col_out[e] = (int32_t)c;
  a.row_out[e] = (int32_t)r;
  a.base_entry[e] = (int32_t)s;
  a.edge_index[e] = c;
  a.edge_index[a.nnz + e] = r;
  if (a.val_out) a.val_out[e] = a.val[s];
}

template <bool kStaged>
__global__ __launch_bounds__(kBlock) void collate_kernel(CollateArgs a) {
  __shared__ int32_t staged[kStaged ? kStageCap : 1];
  const bool nodes = (int64_t)blockIdx.x < a.row_blocks;              // (block-uniform)
  const int32_t* __restrict__ off = nodes ? a.node_off : a.entry_off;
  if (kStaged) {
    for (int64_t i = threadIdx.x; i <= a.B; i += kBlock) staged[i] = off[i];
    __syncthreads();
  }
  if (nodes) {
    const int64_t k = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (k > a.n) return;
    if (kStaged) collate_node((const int32_t*)staged, a, k); else collate_node(off, a, k);
  } else {
    const int64_t e = ((int64_t)blockIdx.x - a.row_blocks) * kBlock + threadIdx.x;
    if (e >= a.nnz) return;
    if (kStaged) collate_entry((const int32_t*)staged, a, e); else collate_entry(off, a, e);
  }
}

__global__ __launch_bounds__(kBlock) void collate_check_kernel(const int32_t* __restrict__ col,
                                                               const int32_t* __restrict__ row_of, int64_t nnz,
                                                               const int64_t* __restrict__ graph_ptr, int64_t G,
                                                               int32_t* __restrict__ first_bad) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= nnz) return;
  const int64_t g = clamp_to(upper_bound(graph_ptr, 0, G + 1, (int64_t)row_of[e]) - 1, 0, G - 1);
  const int64_t c = col[e];
  if (c < graph_ptr[g] || c >= graph_ptr[g + 1]) atomicMin(first_bad, (int32_t)e);
}

}  // namespace mp

using namespace mp;

extern "C" int mp_collate_stage_cap(void) { return kStageCap; }

extern "C" int mp_collate_graphs(const int32_t* rowptr, const int32_t* col, const float* val, int64_t N, int64_t nnz_base,
                                 const int64_t* graph_ptr, int64_t G, const int32_t* ids, const int32_t* node_off,
                                 const int32_t* entry_off, int64_t B, int64_t n, int64_t nnz, int32_t* rowptr_out,
                                 int64_t* owner, int32_t* owner32, int64_t* orig_node, int32_t* col_out, int32_t* row_out,
                                 int32_t* base_entry, int64_t* edge_index, float* val_out, mp_stream_t stream) {
  if (N < 0 || nnz_base < 0 || G < 0 || B < 0 || n < 0 || nnz < 0) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || nnz_base >= INT32_MAX || G >= INT32_MAX || B >= INT32_MAX || n >= INT32_MAX || nnz >= INT32_MAX)
    return MP_ERR_UNSUPPORTED;
  if (B == 0 || n == 0) return MP_OK;
  if (G == 0 || N == 0 || (nnz > 0 && nnz_base == 0)) return MP_ERR_INVALID_ARG;      // a batch of an empty dataset
  if (!rowptr || !graph_ptr || !ids || !node_off || !entry_off) return MP_ERR_INVALID_ARG;
  if (!rowptr_out || !owner || !owner32 || !orig_node) return MP_ERR_INVALID_ARG;
  if (nnz > 0 && (!col || !col_out || !row_out || !base_entry || !edge_index)) return MP_ERR_INVALID_ARG;
  if (val_out && !val) return MP_ERR_INVALID_ARG;
  CollateArgs a;
  a.rowptr = rowptr; a.col = col; a.val = val; a.graph_ptr = graph_ptr;
  a.ids = ids; a.node_off = node_off; a.entry_off = entry_off;
  a.N = N; a.nnz_base = nnz_base; a.G = G; a.B = B; a.n = n; a.nnz = nnz;
  a.row_blocks = ceil_div(n + 1, kBlock);
  a.rowptr_out = rowptr_out; a.owner = owner; a.owner32 = owner32; a.orig_node = orig_node;
  a.col_out = col_out; a.row_out = row_out; a.base_entry = base_entry; a.edge_index = edge_index; a.val_out = val_out;
  const dim3 grid((unsigned)(a.row_blocks + ceil_div(nnz, kBlock)));
  if (B + 1 <= kStageCap)
    hipLaunchKernelGGL(collate_kernel<true>, grid, dim3(kBlock), 0, as_stream(stream), a);
  else
    hipLaunchKernelGGL(collate_kernel<false>, grid, dim3(kBlock), 0, as_stream(stream), a);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

extern "C" int mp_collate_check_entries(const int32_t* col, const int32_t* row_of, int64_t nnz, const int64_t* graph_ptr,
                                        int64_t G, int32_t* first_bad, mp_stream_t stream) {
  if (nnz < 0 || G < 0) return MP_ERR_INVALID_ARG;
  if (nnz >= INT32_MAX || G >= INT32_MAX) return MP_ERR_UNSUPPORTED;
  if (nnz == 0) return MP_OK;
  if (G == 0 || !col || !row_of || !graph_ptr || !first_bad) return MP_ERR_INVALID_ARG;
  hipLaunchKernelGGL(collate_check_kernel, dim3((unsigned)ceil_div(nnz, kBlock)), dim3(kBlock), 0, as_stream(stream), col,
                     row_of, nnz, graph_ptr, G, first_bad);
  MP_LAUNCH_CHECK();
  return MP_OK;
}
