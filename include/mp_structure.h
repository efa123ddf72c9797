/*
 * mp_structure.h — C ABI of the centrality layer of libmpengine.so (csrc/centrality.hip).
 *
 * What it replaces: pagerank_fun, centrality_fun and onehot_fun of graphgym/models/feature_augment.py:55-58,70-73,88-91
 * (nx.pagerank, nx.betweenness_centrality and torch.randperm, one host call per graph), the node features and the
 * label of the synthetic design-space grids (run/grids/design/round1.txt:52,72-73,92, round2.txt:53).
 *
 * The conventions are those of mp_engine.h (device pointers, caller-owned buffers, everything enqueued on `stream`,
 * nothing allocates, nothing synchronises, mp_status return codes).  This header is separate from mp_engine.h, and its
 * entries are bound from a table of their own (graphgym_amd/_lib_structure.py), because the closure tests over
 * mp_engine.h name every entry of that header; the closures over this one are tests/test_centrality_host.py and
 * tests/test_poison_structure_gpu.py.
 *
 * Every entry name starts with mp_struct_.
 *
 * The graph.  rowptr [N + 1] / col [nnz] is the engine's CSR (columns ascending inside a row, no column twice in a row)
 * of a symmetric operator: the disjoint union of the n_graphs graphs graph_ptr [n_graphs + 1] (int64, rising from 0 to
 * N, no empty graph) delimits.  An entry whose column lies outside its row's graph is not followed.  The caller knows
 * the graphs' sizes (it checked graph_ptr) and derives from them the small host-side tables the entries take: PageRank's
 * chunk_ptr / n_chunks, betweenness' slice_ptr / n_slices and max_graph_nodes, the size of the largest graph, which
 * sizes the workspace; a graph above it is left out by the kernels (its outputs are then not written).
 *
 * Order.  No entry uses a float atomic.  Every floating-point sum is formed in an order that depends on the graph alone
 * (its size and its rows), never on the grid, on the other graphs of the batch or on the workspace's contents: a
 * graph's values are the same bits alone and inside any batch, on every run.
 */
#ifndef MP_STRUCTURE_H
#define MP_STRUCTURE_H

#include "mp_engine.h"

#ifdef __cplusplus
extern "C" {
#endif

enum mp_struct_limit {
  /* PageRank: a graph of up to this many nodes is iterated by one workgroup with x, x' and 1/deg in LDS (3 doubles a
     node: 48 KiB of the CU's 160, three workgroups a CU); a larger one by row-parallel steps over the workspace */
  MP_STRUCT_PAGERANK_LDS_NODES = 2048,
  /* PageRank, large form: nodes behind one partial sum of dsum and err (one workgroup's share of a step) */
  MP_STRUCT_PAGERANK_CHUNK = 1024,
  /* betweenness: sources one workgroup walks, in order, into one partial vector */
  MP_STRUCT_BETWEENNESS_SLICE = 32,
  /* betweenness: a graph of up to this many nodes keeps level, sigma, delta and the slice's sum in LDS (28 bytes a
     node: 28 KiB); a larger one keeps them in the workspace */
  MP_STRUCT_BETWEENNESS_LDS_NODES = 1024,
  /* betweenness: the largest graph (the limit of mp_hop_sums) */
  MP_STRUCT_BETWEENNESS_MAX_NODES = 65536
};

/* bytes of the workspace of mp_struct_pagerank for N nodes in n_graphs graphs whose large-form graphs have n_chunks
   chunks in all (below): a token 16 bytes while every graph takes the LDS form (n_chunks = 0), else the two ping-pong
   vectors, 1/deg, the per-chunk partial sums and the per-graph dangling sums.  Host only.  The workspace's contents on
   entry do not matter. */
int mp_struct_pagerank_ws_bytes(int64_t N, int64_t n_graphs, int64_t n_chunks, size_t* bytes);

/* PageRank per graph in float64: nx.pagerank's power iteration (its SciPy form) with uniform personalisation and
   dangling weights.  With n the graph's node count, p = 1 / n, x = p and inv[i] = 1 / (stored entries of row i) (rows
   without entries are dangling), one step is
     y[j]  = sum over the entries i of row j, in stored order, of x[i] inv[i]
     dsum  = sum of x over the dangling nodes
     x'[j] = alpha (y[j] + dsum p) + (1 - alpha) p
     err   = sum over j of |x'[j] - x[j]|
   and the result is the x' of the first step with err < n tol: out [N] receives it and iters [n_graphs] the number of
   that step, counted from 1; a graph that has not stopped after max_iter steps gets iters = -1 (out then holds the x'
   of step max_iter).  Every graph stops on its own count; the stop state lives on the device and nothing is read back.
   Which form a graph takes depends on its own n.  chunk_ptr [n_graphs + 1] (int64) is the exclusive prefix sum of the
   graphs' chunk counts, ceil(n / MP_STRUCT_PAGERANK_CHUNK) for a graph above MP_STRUCT_PAGERANK_LDS_NODES nodes and 0
   for any other, and n_chunks its last value; chunk_ptr may be NULL when n_chunks is 0.  In the large form a chunk's
   share of dsum and err is one workgroup's fixed-order sum and a graph's the sum of its chunks in order; it enqueues
   2 max_iter + 2 launches (the steps of a finished graph return at once).  alpha outside [0, 1], tol < 0 or
   max_iter < 1: MP_ERR_INVALID_ARG. */
int mp_struct_pagerank(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, const int64_t* graph_ptr,
                       int64_t n_graphs, const int64_t* chunk_ptr, int64_t n_chunks, double alpha, double tol,
                       int32_t max_iter, double* out, int32_t* iters, void* ws, size_t ws_bytes, mp_stream_t stream);

/* bytes of the workspace of mp_struct_betweenness: ceil(max_graph_nodes / MP_STRUCT_BETWEENNESS_SLICE) partial vectors
   of N doubles, and as many level / sigma / delta vectors when max_graph_nodes is above
   MP_STRUCT_BETWEENNESS_LDS_NODES.  Host only.  The workspace's contents on entry do not matter. */
int mp_struct_betweenness_ws_bytes(int64_t N, int64_t max_graph_nodes, size_t* bytes);

/* Betweenness centrality per graph in float64: nx.betweenness_centrality (Brandes; unweighted, normalized, without
   endpoints) from every node as source.  Per source a level-synchronous search gives level[v] and the number of
   shortest paths sigma[v] (a double: exact below 2^53), then from the deepest level up
     delta[v] = sum over the entries w of row v with level[w] = level[v] + 1, in stored order, of
                sigma[v] ((1 + delta[w]) / sigma[w])
   Both directions are pulls: a node computes its own value from its row.  The sources of a graph are cut into slices
   of MP_STRUCT_BETWEENNESS_SLICE, counted from the graph's first node; workgroup b takes slice b - slice_ptr[g] of
   graph g (slice_ptr [n_graphs + 1], int64: the exclusive prefix sum of ceil(n / MP_STRUCT_BETWEENNESS_SLICE)), walks its
   sources in order and adds delta (the source's own left out) into the slice's partial vector; a second kernel adds
   a node's partials in slice order and scales by 1 / ((n - 1) (n - 2)) (0 for n <= 2) into out [N].  n_slices is
   slice_ptr's last value.  Self loops play no part, unreachable nodes contribute nothing, and a node no shortest
   path passes through gets exactly 0.0.  max_graph_nodes > MP_STRUCT_BETWEENNESS_MAX_NODES: MP_ERR_UNSUPPORTED. */
int mp_struct_betweenness(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, const int64_t* graph_ptr,
                          int64_t n_graphs, int64_t max_graph_nodes, const int64_t* slice_ptr, int64_t n_slices,
                          double* out, void* ws, size_t ws_bytes, mp_stream_t stream);

/* One-hot ids: out[v] = perm(i) for node v = graph_ptr[g] + i, perm the keyed bijection on [0, n_g) of draws.h
   (mix64-derived round keys from (seed, MP_STRUCT_ONEHOT_STREAM, g), a balanced Feistel network, cycle walking): what
   torch.randperm(num_nodes) is to onehot_fun.  One launch, integer mixing only; the value depends on (seed, g, i, n_g)
   and nothing else. */
int mp_struct_onehot(const int64_t* graph_ptr, int64_t n_graphs, int64_t N, uint64_t seed, int64_t* out,
                     mp_stream_t stream);

/* the stream word of mp_struct_onehot's keys (the place link.hip gives its call offset) */
#define MP_STRUCT_ONEHOT_STREAM 0x6F6E65686F74

#ifdef __cplusplus
}
#endif

#endif /* MP_STRUCTURE_H */
