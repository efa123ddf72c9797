/*
 * mp_neighbor.h — C ABI of the neighbour sampler of libmpengine.so (csrc/neighbor.hip): the sampled computation tree of
 * a batch of seed nodes as ONE subgraph (the form of PyG's NeighborLoader: seeds plus sampled in-neighbours per hop),
 * which a model consumes like any other batch.  GraphGym's train.sampler = neighbor with train.neighbor_sizes
 * (graphgym/config.py:248, graphgym/loader_pyg.py:209-215) asks PyG's older NeighborSampler for per-layer bipartite
 * blocks instead; those are not built.
 *
 * The conventions are those of mp_engine.h (device pointers, caller-owned buffers, everything enqueued on `stream`,
 * nothing allocates, nothing synchronises, mp_status return codes).  This header is separate from mp_engine.h, and its
 * entries are bound from a table of their own (graphgym_amd/_lib_neighbor.py), because the closure tests over
 * mp_engine.h name every entry of that header; the closures over this one are tests/test_neighbor_host.py and
 * tests/test_poison_neighbor_gpu.py.
 *
 * Every entry name starts with mp_nbr_.
 *
 * The base is the engine's CSR: rowptr [N + 1] / col [nnz], row v = the in-edges of v, columns ascending inside a row.
 * A node set is a bitmap of N bits as mp_bitmap_mark writes it (uint32 words, bit c & 31 of word c >> 5), word_rank
 * [ceil(N / 32) + 1] the exclusive prefix sum of its words' popcounts: the new id of a member c is
 * word_rank[c >> 5] + popc(word[c >> 5] & ((1u << (c & 31)) - 1)).
 *
 * The draw, in integers only.  perm(seed, offset, g, i, C) is the keyed bijection of [0, C) of csrc/draws.h (the one
 * mp_sample_non_edges ranks non-edges with).  Every entry below XORs MP_NBR_STREAM into the seed it is given, which
 * keeps these draws apart from the other users of the same seed.  A node v that entered the batch at hop h is sampled
 * with fanout s = sizes[h]: with k = deg v if s = -1 or deg v <= s, and k = s otherwise, its sampled entries are the
 * base positions rowptr[v] + perm(seed ^ MP_NBR_STREAM, step, (h << 32) | v, j, deg v) for j < k (k = deg v: the whole
 * row, no permutation is run).  The sample of a node is a pure function of (seed, step, h, v) and the base: not of the
 * rest of the batch, not of the launch geometry.  No float arithmetic, no atomics but the bitmap's atomicOr: the same
 * bits every run.
 *
 * A fanout is -1 or lies in [1, MP_NBR_MAX_FANOUT]: 0 or below -1 is MP_ERR_INVALID_ARG, above MP_NBR_MAX_FANOUT
 * MP_ERR_UNSUPPORTED.  Null pointers where something is to be read or written, negative sizes and a negative hop:
 * MP_ERR_INVALID_ARG; N >= 2^31 - 1 or nnz above 2^31 - 1 - 16 (a row walk steps up to 16 entries past its row in
 * int32): MP_ERR_UNSUPPORTED.  An empty frontier returns MP_OK without a launch.  A frontier entry outside [0, N) is
 * skipped.
 */
#ifndef MP_NEIGHBOR_H
#define MP_NEIGHBOR_H

#include "mp_engine.h"

#define MP_NBR_MAX_FANOUT 256
#define MP_NBR_STREAM 0x4E42525F53414D50

#ifdef __cplusplus
extern "C" {
#endif

/* The seeds of one batch: out[i] = pool[perm(seed ^ MP_NBR_STREAM, epoch, 2^63, first + i, n_pool)] for i < count;
 * pool = NULL is the identity list of n_pool nodes.  Over first = 0 .. n_pool an epoch visits every pool entry exactly
 * once.  first < 0, count < 0 or first + count > n_pool: MP_ERR_INVALID_ARG; n_pool >= 2^31: MP_ERR_UNSUPPORTED. */
int mp_nbr_seeds(const int32_t* pool, int64_t n_pool, int64_t first, int64_t count, uint64_t seed, uint64_t epoch,
                 int32_t* out, mp_stream_t stream);

/* atomicOr of the sampled columns of every frontier node (all of hop `hop`, fanout `fanout`) into `bitmap`, which the
 * caller has zeroed or filled by earlier marks.  One row per group of 16 lanes. */
int mp_nbr_mark(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, const int32_t* frontier,
                int64_t n_frontier, int32_t hop, int32_t fanout, uint64_t seed, uint64_t step, uint32_t* bitmap,
                mp_stream_t stream);

/* cnt[k] = min(deg v, fanout) (deg v for -1) and hop_out[k] = hop for every frontier node v, k its new id under
 * (bitmap, word_rank): the row length is known without walking the row.  The caller presets cnt to 0 and hop_out to
 * the number of hops for the batch nodes no frontier names (those of the last hop: empty rows).  The frontier holds
 * members of the bitmap, each once. */
int mp_nbr_count(const int32_t* rowptr, int64_t N, const int32_t* frontier, int64_t n_frontier, int32_t hop,
                 int32_t fanout, const uint32_t* bitmap, const int32_t* word_rank, int32_t* cnt, int32_t* hop_out,
                 mp_stream_t stream);

/* The rows of the frontier's nodes: from rowptr_sub[k] on (the exclusive prefix sum of mp_nbr_count's cnt), col_sub
 * holds the new ids of the sampled columns and base_entry their positions in the base CSR, in ascending base position
 * — so col_sub ascends inside a row and repeated and self entries of the base stay as stored.  The k <= 256 drawn
 * positions of a row are ranked by counting inside the 16-lane group that owns the row; a row taken whole is copied in
 * order.  The frontier holds members of the bitmap, each once. */
int mp_nbr_fill(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, const int32_t* frontier,
                int64_t n_frontier, int32_t hop, int32_t fanout, uint64_t seed, uint64_t step, const uint32_t* bitmap,
                const int32_t* word_rank, const int32_t* rowptr_sub, int32_t* col_sub, int32_t* base_entry,
                mp_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* MP_NEIGHBOR_H */
