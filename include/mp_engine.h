/*
 * mp_engine.h — C ABI of the MI355X message-passing engine (libmpengine.so).
 *
 * This is the drop-in boundary for GraphGym's neighbour-aggregation hot path.
 * The reference has no native layer (it is pure Python over torch-scatter /
 * TensorFlow ops), so every entry point below cites the *Python* call site
 * whose arithmetic it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - plain pointers + sizes, no torch / C++ types; all pointers are DEVICE
 *     pointers unless the parameter name ends in `_host`;
 *   - every function returns an mp_status (0 = ok); nothing throws;
 *   - the caller owns every buffer (outputs and workspaces); nothing is
 *     allocated or freed inside the library;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*);
 *     functions do not synchronise unless their comment says so;
 *   - matrices are row-major fp32 with an explicit leading dimension (in
 *     elements); indices inside the engine are int32, the COO boundary takes
 *     the int64 `edge_index` tensors GraphGym batches carry;
 *   - row r of a CSR holds the in-edges of DESTINATION node r; `col` holds
 *     SOURCE node ids (SparseAdj: edge_index[0] = row, [1] = col,
 *     sparse_adj.py:50-56; PyG flow source_to_target: edge_index[1] = i);
 *   - per-edge operands (edge features and what is computed from them: M of
 *     mp_spmm_csr_edge_f32, generalconv.py:203-209) stay in INPUT edge order;
 *     a CSR entry finds its row through `eid`, the entry's position in the
 *     input edge list (-1 - i for a self loop the build inserted).
 */
#ifndef MP_ENGINE_H
#define MP_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* mp_stream_t; /* hipStream_t */

/* Zero extents: an array whose extent is an ARGUMENT of the call (nnz, n, M, n_rows; N for arrays of N rows) may be NULL
 * when that extent is 0 — the call then returns MP_OK without a launch — and is MP_ERR_INVALID_ARG when NULL at a
 * non-zero extent.  Required arrays whose extent the call cannot see (col / eid / the head weights of the aggregation
 * entries, which get N but not nnz; X, which has one row per COLUMN) must have an address: a caller with an empty one
 * does not call, or hands in a row nothing reads (the zero-extent rule). */
enum mp_status {
  MP_OK = 0,
  MP_ERR_INVALID_ARG = 1, /* null pointer, negative size, bad enum */
  MP_ERR_UNSUPPORTED = 2, /* e.g. nnz >= 2^31 */
  MP_ERR_WORKSPACE = 3,   /* workspace too small */
  MP_ERR_HIP = 4,         /* a HIP runtime call failed; see mp_last_hip_error */
  MP_ERR_ALIGNMENT = 5    /* pointer / leading dimension not aligned as required */
};

enum mp_reduce { MP_SUM = 0, MP_MEAN = 1, MP_MAX = 2 };

/* mp_csr_from_coo flags */
enum mp_coo_flags {
  MP_COO_REMOVE_SELF_LOOPS = 1, /* torch_geometric.utils.remove_self_loops (idconv.py:302,370) */
  MP_COO_ADD_SELF_LOOPS = 2,    /* append one (i,i) entry per node: tfg add_self_loop_edge via
                                   SparseAdj.add_self_loop (sparse_adj.py:58-63, TfgIDLayer.py:298,547);
                                   PyG add_self_loops (idconv.py:303) */
  MP_COO_KEEP_LOOP_WEIGHT = 4,  /* with REMOVE|ADD: an existing loop's weight replaces `fill` for
                                   that node = PyG add_remaining_self_loops (idconv.py:52-53,140-141,232-233) */
  MP_COO_RECT = 8               /* a rectangular operator (pooling.py:12-33: rows = graphs, columns = nodes): src ids
                                   may be any value below 2^32, not only [0, N).  Without it both ids share
                                   id_bits(N) bits of the sort key and the sort runs over twice that (N = 6e5: 40
                                   bits instead of 52); not with the self-loop flags */
};

/* degree axis for mp_csr_degree / mp_gcn_norm_edges */
enum mp_axis {
  MP_AXIS_ROW = 0, /* by destination: SparseAdj.reduce_sum(axis=-1) (sparse_adj.py:65-85, TfgIDLayer.py:549) */
  MP_AXIS_COL = 1  /* by source: scatter_add(edge_weight, edge_index[0]) (idconv.py:56,144) */
};

/* epilogue activation fused into the aggregation's row flush (K15) */
enum mp_act { MP_ACT_NONE = 0, MP_ACT_RELU = 1 };

int mp_version(void);
/* streaming device copy of n floats (n % 4 == 0, 16-byte aligned), 16 B per lane: the measured-bandwidth
 * yardstick bench.py reports beside the nominal HBM peak */
int mp_copy_probe_f32(const float* src, float* dst, int64_t n, mp_stream_t stream);
/* read-only stream of n floats; sink must hold 256 * 8 * 256 floats (one per launched lane) */
int mp_read_probe_f32(const float* src, int64_t n, float* sink, mp_stream_t stream);
/* a stream restricted to the compute units set in mask (n_words x 32 bits; hipExtStreamCreateWithCUMask):
 * lets a caller run the HBM-bound aggregation and the MFMA-bound transform side by side on disjoint CUs */
int mp_stream_create_cu_mask(const uint32_t* mask, int n_words, mp_stream_t* stream);
int mp_stream_destroy(mp_stream_t stream);
const char* mp_status_str(int status);
/* text of the last failing HIP call on this thread ("" if none) */
const char* mp_last_hip_error(void);

/* ------------------------------------------------------------------ *
 * Placement probe (no counterpart in the reference: this belongs to the  *
 * path's data layout in HBM).  On MI355X a launch that reads X and       *
 * writes Y is up to ~13 % slower depending on which physical memory      *
 * backs the two (high address bits are hashed into the DRAM bank /       *
 * channel selection).  The library allocates nothing: outputs are the    *
 * caller's buffers.  The host side (graphgym_amd/placement.py) times a   *
 * copy between sample chunks of what a launch reads and a candidate      *
 * output buffer with this entry point and re-allocates on conflict.      *
 * ------------------------------------------------------------------ */
/* timed streaming copy (16 B per lane, non-temporal stores): one untimed launch, then `reps` launches between
 * two events; SYNCHRONISES `stream`; *ms_host = mean milliseconds per launch */
int mp_probe_copy_ms(const void* src, void* dst, size_t bytes, int32_t reps, float* ms_host, mp_stream_t stream);
/* timed gather probe — the access pattern of the aggregation itself: each of the dst_bytes / 1024 rows of dst is the
 * sum of `fan` (1..64) pseudo-random 1 KiB rows taken from ALL of [src, src + src_bytes); one untimed launch, then
 * `reps`; SYNCHRONISES `stream`.  Shows the placement effect at full size (+12-13 % good vs bad position of dst). */
int mp_probe_gather_ms(const void* src, size_t src_bytes, void* dst, size_t dst_bytes, int32_t fan, int32_t reps,
                       float* ms_host, mp_stream_t stream);

/* ------------------------------------------------------------------ *
 * Graph construction: COO edge list -> destination-sorted CSR         *
 * replaces: SparseAdj.__init__/add_self_loop (sparse_adj.py:18-63),   *
 *   add_remaining_self_loops / remove_self_loops / add_self_loops     *
 *   call sites in idconv.py:52,140,232,302-304,370                    *
 * ------------------------------------------------------------------ */

/* bytes of workspace mp_csr_from_coo needs for E input edges, N nodes */
int mp_csr_from_coo_ws_bytes(int64_t E, int64_t N, size_t* bytes_host);

/*
 * dst/src: [E] int64 node ids in [0,N) (src: any id below 2^32 with MP_COO_RECT).  w: [E] fp32 or NULL (= all ones).
 * Outputs (capacity E+N entries each; nnz = rowptr[N] afterwards):
 *   rowptr [N+1] int32, col [cap] int32 (sorted by (row, col, input order)),
 *   val [cap] fp32 (may be NULL when w == NULL and fill == 1: unweighted),
 *   eid [cap] int32: input position of each entry, or -1-i for an inserted
 *   loop of node i (may be NULL).
 * Out-of-range node ids make the result undefined; validate on the host
 * (mp_check_edge_index) in debug paths.
 */
int mp_csr_from_coo(const int64_t* dst, const int64_t* src, const float* w,
                    int64_t E, int64_t N, int flags, float fill,
                    int32_t* rowptr, int32_t* col, float* val, int32_t* eid,
                    void* ws, size_t ws_bytes, mp_stream_t stream);

/* counts entries with dst or src outside [0,N) into *bad (device int32) */
int mp_check_edge_index(const int64_t* dst, const int64_t* src, int64_t E,
                        int64_t N, int32_t* bad, mp_stream_t stream);

/* row id of every stored entry: row_of[e] = r for rowptr[r] <= e < rowptr[r+1] */
int mp_csr_row_ids(const int32_t* rowptr, int64_t N, int64_t nnz,
                   int32_t* row_of, mp_stream_t stream);

/* flag[0] (device) = 0 if the stored square operator equals its transpose — every entry (r, c, v) has its mirror
 * (c, r, v) with the same bits and no (r, c) is stored twice — else 1.  The undirected graphs of the reference's
 * datasets (both directions stored, loader.py / transform.py:11-38) are their own transpose: the backward pass
 * dL/dX = A^T dL/dY then needs no second CSR (mp_csr_transpose: a sort of all entries). */
int mp_csr_is_symmetric(const int32_t* rowptr, const int32_t* col, const float* val, int64_t N, int64_t nnz,
                        int32_t* flag, mp_stream_t stream);

/*
 * Transpose (CSR of A^T, i.e. out-edges by source) for the backward pass
 * dL/dX = A^T dL/dY (autodiff of gather + unsorted_segment_sum,
 * sparse_adj.py:91-97; PyG propagate's backward).
 * pos[k] = index in the source CSR of transposed entry k (so per-edge values
 * such as attention coefficients can be permuted with one gather).
 */
/* n_rows x n_cols source (square graphs: both N; pooling operators are rectangular);
 * the workspace query takes N = n_cols */
int mp_csr_transpose_ws_bytes(int64_t nnz, int64_t N, size_t* bytes_host);
int mp_csr_transpose(const int32_t* rowptr, const int32_t* col, const float* val,
                     int64_t n_rows, int64_t n_cols, int64_t nnz,
                     int32_t* t_rowptr, int32_t* t_col, float* t_val, int32_t* pos,
                     void* ws, size_t ws_bytes, mp_stream_t stream);

/* weighted degree: deg[i] = sum of val over row i (axis ROW) or column i (axis COL);
 * val == NULL counts entries.  (K6: sparse_adj.py:84-85, idconv.py:56,144)
 * AXIS_ROW is a fixed-order (Kahan) row sum: bitwise reproducible.  AXIS_COL on a WEIGHTED operator adds with float
 * atomics (order-dependent in the last ulp; exact for val == NULL): for reproducible by-source degrees run AXIS_ROW on
 * the transposed CSR (mp_csr_transpose), as graphgym_amd.graph.CSRGraph.degree('col') does. */
int mp_csr_degree(const int32_t* rowptr, const int32_t* col, const float* val,
                  int64_t N, int64_t nnz, int axis, float* deg, mp_stream_t stream);

/*
 * GCN symmetric normalisation of the stored entries (K6-K8):
 *   dinv = deg^-1/2 with inf/nan -> 0 ; val_out[e] = dinv[row] * val[e] * dinv[col]
 * replaces gcn_norm_adj (TfgIDLayer.py:528-566) and GCNIDConvLayer.norm
 * (idconv.py:132-148).  dinv_out [N] may be NULL.  val may be NULL (ones).
 */
int mp_gcn_norm_edges(const int32_t* rowptr, const int32_t* col, const float* val,
                      int64_t N, int64_t nnz, int deg_axis,
                      float* val_out, float* dinv_out, mp_stream_t stream);

/* diagonal scalings of the stored entries (A3): val_out[e] = row_scale[row] * val[e] * col_scale[col];
 * either scale NULL = ones.  diag @ A = SparseAdj.rmatmul_diag / diag_sparse_matmul (sparse_adj.py:116-119,
 * sparse_ops.py:11-12); A @ diag = matmul_diag / sparse_diag_matmul (sparse_adj.py:110-113, sparse_ops.py:6-7) */
int mp_csr_scale_f32(const int32_t* rowptr, const int32_t* col, const float* val, int64_t N, int64_t nnz,
                     const float* row_scale, const float* col_scale, float* val_out, mp_stream_t stream);

/* mark entries whose SOURCE is an identity node: col_out[e] = col[e] | 0x80000000
 * when is_id[col[e]] != 0.  is_id: [N] uint8 scratch filled from id_index. */
int mp_mark_id_sources(const int32_t* col, int64_t nnz, const int64_t* id_index,
                       int64_t n_id, int64_t N, uint8_t* is_id, int32_t* col_out,
                       mp_stream_t stream);

/* ------------------------------------------------------------------ *
 * Aggregation plan: nnz-balanced row segments + split of hub rows     *
 * (no counterpart in the reference; built once per graph and cached)  *
 * ------------------------------------------------------------------ */
/* cfg_host: {seg_cost, row_cost, hub_deg, piece_edges} or NULL for the defaults {320, 4, 1024, 256}: a segment is a
 * run of whole rows of cost ~seg_cost (1 per stored entry + row_cost per row); rows with more than hub_deg entries
 * are split into pieces of piece_edges.  The configuration travels with the plan (counts_host[5..7]); there is no
 * process-wide state. */
int mp_spmm_plan_bytes(int64_t N, int64_t nnz, const int32_t* cfg_host, size_t* bytes_host);
/* counts_host[8] <- {n_seg, n_hub, n_piece, cap_hub, cap_piece, seg_cost, hub_deg,
 * piece_edges}; SYNCHRONISES `stream` (once per graph) */
int mp_spmm_plan_build(const int32_t* rowptr, int64_t N, int64_t nnz, const int32_t* cfg_host,
                       int32_t* plan, size_t plan_bytes, int32_t* counts_host,
                       mp_stream_t stream);
/* workspace bytes for an aggregation of width d with this plan */
int mp_spmm_ws_bytes(const int32_t* counts_host, int32_t d, int reduce,
                     int two_branch, size_t* bytes_host);

/* ------------------------------------------------------------------ *
 * The hot path: Y = reduce_{e in row r} val[e] * X[col[e], :]         *
 * replaces SparseAdj.matmul (sparse_adj.py:91-97) = tf.gather * w ->  *
 * unsorted_segment_sum; PyG MessagePassing.propagate + torch_scatter  *
 * (idconv.py:89,177,235,315,371; generalconv.py:86); mean_reducer     *
 * (TfgIDLayer.py:98); aggr='max' (generalconv.py:18).                 *
 * ------------------------------------------------------------------ */
/*
 * X [n_src, d] (ldx), Y [N, d] (ldy).  val NULL = unweighted.
 * reduce: MP_SUM | MP_MEAN (sum / row entry count; empty row -> 0) |
 *         MP_MAX (empty row -> 0; argmax [N, d] int32 receives the CSR entry
 *         index of the winner, -1 for empty rows; may be NULL).
 * Epilogue, applied per output row before the store (K15, K17):
 *   y = act( y + self_scale * S[r, :] + bias )
 *   S (lds) NULL = no self term (GIN's (1+eps)*x_i: TfgIDLayer.py:157-159,
 *   idconv.py:371); bias [d] NULL = none.
 */
int mp_spmm_csr_f32(const int32_t* rowptr, const int32_t* col, const float* val,
                    int64_t N, const int32_t* plan, const int32_t* counts_host,
                    const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t d,
                    int reduce, const float* S, int64_t lds, float self_scale,
                    const float* bias, int act, int32_t* argmax,
                    void* ws, size_t ws_bytes, mp_stream_t stream);

/*
 * Inference-time fusion of the layer's post-ops (graphgym/models/layer.py:26-47,
 * gnn.py:79-80) into the row flush:
 *   y = act( (reduce + self_scale * S[r]) * col_scale + col_shift ) ; optionally y /= max(||y||_2, l2_eps)
 * col_scale / col_shift [d] fold conv bias + BatchNorm1d in eval mode (gamma / sqrt(var + eps), ...).
 * l2_normalize needs the whole row in one wave: d <= 256 (MP_ERR_UNSUPPORTED otherwise).
 */
int mp_spmm_csr_epilogue_f32(const int32_t* rowptr, const int32_t* col, const float* val,
                             int64_t N, const int32_t* plan, const int32_t* counts_host,
                             const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t d,
                             int reduce, const float* S, int64_t lds, float self_scale,
                             const float* col_scale, const float* col_shift, int act,
                             int l2_normalize, float l2_eps,
                             void* ws, size_t ws_bytes, mp_stream_t stream);

/*
 * ID-GNN two-branch aggregation in one pass over the edges (A7):
 *   P[r,:] = sum_e val[e] * X[col[e],:]
 *   Q[r,:] = sum_{e : source is an identity node} val[e] * X[col[e],:]
 * so that  P W + Q W_id  ==  A_hat (X W + S X W_id)  of gcn_id
 * (TfgIDLayer.py:510-517) / GCNIDConvLayer.forward (idconv.py:152-177).
 * col must carry the identity mark of mp_mark_id_sources.
 */
int mp_idgnn_agg_f32(const int32_t* rowptr, const int32_t* col_marked, const float* val,
                     int64_t N, const int32_t* plan, const int32_t* counts_host,
                     const float* X, int64_t ldx, float* P, int64_t ldp,
                     float* Q, int64_t ldq, int32_t d,
                     void* ws, size_t ws_bytes, mp_stream_t stream);

/* backward of MP_MAX: dX[col[e], c] += val[e] * dY[r,c] with e = argmax[r,c] >= 0
 * (dX pre-zeroed by the caller; val NULL = ones) */
int mp_spmm_max_bwd_f32(const int32_t* col, const float* val, const int32_t* argmax,
                        const float* dY, int64_t ldy, int64_t N, int32_t d,
                        float* dX, int64_t ldx, mp_stream_t stream);

/* ------------------------------------------------------------------ *
 * bf16 storage, fp32 accumulation                     *
 * ------------------------------------------------------------------ */
/*
 * The contract of mp_spmm_csr_f32 with X, S and Y as bf16 (element strides ldx, lds, ldy); val and bias stay fp32.
 * Rows are widened to fp32 as they are read (exact) and reduced, averaged and run through the epilogue in fp32 in the
 * fp32 kernel's order (entry order within a row, hub pieces in piece order); every output element is rounded once to
 * bf16, to nearest even.  So Y is bit for bit mp_spmm_csr_f32 on the widened X (and S) with the same plan, rounded to
 * bf16, and argmax is bit for bit its argmax.  Any d >= 1, ldx >= d; the workspace is mp_spmm_ws_bytes' (fp32
 * partials).  N >= 2^31: MP_ERR_UNSUPPORTED.
 */
int mp_spmm_csr_bf16(const int32_t* rowptr, const int32_t* col, const float* val,
                     int64_t N, const int32_t* plan, const int32_t* counts_host,
                     const void* X, int64_t ldx, void* Y, int64_t ldy, int32_t d,
                     int reduce, const void* S, int64_t lds, float self_scale,
                     const float* bias, int act, int32_t* argmax,
                     void* ws, size_t ws_bytes, mp_stream_t stream);
/* mp_idgnn_agg_f32 with X, P and Q as bf16: P and Q are that kernel's fp32 rows on the widened X, rounded once */
int mp_idgnn_agg_bf16(const int32_t* rowptr, const int32_t* col_marked, const float* val,
                      int64_t N, const int32_t* plan, const int32_t* counts_host,
                      const void* X, int64_t ldx, void* P, int64_t ldp,
                      void* Q, int64_t ldq, int32_t d,
                      void* ws, size_t ws_bytes, mp_stream_t stream);
/* mp_spmm_max_bwd_f32 with a bf16 dY: dX (fp32, zeroed by the caller) accumulates the widened gradients; the caller
 * rounds it once */
int mp_spmm_max_bwd_bf16(const int32_t* col, const float* val, const int32_t* argmax,
                         const void* dY, int64_t ldy, int64_t N, int32_t d,
                         float* dX, int64_t ldx, mp_stream_t stream);

/* ------------------------------------------------------------------ *
 * BatchNorm1d over the node axis in training mode with the activation  *
 * fused (K20 / SURVEY §8f rank 3): graphgym/models/layer.py:26-35,      *
 * keras BatchNormalization of main_zd.py:181-186.                       *
 *   fwd: mean / biased var over the N rows, y = act((x - mean) * invstd *
 *        * gamma + beta); var_unbiased feeds the running statistics.    *
 *   bwd: g = dy * [y > 0] (y NULL = no activation); dgamma, dbeta, dx.  *
 * Column sums are combined in double precision in a fixed order.        *
 * ------------------------------------------------------------------ */
int mp_bn_ws_bytes(int64_t N, int32_t d, size_t* bytes_host);
int mp_bn_train_fwd_f32(const float* x, int64_t ldx, int64_t N, int32_t d,
                        const float* gamma, const float* beta, float eps, int relu,
                        float* y, int64_t ldy, float* mean, float* invstd, float* var_unbiased,
                        void* ws, size_t ws_bytes, mp_stream_t stream);
int mp_bn_train_bwd_f32(const float* dy, int64_t lddy, const float* y, int64_t ldy,
                        const float* x, int64_t ldx, int64_t N, int32_t d,
                        const float* gamma, const float* mean, const float* invstd,
                        float* dx, int64_t lddx, float* dgamma, float* dbeta,
                        void* ws, size_t ws_bytes, mp_stream_t stream);
/* The backward of BatchNorm + ReLU without the forward's output: the mask [y > 0] is recomputed from x —
 * y = relu(fmaf(x - mean, float(gamma * invstd), beta)), the forward's own expression on the forward's own operands,
 * so the mask is the forward's bit for bit — and the two passes read dy and x only (50 instead of 70 GB at
 * 10^7 x 256).  gamma / beta NULL = 1 / 0. */
int mp_bn_train_bwd_relu_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t N, int32_t d,
                             const float* gamma, const float* beta, const float* mean, const float* invstd,
                             float* dx, int64_t lddx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                             mp_stream_t stream);
/* The skip block of GraphGym's skipsum / skipconcat stages (graphgym/models/gnn.py:30-60) behind a last layer without
 * activation, with the statistics and workspace of mp_bn_train_fwd_f32 and ONE apply launch:
 *   MP_BN_SKIP_SUM    (d_skip == d): out[N, d]          = act(skip + BN(x))
 *   MP_BN_SKIP_CONCAT              : out[N, d_skip + d] = [act(skip) | act(BN(x))]
 * act = ReLU when relu != 0.  BN(x) is mp_bn_train_fwd_f32's own expression: with skip == 0 (SUM), or in the right
 * slab (CONCAT), out equals its y.  A launch takes its 4-wide form when every pointer it forms is 16-byte aligned and
 * every stride a multiple of 4 (CONCAT: out + d_skip included).
 *   bwd (SUM): g = dy * [out > 0] is written to dskip by the statistics pass and read back by the apply pass (7 N d
 *   elements moved instead of 8); dx, dgamma, dbeta are mp_bn_train_bwd_f32(dy, y = out, ...)'s bits.  out NULL = no
 *   activation: d(skip) is dy itself, dskip is not written and may be NULL.
 *   bwd (CONCAT): mp_bn_train_bwd_f32 on the column views dy + d_skip, out + d_skip. */
#define MP_BN_SKIP_SUM 0
#define MP_BN_SKIP_CONCAT 1
int mp_bn_train_fwd_skip_f32(const float* x, int64_t ldx, const float* skip, int64_t ldskip, int64_t N, int32_t d,
                             int32_t d_skip, int mode, const float* gamma, const float* beta, float eps, int relu,
                             float* out, int64_t ldo, float* mean, float* invstd, float* var_unbiased, void* ws,
                             size_t ws_bytes, mp_stream_t stream);
int mp_bn_train_bwd_skip_f32(const float* dy, int64_t lddy, const float* out, int64_t ldo, const float* x, int64_t ldx,
                             int64_t N, int32_t d, const float* gamma, const float* mean, const float* invstd,
                             float* dx, int64_t lddx, float* dskip, int64_t lddskip, float* dgamma, float* dbeta,
                             void* ws, size_t ws_bytes, mp_stream_t stream);

/* The four passes above with ANY activation of GraphGym's act_dict (graphgym/models/act.py:6-14) or SiLU.  On the fp32
 * pre-activation z (the BN term, plus skip in SUM; skip itself in CONCAT's left slab):
 *   MP_ACT_NONE   z                                          MP_ACT_RELU   z > 0 ? z : 0
 *   MP_ACT_LRELU  z > 0 ? z : act_param * z                  MP_ACT_PRELU  z > 0 ? z : slope[0] * z
 *   MP_ACT_ELU    z > 0 ? z : act_param * expm1(z)           MP_ACT_SELU   scale * ELU_alpha(z), torch's two constants
 *   MP_ACT_SILU   z * sigmoid(z)
 * act_param: LRELU's negative slope / ELU's alpha (ignored otherwise).  slope: DEVICE pointer to PRELU's one fp32
 * slope (nn.PReLU()), read by the kernels and never on the host; NULL for the other kinds.
 *   fwd: the statistics and finalize launches of mp_bn_train_fwd_f32 / _skip_f32, then one apply launch; with NONE or
 *        RELU the output has those entries' bits.
 *   bwd: never reads the forward's output: z is recomputed from x, mean, invstd, gamma, beta (and skip) with the
 *        forward's own expression, as mp_bn_train_bwd_relu_f32 recomputes its mask; g = dy * act'(z), then as above.
 *        SUM: the statistics pass writes g to dskip and the apply pass reads it (7 N d); dskip NULL = not asked for,
 *        the apply pass recomputes g.  CONCAT: dskip = dy[:, :d_skip] * act'(skip) in a launch of its own.  NONE:
 *        dskip is not written (d(skip) is dy itself).
 *        PRELU: dslope[0] = sum dy * min(z, 0) over every element the slope touched (CONCAT: both slabs) — one partial
 *        per workgroup, added in double in a fixed order, no atomics; dslope NULL = not asked for.  The other kinds
 *        neither compute nor store it.
 * Unknown kind, PRELU without slope, or a skip shape that does not fit: MP_ERR_INVALID_ARG before any launch.
 * The workspace is mp_bn_act_ws_bytes' (mp_bn_ws_bytes keeps its value). */
#define MP_ACT_NONE 0
#define MP_ACT_RELU 1
#define MP_ACT_LRELU 2
#define MP_ACT_PRELU 3
#define MP_ACT_ELU 4
#define MP_ACT_SELU 5
#define MP_ACT_SILU 6
int mp_bn_act_ws_bytes(int64_t N, int32_t d, size_t* bytes_host);
int mp_bn_train_fwd_act_f32(const float* x, int64_t ldx, int64_t N, int32_t d, const float* gamma, const float* beta,
                            float eps, int act, float act_param, const float* slope, float* y, int64_t ldy,
                            float* mean, float* invstd, float* var_unbiased, void* ws, size_t ws_bytes,
                            mp_stream_t stream);
int mp_bn_train_bwd_act_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t N, int32_t d,
                            const float* gamma, const float* beta, const float* mean, const float* invstd, int act,
                            float act_param, const float* slope, float* dx, int64_t lddx, float* dgamma, float* dbeta,
                            float* dslope, void* ws, size_t ws_bytes, mp_stream_t stream);
int mp_bn_train_fwd_skip_act_f32(const float* x, int64_t ldx, const float* skip, int64_t ldskip, int64_t N, int32_t d,
                                 int32_t d_skip, int mode, const float* gamma, const float* beta, float eps, int act,
                                 float act_param, const float* slope, float* out, int64_t ldo, float* mean,
                                 float* invstd, float* var_unbiased, void* ws, size_t ws_bytes, mp_stream_t stream);
int mp_bn_train_bwd_skip_act_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* skip,
                                 int64_t ldskip, int64_t N, int32_t d, int32_t d_skip, int mode, const float* gamma,
                                 const float* beta, const float* mean, const float* invstd, int act, float act_param,
                                 const float* slope, float* dx, int64_t lddx, float* dskip, int64_t lddskip,
                                 float* dgamma, float* dbeta, float* dslope, void* ws, size_t ws_bytes,
                                 mp_stream_t stream);

/* The *_act passes with gnn.dropout between the BatchNorm and the activation (graphgym/models/layer.py:26-35; in a skip
 * block on the last layer, before the skip operand: gnn.py:49-60), through a KEYED mask m that is never stored:
 *   q = ceil(d / 4);  key = mix64((mix64(seed + G) ^ offset) + G);  h = mix64((key ^ (r * q + c / 4)) + G)
 *   m(r, c) = ((h >> 16 * (c % 4)) & 0xffff) >= T          (mix64: the splitmix64 finaliser, G = 0x9E3779B97F4A7C15)
 * a pure function of seed, offset and the LOGICAL row r and column c of the [N, d] operand x — not of addresses, leading
 * dimensions or launch geometry.  T = round(p * 65536) in [0, 65536]; kept elements are multiplied by
 * scale = float(65536 / (65536 - T)) (0 when T = 65536), dropped ones are +0.
 *   plain : y   = act(m * scale * BN(x))
 *   SUM   : out = act(skip + m * scale * BN(x))           CONCAT: out = [act(skip) | act(m * scale * BN(x))]
 *   bwd   : z and m are recomputed; g = dy * act'(z); dskip = g is NOT masked (CONCAT: the left slab never sees the
 *           mask); the gradient into the BatchNorm is m * scale * g; PRELU's dslope sums dy * min(z, 0) on the masked z.
 * MP_ACT_NONE has passes of its own here (a layer without activation still drops).  With T = 0 the forward's outputs
 * are mp_bn_train_fwd_act_f32's / _skip_act_f32's.  Everything else — arguments, dskip / dslope NULL, determinism
 * (no atomics) — is as in the *_act entries; T outside [0, 65536]: MP_ERR_INVALID_ARG.
 * The backward keeps what the scale's extra rounding and an fp32 partial sum would lose (the column sums carry their
 * low-order parts in a second slab per statistics workgroup) and, for ELU / SELU / SILU, takes the derivative at z with
 * the residue of the fp32 mean folded in (one more read of x); dx = A g + B (x - mean) + C is evaluated in double and
 * rounded once.  The workspace of the four entries is mp_bn_drop_ws_bytes': mp_bn_act_ws_bytes' layout with two partial
 * slabs per statistics workgroup, then three double vectors of d. */
int mp_bn_drop_ws_bytes(int64_t N, int32_t d, size_t* bytes_host);
int mp_bn_train_fwd_drop_act_f32(const float* x, int64_t ldx, int64_t N, int32_t d, const float* gamma,
                                 const float* beta, float eps, int act, float act_param, const float* slope, int32_t T,
                                 uint64_t seed, uint64_t offset, float* y, int64_t ldy, float* mean, float* invstd,
                                 float* var_unbiased, void* ws, size_t ws_bytes, mp_stream_t stream);
int mp_bn_train_bwd_drop_act_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, int64_t N, int32_t d,
                                 const float* gamma, const float* beta, const float* mean, const float* invstd,
                                 int act, float act_param, const float* slope, int32_t T, uint64_t seed,
                                 uint64_t offset, float* dx, int64_t lddx, float* dgamma, float* dbeta, float* dslope,
                                 void* ws, size_t ws_bytes, mp_stream_t stream);
int mp_bn_train_fwd_drop_skip_act_f32(const float* x, int64_t ldx, const float* skip, int64_t ldskip, int64_t N,
                                      int32_t d, int32_t d_skip, int mode, const float* gamma, const float* beta,
                                      float eps, int act, float act_param, const float* slope, int32_t T,
                                      uint64_t seed, uint64_t offset, float* out, int64_t ldo, float* mean,
                                      float* invstd, float* var_unbiased, void* ws, size_t ws_bytes,
                                      mp_stream_t stream);
int mp_bn_train_bwd_drop_skip_act_f32(const float* dy, int64_t lddy, const float* x, int64_t ldx, const float* skip,
                                      int64_t ldskip, int64_t N, int32_t d, int32_t d_skip, int mode,
                                      const float* gamma, const float* beta, const float* mean, const float* invstd,
                                      int act, float act_param, const float* slope, int32_t T, uint64_t seed,
                                      uint64_t offset, float* dx, int64_t lddx, float* dskip, int64_t lddskip,
                                      float* dgamma, float* dbeta, float* dslope, void* ws, size_t ws_bytes,
                                      mp_stream_t stream);
/* The mask alone over an [N, d] fp32 view: out = m * scale * x (a dropout with no BatchNorm in front of it).  Its
 * backward is the same call on dy. */
int mp_dropout_keyed_f32(const float* x, int64_t ldx, int64_t N, int32_t d, int32_t T, uint64_t seed, uint64_t offset,
                         float* out, int64_t ldo, mp_stream_t stream);

/* ------------------------------------------------------------------ *
 * Aggregate -> transform in one kernel                                *
 * ------------------------------------------------------------------ */
/* out[N, d_out] = act( (A X + self_scale * S) W + bias ): SparseAdj.matmul (sparse_adj.py:91-97) followed by
 * the layer's kernel product (gcn_id in the aggregate-first order, TfgIDLayer.py:510-523; GIN's
 * (1 + eps) x + sum -> first Linear, idconv.py:371-399, TfgIDLayer.py:447-456) without the [N, F] intermediate
 * going through HBM: a workgroup reduces a 32-row tile into LDS and multiplies it by W on the matrix cores
 * while the other workgroups of the compute unit gather.  reduce = MP_SUM | MP_MEAN (mean: rows divided by
 * their entry count, S must be NULL); stored values (val NULL = ones).
 * F must be 64, 128, 256 or 512 and d_out even (F = 512: two K halves over the same row tile, d_out <= 512;
 * MP_ERR_UNSUPPORTED otherwise: use mp_spmm_csr_f32 + mp_dense_fused_f32).  P (optional, [N, F]) receives the
 * aggregated rows (kept for the weight gradient).  defer_act (optional, [N] uint8): rows with a nonzero flag are
 * stored WITHOUT the activation (mp_id_fixup_f32 finishes them).  A sign-bit identity mark on col
 * (mp_mark_id_sources) is ignored.  No plan, no workspace, no process-wide state; bitwise reproducible.
 * W_split (optional): W split three ways into bf16 — [3][F / 8][d_out][8] bf16 (element [s][k / 8][c][k % 8] =
 * plane s of W[k][c]), plane s holding bf16(W - sum of the planes before it) — switches the product to the bf16 matrix pipe with all six significant
 * cross terms (fp32-accurate to ~2^-24 of the result; 3/8 of the MFMA cycles of the exact-fp32 form, which gfx950 runs at
 * 1/16 of the bf16 rate).  NULL = v_mfma_f32_32x32x2_f32 on W itself. */
int mp_agg_dense_f32(const int32_t* rowptr, const int32_t* col, const float* val, int64_t N, int reduce,
                     const float* X, int64_t ldx, int32_t F, const float* S, int64_t lds, float self_scale, const float* W,
                     int64_t ldw, int32_t d_out, const float* bias, int act, const uint8_t* defer_act, float* P,
                     int64_t ldp, float* out, int64_t ldo, const void* W_split, mp_stream_t stream);

/* The same with a residual added before the activation: out = act((A X + self_scale * S) W + bias + R), R [N, d_out]
 * (ldr; 8-byte aligned rows; may be `out` itself: every element is read before it is written, by the same lane).  The
 * input gradient of a concatenating layer — dx = g_self W_self^T + (A^T g_nbr) W_nbr^T (MeanGraphSage,
 * TfgIDLayer.py:100-117) — is this call with R = g_self W_self^T, instead of an extra read-read-write pass over
 * [N, d]. */
int mp_agg_dense_add_f32(const int32_t* rowptr, const int32_t* col, const float* val, int64_t N, int reduce,
                         const float* X, int64_t ldx, int32_t F, const float* S, int64_t lds, float self_scale,
                         const float* W, int64_t ldw, int32_t d_out, const float* bias, int act,
                         const uint8_t* defer_act, float* P, int64_t ldp, float* out, int64_t ldo, const void* W_split,
                         const float* R, int64_t ldr, mp_stream_t stream);

/* The aggregation ALONE on the same workgroup structure (round 3): out[N, F] = reduce_j w_ij X[j] (+ self_scale * S) —
 * SparseAdj.matmul (sparse_adj.py:91-97), the same contract as mp_spmm_csr_f32 with reduce = MP_SUM | MP_MEAN | MP_MAX
 * (max: values only, S must be NULL, rows without entries are 0; bit for bit the rows of mp_spmm_csr_f32, whose argmax
 * the backward pass uses) and no epilogue.  Four waves of a workgroup gather 64-row tiles into LDS while four others store the finished tile with
 * full-line non-temporal stores; tiles are drawn from a counter (no plan, no workspace).  F = 128, 256 or 512, 16-byte
 * aligned rows, rows of at most 2^18 stored entries (longer rows: mp_spmm_csr_f32, whose plan spreads them over many
 * waves); MP_ERR_UNSUPPORTED otherwise.  Faster than the plan-based kernel at these widths (19.6 against 20.6 ms at
 * 10^7 rows, 1.1e8 entries, F = 256).  Bitwise reproducible; a row cut between two waves of a tile is summed in wave
 * order, so results agree with mp_spmm_csr_f32 to fp32 rounding of the row sum, not bit for bit. */
int mp_agg_rows_tiles_f32(const int32_t* rowptr, const int32_t* col, const float* val, int64_t N, int reduce,
                          const float* X, int64_t ldx, int32_t F, const float* S, int64_t lds, float self_scale,
                          float* out, int64_t ldo, mp_stream_t stream);

/* mp_agg_rows_tiles_f32 with cache hints in the column indices: col_hot[e] = col[e] | 0x80000000 on the entries whose
 * source row of X should stay in the caches (the most-used columns: graph.py, CSRGraph.hot_col); those rows are
 * gathered with the default cache policy, all others non-temporal.  Same arguments, same results bit for bit. */
int mp_agg_rows_tiles_hot_f32(const int32_t* rowptr, const int32_t* col_hot, const float* val, int64_t N, int reduce,
                              const float* X, int64_t ldx, int32_t F, const float* S, int64_t lds, float self_scale,
                              float* out, int64_t ldo, mp_stream_t stream);

/* The identity branch of the ID layers on top of mp_agg_dense_f32: out = act(A (X W + S X W_id) + b)
 * (gcn_id, TfgIDLayer.py:510-523; GCNIDConvLayer.forward, idconv.py:150-177) equals
 * act((A X) W + b + A_id Z) with Z = X[id] W_id (n_id rows: a small product the caller makes) and A_id the stored
 * entries whose source is an identity node.  mp_agg_dense_f32 is run with defer_act[r] != 0 on the rows that own
 * such an entry (they are stored without the activation), then this call finishes exactly those rows:
 *   out[rows[k], :] = act(out[rows[k], :] + sum_{e in [crp[k], crp[k+1])} val[e] * Z[slot[e], :])
 * rows [n_rows] ascending row ids, crp [n_rows + 1], slot [crp[n_rows]] = row of Z, val NULL = ones. */
int mp_id_fixup_f32(const int32_t* rows, const int32_t* crp, const int32_t* slot, const float* val, int64_t n_rows,
                    const float* Z, int64_t ldz, float* out, int64_t ldo, int32_t d, int act, mp_stream_t stream);

/* The two-branch aggregation of gcn_id (TfgIDLayer.py:510-517; the contract of mp_idgnn_agg_f32: P = A X, Q = A S X
 * with S selecting the identity nodes' rows) on the tile structure of mp_agg_rows_tiles_f32:
 *   P = A X (col: plain or sign-marked indices) and, in the same pass, the rows of Q written as zeros — except the rows
 *   with id_rows[r] != 0 (the rows that own an entry from an identity node), which a small kernel launched behind the
 *   tile kernel writes as
 *   Q[rows[k], :] = sum_{e in [crp[k], crp[k+1])} val_id[e] * Z[slot[e], :]  with Z = X[id]
 *   (rows / crp / slot / val_id: as for mp_id_fixup_f32; id_rows [N] uint8 = 1 exactly on `rows`).
 * Every row of Q is written exactly once; the identity entries (1 % of the operator at 1 % identity nodes) are gathered
 * from an [n_id, F] matrix.  n_rows = 0: Q = 0.  F = 128, 256 or 512, 16-byte aligned rows; MP_ERR_UNSUPPORTED otherwise.
 * mp_id_rows_f32 is the small kernel alone (the row's old contents are not read): it writes out[rows[k], :] for the
 * n_rows listed rows; every other row of out is left untouched and is undefined in a fresh buffer. */
int mp_idgnn_agg_tiles_f32(const int32_t* rowptr, const int32_t* col, const float* val, int64_t N, const float* X,
                           int64_t ldx, int32_t F, const uint8_t* id_rows, const int32_t* rows, const int32_t* crp,
                           const int32_t* slot, const float* val_id, int64_t n_rows, const float* Z, int64_t ldz, float* P,
                           int64_t ldp, float* Q, int64_t ldq, mp_stream_t stream);
int mp_id_rows_f32(const int32_t* rows, const int32_t* crp, const int32_t* slot, const float* val, int64_t n_rows,
                   const float* Z, int64_t ldz, float* out, int64_t ldo, int32_t d, mp_stream_t stream);

/* ------------------------------------------------------------------ *
 * Dense transform after the aggregation, fused (K10 / K11 / K15):       *
 *   out = act( P @ W [+ Q @ W_id] + bias )                              *
 * P, Q [M, F] (ldp, ldq), W, W_id [F, d] row-major contiguous, bias [d] *
 * or NULL, out [M, d] (ldo).  Q == W_id == NULL gives the single        *
 * product.  fp32 on the matrix cores (v_mfma_f32_32x32x2_f32).          *
 * Replaces x @ kernel, x_id @ kernel_id, scatter-add, + bias, activation *
 * of gcn_id in its post-aggregation form (TfgIDLayer.py:510-523;        *
 * idconv.py:152-184).  Any F, d and leading dimensions; 16-byte loads  *
 * when F % 8 == 0, d % 4 == 0 and rows are 16-byte aligned.             *
 * ------------------------------------------------------------------ */
int mp_dense_fused_f32(const float* P, int64_t ldp, const float* W,
                       const float* Q, int64_t ldq, const float* W_id,
                       const float* bias, int act, float* out, int64_t ldo,
                       int64_t M, int32_t F, int32_t d, mp_stream_t stream);

/* The same transform at its hot shape, as a streaming kernel (dense_x3.hip): out = act(P @ W + bias) with
 * d = 64 / 128 / 256, F % 32 == 0 and F >= 64 (MP_ERR_UNSUPPORTED otherwise: use mp_dense_fused_f32), P and out 16-byte
 * aligned with ldp % 4 == 0 and ldo % 4 == 0 (MP_ERR_ALIGNMENT).  The Linear / kernel product of every layer (x @ kernel, TfgIDLayer.py:510-523;
 * GeneralLayer's Linear, layer.py:136-147; the GIN MLPs, idconv.py:371-399) and, with W_split made from W^T, the
 * input gradient of that product.  W_split = W three-way split into bf16 by mp_split_w_bf16x3 (the layout
 * mp_agg_dense_f32 takes); the product runs on the bf16 matrix pipe with all six significant cross terms
 * (fp32-accurate), P staged by LDS-DMA and read from HBM once. */
int mp_dense_x3_f32(const float* P, int64_t ldp, const void* W_split, const float* bias, int32_t act, float* out,
                    int64_t ldo, int64_t M, int32_t F, int32_t d, mp_stream_t stream);

/* W_split [3][K / 8][n][8] bf16 (6 K n bytes, 16-byte aligned) from fp32 weights: element [s][k / 8][c][k % 8] =
 * plane s of B[k][c], plane s = bf16(B - sum of the planes before it).  trans == 0: B = W, W [K, n] with leading
 * dimension ldw; trans != 0: B = W^T, W [n, K].  K % 8 == 0. */
int mp_split_w_bf16x3(const float* W, int64_t ldw, int32_t K, int32_t n, int32_t trans, void* W_split,
                      mp_stream_t stream);

/* weight gradient of the transform: dW [F, d] = P^T @ G with P [M, F], G [M, d] (backward of K11 under
 * loss.backward(), graphgym/train.py:24).  Split over the node axis into slabs in `ws`
 * (mp_dense_wgrad_ws_bytes), summed in a fixed order: bitwise reproducible.  Any F, d.
 * dbias (optional, [d]) receives the bias gradient sum_m G[m, :] from the same pass over G. */
int mp_dense_wgrad_ws_bytes(int64_t M, int32_t F, int32_t d, size_t* bytes_host);
int mp_dense_wgrad_f32(const float* P, int64_t ldp, const float* G, int64_t ldg, int64_t M,
                       int32_t F, int32_t d, float* dW, float* dbias, void* ws, size_t ws_bytes,
                       mp_stream_t stream);

/* The same pass with the backward of a ReLU epilogue folded in: G is masked by [Y > 0] (Y = the forward output of the
 * transform whose gradient this is) as it is read, dW = P^T (G * [Y > 0]), dbias its column sums, and GM (optional,
 * [M, d], may alias G) receives the masked gradient for the input-gradient launch that follows — the separate
 * elementwise masking pass of loss.backward() (graphgym/train.py:24) disappears. */
int mp_dense_wgrad_relu_f32(const float* P, int64_t ldp, const float* G, int64_t ldg, const float* Y, int64_t ldy,
                            float* GM, int64_t ldgm, int64_t M, int32_t F, int32_t d, float* dW, float* dbias,
                            void* ws, size_t ws_bytes, mp_stream_t stream);

/* ------------------------------------------------------------------ *
 * Loss of the training step that drives the path: softmax cross-entropy  *
 * over the labelled rows (graphgym/loss.py:53-68 masked_logits =          *
 * logits[node_label_index], mean softmax-CE; loss.py:20-37 torch path).   *
 * logits [n_rows, C]; index [n_sel] int64 selects rows of logits (NULL  *
 * = rows 0..n_sel-1); labels [n_sel] int64 in [0, C).  A label outside  *
 * [0, C) (torch's ignore_index is NOT implemented) or an index outside  *
 * [0, n_rows) is never dereferenced: that row's loss is NaN (so the mean *
 * is NaN) and it receives no gradient.                                   *
 *   rows:  row_loss[k] = logsumexp(z_i) - z_i[y_k]                        *
 *   bwd:   dlogits[i, :] (+)= (softmax(z_i) - onehot(y_k)) * gscale[0] * inv_n *
 *          (gscale: device scalar, the upstream gradient).  With an index *
 *          the caller zeroes dlogits first and rows ACCUMULATE, so a row  *
 *          listed k times gets k terms, like F.cross_entropy(logits[index]) *
 * ------------------------------------------------------------------ */
int mp_softmax_ce_rows_f32(const float* logits, int64_t ld, int64_t n_rows, const int64_t* labels,
                           const int64_t* index, int64_t n_sel, int32_t C, float* row_loss, mp_stream_t stream);
int mp_softmax_ce_bwd_f32(const float* logits, int64_t ld, int64_t n_rows, const int64_t* labels,
                          const int64_t* index, int64_t n_sel, int32_t C, const float* gscale, float inv_n,
                          float* dlogits, int64_t ldd, mp_stream_t stream);

/* ------------------------------------------------------------------ *
 * Identity-row update (K10): H[id[k], :] += U[k, :]                   *
 * replaces tf.tensor_scatter_nd_add (TfgIDLayer.py:107,165,330,515)   *
 * and x.index_add_(0, id, x_id) (idconv.py:67,155,251,310,375).       *
 * Duplicate ids accumulate (atomics); GraphGym's ids are unique.      *
 * ------------------------------------------------------------------ */
int mp_rows_gather_f32(const float* X, int64_t ldx, const int64_t* idx, int64_t n,
                       int32_t d, float* out, int64_t ldo, mp_stream_t stream);
int mp_rows_scatter_add_f32(float* H, int64_t ldh, const int64_t* idx, int64_t n,
                            int32_t d, const float* U, int64_t ldu, mp_stream_t stream);

/* ------------------------------------------------------------------ *
 * Integer-coded features (graphgym/models/feature_encoder.py:13-103;  *
 * the bond term of graphgym/contrib/layer/generalconv_ogb.py:30-35)    *
 * ------------------------------------------------------------------ */
/* out[r] = ((0 + table[off_0 + codes[r,0]]) + table[off_1 + codes[r,1]]) + ... — AtomEncoder.forward's loop
 * (feature_encoder.py:74-81) with the K tables stacked into one [C, d] operand; the additions run in that order, so
 * the result has the bits of the fp32 loop.  codes [R, K] int32 (dense), offsets [K] int32 on the DEVICE (NULL:
 * zeros), table rows unit-stride with leading dimension ldt >= d, out with ldo >= d.  The CALLER has checked every
 * code against its table's row count; the kernel does not.  K > 64: MP_ERR_UNSUPPORTED. */
int mp_embed_sum_f32(const int32_t* codes, int32_t K, const int32_t* offsets, const float* table, int64_t ldt,
                     int64_t R, int32_t d, float* out, int64_t ldo, mp_stream_t stream);
/* the largest C mp_code_reduce_f32 takes (208: 52 KiB of LDS per wave, three waves per CU) */
int mp_code_reduce_max_codes(void);
/* workspace of mp_code_reduce_f32: n_slabs * C * d floats, n_slabs = clamp(R / (16 C), 1, 1024) (also written to
 * *n_slabs when not NULL) — at most max(C d, R d / 16) floats.  C above the cap: MP_ERR_UNSUPPORTED. */
int mp_code_reduce_ws_bytes(int64_t R, int32_t C, int32_t d, int32_t* n_slabs, size_t* bytes);
/* dT[c, :] = sum over the items i with code_i = c of w_i * dY[row_i, :] — the gradient of mp_embed_sum_f32 into the
 * table, and of a table term gathered per CSR entry.  Every row of dT [C, d] is WRITTEN (a code no item carries gets
 * exactly 0).  No float atomics: a wave owns a range of rows and 64 columns, accumulates in lane-private LDS words and
 * stores one [C, 64] partial; the partials are added in index order.  The grid depends on (R, C, d) only: the same
 * bits every run.  Items of row r:
 *   rowptr NULL, sel NULL   K per row: item k has code offsets[k] + codes[r*K + k] and weight w[r*K + k]; K <= 64.
 *                           tables_disjoint != 0 promises that the K codes of a row differ (K stacked tables, each
 *                           code inside its own): K = 3 and K = 9 then update all K accumulators at once
 *   rowptr given            entries rowptr[r] .. rowptr[r+1]: code codes[i] (< 0: no term), weight w[i]; rows [nnz]
 *                           holds the row of every entry (a mean is the caller's weights w[i] / row count)
 *   sel given [R, d], lds   one item per row AND column, sel[r*lds + c] (< 0: none): code codes[item], weight w[item]
 *                           (the argmax of a max aggregation; rowptr must be NULL)
 * w NULL = ones; offsets on the DEVICE, NULL = zeros.  Codes are the caller's to check; one outside [0, C) adds
 * nothing.  C > mp_code_reduce_max_codes() or R >= 2^31: MP_ERR_UNSUPPORTED. */
int mp_code_reduce_f32(const int32_t* rowptr, const int32_t* rows, int32_t K, const int32_t* codes,
                       const int32_t* offsets, int tables_disjoint, const float* w, const int32_t* sel, int64_t lds,
                       int64_t R, int32_t C, const float* dY, int64_t ldy, int32_t d, float* dT, int64_t ldt, void* ws,
                       size_t ws_bytes, mp_stream_t stream);

/* ------------------------------------------------------------------ *
 * Attention pieces (K12, K13) for the GAT layers                      *
 * ------------------------------------------------------------------ */
/* dot-product scores: s[e*H+h] = scale * <Qm[row, h-th slice], Km[col, h-th slice]>
 * (TfgIDLayer.py:333-339); H heads split the feature axis evenly. */
int mp_sddmm_dot_f32(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz,
                     const float* Qm, int64_t ldq, const float* Km, int64_t ldk,
                     int32_t d, int32_t heads, float scale, float* s,
                     mp_stream_t stream);
/* the same scores on the entry-balanced kernel: needs row_of (mp_csr_row_ids) instead of rowptr;
 * heads > 1 needs d <= 256 and (d / heads / vector width) a power of two (MP_ERR_UNSUPPORTED
 * otherwise: use mp_sddmm_dot_f32) */
int mp_sddmm_dot_stream_f32(const int32_t* row_of, const int32_t* col, int64_t nnz,
                            const float* A, int64_t lda, const float* B, int64_t ldb,
                            int32_t d, int32_t heads, float scale, float* s, mp_stream_t stream);
/* additive scores: s[e] = leaky_relu(ai[row] + aj[col], slope) (idconv.py:319-326
 * with ai = <z, att[:d]>, aj = <z, att[d:]> precomputed per node) */
int mp_sddmm_add_f32(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz,
                     const float* ai, const float* aj, float slope, float* s,
                     mp_stream_t stream);
/* additive attention coefficients in one pass, all heads (idconv.py:319-327; torch_geometric GATConv [3P]):
 * alpha[e*H+h] = softmax over the entries e of row r of leaky_relu(a_dst[r*H+h] + a_src[col[e]*H+h], slope);
 * the scores are never stored.  a_dst, a_src [N, H]. */
int mp_gat_alpha_f32(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, int32_t heads,
                     const float* a_dst, const float* a_src, float slope, float* alpha, mp_stream_t stream);
/* the same with an edge term — the attention coefficients of the edge-feature attention layers (attconv.py:342-357),
 * whose score <linear(cat([x_i,] x_j, ef_e))^h, att_msg^h> splits into per-node and per-edge scalars:
 * alpha[e*H+h] = softmax over the entries e of row r of
 *   leaky_relu(a_dst[r*H+h] + a_src[col[e]*H+h] + a_edge[eid[e]*H+h], slope),
 * a_src [n, H], a_edge [E, H] in INPUT edge order (an entry with eid < 0 has no edge term), a_dst [N, H] or NULL (absent:
 * msg_direction 'single').  One launch for all heads on the row loop of mp_gat_alpha_f32; the scores are never stored.
 * N or nnz >= 2^31: MP_ERR_UNSUPPORTED. */
int mp_edge_att_alpha_f32(const int32_t* rowptr, const int32_t* col, const int32_t* eid, int64_t N, int64_t nnz,
                          int32_t heads, const float* a_dst, const float* a_src, const float* a_edge, float slope,
                          float* alpha, mp_stream_t stream);
/* softmax over each row's entries, per head: segment_softmax (sparse_adj.py:136-151),
 * torch_geometric.utils.softmax (idconv.py:327).  In-place allowed. */
int mp_csr_row_softmax_f32(const int32_t* rowptr, int64_t N, int32_t heads,
                           const float* s, float* out, mp_stream_t stream);
/* backward of the row softmax: ds = p * (dp - sum_row(p*dp)) */
int mp_csr_row_softmax_bwd_f32(const int32_t* rowptr, int64_t N, int32_t heads,
                               const float* p, const float* dp, float* ds,
                               mp_stream_t stream);
/* multi-head weighted aggregation on the segment plan — ALL heads in one launch of the hot kernel (full-row loads; a lane
 * applies the weight of the head its columns belong to): Y[r, slice h] = reduce_e a[e*H+h] * V[col[e], slice h] with
 * reduce MP_SUM, MP_MEAN or MP_MAX over each row's entries — the attention sum (TfgIDLayer.py:340-355 with
 * split_value_heads; idconv.py:317-332) and the attention layers' propagate with aggr = cfg.gnn.agg
 * (graphgym/contrib/layer/attconv.py:93-104 add attention, :196-205 mul attention).  The semantics of
 * mp_spmm_csr_f32: mean divides by the row's entry count, an empty row gives 0, max keeps the first entry in CSR
 * order among equal candidates and writes its index to argmax [N, d] (row stride d; NULL: not written; -1 where no
 * entry won; hub pieces are merged in piece order).  heads 1 (one weight per entry) or 2, 4, 8 with d % heads == 0;
 * other head counts return MP_ERR_UNSUPPORTED (run one launch per head on column slices of mp_spmm_csr_f32).
 * Workspace: mp_spmm_ws_bytes for this reduce (MAX adds the argmax partials of the hub pieces). */
int mp_spmm_csr_heads_reduce_f32(const int32_t* rowptr, const int32_t* col, const float* a, int64_t N,
                                 const int32_t* plan, const int32_t* counts_host, int32_t heads, int reduce,
                                 const float* V, int64_t ldv, float* Y, int64_t ldy, int32_t d, int32_t* argmax,
                                 void* ws, size_t ws_bytes, mp_stream_t stream);
/* two-gather aggregation of messages that carry an edge feature — GeneralEdgeConvLayer.message, generalconv.py:203-209:
 * linear_msg(cat(x_i, x_j, edge_feature)) = T[r] + X[col] + M[eid] with X = x W_j^T [n, d], M = edge_feature W_e^T
 * [E, d] in INPUT edge order and T = x W_i^T [N, d] (msg_direction 'both'; NULL for 'single'):
 *   Y[r] = reduce_{e in row r} val[e] * (X[col[e]] + M[eid[e]] + T[r]) (+ bias),  reduce MP_SUM / MP_MEAN / MP_MAX.
 * One pass of the plan kernel with two coalesced row loads per entry: no [nnz, d] message tensor is written or read.
 * val NULL = ones; T, bias NULL = absent; an entry with eid < 0 (an inserted self loop) has no M term (its load reads
 * row 0: M must hold at least one row, and more rows than the largest eid).  mean divides by the row's entry count, an
 * empty row gives 0 (+ bias); max keeps the first entry in CSR order among equal candidates and writes its ENTRY index
 * to argmax [N, d] (row stride d; NULL: not written; -1 where the row is empty) — the convention of mp_spmm_csr_f32, so
 * mp_spmm_max_bwd_f32 gives dX.  Rows longer than the plan's hub_deg go through the piece / finalize path.  No atomics:
 * the same bits every run.  Any d >= 1, leading dimensions >= d (MP_ERR_INVALID_ARG otherwise); N >= 2^31:
 * MP_ERR_UNSUPPORTED.  Workspace: mp_spmm_ws_bytes(counts_host, d, reduce, 0). */
int mp_spmm_csr_edge_f32(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const float* val, int64_t N,
                         const int32_t* plan, const int32_t* counts_host, const float* X, int64_t ldx, const float* M,
                         int64_t ldm, const float* T, int64_t ldt, float* Y, int64_t ldy, int32_t d, int reduce,
                         const float* bias, int32_t* argmax, void* ws, size_t ws_bytes, mp_stream_t stream);
/* backward of mp_spmm_csr_edge_f32 into M (the gradient of the messages of generalconv.py:203-209 with respect to the
 * edge term), dM [E, d] ZEROED by the caller:
 *   MP_SUM / MP_MEAN: dM[eid[e]] = val[e] (/ entry count of the row) * dY[row of e];
 *   MP_MAX:           dM[eid[e], c] = val[e] * dY[r, c] for e = argmax[r, c] >= 0 (argmax row stride d; required).
 * Entries with eid < 0 write nothing.  An entry belongs to one row and an input edge to at most one entry, so every
 * target is written at most once: plain stores, the same bits every run.  N or nnz >= 2^31: MP_ERR_UNSUPPORTED. */
int mp_spmm_edge_bwd_f32(const int32_t* rowptr, const int32_t* eid, const float* val, const int32_t* argmax, int64_t N,
                         int64_t nnz, int reduce, const float* dY, int64_t ldy, int32_t d, float* dM, int64_t ldm,
                         mp_stream_t stream);
/* mp_spmm_csr_edge_f32 with per-head weights a [nnz, H] in the place of val — the propagate of the edge-feature attention
 * layers (attconv.py:342-360) with a = norm * alpha:
 *   Y[r, slice h] = reduce_{e in row r} a[e*H+h] * (X[col[e]] + M[eid[e]] + T[r])[slice h] (+ bias).
 * Everything else as mp_spmm_csr_edge_f32: reduce MP_SUM / MP_MEAN / MP_MAX, its argmax convention, eid < 0, hub rows
 * through pieces / finalize, no atomics, the workspace.  heads 2, 4, 8 with d % heads == 0 run in one launch (a lane's
 * columns stay inside one head); heads == 1 is mp_spmm_csr_edge_f32 with val = a; other head counts return
 * MP_ERR_UNSUPPORTED (run mp_spmm_csr_edge_f32 per head on column slices). */
int mp_spmm_csr_edge_heads_f32(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const float* a, int64_t N,
                               const int32_t* plan, const int32_t* counts_host, int32_t heads, const float* X,
                               int64_t ldx, const float* M, int64_t ldm, const float* T, int64_t ldt, float* Y,
                               int64_t ldy, int32_t d, int reduce, const float* bias, int32_t* argmax, void* ws,
                               size_t ws_bytes, mp_stream_t stream);
/* backward of mp_spmm_csr_edge_heads_f32 into M, dM [E, d] ZEROED by the caller: mp_spmm_edge_bwd_f32 with the weight of
 * column c's head, dM[eid[e], c] = a[e*H + c/(d/H)] (/ entry count of the row for MP_MEAN) * dY[row of e, c]; MP_MAX
 * writes only where e == argmax[r, c].  Any heads >= 1 with d % heads == 0.  Plain stores, the same bits every run. */
int mp_spmm_edge_heads_bwd_f32(const int32_t* rowptr, const int32_t* eid, const float* a, int32_t heads,
                               const int32_t* argmax, int64_t N, int64_t nnz, int reduce, const float* dY, int64_t ldy,
                               int32_t d, float* dM, int64_t ldm, mp_stream_t stream);
/* backward of the multi-head weighted max into V: dV[col[e], c] += a[e*H + c/(d/H)] * dY[r, c] for e = argmax[r, c]
 * >= 0 (attconv.py:93-104, :196-205 with aggr 'max').  One launch for all heads; no-return float atomics, so dV
 * (zeroed by the caller) is not bitwise reproducible.  N >= 2^31: MP_ERR_UNSUPPORTED. */
int mp_spmm_heads_max_bwd_f32(const int32_t* col, const float* a, int32_t heads, const int32_t* argmax, int64_t N,
                              int32_t d, const float* dY, int64_t ldy, float* dV, int64_t ldv, mp_stream_t stream);
/* backward of the multi-head weighted max into the weights, a masked per-entry dot on the entry-balanced kernel of
 * mp_sddmm_dot_stream_f32: da[e*H+h] = sum over the columns c of head h with argmax[row_e*ldm + c] == e of
 * dY[row_e, c] * V[col_e, c].  Every da[e*H+h] is written (0 where e won nothing); no atomics, the same bits every
 * run.  row_of from mp_csr_row_ids.  Head layouts of mp_sddmm_dot_stream_f32 only (MP_ERR_UNSUPPORTED otherwise: call
 * it per head with heads = 1 on column slices of argmax, dY and V). */
int mp_spmm_heads_max_da_f32(const int32_t* row_of, const int32_t* col, int64_t nnz, const int32_t* argmax,
                             int64_t ldm, const float* dY, int64_t ldy, const float* V, int64_t ldv, int32_t d,
                             int32_t heads, float* da, mp_stream_t stream);

/* ------------------------------------------------------------------ *
 * Ego-net batcher: graphgym/models/transform.py:11-38 *
 * for a batch of centre nodes, on the device.  The base CSR must be    *
 * symmetric (the reference's graphs are undirected nx.Graph).          *
 *   new ids: centre c -> c (0..B-1); other members of ego c -> fresh    *
 *   consecutive ids in ascending original id, egos one after another    *
 *   (transform.py:24-36); radius > 4 takes the whole graph (:17-18).    *
 * Cost follows the ego nets: the work and every buffer are sized by the *
 * members and candidate neighbours of the level at hand, nothing by N   *
 * (rounds 1-3 kept B x N bitmaps).  Sizes are data, so the engine asks  *
 * the CALLER for memory through a callback (e.g. torch's caching        *
 * allocator) — scratch is handed back level by level, the four outputs  *
 * stay with the caller.  One call; SYNCHRONISES the stream (radius + 2  *
 * reads of counters).                                                   *
 * ------------------------------------------------------------------ */
enum mp_ego_tag { MP_EGO_TAG_SCRATCH = 0, MP_EGO_TAG_EDGES = 1, MP_EGO_TAG_ORIG = 2, MP_EGO_TAG_EGO_OF = 3,
                  MP_EGO_TAG_ROWPTR = 4, MP_EGO_TAG_COL = 5, MP_EGO_TAG_EID = 6 };
/* flags of mp_ego_expand.  The edge list always comes out in the engine's CSR order (rows = destinations by new id,
 * inside a row by new source id), so MP_EGO_CSR can hand back the batch's CSR itself — rowptr / col / eid as
 * mp_csr_from_coo would build them from that list, without the sort.  MP_EGO_CSR_SELF_LOOPS adds one self entry per row
 * to the CSR at its sorted place (eid = -1 - row: mp_csr_from_coo's MP_COO_ADD_SELF_LOOPS on a loop-free input; the
 * base graph must hold no explicit self loops).  Both are ignored when radius > 4. */
enum mp_ego_flags { MP_EGO_CSR = 1, MP_EGO_CSR_SELF_LOOPS = 2 };
/* device memory of `bytes` bytes, 256-byte aligned, usable on the call's stream; NULL = failure (MP_ERR_WORKSPACE) */
typedef void* (*mp_alloc_fn)(size_t bytes, int32_t tag, void* user);
/* a MP_EGO_TAG_SCRATCH block is no longer needed (work that uses it is already enqueued on the call's stream: the
 * allocator must be stream-ordered, as torch's is); may be NULL (scratch then lives until the caller drops it) */
typedef void (*mp_free_fn)(void* ptr, void* user);
typedef struct mp_ego_result {
  int64_t n_nodes;            /* nodes of the expanded graph = sum of the ego nets' sizes                       */
  int64_t n_edges;            /* directed edges (both directions of an undirected edge)                         */
  int64_t* src;               /* [n_edges] new ids; ordered by (dst, src) in the new ids.  src and dst are the two rows */
  int64_t* dst;               /* of ONE [2, n_edges] block (MP_EGO_TAG_EDGES): dst == src + n_edges                 */
  int64_t* orig;              /* [n_nodes] original id of every new node, MP_EGO_TAG_ORIG                       */
  int32_t* ego_of;            /* [n_nodes] owning centre (index into `centres`), MP_EGO_TAG_EGO_OF              */
  int32_t* rowptr;            /* MP_EGO_CSR: [n_nodes + 1], MP_EGO_TAG_ROWPTR (else NULL)                       */
  int32_t* col;               /* MP_EGO_CSR: [nnz] source ids, MP_EGO_TAG_COL                                   */
  int32_t* eid;               /* MP_EGO_CSR: [nnz] position in the edge list, -1 - row for a self entry, TAG_EID */
  int64_t nnz;                /* MP_EGO_CSR: n_edges (+ n_nodes with MP_EGO_CSR_SELF_LOOPS), else 0              */
  int64_t candidates;         /* neighbour entries pushed over all levels                                       */
  size_t scratch_peak_bytes;  /* most scratch held at once                                                      */
} mp_ego_result_t;
int mp_ego_expand(const int32_t* rowptr, const int32_t* col, int64_t N,
                  const int64_t* centres, int64_t n_centres, int32_t radius, int32_t flags,
                  mp_alloc_fn alloc, mp_free_fn release, void* user,
                  mp_ego_result_t* out, mp_stream_t stream);

/* ------------------------------------------------------------------ *
 * Edge-net batches (graphgym/models/transform.py:41-65) on the device. *
 * The base CSR (engine convention: row = destination, columns         *
 * ascending inside a row) is the disjoint union of n_graphs graphs,   *
 * graph g = nodes graph_ptr[g] .. graph_ptr[g+1] (device, int64).     *
 * Copy c (device tables) is a relabelled copy of graph copy_graph[c]  *
 * whose identity node is its local node copy_src[c]: node j of copy c *
 * gets the new id node_base[c] + j.  node_base / entry_base [C+1] are *
 * the caller's prefix sums of the copies' nodes and stored entries    *
 * (N' = node_base[C], E' = entry_base[C]); max_graph_size bounds the  *
 * nodes and the entries of any copied graph.  Every output is          *
 * preallocated and written once:                                       *
 *   edge_index [2, E'] int64: row 0 sources, row 1 destinations (PyG), *
 *     listed in the engine's CSR order (dst, src in the new ids);      *
 *   orig_node [N'] base node, copy_of_node [N'] int32,                 *
 *   orig_edge [E'] eid[base entry] (the entry's position in the base's *
 *     edge_index), or the base entry itself where eid is NULL;         *
 *   id_index [C] node_base[c] + copy_src[c];                           *
 *   flags MP_EGO_CSR (| MP_EGO_CSR_SELF_LOOPS): csr_rowptr [N'+1],      *
 *     csr_col / csr_eid [E' (+ N')] as mp_csr_from_coo builds them from *
 *     edge_index (an inserted self entry: eid = -1 - row).              *
 * `row` is the base's row of every stored entry (mp_csr_row_ids).      *
 * N' or E' (+ N') beyond int32: MP_ERR_UNSUPPORTED.  No synchronisation.*
 * ------------------------------------------------------------------ */
int mp_edge_expand(const int32_t* rowptr, const int32_t* col, const int32_t* row, const int32_t* eid,
                   int64_t N, int64_t nnz, const int64_t* graph_ptr, int64_t n_graphs,
                   const int32_t* copy_graph, const int32_t* copy_src, const int64_t* node_base,
                   const int64_t* entry_base, int64_t n_copies, int64_t n_out_nodes, int64_t n_out_edges,
                   int64_t max_graph_size, int32_t flags, int64_t* edge_index, int64_t* orig_node,
                   int32_t* copy_of_node, int64_t* orig_edge, int64_t* id_index, int32_t* csr_rowptr,
                   int32_t* csr_col, int32_t* csr_eid, mp_stream_t stream);
/* Hop distances (transform.py:68-90's nx shortest path lengths): dist[pair_pos[p]] = the number of hops of the shortest
 * path from sources[s] to pair_dst[p] (p in pair_off[s] .. pair_off[s+1], pairs grouped by source) along the rows of the
 * CSR (row u = the nodes u reaches in one hop: pass the transpose of a directed engine CSR), inside the source's graph
 * source_graph[s]; 0 for the source itself, -1 if unreachable or in another graph.  Exact at any depth.  One workgroup
 * per distinct source with its bitmaps in LDS: max_graph_nodes (largest graph that holds a source) above 65536 is
 * MP_ERR_UNSUPPORTED.  No synchronisation. */
int mp_hop_distances(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz,
                     const int64_t* graph_ptr, int64_t n_graphs, int64_t max_graph_nodes,
                     const int64_t* sources, const int32_t* source_graph, int64_t n_sources,
                     const int64_t* pair_off, const int64_t* pair_dst, const int64_t* pair_pos,
                     int64_t n_pairs, int32_t* dist, mp_stream_t stream);

/* ------------------------------------------------------------------ *
 * Link-prediction labels: the pair space of a batch and a sampler of   *
 * distinct non-edges (GraphGym's edge_negative_sampling_ratio and      *
 * resample_negative, graphgym/config.py:147-163).  The base CSR as     *
 * above (row = destination, columns ascending inside a row), no column *
 * twice in a row; graph g = nodes graph_ptr[g] .. graph_ptr[g+1]       *
 * (device, int64).  A candidate pair lies inside one graph:            *
 *   MP_PAIRS_UNDIRECTED  (r, c) with c > r: every unordered pair once; *
 *   MP_PAIRS_DIRECTED    (src = c, dst = r) with c != r.               *
 * N or nnz >= 2^31: MP_ERR_UNSUPPORTED.  Nothing is allocated, no       *
 * synchronisation.                                                     *
 * ------------------------------------------------------------------ */
enum mp_pair_mode { MP_PAIRS_UNDIRECTED = 0, MP_PAIRS_DIRECTED = 1 };
/* free_out[r] <- the number of candidate partners of row r that the row does not store (a stored diagonal entry is no
 * candidate in either mode).  flags [2] (device, zeroed by the call): flags[0] <- 1 if a row stores a column twice,
 * flags[1] <- 1 if a row stores a column outside its graph; free_out is meaningless then. */
int mp_pair_space_rows(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz,
                       const int64_t* graph_ptr, int64_t n_graphs, int32_t mode, int64_t* free_out,
                       int32_t* flags, mp_stream_t stream);
/* Draws K_g = slot_base[g+1] - slot_base[g] distinct non-edges of every graph g: sample i of graph g goes to slot
 * slot_base[g] + i of out [2, K] (global ids; row 0 = src, row 1 = dst; undirected pairs as (r, c), r < c).  prefix
 * [N+1] is the exclusive prefix sum of mp_pair_space_rows' free_out (prefix[N] = the total); C_g = prefix[graph_ptr[g+1]]
 * - prefix[graph_ptr[g]] and the caller guarantees K_g <= C_g (a slot beyond C_g receives (-1, -1)).  The non-edges of
 * a graph in (row, column) order are numbered 0 .. C_g - 1 and sample i is number perm_g(i), perm_g a keyed bijection
 * of [0, C_g) (a 6-round balanced Feistel network with cycle walking, keys from (seed, offset, g)): no rejection, no
 * repeated pair, K_g = C_g returns the whole complement, and sample i does not depend on K. */
int mp_sample_non_edges(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz,
                        const int64_t* graph_ptr, int64_t n_graphs, const int64_t* prefix,
                        const int64_t* slot_base, int64_t K, int32_t mode, uint64_t seed, uint64_t offset,
                        int64_t* out, mp_stream_t stream);

/* ------------------------------------------------------------------ *
 * Mini-batch subgraph samplers (GraphGym's train.sampler: random_node, *
 * saint_node, saint_edge, saint_rw; graphgym/loader_pyg.py:204-255):   *
 * keyed draws of a node set, the set as a bitmap of N bits, and the    *
 * induced subgraph written in the engine's CSR order from the selected *
 * rows only.  key(seed, offset, i, t) = four chained splitmix64 steps  *
 * (csrc/sample.hip states it); a bounded draw is the high 64 bits of   *
 * key * n.  Draw i depends on (seed, offset, i, t) and the graph       *
 * alone.  int32 node ids throughout; N or nnz >= 2^31:                 *
 * MP_ERR_UNSUPPORTED.  Nothing is allocated, no synchronisation.       *
 * ------------------------------------------------------------------ */
/* part[v] <- mulhi(key(seed, epoch, v, 0), num_parts) for v in [0, N): the parts of an epoch partition the nodes. */
int mp_sample_parts(int64_t N, int64_t num_parts, uint64_t seed, uint64_t epoch, int32_t* part, mp_stream_t stream);
/* out[i] <- the row that holds stored entry mulhi(key(seed, offset, i, 0), nnz), i in [0, K): a node is drawn with
 * probability proportional to its stored in-degree, with replacement.  K > 0 with nnz == 0: MP_ERR_INVALID_ARG. */
int mp_sample_entry_rows(const int32_t* rowptr, int64_t N, int64_t nnz, int64_t K, uint64_t seed, uint64_t offset,
                         int32_t* out, mp_stream_t stream);
/* K walks of walk_length steps along the rows of the CSR (row u = the nodes u moves to: pass the transpose of a
 * directed engine CSR to follow out-edges), out [K, walk_length + 1] row-major.  The root of walk i is
 * pool[mulhi(key(.., i, 0), n_pool)], or mulhi(key(.., i, 0), N) with pool == NULL; step t >= 1 moves to
 * col[rowptr[cur] + mulhi(key(.., i, t), deg(cur))]; a node with an empty row stays where it is. */
int mp_sample_walks(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, const int32_t* pool,
                    int64_t n_pool, int64_t K, int32_t walk_length, uint64_t seed, uint64_t offset, int32_t* out,
                    mp_stream_t stream);
/* bitmap [ceil(N / 32)] uint32 (bit v & 31 of word v >> 5) |= the nodes[0 .. n): an entry below 0 is skipped (no draw),
 * one at or above N is skipped and sets flags[0] (int32, device).  The caller zeroes bitmap and flags. */
int mp_bitmap_mark(const int32_t* nodes, int64_t n, int64_t N, uint32_t* bitmap, int32_t* flags, mp_stream_t stream);
/* counts[w] <- popcount(bitmap[w]).  word_rank [n_words + 1] = 0 followed by the caller's inclusive prefix sum. */
int mp_bitmap_word_counts(const uint32_t* bitmap, int64_t n_words, int32_t* counts, mp_stream_t stream);
/* orig [word_rank[n_words]] <- the set bits in ascending order: word w writes from word_rank[w] on. */
int mp_bitmap_nodes(const uint32_t* bitmap, const int32_t* word_rank, int64_t n_words, int32_t* orig, mp_stream_t stream);
/* cnt[k] <- the entries of row orig[k] of the base whose column is in the bitmap, k in [0, n_sub).  orig ascending,
 * every id in [0, N).  A row is walked by 16 lanes in chunks. */
int mp_induced_count(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, const int32_t* orig,
                     int64_t n_sub, const uint32_t* bitmap, int32_t* cnt, mp_stream_t stream);
/* The induced subgraph's entries: for row k, from rowptr_sub[k] on (rowptr_sub [n_sub + 1] = 0 followed by the inclusive
 * prefix sum of mp_induced_count's cnt), col_sub <- the new id of every member column, word_rank[c >> 5] +
 * popcount(bitmap[c >> 5] below bit c & 31), and base_entry <- the entry's position in the base CSR, in stored order:
 * col_sub ascends inside a row, equal entries keep the base's order, self and repeated entries are kept as stored. */
int mp_induced_fill(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, const int32_t* orig,
                    int64_t n_sub, const uint32_t* bitmap, const int32_t* word_rank, const int32_t* rowptr_sub,
                    int32_t* col_sub, int32_t* base_entry, mp_stream_t stream);

/* ------------------------------------------------------------------ *
 * Graph-task batches (GraphGym's dataset.task = graph: the collation   *
 * of graphgym/loader.py:247-260).  A dataset is one base CSR holding   *
 * the disjoint union of G graphs, graph g = nodes graph_ptr[g] ..      *
 * graph_ptr[g+1] (device, int64) and so entries rowptr[graph_ptr[g]]   *
 * .. rowptr[graph_ptr[g+1]].  int32 node and entry ids; any size at or *
 * above 2^31 - 1: MP_ERR_UNSUPPORTED.  Nothing is allocated, nothing   *
 * is read back, no synchronisation.                                    *
 * ------------------------------------------------------------------ */
/* The batch of the graphs ids [B] (device int32, batch order, any order, repeats allowed).  node_off / entry_off [B + 1]
 * (device int32): the exclusive prefix sums of the listed graphs' node and entry counts, computed by the caller from its
 * host mirrors of graph_ptr and of rowptr[graph_ptr]; n = node_off[B], nnz = entry_off[B].  One thread per output element,
 * one launch.  Batch node k of batch graph j (node_off[j] <= k < node_off[j+1]) is base node v = graph_ptr[ids[j]] + k -
 * node_off[j]:  rowptr_out[k] <- rowptr[v] - rowptr[graph_ptr[ids[j]]] + entry_off[j] (rowptr_out[n] <- nnz),
 * owner[k] <- j (int64) and owner32[k] <- j, orig_node[k] <- v.  Batch entry e of batch graph j is base entry s =
 * rowptr[graph_ptr[ids[j]]] + e - entry_off[j]:  col_out[e] <- col[s] - graph_ptr[ids[j]] + node_off[j], row_out[e] <-
 * the batch row that holds e, base_entry[e] <- s, edge_index [2, nnz] (int64, row-major) <- (col_out; row_out), and
 * val_out[e] <- val[s] when val_out is given (val then must be).  The owner search is an upper bound over the B + 1
 * offsets, staged in LDS up to mp_collate_stage_cap() offsets, read from global memory above.  B == 0 or n == 0: MP_OK
 * without a launch; nnz == 0 writes the node arrays only (the entry outputs may be NULL). */
int mp_collate_stage_cap(void);
int mp_collate_graphs(const int32_t* rowptr, const int32_t* col, const float* val, int64_t N, int64_t nnz_base,
                      const int64_t* graph_ptr, int64_t G, const int32_t* ids, const int32_t* node_off,
                      const int32_t* entry_off, int64_t B, int64_t n, int64_t nnz, int32_t* rowptr_out, int64_t* owner,
                      int32_t* owner32, int64_t* orig_node, int32_t* col_out, int32_t* row_out, int32_t* base_entry,
                      int64_t* edge_index, float* val_out, mp_stream_t stream);
/* first_bad[0] (device int32, set to INT32_MAX by the caller) <- the smallest stored entry whose column lies outside the
 * graph of its row (row_of from mp_csr_row_ids): an entry that joins two graphs.  nnz == 0: MP_OK without a launch. */
int mp_collate_check_entries(const int32_t* col, const int32_t* row_of, int64_t nnz, const int64_t* graph_ptr, int64_t G,
                             int32_t* first_bad, mp_stream_t stream);

/* ------------------------------------------------------------------ *
 * Structural labels and features (graphgym/models/feature_augment.py)  *
 * The engine's CSR, columns ascending inside a row.  Integer results:  *
 * bit-reproducible.  Nothing is allocated, no synchronisation.         *
 * ------------------------------------------------------------------ */
/* The integers of nx.clustering (clustering_coefficient_fun, feature_augment.py:81-82; nx.average_clustering of
 * graph_clustering_fun, :105-107) for a SYMMETRIC operator that stores no (r, c) twice: deg[u] = the entries of row u
 * with col != u, tri2[u] = the sum over the stored entries (u, v), v != u, of |{w in row u and row v : w != u, w != v}|
 * = twice the triangles through u, the t that networkx divides by d (d - 1).  Explicit self loops are skipped, as
 * networkx skips them.  tri2 is zeroed by the call (an async memset on the stream).  row_of from mp_csr_row_ids: the
 * work is shared by stored entry, so a hub row is spread over many waves.  N = 0 or nnz = 0: MP_OK without a launch. */
int mp_csr_triangles(const int32_t* rowptr, const int32_t* col, const int32_t* row_of, int64_t N, int64_t nnz,
                     int64_t* tri2, int32_t* deg, mp_stream_t stream);
/* The integers of path_len_fun (feature_augment.py:60-63: the mean of nx.shortest_path_length(G, source=x) over the
 * nodes x reaches, itself included) and of nx.average_shortest_path_length (graph_path_len_fun, :101-103): for source
 * sources[s] (global id) inside its graph source_graph[s] of graph_ptr [n_graphs + 1], dist_sum[s] = the sum of the hop
 * distances to every node it reaches and reached[s] = their number, the source (distance 0) included.  The search of
 * mp_hop_distances, one workgroup per source, bitmaps in LDS: max_graph_nodes (largest graph that holds a source) above
 * 65536 is MP_ERR_UNSUPPORTED. */
int mp_hop_sums(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz,
                const int64_t* graph_ptr, int64_t n_graphs, int64_t max_graph_nodes,
                const int64_t* sources, const int32_t* source_graph, int64_t n_sources,
                int64_t* dist_sum, int32_t* reached, mp_stream_t stream);

/* ------------------------------------------------------------------ *
 * Host-side sharding of independent units over ranks (not a device op) *
 * graphgym/loader.py:247-251 (a batch is a disjoint union of graphs),  *
 * graphgym/models/transform.py:24-36 (ego nets are disjoint): units by  *
 * descending cost, each to the least-loaded rank (LPT; ties: lower      *
 * index / lower rank).  owner_host[i] <- rank of unit i.                *
 * ------------------------------------------------------------------ */
int mp_lpt_partition_host(const int64_t* costs_host, int64_t n, int32_t world, int32_t* owner_host);

/* ------------------------------------------------------------------ *
 * Host-side synthetic graph generator (bench / tests; not a device op) *
 * Barabasi-Albert preferential attachment, m links per new node,      *
 * family of datasets/syn_graph.py:42.  Writes m*(n-m) undirected      *
 * (u > v) pairs to HOST arrays; returns the count via *n_edges_host.  *
 * ------------------------------------------------------------------ */
int mp_gen_ba_edges_host(int64_t n, int32_t m, uint64_t seed,
                         int64_t* u_host, int64_t* v_host, int64_t* n_edges_host);

/* Holme-Kim powerlaw-cluster growth (networkx.powerlaw_cluster_graph(n, m, p), datasets/syn_graph.py:42):
 * preferential attachment with probability-p triangle closing.  At most m*(n-m) pairs (u > v). */
int mp_gen_powerlaw_cluster_edges_host(int64_t n, int32_t m, double p, uint64_t seed,
                                       int64_t* u_host, int64_t* v_host, int64_t* n_edges_host);

#ifdef __cplusplus
}
#endif
#endif /* MP_ENGINE_H */
