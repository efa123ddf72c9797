// Neighbour aggregation (CSR SpMM with sum / mean / max and the ID-GNN two-branch
// form) for gfx950.  Replaces SparseAdj.matmul (sparse_adj.py:91-97) and PyG
// propagate + torch_scatter (idconv.py:89,177,235,315,371) — see mp_engine.h.
//
// Shape of the kernel:
//   * one wavefront walks one *segment*: a run of consecutive destination rows
//     whose cost (entries + row_cost per row) is ~seg_cost, found at plan time
//     by a binary search over rowptr, so waves carry equal work on power-law
//     degree distributions;
//   * the wave reads the segment's column indices 64 at a time (one coalesced
//     load), broadcasts one index per step through v_readlane into an SGPR and
//     issues a fully coalesced row load of X (64 lanes x W floats: 1 KiB per
//     instruction at d = 256), U rows in flight per wave;
//   * rows are reduced in registers by the whole wave (a segmented reduction
//     whose segment boundaries are wave-uniform scalars), each output row is
//     written exactly once with the epilogue fused: no atomics, no memset,
//     bitwise reproducible;
//   * rows longer than hub_deg are cut into pieces that separate waves reduce
//     into a small partial buffer, summed in piece order by a finalize kernel.
//
// One body serves two stored element types, chosen by the traits E: F32, and Bf16, where X, S, Y and
// Q are stored as bf16 and every reduction and epilogue step runs in fp32.  A gathered bf16 row is kept as packed
// words until it is used and then widened (a 16-bit shift, exact), so the terms, their order and every fp32 operation
// on them are those of the F32 kernel on the widened X: each bf16 output is that kernel's fp32 value rounded once
// (round to nearest even, v_cvt_pk_bf16_f32).  A lane reads W bf16 (2W bytes, up to 16 B); a 512-byte row (d = 256,
// W = 4) is half the bytes of the fp32 1 KiB row per load instruction, so Bf16 keeps twice the rows in flight per
// wave below W = 8.  The partials of the hub path are fp32 for both.
//
// What a wave gathers per stored entry is a policy of the two gather kernels (the entry sources below): XRows, the row
// X[col], or EdgeRows, the rows X[col] and M[eid] of the two-gather form (fp32).  Both walk the entries through
// MP_WALK_ENTRIES and share the launcher, the argument checks and the width choice.  SplineAggRows and SplineFoldRows
// (mp_spline.h: two weights per entry; one gather into two sums, and its adjoint) are two more sources on the same walk,
// MaxBwdRows (the backward of max as a gather over the transposed pattern: ops.deterministic()) a fifth.
#include "common.h"
#include "vecio.h"
#include "../../include/mp_spline.h"
#include "../../include/mp_maxbwd.h"
#include <limits.h>
#include <type_traits>

namespace mp {

// The stored element of X, S, Y and Q: how a gathered row is loaded (Raw: its per-lane register form) and widened to
// fp32, how S is loaded, a row stored and one element of dY widened (max backward), the widest lane vector and the
// rows in flight U per wave.
struct F32 {
  using T = float;
  template <int W> using Raw = float[W];
  static constexpr int kMaxW = 4;
  template <int W> static constexpr int kU = 8;
  static constexpr bool kExtras = true;      // the col_scale / L2 epilogue and multi-head weights
  static constexpr bool kNtFinalize = true;  // the hub finalize stores Y non-temporally
  template <int W> static __device__ __forceinline__ void load_raw(const T* p, Raw<W>& r) { load_vec<W>(p, r); }
  template <int W> static __device__ __forceinline__ void widen(const Raw<W>& r, float (&v)[W]) {
#pragma unroll
    for (int k = 0; k < W; ++k) v[k] = r[k];
  }
  template <int W> static __device__ __forceinline__ void load(const T* p, float (&v)[W]) { load_vec<W>(p, v); }
  static __device__ __forceinline__ float to_f32(T x) { return x; }
  template <int W, bool NT> static __device__ __forceinline__ void store(T* p, const float (&v)[W]) {
    if constexpr (NT) store_vec_nt<W>(p, v);
    else store_vec<W>(p, v);
  }
};

struct Bf16 {
  using T = uint16_t;
  template <int W> using Raw = uint32_t[bf16_words<W>()];
  static constexpr int kMaxW = 8;
  template <int W> static constexpr int kU = W == 8 ? 8 : 16;  // the same bytes outstanding per lane (128) at W = 8, 4
  static constexpr bool kExtras = false;
  static constexpr bool kNtFinalize = false;
  template <int W> static __device__ __forceinline__ void load_raw(const T* p, Raw<W>& r) { load_bf16_raw<W>(p, r); }
  template <int W> static __device__ __forceinline__ void widen(const Raw<W>& r, float (&v)[W]) { widen_bf16<W>(r, v); }
  template <int W> static __device__ __forceinline__ void load(const T* p, float (&v)[W]) { load_bf16<W>(p, v); }
  static __device__ __forceinline__ float to_f32(T x) { return __builtin_bit_cast(float, (uint32_t)x << 16); }
  template <int W, bool NT> static __device__ __forceinline__ void store(T* p, const float (&v)[W]) {
    store_bf16<W, NT>(p, v);
  }
};

template <class E>
struct AggArgs {
  using T = typename E::T;
  const int32_t* rowptr;
  const int32_t* col;
  const float* val;
  const int32_t* seg_row;
  int32_t n_seg;
  int32_t hub_deg;
  const T* X; int64_t ldx;
  T* Y; int64_t ldy;
  T* Q; int64_t ldq;
  const T* S; int64_t lds; float self_scale;
  const float* bias;
  const float* col_scale;   // per-column multiplier applied before bias (BatchNorm in eval mode folded)
  int32_t act;
  int32_t l2norm;           // normalise the finished row to unit L2 norm (single column tile only)
  float l2_eps;
  int32_t* argmax;
  int32_t d;
  int32_t head_width;       // NH > 1: val is [nnz, NH] and head h owns columns [h * head_width, (h + 1) * head_width)
  // hub path
  const int32_t* header;
  const int32_t* hub_row;
  const int32_t* hub_base;
  const int32_t* hub_np;
  const int32_t* piece_hub;
  const int32_t* piece_k;
  int32_t piece_edges;
  float* part;
  float* part2;
  int32_t* part_arg;
};

// Running reduction of one output row, W columns per lane.
template <class E, int W, int REDUCE, bool BRANCH2>
struct RowAcc {
  float a[W];
  float b[BRANCH2 ? W : 1];
  int arg[REDUCE == MP_MAX ? W : 1];

  __device__ __forceinline__ void reset() {
#pragma unroll
    for (int k = 0; k < W; ++k) {
      a[k] = (REDUCE == MP_MAX) ? -INFINITY : 0.f;
      if constexpr (BRANCH2) b[k] = 0.f;
      if constexpr (REDUCE == MP_MAX) arg[k] = -1;
    }
  }
  // one neighbour row r (raw, widened here) scaled by w; `marked`: source is an identity node; e: entry index
  __device__ __forceinline__ void add(const typename E::template Raw<W>& r, float w, bool marked, int e) {
    float v[W];
    E::template widen<W>(r, v);
#pragma unroll
    for (int k = 0; k < W; ++k) {
      if constexpr (REDUCE == MP_MAX) {
        float m = w * v[k];
        if (m > a[k]) { a[k] = m; arg[k] = e; }
      } else {
        a[k] = fmaf(w, v[k], a[k]);
      }
    }
    if constexpr (BRANCH2) {
      if (marked) {   // wave-uniform
#pragma unroll
        for (int k = 0; k < W; ++k) b[k] = fmaf(w, v[k], b[k]);
      }
    }
  }
};

// Epilogue + store of one finished output row (K15/K17 fused into the flush).
template <class E, int W, int REDUCE, bool BRANCH2, bool NT>
__device__ __forceinline__ void finish_row(const AggArgs<E>& a, int row, int deg,
                                           RowAcc<E, W, REDUCE, BRANCH2>& acc,
                                           int c0, int c0ld, bool lane_on) {
  float out[W];
#pragma unroll
  for (int k = 0; k < W; ++k) {
    if (REDUCE == MP_MEAN) out[k] = deg > 0 ? acc.a[k] / (float)deg : 0.f;
    else if (REDUCE == MP_MAX) out[k] = deg > 0 ? acc.a[k] : 0.f;
    else out[k] = acc.a[k];
  }
  if (a.S != nullptr) {
    float s[W];
    E::template load<W>(a.S + (int64_t)row * a.lds + c0ld, s);
#pragma unroll
    for (int k = 0; k < W; ++k) out[k] = fmaf(a.self_scale, s[k], out[k]);
  }
  if (E::kExtras && a.col_scale != nullptr) {
    float sv[W];
    load_f32<W>(a.col_scale + c0ld, sv);
#pragma unroll
    for (int k = 0; k < W; ++k) out[k] *= sv[k];
  }
  if (a.bias != nullptr) {
    float bv[W];
    load_f32<W>(a.bias + c0ld, bv);
#pragma unroll
    for (int k = 0; k < W; ++k) out[k] += bv[k];
  }
  if (a.act == MP_ACT_RELU) {
#pragma unroll
    for (int k = 0; k < W; ++k) out[k] = fmaxf(out[k], 0.f);
  }
  if (E::kExtras && a.l2norm) {
    // F.normalize(p=2, dim=-1) (layer.py:43-46, gnn.py:79-80): the wave holds the whole row
    float ss = 0.f;
    if (lane_on) {
#pragma unroll
      for (int k = 0; k < W; ++k) ss = fmaf(out[k], out[k], ss);
    }
    for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, kWave);
    const float inv = 1.0f / fmaxf(sqrtf(ss), a.l2_eps);
#pragma unroll
    for (int k = 0; k < W; ++k) out[k] *= inv;
  }
  if (lane_on) {
    E::template store<W, NT>(a.Y + (int64_t)row * a.ldy + c0, out);
    if constexpr (BRANCH2) E::template store<W, false>(a.Q + (int64_t)row * a.ldq + c0, acc.b);
    if constexpr (REDUCE == MP_MAX) {
      if (a.argmax != nullptr) store_i32<W>(a.argmax + (int64_t)row * a.d + c0, acc.arg);
    }
  }
  acc.reset();
}

// ---- entry sources: what a wave gathers for one stored entry, and how that becomes the entry's fp32 message ---------
// A source holds the wave's side of the gather: the lane's operand pointers and its index words of the current 64
// entries.  issue() broadcasts entry j's indices to the scalar unit and issues its row loads into a Rows, returning
// the index word that consume() needs; consume() turns the two into the message and adds it to the row.  Rows keeps
// the loaded rows in their raw per-lane form (bf16: packed words, widened in consume — see the file header): U entries
// are issued before the first is consumed.  start_row() is called when the wave begins a destination row.

// One gather: the message is X[col].  Under BRANCH2 col carries the identity mark in its sign bit.
template <class E_, int W>
struct XRows {
  using E = E_;
  using Args = AggArgs<E>;
  static constexpr int kW = W;
  static constexpr bool kMarks = true;   // the two-branch form exists
  using Rows = typename E::template Raw<W>;
  static __host__ __device__ __forceinline__ const AggArgs<E>& agg(const Args& g) { return g; }

  const Args& g;
  const typename E::T* xlane;
  int cv;

  __device__ __forceinline__ XRows(const Args& g_, int c0ld) : g(g_), xlane(g_.X + c0ld) {}
  __device__ __forceinline__ void start_row(int) {}
  __device__ __forceinline__ void load_index(int me) { cv = g.col[me]; }
  template <bool BRANCH2>
  __device__ __forceinline__ void issue(int j, Rows& x, int& cj) const {
    cj = bcast_i(cv, j);
    const int c = BRANCH2 ? (cj & 0x7fffffff) : cj;
    E::template load_raw<W>(xlane + (int64_t)c * g.ldx, x);
  }
  template <int REDUCE, bool BRANCH2>
  __device__ __forceinline__ void consume(const Rows& x, int cj, float w, int e,
                                          RowAcc<E, W, REDUCE, BRANCH2>& acc) const {
    acc.add(x, w, BRANCH2 && cj < 0, e);
  }
};

// ---- two-gather aggregation: messages that carry an edge feature (generalconv.py:203-209) ---------------------------
// y[r] = reduce_e val_e * (X[col_e] + M[eid_e] + T[r]) (+ bias): X = x W_j^T by source, M = edge_feature W_e^T by input
// edge, T = x W_i^T by destination (msg_direction 'both').  The same kernels on a source with a second gathered operand:
// the wave reads 64 col and 64 eid words with one coalesced load each, broadcasts an entry's pair to the scalar unit and
// issues two coalesced row loads for it, U entries = 2U row loads in flight.  No per-entry tensor of width d is written or
// read.  An inserted self loop (eid < 0) has no M term: its load reads row 0 of M (M holds at least one row) and is
// dropped, so every entry issues the same two loads and the waits stay counted.  T[r] is loaded once when row r starts;
// on the hub path T[row] is inside every term of a piece, so the partials need no fix-up.  fp32, no marks.  Under NH > 1
// (edge-feature attention, attconv.py:342-360) the entry's NH weights meet the summed message exactly as they meet X[col]
// in the one-gather form: the walk hands consume() the weight of the lane's head.
struct EdgeOperands {
  const int32_t* eid;
  const float* M; int64_t ldm;
  const float* T; int64_t ldt;
};

struct EdgeArgs {
  AggArgs<F32> a;
  EdgeOperands o;
};

template <int W, bool HAS_T>
__device__ __forceinline__ void edge_message(const float (&x)[W], const float (&m)[W], bool has_m,
                                             const float (&t)[W], float (&v)[W]) {
#pragma unroll
  for (int k = 0; k < W; ++k) {
    v[k] = x[k] + (has_m ? m[k] : 0.f);
    if constexpr (HAS_T) v[k] += t[k];
  }
}

template <int W, bool HAS_T>
struct EdgeRows {
  using E = F32;
  using Args = EdgeArgs;
  static constexpr int kW = W;
  static constexpr bool kMarks = false;
  struct Rows { float x[W], m[W]; };
  static __host__ __device__ __forceinline__ const AggArgs<F32>& agg(const Args& g) { return g.a; }

  const Args& g;
  const float* xlane;
  const float* mlane;
  int c0ld;
  int cv, ev;
  float t[W];

  __device__ __forceinline__ EdgeRows(const Args& g_, int c0ld_)
      : g(g_), xlane(g_.a.X + c0ld_), mlane(g_.o.M + c0ld_), c0ld(c0ld_) {
#pragma unroll
    for (int k = 0; k < W; ++k) t[k] = 0.f;
  }
  __device__ __forceinline__ void start_row(int r) {
    if constexpr (HAS_T) load_vec<W>(g.o.T + (int64_t)r * g.o.ldt + c0ld, t);
  }
  __device__ __forceinline__ void load_index(int me) { cv = g.a.col[me]; ev = g.o.eid[me]; }
  template <bool BRANCH2>
  __device__ __forceinline__ void issue(int j, Rows& xm, int& ej) const {
    static_assert(!BRANCH2, "the two-gather form has no second branch");
    const int c = bcast_i(cv, j);
    ej = bcast_i(ev, j);
    load_vec<W>(xlane + (int64_t)c * g.a.ldx, xm.x);
    load_vec<W>(mlane + (int64_t)max(ej, 0) * g.o.ldm, xm.m);
  }
  template <int REDUCE>
  __device__ __forceinline__ void consume(const Rows& xm, int ej, float w, int e,
                                          RowAcc<F32, W, REDUCE, false>& acc) const {
    float v[W];
    edge_message<W, HAS_T>(xm.x, xm.m, ej >= 0, t, v);
    acc.add(v, w, false, e);
  }
};

// ---- one gather, two sums: messages weighted by an open degree-1 B-spline with two kernel matrices (layer.py:177-186) -
// Every entry carries two weights w[e] = (w0, w1) of its own, in ENTRY order (mp_spline.h).  The two kernels are each
// other's adjoint on the transposed pattern:
//   SplineAggRows   P[r] = sum_e w0 X[col_e], Q[r] = sum_e w1 X[col_e]: one row load per entry, two running sums per row
//                   (RowAcc::b, as the ID-GNN form keeps them).  The caller binds P and Q = P + d to the two halves of one
//                   [N, 2d] row, so finish_row and the hub path store them as they store any P and Q.
//   SplineFoldRows  Y[r] = sum_e (w0 Z[col_e, 0:d] + w1 Z[col_e, d:2d]): two row loads from one index, one sum.
// The walk's own weight word is unused (WEIGHTED = false): a lane loads its entry's two weights beside its index word
// and issue() broadcasts them with the index, so they travel in Rows to consume() as the index word does.  fp32, no marks.
struct SplineArgs {
  AggArgs<F32> a;
  const float* w2;   // [nnz, 2]
};

template <int W>
struct SplineAggRows {
  using E = F32;
  using Args = SplineArgs;
  static constexpr int kW = W;
  static constexpr bool kMarks = false;
  struct Rows { float x[W]; float w0, w1; };
  static __host__ __device__ __forceinline__ const AggArgs<F32>& agg(const Args& g) { return g.a; }

  const Args& g;
  const float* xlane;
  int cv;
  float w0v, w1v;

  __device__ __forceinline__ SplineAggRows(const Args& g_, int c0ld) : g(g_), xlane(g_.a.X + c0ld) {}
  __device__ __forceinline__ void start_row(int) {}
  __device__ __forceinline__ void load_index(int me) {
    cv = g.a.col[me];
    w0v = g.w2[2 * (int64_t)me];
    w1v = g.w2[2 * (int64_t)me + 1];
  }
  template <bool BRANCH2>
  __device__ __forceinline__ void issue(int j, Rows& r, int& cj) const {
    static_assert(BRANCH2, "the two sums are the two branches");
    cj = bcast_i(cv, j);
    r.w0 = bcast_f(w0v, j);
    r.w1 = bcast_f(w1v, j);
    load_vec<W>(xlane + (int64_t)cj * g.a.ldx, r.x);
  }
  template <int REDUCE>
  __device__ __forceinline__ void consume(const Rows& r, int, float, int, RowAcc<F32, W, REDUCE, true>& acc) const {
#pragma unroll
    for (int k = 0; k < W; ++k) {
      acc.a[k] = fmaf(r.w0, r.x[k], acc.a[k]);
      acc.b[k] = fmaf(r.w1, r.x[k], acc.b[k]);
    }
  }
};

template <int W>
struct SplineFoldRows {
  using E = F32;
  using Args = SplineArgs;
  static constexpr int kW = W;
  static constexpr bool kMarks = false;
  struct Rows { float a[W], b[W]; float w0, w1; };
  static __host__ __device__ __forceinline__ const AggArgs<F32>& agg(const Args& g) { return g.a; }

  const Args& g;
  const float* alane;
  const float* blane;
  int cv;
  float w0v, w1v;

  __device__ __forceinline__ SplineFoldRows(const Args& g_, int c0ld)
      : g(g_), alane(g_.a.X + c0ld), blane(g_.a.X + g_.a.d + c0ld) {}
  __device__ __forceinline__ void start_row(int) {}
  __device__ __forceinline__ void load_index(int me) {
    cv = g.a.col[me];
    w0v = g.w2[2 * (int64_t)me];
    w1v = g.w2[2 * (int64_t)me + 1];
  }
  template <bool BRANCH2>
  __device__ __forceinline__ void issue(int j, Rows& r, int& cj) const {
    static_assert(!BRANCH2, "the fold has one sum");
    cj = bcast_i(cv, j);
    r.w0 = bcast_f(w0v, j);
    r.w1 = bcast_f(w1v, j);
    load_vec<W>(alane + (int64_t)cj * g.a.ldx, r.a);
    load_vec<W>(blane + (int64_t)cj * g.a.ldx, r.b);
  }
  template <int REDUCE>
  __device__ __forceinline__ void consume(const Rows& r, int, float w, int e, RowAcc<F32, W, REDUCE, false>& acc) const {
    float v[W];
#pragma unroll
    for (int k = 0; k < W; ++k) v[k] = fmaf(r.w1, r.b[k], r.w0 * r.a[k]);
    acc.add(v, w, false, e);
  }
};

// ---- two gathers, one masked sum: the backward of max in pull form ---------------------------------
// The walk runs over the TRANSPOSED pattern: a row is a source j, an entry t of it is one forward entry e = pos[t] of
// destination i = col[t], and
//   dX[j, c] = sum over row j's entries t, in their stored order, of [argmax[i_t, c] == pos_t] * w_t * dY[i_t, c]
// with w the forward weights permuted into the transposed order (the walk's own weight word: val [nnz], or [nnz, NH]
// for the heads form).  A lane loads its entry's (col, pos) pair; issue() broadcasts the pair and issues the row loads
// of argmax[i] (int32) and dY[i]; consume() turns the match mask into the message.  Both loads are issued for every
// entry, whatever the argmax row says: the dY load would otherwise depend on the argmax load's return (two round trips
// in a row per entry), and a per-lane predicate on it saves no traffic at all — a 128-byte line of dY is fetched when
// any of its 32 columns matched.  An empty destination row has argmax = -1, which equals no pos: no branch.  E = Bf16
// reads a bf16 dY, sums in fp32 and stores a bf16 dX rounded once.  No marks, no second branch, sum only.
template <class E>
struct MaxBwdArgs {
  AggArgs<E> a;              // the transposed pattern; X = dY (rows by destination), Y = dX (rows by source)
  const int32_t* pos;        // [nnz] forward entry of every transposed entry
  const int32_t* argmax;     // [N_dst, >= d] winning forward entry per destination and column, -1: none
  int64_t lda;
};

template <class E_, int W>
struct MaxBwdRows {
  using E = E_;
  using Args = MaxBwdArgs<E>;
  static constexpr int kW = W;
  static constexpr bool kMarks = false;
  struct Rows { typename E::template Raw<W> g; int am[W]; };
  static __host__ __device__ __forceinline__ const AggArgs<E>& agg(const Args& g) { return g.a; }

  const Args& g;
  const typename E::T* glane;
  const int32_t* alane;
  int cv, pv;

  __device__ __forceinline__ MaxBwdRows(const Args& g_, int c0ld)
      : g(g_), glane(g_.a.X + c0ld), alane(g_.argmax + c0ld) {}
  __device__ __forceinline__ void start_row(int) {}
  __device__ __forceinline__ void load_index(int me) { cv = g.a.col[me]; pv = g.pos[me]; }
  template <bool BRANCH2>
  __device__ __forceinline__ void issue(int j, Rows& r, int& pj) const {
    static_assert(!BRANCH2, "the pull form has one sum");
    const int i = bcast_i(cv, j);
    pj = bcast_i(pv, j);
    E::template load_raw<W>(glane + (int64_t)i * g.a.ldx, r.g);
    load_i32<W>(alane + (int64_t)i * g.lda, r.am);
  }
  template <int REDUCE>
  __device__ __forceinline__ void consume(const Rows& r, int pj, float w, int, RowAcc<E, W, REDUCE, false>& acc) const {
    static_assert(REDUCE == MP_SUM, "the pull form is a sum");
    float v[W];
    E::template widen<W>(r.g, v);
#pragma unroll
    for (int k = 0; k < W; ++k) acc.a[k] = fmaf(w, r.am[k] == pj ? v[k] : 0.f, acc.a[k]);
  }
};

// The entry walk of every gather kernel: entries [e0, e1) of one wave, 64 at a time.  The wave loads the lanes' index
// and weight words, then per U entries issues all of their row loads before it consumes them in order; BEFORE runs
// ahead of entry e's consume (the rows kernel closes finished rows there).  NH > 1: the lane takes the weight of head myh.
// A macro, expanded in the scope of both kernels (src, a, acc, e0, e1, lane, myh), not a function template: behind a
// function boundary the compiler orders the loads and allocates registers differently, at the cost of a wave of
// occupancy in some hub-piece kernels (profiles/r08_spmm_unify.md).
#define MP_WALK_ENTRIES(...)                                                                    \
  for (int ec = e0; ec < e1; ec += kWave) {                                                        \
    const int me = min(ec + lane, e1 - 1);                                                         \
    src.load_index(me);                                                                            \
    float wv[NH];                                                                                  \
    _Pragma("unroll") for (int h = 0; h < NH; ++h) wv[h] = WEIGHTED ? a.val[(int64_t)me * NH + h] : 1.f; \
    const int n = min(kWave, e1 - ec);                                                             \
    for (int jb = 0; jb < n; jb += U) {                                                            \
      typename S::Rows rows[U];                                                                    \
      int ix[U]; /* two arrays: one struct of both changes the order of the generated loads */     \
      _Pragma("unroll") for (int j = 0; j < U; ++j) src.template issue<BRANCH2>(jb + j, rows[j], ix[j]); \
      _Pragma("unroll") for (int j = 0; j < U; ++j) {                                              \
        const int e = ec + jb + j;                                                                 \
        if (e < e1) {                                                                              \
          __VA_ARGS__;                                                                             \
          float w = WEIGHTED ? bcast_f(wv[0], jb + j) : 1.f;                                       \
          _Pragma("unroll") for (int h = 1; h < NH; ++h) {                                         \
            const float wh = bcast_f(wv[h], jb + j);                                               \
            w = myh == h ? wh : w;                                                                 \
          }                                                                                        \
          src.consume(rows[j], ix[j], w, e, acc);                                                  \
        }                                                                                          \
      }                                                                                            \
    }                                                                                              \
  }

// Main kernel: one wave per segment of whole rows.  Kept from the round-1 variant study: U = 8 rows
// in flight (fp32; Bf16::kU for bf16), non-temporal stores of Y (-1.2 %); non-temporal index loads, index prefetch
// and an LDS-staged index tile measured within 0.3 % and are not built.
// NH > 1 (multi-head attention, TfgIDLayer.py:333-355): every entry carries NH weights (val [nnz, NH]); a lane applies
// the weight of the head its columns belong to, so all heads aggregate in one launch on full 1 KiB row loads.
template <class S, int REDUCE, bool WEIGHTED, bool BRANCH2, int U, int NH = 1>
__global__ __launch_bounds__(kBlock) void agg_rows_kernel(typename S::Args g) {
  using E = typename S::E;
  constexpr int W = S::kW;
  const AggArgs<E>& a = S::agg(g);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int seg = blockIdx.x * kWavesPerBlock + wave;
  if (seg >= a.n_seg) return;
  const int c0 = (blockIdx.y * kWave + lane) * W;
  const bool lane_on = c0 < a.d;
  const int c0ld = lane_on ? c0 : 0;  // idle lanes re-read column 0, never store

  const int r0 = a.seg_row[seg];
  int r1 = a.seg_row[seg + 1];
  if (r0 >= r1) return;
  const int e0 = a.rowptr[r0];
  int e1 = a.rowptr[r1];
  {
    // a hub row can only be the last row that starts in a segment; the hub path owns it
    const int last_start = a.rowptr[r1 - 1];
    if (e1 - last_start > a.hub_deg) { r1 -= 1; e1 = last_start; }
  }
  if (r0 >= r1) return;

  S src(g, c0ld);
  const int myh = NH > 1 ? c0ld / a.head_width : 0;

  // row ends of up to 64 rows live in one VGPR; the current one is broadcast to an SGPR
  int rbase = r0;
  int rendv = (rbase + lane < r1) ? a.rowptr[rbase + 1 + lane] : INT_MAX;
  int r = r0;
  int rstart = e0;
  int rend = bcast_i(rendv, 0);

  RowAcc<E, W, REDUCE, BRANCH2> acc;
  acc.reset();
  src.start_row(r);

  auto advance = [&]() {   // move to the next row
    r += 1;
    rstart = rend;
    if (r - rbase == kWave) {
      rbase = r;
      rendv = (rbase + lane < r1) ? a.rowptr[rbase + 1 + lane] : INT_MAX;
    }
    rend = (r < r1) ? bcast_i(rendv, r - rbase) : INT_MAX;
    if (r < r1) src.start_row(r);
  };

  MP_WALK_ENTRIES(while (e >= rend) {
    finish_row<E, W, REDUCE, BRANCH2, true>(a, r, rend - rstart, acc, c0, c0ld, lane_on);
    advance();
  })
  while (r < r1) {
    finish_row<E, W, REDUCE, BRANCH2, true>(a, r, rend - rstart, acc, c0, c0ld, lane_on);
    advance();
  }
}

// Hub path 1/2: one wave reduces one piece (<= piece_edges entries) of a hub row.
template <class S, int REDUCE, bool WEIGHTED, bool BRANCH2, int U, int NH = 1>
__global__ __launch_bounds__(kBlock) void agg_hub_pieces_kernel(typename S::Args g) {
  using E = typename S::E;
  constexpr int W = S::kW;
  const AggArgs<E>& a = S::agg(g);
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int c0 = (blockIdx.y * kWave + lane) * W;
  const bool lane_on = c0 < a.d;
  const int c0ld = lane_on ? c0 : 0;
  S src(g, c0ld);
  const int myh = NH > 1 ? c0ld / a.head_width : 0;
  const int n_piece = a.header[PW_NPIECE];

  for (int p = blockIdx.x * kWavesPerBlock + wave; p < n_piece; p += gridDim.x * kWavesPerBlock) {
    const int h = a.piece_hub[p];
    const int k = a.piece_k[p];
    const int row = a.hub_row[h];
    const int rs = a.rowptr[row];
    const int re = a.rowptr[row + 1];
    const int e0 = rs + k * a.piece_edges;
    const int e1 = min(e0 + a.piece_edges, re);

    src.start_row(row);
    RowAcc<E, W, REDUCE, BRANCH2> acc;
    acc.reset();
    MP_WALK_ENTRIES((void)0)
    if (lane_on) {
      store_f32<W>(a.part + (int64_t)p * a.d + c0, acc.a);
      if constexpr (BRANCH2) store_f32<W>(a.part2 + (int64_t)p * a.d + c0, acc.b);
      if constexpr (REDUCE == MP_MAX) store_i32<W>(a.part_arg + (int64_t)p * a.d + c0, acc.arg);
    }
  }
}

// Hub path 2/2: combine a hub row's pieces in piece order, run the epilogue, store.
template <class E, int W, int REDUCE, bool BRANCH2>
__global__ __launch_bounds__(kBlock) void agg_hub_finalize_kernel(AggArgs<E> a) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int c0 = (blockIdx.y * kWave + lane) * W;
  const bool lane_on = c0 < a.d;
  const int c0ld = lane_on ? c0 : 0;
  const int n_hub = a.header[PW_NHUB];

  for (int h = blockIdx.x * kWavesPerBlock + wave; h < n_hub; h += gridDim.x * kWavesPerBlock) {
    const int row = a.hub_row[h];
    const int base = a.hub_base[h];
    const int np = a.hub_np[h];
    const int deg = a.rowptr[row + 1] - a.rowptr[row];
    RowAcc<E, W, REDUCE, BRANCH2> acc;
    acc.reset();
    for (int p = base; p < base + np; ++p) {
      float v[W];
      load_f32<W>(a.part + (int64_t)p * a.d + c0ld, v);
      if constexpr (REDUCE == MP_MAX) {
        int ai[W];
        load_i32<W>(a.part_arg + (int64_t)p * a.d + c0ld, ai);
#pragma unroll
        for (int k = 0; k < W; ++k)
          if (v[k] > acc.a[k]) { acc.a[k] = v[k]; acc.arg[k] = ai[k]; }
      } else {
#pragma unroll
        for (int k = 0; k < W; ++k) acc.a[k] += v[k];
      }
      if constexpr (BRANCH2) {
        float v2[W];
        load_f32<W>(a.part2 + (int64_t)p * a.d + c0ld, v2);
#pragma unroll
        for (int k = 0; k < W; ++k) acc.b[k] += v2[k];
      }
    }
    finish_row<E, W, REDUCE, BRANCH2, E::kNtFinalize>(a, row, deg, acc, c0, c0ld, lane_on);
  }
}

// The head c / hw of a lane's column c = lane, lane + 64, ...: one division per thread, then a step of 64 columns is
// 64 / hw heads and 64 % hw columns further, with at most one carry (both remainders are below hw).
struct HeadOfColumn {
  int h, rem, dh, drem, hw;
  __device__ __forceinline__ HeadOfColumn(int lane, int hw_)
      : h(lane / hw_), rem(lane % hw_), dh(kWave / hw_), drem(kWave % hw_), hw(hw_) {}
  __device__ __forceinline__ void step() {
    h += dh;
    rem += drem;
    if (rem >= hw) { rem -= hw; h += 1; }
  }
};

// Backward of the two-gather form into M, sum / mean: dM[eid_e] = val_e (/ deg) * dY[row_e].  One wave per 64 stored
// entries (balanced whatever the degrees): the row of the first entry by a binary search over rowptr, later rows by
// walking it; every entry writes one whole row of dM, an input edge belongs to at most one entry — plain stores.
// HEADS: val is [nnz, heads] and column c takes the weight of its head c / hw (mp_spmm_edge_heads_bwd_f32).
template <bool HEADS>
__global__ __launch_bounds__(kBlock) void edge_bwd_rows_kernel(const int32_t* __restrict__ rowptr,
                                                               const int32_t* __restrict__ eid,
                                                               const float* __restrict__ val, int32_t heads, int32_t hw,
                                                               int32_t N, int32_t nnz,
                                                               int mean, const float* __restrict__ dY, int64_t ldy,
                                                               int32_t d, float* __restrict__ dM, int64_t ldm) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t n_chunk = ((int64_t)nnz + kWave - 1) / kWave;
  const HeadOfColumn hc(lane, HEADS ? hw : 1);
  for (int64_t ch = (int64_t)blockIdx.x * kWavesPerBlock + wave; ch < n_chunk; ch += (int64_t)gridDim.x * kWavesPerBlock) {
    const int ec = (int)(ch * kWave);
    const int n = min(kWave, nnz - ec);
    const int me = min(ec + lane, nnz - 1);
    const int ev = eid[me];
    const float wv = (!HEADS && val) ? val[me] : 1.f;
    int lo = 0, hi = N;                    // the row r with rowptr[r] <= ec < rowptr[r + 1]
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (rowptr[mid + 1] <= ec) lo = mid + 1; else hi = mid;
    }
    int r = lo;
    int rend = rowptr[r + 1];
    for (int j = 0; j < n; ++j) {
      const int e = ec + j;
      while (e >= rend) { r += 1; rend = rowptr[r + 1]; }
      const int ei = bcast_i(ev, j);
      if (ei < 0) continue;
      const float* __restrict__ g = dY + (int64_t)r * ldy;
      float* __restrict__ o = dM + (int64_t)ei * ldm;
      if constexpr (HEADS) {
        const float cnt = (float)(rend - rowptr[r]);
        const float* __restrict__ wh = val + (int64_t)e * heads;
        HeadOfColumn k = hc;
        for (int c = lane; c < d; c += kWave, k.step()) {
          float w = wh[k.h];
          if (mean) w /= cnt;
          o[c] = w * g[c];
        }
      } else {
        float w = bcast_f(wv, j);
        if (mean) w /= (float)(rend - rowptr[r]);
        for (int c = lane; c < d; c += kWave) o[c] = w * g[c];
      }
    }
  }
}

// ... max: dM[eid[e], c] = val[e] * dY[r, c] for e = argmax[r, c] >= 0.  One wave per output row, lanes across columns;
// a column of a row has one winner and an input edge one entry, so every target is written at most once.  HEADS: as above.
template <bool HEADS>
__global__ __launch_bounds__(kBlock) void edge_bwd_max_kernel(const int32_t* __restrict__ eid,
                                                              const float* __restrict__ val, int32_t heads, int32_t hw,
                                                              const int32_t* __restrict__ argmax, int64_t N,
                                                              const float* __restrict__ dY, int64_t ldy, int32_t d,
                                                              float* __restrict__ dM, int64_t ldm) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const HeadOfColumn hc(lane, HEADS ? hw : 1);
  for (int64_t r = (int64_t)blockIdx.x * kWavesPerBlock + wave; r < N; r += (int64_t)gridDim.x * kWavesPerBlock) {
    HeadOfColumn k = hc;
    for (int c = lane; c < d; c += kWave, k.step()) {
      const int e = argmax[r * d + c];
      if (e < 0) continue;
      const int ei = eid[e];
      if (ei < 0) continue;
      float w;
      if constexpr (HEADS) w = val[(int64_t)e * heads + k.h];
      else w = val ? val[e] : 1.f;
      dM[(int64_t)ei * ldm + c] = w * dY[r * ldy + c];
    }
  }
}

// ---- plan ---------------------------------------------------------------

// The segmentation's tunables travel with the plan (its header words and counts_host carry them): a segment is a
// run of whole rows of cost ~seg_cost (1 per stored entry + row_cost per row); rows with more than hub_deg entries
// are split into pieces of piece_edges.
static const PlanCfg kDefaultCfg = {320, 4, 1024, 256};

static int cfg_from(const int32_t* cfg_host, PlanCfg* c) {
  if (!cfg_host) { *c = kDefaultCfg; return MP_OK; }
  PlanCfg v = {cfg_host[0], cfg_host[1], cfg_host[2], cfg_host[3]};
  if (v.seg_cost < 64 || v.row_cost < 0 || v.hub_deg < v.seg_cost || v.piece_edges < 64) return MP_ERR_INVALID_ARG;
  *c = v;
  return MP_OK;
}

static int32_t n_seg_of(int64_t N, int64_t nnz, const PlanCfg& c) {
  int64_t total = nnz + (int64_t)c.row_cost * N;
  int64_t s = ceil_div(total, c.seg_cost);
  return (int32_t)(s < 1 ? 1 : s);
}

static size_t plan_words(int64_t N, int64_t nnz, const PlanCfg& c) {
  int64_t n_seg = n_seg_of(N, nnz, c);
  int64_t cap_hub = nnz / c.hub_deg + 1;
  int64_t cap_piece = nnz / c.piece_edges + cap_hub + 1;
  return (size_t)(PW_HEADER_WORDS + (n_seg + 1) + 3 * cap_hub + 2 * cap_piece);
}

static PlanView plan_view(const int32_t* plan, int64_t N, int64_t nnz, const PlanCfg& c) {
  PlanView v;
  v.n_seg = n_seg_of(N, nnz, c);
  v.cap_hub = (int32_t)(nnz / c.hub_deg + 1);
  v.cap_piece = (int32_t)(nnz / c.piece_edges + v.cap_hub + 1);
  v.header = plan;
  v.seg_row = plan + PW_HEADER_WORDS;
  v.hub_row = v.seg_row + (v.n_seg + 1);
  v.hub_base = v.hub_row + v.cap_hub;
  v.hub_np = v.hub_base + v.cap_hub;
  v.piece_hub = v.hub_np + v.cap_hub;
  v.piece_k = v.piece_hub + v.cap_piece;
  return v;
}

__global__ void plan_header_kernel(int32_t* plan, int32_t n_seg, PlanCfg c, int32_t cap_hub,
                                   int32_t cap_piece) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    plan[PW_MAGIC] = kPlanMagic;
    plan[PW_NSEG] = n_seg;
    plan[PW_SEG_COST] = c.seg_cost;
    plan[PW_ROW_COST] = c.row_cost;
    plan[PW_HUB_DEG] = c.hub_deg;
    plan[PW_PIECE_EDGES] = c.piece_edges;
    plan[PW_NHUB] = 0;
    plan[PW_NPIECE] = 0;
    plan[PW_CAP_HUB] = cap_hub;
    plan[PW_CAP_PIECE] = cap_piece;
  }
}

// seg_row[s] = first row r with rowptr[r] + row_cost * r >= s * seg_cost  (s < n_seg);
// seg_row[n_seg] = N.
__global__ __launch_bounds__(kBlock) void plan_seg_kernel(const int32_t* __restrict__ rowptr,
                                                          int32_t N, int32_t n_seg, int seg_cost,
                                                          int row_cost, int32_t* seg_row) {
  for (int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; s <= n_seg;
       s += (int64_t)gridDim.x * blockDim.x) {
    if (s == n_seg) { seg_row[s] = N; continue; }
    const int64_t target = s * (int64_t)seg_cost;
    int lo = 0, hi = N;  // answer in [0, N]
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      const int64_t p = (int64_t)rowptr[mid] + (int64_t)row_cost * mid;
      if (p >= target) hi = mid; else lo = mid + 1;
    }
    seg_row[s] = lo;
  }
}

__global__ __launch_bounds__(kBlock) void plan_hub_kernel(const int32_t* __restrict__ rowptr,
                                                          int32_t N, int hub_deg, int piece_edges,
                                                          int32_t* header, int32_t* hub_row,
                                                          int32_t* hub_base, int32_t* hub_np,
                                                          int32_t* piece_hub, int32_t* piece_k) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < N;
       r += (int64_t)gridDim.x * blockDim.x) {
    const int deg = rowptr[r + 1] - rowptr[r];
    if (deg > hub_deg) {
      const int np = (deg + piece_edges - 1) / piece_edges;
      const int h = atomicAdd(&header[PW_NHUB], 1);
      const int base = atomicAdd(&header[PW_NPIECE], np);
      hub_row[h] = (int32_t)r;
      hub_base[h] = base;
      hub_np[h] = np;
      for (int k = 0; k < np; ++k) {
        piece_hub[base + k] = h;
        piece_k[base + k] = k;
      }
    }
  }
}

// ---- dispatch -------------------------------------------------------------

// the rows kernel over every segment; with hub rows in the plan, their pieces and the finalize pass
template <class S, int REDUCE, bool WEIGHTED, bool BRANCH2, int NH = 1>
static int launch_agg(const typename S::Args& g, const int32_t* counts, hipStream_t st) {
  using E = typename S::E;
  constexpr int W = S::kW;
  constexpr int U = E::template kU<W>;
  const AggArgs<E>& a = S::agg(g);
  const int tiles = (int)ceil_div(a.d, kWave * W);
  dim3 grid((unsigned)ceil_div(a.n_seg, kWavesPerBlock), (unsigned)tiles);
  hipLaunchKernelGGL((agg_rows_kernel<S, REDUCE, WEIGHTED, BRANCH2, U, NH>), grid, dim3(kBlock), 0, st, g);
  MP_LAUNCH_CHECK();
  const int n_hub = counts[1], n_piece = counts[2];
  if (n_hub > 0) {
    int pb = (int)ceil_div(n_piece, kWavesPerBlock);
    if (pb > kNumCU * 8) pb = kNumCU * 8;
    hipLaunchKernelGGL((agg_hub_pieces_kernel<S, REDUCE, WEIGHTED, BRANCH2, U, NH>), dim3(pb, tiles),
                       dim3(kBlock), 0, st, g);
    MP_LAUNCH_CHECK();
    int hb = (int)ceil_div(n_hub, kWavesPerBlock);
    if (hb > kNumCU * 8) hb = kNumCU * 8;
    hipLaunchKernelGGL((agg_hub_finalize_kernel<E, W, REDUCE, BRANCH2>), dim3(hb, tiles), dim3(kBlock),
                       0, st, a);
    MP_LAUNCH_CHECK();
  }
  return MP_OK;
}

// NH > 1: every entry carries NH weights (val [nnz, NH], required; no second branch).  Mean and max take the same body:
// mean divides by the row's entry count in finish_row, max keeps the first winning entry per column (argmax, merged
// across hub pieces in piece order by the finalize kernel).
template <class S, int NH = 1>
static int dispatch_reduce(const typename S::Args& g, const int32_t* counts, int reduce, hipStream_t st) {
  const auto& a = S::agg(g);
  if constexpr (NH > 1) {
    switch (reduce) {
      case MP_SUM: return launch_agg<S, MP_SUM, true, false, NH>(g, counts, st);
      case MP_MEAN: return launch_agg<S, MP_MEAN, true, false, NH>(g, counts, st);
      case MP_MAX: return launch_agg<S, MP_MAX, true, false, NH>(g, counts, st);
    }
    return MP_ERR_INVALID_ARG;
  } else {
    const bool weighted = a.val != nullptr;
    if constexpr (S::kMarks) {
      if (a.Q != nullptr) {
        return weighted ? launch_agg<S, MP_SUM, true, true>(g, counts, st)
                        : launch_agg<S, MP_SUM, false, true>(g, counts, st);
      }
    }
    switch (reduce) {
      case MP_SUM:
        return weighted ? launch_agg<S, MP_SUM, true, false>(g, counts, st)
                        : launch_agg<S, MP_SUM, false, false>(g, counts, st);
      case MP_MEAN:
        return weighted ? launch_agg<S, MP_MEAN, true, false>(g, counts, st)
                        : launch_agg<S, MP_MEAN, false, false>(g, counts, st);
      case MP_MAX:
        return weighted ? launch_agg<S, MP_MAX, true, false>(g, counts, st)
                        : launch_agg<S, MP_MAX, false, false>(g, counts, st);
    }
    return MP_ERR_INVALID_ARG;
  }
}

// the head count: one weight per entry, or 2 / 4 / 8 of them in one launch (fp32 sources)
template <class S>
static int dispatch_heads(const typename S::Args& g, const int32_t* counts, int reduce, int heads, hipStream_t st) {
  if (heads <= 1) return dispatch_reduce<S>(g, counts, reduce, st);
  if constexpr (S::E::kExtras) {
    switch (heads) {
      case 2: return dispatch_reduce<S, 2>(g, counts, reduce, st);
      case 4: return dispatch_reduce<S, 4>(g, counts, reduce, st);
      case 8: return dispatch_reduce<S, 8>(g, counts, reduce, st);
    }
  }
  return MP_ERR_UNSUPPORTED;
}

// the source: two gathers when the call brings the operands of the two-gather form (fp32 only), else one
template <class E, int W>
static int dispatch_source(const AggArgs<E>& a, const EdgeOperands* eo, const int32_t* counts, int reduce, int heads,
                           hipStream_t st) {
  if (eo) {
    if constexpr (std::is_same<E, F32>::value) {
      const EdgeArgs g = {a, *eo};
      return eo->T ? dispatch_heads<EdgeRows<W, true>>(g, counts, reduce, heads, st)
                   : dispatch_heads<EdgeRows<W, false>>(g, counts, reduce, heads, st);
    } else {
      return MP_ERR_UNSUPPORTED;
    }
  }
  return dispatch_heads<XRows<E, W>>(a, counts, reduce, heads, st);
}

static bool aligned(const void* p, size_t a) { return p == nullptr || ((uintptr_t)p % a) == 0; }

// widest per-lane vector every operand allows, then no wider than the row needs
template <class E>
static int pick_width(const AggArgs<E>& a, const EdgeOperands* eo) {
  auto ok = [&](int w) {
    const size_t eb = sizeof(typename E::T) * w;   // X, S, Y, Q: one access of w elements per lane
    const size_t fb = 4u * (w < 4 ? w : 4);        // fp32 / int32 operands: vectors of at most 4
    if (a.d % w) return false;
    if (a.head_width > 0 && a.head_width % w) return false;   // a lane's columns stay inside one head
    if (a.ldx % w || a.ldy % w) return false;
    if (a.Q && a.ldq % w) return false;
    if (a.S && a.lds % w) return false;
    if (eo && (eo->ldm % w || !aligned(eo->M, fb))) return false;
    if (eo && eo->T && (eo->ldt % w || !aligned(eo->T, fb))) return false;
    return aligned(a.X, eb) && aligned(a.Y, eb) && aligned(a.Q, eb) && aligned(a.S, eb) &&
           aligned(a.bias, fb) && aligned(a.col_scale, fb) && aligned(a.argmax, fb) &&
           aligned(a.part, fb) && aligned(a.part2, fb) && aligned(a.part_arg, fb);
  };
  int w = E::kMaxW;
  while (w > 1 && !ok(w)) w >>= 1;
  while (w > 1 && kWave * (w / 2) >= a.d) w >>= 1;  // d = 256 -> 4, d = 128 -> 2, d = 64 -> 1: keep all lanes busy
  return w;
}

// the hub arrays of the plan (behind seg_row; counts[3], counts[4] = their capacities) and the partial buffers of the
// hub pieces inside the caller's workspace (mp_spmm_ws_bytes); a.seg_row, a.d and a.Q are set
template <class E>
static void bind_hub(AggArgs<E>& a, const int32_t* counts, int reduce, void* ws) {
  const int32_t n_seg = counts[0], n_piece = counts[2];
  a.hub_row = a.hub_base = a.hub_np = a.piece_hub = a.piece_k = nullptr;
  a.part = a.part2 = nullptr; a.part_arg = nullptr;
  if (n_piece > 0) {
    const int32_t cap_hub = counts[3], cap_piece = counts[4];
    a.hub_row = a.seg_row + (n_seg + 1);
    a.hub_base = a.hub_row + cap_hub;
    a.hub_np = a.hub_base + cap_hub;
    a.piece_hub = a.hub_np + cap_hub;
    a.piece_k = a.piece_hub + cap_piece;
    char* w = (char*)ws;
    const size_t slab = align_up((size_t)n_piece * a.d * 4, 256);
    a.part = (float*)w; w += slab;
    if (a.Q) { a.part2 = (float*)w; w += slab; }
    if (reduce == MP_MAX) { a.part_arg = (int32_t*)w; w += slab; }
  }
}

template <class E>
static int agg_common(const int32_t* rowptr, const int32_t* col, const float* val, int64_t N,
                      const int32_t* plan, const int32_t* counts, const typename E::T* X, int64_t ldx,
                      typename E::T* Y, int64_t ldy, typename E::T* Q, int64_t ldq, int32_t d, int reduce,
                      const typename E::T* S, int64_t lds, float self_scale, const float* bias, int act,
                      int32_t* argmax, void* ws, size_t ws_bytes, hipStream_t st,
                      const float* col_scale = nullptr, int l2norm = 0, float l2_eps = 1e-12f, int heads = 1,
                      const EdgeOperands* eo = nullptr) {
  if (!rowptr || !plan || !counts) return MP_ERR_INVALID_ARG;
  if (N < 0 || d <= 0 || ldx < d || ldy < d) return MP_ERR_INVALID_ARG;
  if (reduce < MP_SUM || reduce > MP_MAX) return MP_ERR_INVALID_ARG;
  if (act != MP_ACT_NONE && act != MP_ACT_RELU) return MP_ERR_INVALID_ARG;
  if (Q && ldq < d) return MP_ERR_INVALID_ARG;
  if (S && lds < d) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX) return MP_ERR_UNSUPPORTED;
  if (N == 0) return MP_OK;           // no row: the arrays of N rows (Y; X of a square operator) may have no address
  if (!X || !Y) return MP_ERR_INVALID_ARG;
  const int32_t n_seg = counts[0], n_piece = counts[2];
  if (n_seg < 1) return MP_ERR_INVALID_ARG;
  if (!col && n_piece > 0) return MP_ERR_INVALID_ARG;

  size_t need = 0;
  mp_spmm_ws_bytes(counts, d, reduce, Q != nullptr, &need);
  if (need > 0 && (!ws || ws_bytes < need)) return MP_ERR_WORKSPACE;

  AggArgs<E> a;
  a.rowptr = rowptr; a.col = col; a.val = val;
  a.header = plan;
  a.seg_row = plan + PW_HEADER_WORDS;
  a.n_seg = n_seg;
  a.hub_deg = counts[6];       // the config the plan was built under
  a.piece_edges = counts[7];
  a.X = X; a.ldx = ldx; a.Y = Y; a.ldy = ldy; a.Q = Q; a.ldq = ldq;
  a.S = S; a.lds = lds; a.self_scale = self_scale; a.bias = bias; a.act = act;
  a.col_scale = col_scale; a.l2norm = l2norm; a.l2_eps = l2_eps;
  a.argmax = argmax; a.d = d;
  a.head_width = heads > 1 ? d / heads : 0;
  bind_hub(a, counts, reduce, ws);

  const int w = pick_width(a, eo);
  if (l2norm && d > kWave * w) return MP_ERR_UNSUPPORTED;   // the row must sit in one wave
  if (heads > 1 && (!E::kExtras || !val || Q || d % heads)) return MP_ERR_INVALID_ARG;
  if constexpr (E::kMaxW == 8) {
    if (w == 8) return dispatch_source<E, 8>(a, eo, counts, reduce, heads, st);
  }
  switch (w) {
    case 4: return dispatch_source<E, 4>(a, eo, counts, reduce, heads, st);
    case 2: return dispatch_source<E, 2>(a, eo, counts, reduce, heads, st);
    default: return dispatch_source<E, 1>(a, eo, counts, reduce, heads, st);
  }
}

// mp_spline_agg_f32 (FOLD false: X [n, d] -> the halves of Y [N, 2d]) and mp_spline_fold_f32 (FOLD true: X [n, 2d] ->
// Y [N, d]): the checks of agg_common on their shapes, then the sum kernels on the two sources above.  The second half
// of a row starts d elements behind the first: pick_width sees it as Q (agg) or through d % w == 0 on an aligned X (fold).
template <bool FOLD>
static int spline_common(const int32_t* rowptr, const int32_t* col, const float* w2, int64_t N, const int32_t* plan,
                         const int32_t* counts, const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t d, void* ws,
                         size_t ws_bytes, hipStream_t st) {
  if (!rowptr || !plan || !counts) return MP_ERR_INVALID_ARG;
  if (N < 0 || d <= 0) return MP_ERR_INVALID_ARG;
  if (d > INT32_MAX / 2) return MP_ERR_UNSUPPORTED;
  if (ldx < (FOLD ? 2 : 1) * (int64_t)d || ldy < (FOLD ? 1 : 2) * (int64_t)d) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX) return MP_ERR_UNSUPPORTED;
  if (N == 0) return MP_OK;
  if (!X || !Y) return MP_ERR_INVALID_ARG;
  const int32_t n_seg = counts[0], n_piece = counts[2];
  if (n_seg < 1) return MP_ERR_INVALID_ARG;
  if ((!col || !w2) && n_piece > 0) return MP_ERR_INVALID_ARG;   // (an operator without entries has neither)

  size_t need = 0;
  mp_spmm_ws_bytes(counts, d, MP_SUM, FOLD ? 0 : 1, &need);
  if (need > 0 && (!ws || ws_bytes < need)) return MP_ERR_WORKSPACE;

  SplineArgs g;
  AggArgs<F32>& a = g.a;
  g.w2 = w2;
  a.rowptr = rowptr; a.col = col; a.val = nullptr;
  a.header = plan;
  a.seg_row = plan + PW_HEADER_WORDS;
  a.n_seg = n_seg;
  a.hub_deg = counts[6];
  a.piece_edges = counts[7];
  a.X = X; a.ldx = ldx; a.Y = Y; a.ldy = ldy;
  a.Q = FOLD ? nullptr : Y + d; a.ldq = FOLD ? 0 : ldy;
  a.S = nullptr; a.lds = 0; a.self_scale = 0.f; a.bias = nullptr; a.act = MP_ACT_NONE;
  a.col_scale = nullptr; a.l2norm = 0; a.l2_eps = 1e-12f;
  a.argmax = nullptr; a.d = d;
  a.head_width = 0;
  bind_hub(a, counts, MP_SUM, ws);

  auto launch = [&](auto wc) {
    constexpr int W = decltype(wc)::value;
    if constexpr (FOLD) return launch_agg<SplineFoldRows<W>, MP_SUM, false, false>(g, counts, st);
    else return launch_agg<SplineAggRows<W>, MP_SUM, false, true>(g, counts, st);
  };
  switch (pick_width(a, nullptr)) {
    case 4: return launch(std::integral_constant<int, 4>());
    case 2: return launch(std::integral_constant<int, 2>());
    default: return launch(std::integral_constant<int, 1>());
  }
}

// mp_spmm_max_bwd_pull_f32 / _bf16 / mp_spmm_heads_max_bwd_pull_f32: the checks of agg_common on the transposed
// operator, then the sum kernels on MaxBwdRows.  heads <= 1: w [nnz] or NULL (ones); 2 / 4 / 8 (fp32): w [nnz, heads].
template <class E>
static int max_bwd_pull_common(const int32_t* t_rowptr, const int32_t* t_col, const int32_t* t_pos, const float* w,
                               int64_t n_src, int64_t nnz, const int32_t* plan, const int32_t* counts, int32_t heads,
                               const int32_t* argmax, int64_t lda, const typename E::T* dY, int64_t ldy, int32_t d,
                               typename E::T* dX, int64_t ldx, void* ws, size_t ws_bytes, hipStream_t st) {
  if (!t_rowptr || !plan || !counts) return MP_ERR_INVALID_ARG;
  if (n_src < 0 || nnz < 0 || d <= 0 || lda < d || ldy < d || ldx < d) return MP_ERR_INVALID_ARG;
  if (heads < 1 || d % heads || (heads > 1 && !w)) return MP_ERR_INVALID_ARG;
  if (n_src >= INT32_MAX || nnz >= INT32_MAX) return MP_ERR_UNSUPPORTED;
  if (heads > 1 && (!E::kExtras || (heads != 2 && heads != 4 && heads != 8))) return MP_ERR_UNSUPPORTED;
  if (n_src == 0) return MP_OK;
  if (!dX) return MP_ERR_INVALID_ARG;
  if (nnz > 0 && (!t_col || !t_pos || !argmax || !dY)) return MP_ERR_INVALID_ARG;   // (without entries nothing reads them)
  const int32_t n_seg = counts[0];
  if (n_seg < 1) return MP_ERR_INVALID_ARG;

  size_t need = 0;
  mp_spmm_ws_bytes(counts, d, MP_SUM, 0, &need);
  if (need > 0 && (!ws || ws_bytes < need)) return MP_ERR_WORKSPACE;

  MaxBwdArgs<E> g;
  AggArgs<E>& a = g.a;
  g.pos = t_pos; g.argmax = argmax; g.lda = lda;
  a.rowptr = t_rowptr; a.col = t_col; a.val = w;
  a.header = plan;
  a.seg_row = plan + PW_HEADER_WORDS;
  a.n_seg = n_seg;
  a.hub_deg = counts[6];
  a.piece_edges = counts[7];
  a.X = dY; a.ldx = ldy; a.Y = dX; a.ldy = ldx; a.Q = nullptr; a.ldq = 0;
  a.S = nullptr; a.lds = 0; a.self_scale = 0.f; a.bias = nullptr; a.act = MP_ACT_NONE;
  a.col_scale = nullptr; a.l2norm = 0; a.l2_eps = 1e-12f;
  a.argmax = nullptr; a.d = d;
  a.head_width = heads > 1 ? d / heads : 0;
  bind_hub(a, counts, MP_SUM, ws);

  auto launch = [&](auto wc) {
    using S = MaxBwdRows<E, decltype(wc)::value>;
    if constexpr (E::kExtras) {
      switch (heads) {
        case 2: return launch_agg<S, MP_SUM, true, false, 2>(g, counts, st);
        case 4: return launch_agg<S, MP_SUM, true, false, 4>(g, counts, st);
        case 8: return launch_agg<S, MP_SUM, true, false, 8>(g, counts, st);
      }
    }
    return w ? launch_agg<S, MP_SUM, true, false>(g, counts, st) : launch_agg<S, MP_SUM, false, false>(g, counts, st);
  };
  int wd = pick_width(a, nullptr);
  while (wd > 1 && (lda % wd || !aligned(argmax, 4u * (wd < 4 ? wd : 4)))) wd >>= 1;   // the argmax row: int32 vectors of <= 4
  if constexpr (E::kMaxW == 8) {
    if (wd == 8) return launch(std::integral_constant<int, 8>());
  }
  switch (wd) {
    case 4: return launch(std::integral_constant<int, 4>());
    case 2: return launch(std::integral_constant<int, 2>());
    default: return launch(std::integral_constant<int, 1>());
  }
}

template <class E>
__global__ __launch_bounds__(kBlock) void max_bwd_kernel(const int32_t* __restrict__ col,
                                                         const float* __restrict__ val,
                                                         const int32_t* __restrict__ argmax,
                                                         const typename E::T* __restrict__ dY, int64_t ldy,
                                                         int64_t N, int32_t d, float* dX, int64_t ldx) {
  const int64_t total = N * d;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / d;
    const int c = (int)(i - r * d);
    const int e = argmax[i];
    if (e >= 0) atomicAdd(&dX[(int64_t)col[e] * ldx + c], (val ? val[e] : 1.f) * E::to_f32(dY[r * ldy + c]));
  }
}

// Backward of the multi-head weighted max into V: dV[col[e], c] += a[e * H + c / hw] * dY[r, c] for e = argmax[r, c].
// One wave per output row (no 64-bit index division), lanes across the columns: argmax and dY are read coalesced, the
// adds are no-return float atomics (global_atomic_add_f32), one launch for every head.
__global__ __launch_bounds__(kBlock) void heads_max_bwd_kernel(const int32_t* __restrict__ col,
                                                               const float* __restrict__ a, int32_t heads, int32_t hw,
                                                               const int32_t* __restrict__ argmax,
                                                               const float* __restrict__ dY, int64_t ldy, int64_t N,
                                                               int32_t d, float* dV, int64_t ldv) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  for (int64_t r = (int64_t)blockIdx.x * kWavesPerBlock + wave; r < N; r += (int64_t)gridDim.x * kWavesPerBlock) {
    for (int c = lane; c < d; c += kWave) {
      const int e = argmax[r * d + c];
      if (e >= 0) atomicAdd(&dV[(int64_t)col[e] * ldv + c], a[(int64_t)e * heads + c / hw] * dY[r * ldy + c]);
    }
  }
}

}  // namespace mp

using namespace mp;

extern "C" {

int mp_spmm_plan_bytes(int64_t N, int64_t nnz, const int32_t* cfg_host, size_t* bytes_host) {
  if (!bytes_host || N < 0 || nnz < 0) return MP_ERR_INVALID_ARG;
  if (nnz >= INT32_MAX || N >= INT32_MAX) return MP_ERR_UNSUPPORTED;
  PlanCfg c;
  if (int st = cfg_from(cfg_host, &c)) return st;
  *bytes_host = plan_words(N, nnz, c) * sizeof(int32_t);
  return MP_OK;
}

// counts_host: {n_seg, n_hub, n_piece, cap_hub, cap_piece, seg_cost, hub_deg, piece_edges}
int mp_spmm_plan_build(const int32_t* rowptr, int64_t N, int64_t nnz, const int32_t* cfg_host, int32_t* plan,
                       size_t plan_bytes, int32_t* counts_host, mp_stream_t stream) {
  if (!rowptr || !plan || !counts_host || N < 0 || nnz < 0) return MP_ERR_INVALID_ARG;
  if (nnz >= INT32_MAX || N >= INT32_MAX) return MP_ERR_UNSUPPORTED;
  PlanCfg c;
  if (int cst = cfg_from(cfg_host, &c)) return cst;
  if (plan_bytes < plan_words(N, nnz, c) * sizeof(int32_t)) return MP_ERR_WORKSPACE;
  hipStream_t st = as_stream(stream);
  PlanView v = plan_view(plan, N, nnz, c);
  hipLaunchKernelGGL(plan_header_kernel, dim3(1), dim3(64), 0, st, plan, v.n_seg, c, v.cap_hub,
                     v.cap_piece);
  MP_LAUNCH_CHECK();
  hipLaunchKernelGGL(plan_seg_kernel, dim3(flat_grid(v.n_seg + 1)), dim3(kBlock), 0, st, rowptr,
                     (int32_t)N, v.n_seg, c.seg_cost, c.row_cost, (int32_t*)v.seg_row);
  MP_LAUNCH_CHECK();
  if (N > 0) {
    hipLaunchKernelGGL(plan_hub_kernel, dim3(flat_grid(N)), dim3(kBlock), 0, st, rowptr, (int32_t)N,
                       c.hub_deg, c.piece_edges, plan, (int32_t*)v.hub_row, (int32_t*)v.hub_base,
                       (int32_t*)v.hub_np, (int32_t*)v.piece_hub, (int32_t*)v.piece_k);
    MP_LAUNCH_CHECK();
  }
  int32_t hdr[PW_HEADER_WORDS];
  MP_HIP(hipMemcpyAsync(hdr, plan, sizeof(hdr), hipMemcpyDeviceToHost, st));
  MP_HIP(hipStreamSynchronize(st));
  counts_host[0] = hdr[PW_NSEG];
  counts_host[1] = hdr[PW_NHUB];
  counts_host[2] = hdr[PW_NPIECE];
  counts_host[3] = hdr[PW_CAP_HUB];
  counts_host[4] = hdr[PW_CAP_PIECE];
  counts_host[5] = hdr[PW_SEG_COST];
  counts_host[6] = hdr[PW_HUB_DEG];
  counts_host[7] = hdr[PW_PIECE_EDGES];
  return MP_OK;
}

int mp_spmm_ws_bytes(const int32_t* counts_host, int32_t d, int reduce, int two_branch,
                     size_t* bytes_host) {
  if (!counts_host || !bytes_host || d <= 0) return MP_ERR_INVALID_ARG;
  const size_t slab = align_up((size_t)counts_host[2] * d * 4, 256);
  size_t n = counts_host[2] > 0 ? slab : 0;
  if (counts_host[2] > 0 && two_branch) n += slab;
  if (counts_host[2] > 0 && reduce == MP_MAX) n += slab;
  *bytes_host = n;
  return MP_OK;
}

int mp_spmm_csr_f32(const int32_t* rowptr, const int32_t* col, const float* val, int64_t N,
                    const int32_t* plan, const int32_t* counts_host, const float* X, int64_t ldx,
                    float* Y, int64_t ldy, int32_t d, int reduce, const float* S, int64_t lds,
                    float self_scale, const float* bias, int act, int32_t* argmax, void* ws,
                    size_t ws_bytes, mp_stream_t stream) {
  return agg_common<F32>(rowptr, col, val, N, plan, counts_host, X, ldx, Y, ldy, nullptr, 0, d, reduce, S,
                         lds, self_scale, bias, act, argmax, ws, ws_bytes, as_stream(stream));
}

int mp_spmm_csr_epilogue_f32(const int32_t* rowptr, const int32_t* col, const float* val, int64_t N,
                             const int32_t* plan, const int32_t* counts_host, const float* X, int64_t ldx,
                             float* Y, int64_t ldy, int32_t d, int reduce, const float* S, int64_t lds,
                             float self_scale, const float* col_scale, const float* col_shift, int act,
                             int l2_normalize, float l2_eps, void* ws, size_t ws_bytes, mp_stream_t stream) {
  return agg_common<F32>(rowptr, col, val, N, plan, counts_host, X, ldx, Y, ldy, nullptr, 0, d, reduce, S, lds,
                         self_scale, col_shift, act, nullptr, ws, ws_bytes, as_stream(stream), col_scale,
                         l2_normalize ? 1 : 0, l2_eps);
}

int mp_idgnn_agg_f32(const int32_t* rowptr, const int32_t* col_marked, const float* val, int64_t N,
                     const int32_t* plan, const int32_t* counts_host, const float* X, int64_t ldx,
                     float* P, int64_t ldp, float* Q, int64_t ldq, int32_t d, void* ws,
                     size_t ws_bytes, mp_stream_t stream) {
  if (N != 0 && !Q) return MP_ERR_INVALID_ARG;
  return agg_common<F32>(rowptr, col_marked, val, N, plan, counts_host, X, ldx, P, ldp, Q, ldq, d, MP_SUM,
                         nullptr, 0, 0.f, nullptr, MP_ACT_NONE, nullptr, ws, ws_bytes, as_stream(stream));
}

int mp_spline_agg_f32(const int32_t* rowptr, const int32_t* col, const float* w, int64_t N, const int32_t* plan,
                      const int32_t* counts_host, const float* X, int64_t ldx, float* Y, int64_t ldy, int32_t d, void* ws,
                      size_t ws_bytes, mp_stream_t stream) {
  return spline_common<false>(rowptr, col, w, N, plan, counts_host, X, ldx, Y, ldy, d, ws, ws_bytes, as_stream(stream));
}

int mp_spline_fold_f32(const int32_t* rowptr, const int32_t* col, const float* w, int64_t N, const int32_t* plan,
                       const int32_t* counts_host, const float* Z, int64_t ldz, float* Y, int64_t ldy, int32_t d, void* ws,
                       size_t ws_bytes, mp_stream_t stream) {
  return spline_common<true>(rowptr, col, w, N, plan, counts_host, Z, ldz, Y, ldy, d, ws, ws_bytes, as_stream(stream));
}

int mp_spmm_csr_heads_reduce_f32(const int32_t* rowptr, const int32_t* col, const float* a, int64_t N,
                                 const int32_t* plan, const int32_t* counts_host, int32_t heads, int reduce,
                                 const float* V, int64_t ldv, float* Y, int64_t ldy, int32_t d, int32_t* argmax,
                                 void* ws, size_t ws_bytes, mp_stream_t stream) {
  if (heads < 1 || !a || !col || d <= 0 || d % heads) return MP_ERR_INVALID_ARG;
  if (reduce < MP_SUM || reduce > MP_MAX) return MP_ERR_INVALID_ARG;
  return agg_common<F32>(rowptr, col, a, N, plan, counts_host, V, ldv, Y, ldy, nullptr, 0, d, reduce, nullptr, 0, 0.f,
                         nullptr, MP_ACT_NONE, reduce == MP_MAX ? argmax : nullptr, ws, ws_bytes, as_stream(stream),
                         nullptr, 0, 1e-12f, heads);
}

int mp_spmm_heads_max_bwd_f32(const int32_t* col, const float* a, int32_t heads, const int32_t* argmax, int64_t N,
                              int32_t d, const float* dY, int64_t ldy, float* dV, int64_t ldv, mp_stream_t stream) {
  if (!col || !a || !argmax || !dY || !dV || N < 0 || d <= 0 || heads < 1 || d % heads) return MP_ERR_INVALID_ARG;
  if (ldy < d || ldv < d) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX) return MP_ERR_UNSUPPORTED;
  if (N == 0) return MP_OK;
  hipLaunchKernelGGL(heads_max_bwd_kernel, dim3(row_grid(N)), dim3(kBlock), 0, as_stream(stream), col, a, heads,
                     d / heads, argmax, dY, ldy, N, d, dV, ldv);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_spmm_csr_edge_f32(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const float* val, int64_t N,
                         const int32_t* plan, const int32_t* counts_host, const float* X, int64_t ldx, const float* M,
                         int64_t ldm, const float* T, int64_t ldt, float* Y, int64_t ldy, int32_t d, int reduce,
                         const float* bias, int32_t* argmax, void* ws, size_t ws_bytes, mp_stream_t stream) {
  if (!col || !eid || !M || ldm < d || (T && ldt < d)) return MP_ERR_INVALID_ARG;
  const EdgeOperands eo = {eid, M, ldm, T, T ? ldt : 0};
  return agg_common<F32>(rowptr, col, val, N, plan, counts_host, X, ldx, Y, ldy, nullptr, 0, d, reduce, nullptr, 0, 0.f,
                         bias, MP_ACT_NONE, reduce == MP_MAX ? argmax : nullptr, ws, ws_bytes, as_stream(stream),
                         nullptr, 0, 1e-12f, 1, &eo);
}

int mp_spmm_csr_edge_heads_f32(const int32_t* rowptr, const int32_t* col, const int32_t* eid, const float* a, int64_t N,
                               const int32_t* plan, const int32_t* counts_host, int32_t heads, const float* X,
                               int64_t ldx, const float* M, int64_t ldm, const float* T, int64_t ldt, float* Y,
                               int64_t ldy, int32_t d, int reduce, const float* bias, int32_t* argmax, void* ws,
                               size_t ws_bytes, mp_stream_t stream) {
  if (!col || !eid || !a || !M || heads < 1 || d <= 0 || d % heads || ldm < d || (T && ldt < d))
    return MP_ERR_INVALID_ARG;
  if (heads != 1 && heads != 2 && heads != 4 && heads != 8) return MP_ERR_UNSUPPORTED;
  const EdgeOperands eo = {eid, M, ldm, T, T ? ldt : 0};
  return agg_common<F32>(rowptr, col, a, N, plan, counts_host, X, ldx, Y, ldy, nullptr, 0, d, reduce, nullptr, 0, 0.f,
                         bias, MP_ACT_NONE, reduce == MP_MAX ? argmax : nullptr, ws, ws_bytes, as_stream(stream),
                         nullptr, 0, 1e-12f, heads, &eo);
}

// the two backward launches into M: one weight per entry (heads <= 1; val may be NULL) or val [nnz, heads]
static int edge_bwd_launch(const int32_t* rowptr, const int32_t* eid, const float* val, int32_t heads,
                           const int32_t* argmax, int64_t N, int64_t nnz, int reduce, const float* dY, int64_t ldy,
                           int32_t d, float* dM, int64_t ldm, hipStream_t st) {
  if (!rowptr || N < 0 || nnz < 0 || d < 1) return MP_ERR_INVALID_ARG;
  if (reduce < MP_SUM || reduce > MP_MAX) return MP_ERR_INVALID_ARG;
  if (ldy < d || ldm < d) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || nnz >= INT32_MAX) return MP_ERR_UNSUPPORTED;
  if (N == 0 || nnz == 0) return MP_OK;     // no row or no entry: eid, and dY / argmax of no rows, may have no address
  if (!eid || !dY || !dM || (reduce == MP_MAX && !argmax)) return MP_ERR_INVALID_ARG;
  const int32_t hw = heads > 1 ? d / heads : d;
  if (reduce == MP_MAX) {
    const dim3 grid(row_grid(N));
    if (heads > 1)
      hipLaunchKernelGGL(edge_bwd_max_kernel<true>, grid, dim3(kBlock), 0, st, eid, val, heads, hw,
                         argmax, N, dY, ldy, d, dM, ldm);
    else
      hipLaunchKernelGGL(edge_bwd_max_kernel<false>, grid, dim3(kBlock), 0, st, eid, val, 1, hw,
                         argmax, N, dY, ldy, d, dM, ldm);
  } else {
    const dim3 grid(row_grid(ceil_div(nnz, kWave)));
    const int mean = reduce == MP_MEAN ? 1 : 0;
    if (heads > 1)
      hipLaunchKernelGGL(edge_bwd_rows_kernel<true>, grid, dim3(kBlock), 0, st, rowptr, eid, val,
                         heads, hw, (int32_t)N, (int32_t)nnz, mean, dY, ldy, d, dM, ldm);
    else
      hipLaunchKernelGGL(edge_bwd_rows_kernel<false>, grid, dim3(kBlock), 0, st, rowptr, eid, val, 1,
                         hw, (int32_t)N, (int32_t)nnz, mean, dY, ldy, d, dM, ldm);
  }
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_spmm_edge_bwd_f32(const int32_t* rowptr, const int32_t* eid, const float* val, const int32_t* argmax, int64_t N,
                         int64_t nnz, int reduce, const float* dY, int64_t ldy, int32_t d, float* dM, int64_t ldm,
                         mp_stream_t stream) {
  return edge_bwd_launch(rowptr, eid, val, 1, argmax, N, nnz, reduce, dY, ldy, d, dM, ldm, as_stream(stream));
}

int mp_spmm_edge_heads_bwd_f32(const int32_t* rowptr, const int32_t* eid, const float* a, int32_t heads,
                               const int32_t* argmax, int64_t N, int64_t nnz, int reduce, const float* dY, int64_t ldy,
                               int32_t d, float* dM, int64_t ldm, mp_stream_t stream) {
  if (!a || heads < 1 || d < 1 || d % heads) return MP_ERR_INVALID_ARG;
  return edge_bwd_launch(rowptr, eid, a, heads, argmax, N, nnz, reduce, dY, ldy, d, dM, ldm, as_stream(stream));
}

int mp_spmm_max_bwd_f32(const int32_t* col, const float* val, const int32_t* argmax, const float* dY,
                        int64_t ldy, int64_t N, int32_t d, float* dX, int64_t ldx, mp_stream_t stream) {
  if (!col || !argmax || !dY || !dX || N < 0 || d <= 0) return MP_ERR_INVALID_ARG;
  if (N == 0) return MP_OK;
  hipLaunchKernelGGL(max_bwd_kernel<F32>, dim3(flat_grid(N * d)), dim3(kBlock), 0, as_stream(stream), col,
                     val, argmax, dY, ldy, N, d, dX, ldx);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_spmm_csr_bf16(const int32_t* rowptr, const int32_t* col, const float* val, int64_t N,
                     const int32_t* plan, const int32_t* counts_host, const void* X, int64_t ldx,
                     void* Y, int64_t ldy, int32_t d, int reduce, const void* S, int64_t lds,
                     float self_scale, const float* bias, int act, int32_t* argmax, void* ws,
                     size_t ws_bytes, mp_stream_t stream) {
  return agg_common<Bf16>(rowptr, col, val, N, plan, counts_host, (const uint16_t*)X, ldx, (uint16_t*)Y, ldy,
                          nullptr, 0, d, reduce, (const uint16_t*)S, lds, self_scale, bias, act, argmax, ws, ws_bytes,
                          as_stream(stream));
}

int mp_idgnn_agg_bf16(const int32_t* rowptr, const int32_t* col_marked, const float* val, int64_t N,
                      const int32_t* plan, const int32_t* counts_host, const void* X, int64_t ldx,
                      void* P, int64_t ldp, void* Q, int64_t ldq, int32_t d, void* ws,
                      size_t ws_bytes, mp_stream_t stream) {
  if (N != 0 && !Q) return MP_ERR_INVALID_ARG;
  return agg_common<Bf16>(rowptr, col_marked, val, N, plan, counts_host, (const uint16_t*)X, ldx, (uint16_t*)P, ldp,
                          (uint16_t*)Q, ldq, d, MP_SUM, nullptr, 0, 0.f, nullptr, MP_ACT_NONE, nullptr, ws, ws_bytes,
                          as_stream(stream));
}

int mp_spmm_max_bwd_bf16(const int32_t* col, const float* val, const int32_t* argmax, const void* dY,
                         int64_t ldy, int64_t N, int32_t d, float* dX, int64_t ldx, mp_stream_t stream) {
  if (!col || !argmax || !dY || !dX || N < 0 || d <= 0) return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX) return MP_ERR_UNSUPPORTED;
  if (N == 0) return MP_OK;
  hipLaunchKernelGGL(max_bwd_kernel<Bf16>, dim3(flat_grid(N * d)), dim3(kBlock), 0, as_stream(stream), col,
                     val, argmax, (const uint16_t*)dY, ldy, N, d, dX, ldx);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_spmm_max_bwd_pull_f32(const int32_t* t_rowptr, const int32_t* t_col, const int32_t* t_pos, const float* t_val,
                             int64_t n_src, int64_t nnz, const int32_t* plan, const int32_t* counts_host,
                             const int32_t* argmax, int64_t lda, const float* dY, int64_t ldy, int32_t d, float* dX,
                             int64_t ldx, void* ws, size_t ws_bytes, mp_stream_t stream) {
  return max_bwd_pull_common<F32>(t_rowptr, t_col, t_pos, t_val, n_src, nnz, plan, counts_host, 1, argmax, lda, dY, ldy,
                                  d, dX, ldx, ws, ws_bytes, as_stream(stream));
}

int mp_spmm_max_bwd_pull_bf16(const int32_t* t_rowptr, const int32_t* t_col, const int32_t* t_pos, const float* t_val,
                              int64_t n_src, int64_t nnz, const int32_t* plan, const int32_t* counts_host,
                              const int32_t* argmax, int64_t lda, const void* dY, int64_t ldy, int32_t d, void* dX,
                              int64_t ldx, void* ws, size_t ws_bytes, mp_stream_t stream) {
  return max_bwd_pull_common<Bf16>(t_rowptr, t_col, t_pos, t_val, n_src, nnz, plan, counts_host, 1, argmax, lda,
                                   (const uint16_t*)dY, ldy, d, (uint16_t*)dX, ldx, ws, ws_bytes, as_stream(stream));
}

int mp_spmm_heads_max_bwd_pull_f32(const int32_t* t_rowptr, const int32_t* t_col, const int32_t* t_pos,
                                   const float* t_a, int32_t heads, int64_t n_src, int64_t nnz, const int32_t* plan,
                                   const int32_t* counts_host, const int32_t* argmax, int64_t lda, const float* dY,
                                   int64_t ldy, int32_t d, float* dV, int64_t ldv, void* ws, size_t ws_bytes,
                                   mp_stream_t stream) {
  if (!t_a) return MP_ERR_INVALID_ARG;
  return max_bwd_pull_common<F32>(t_rowptr, t_col, t_pos, t_a, n_src, nnz, plan, counts_host, heads, argmax, lda, dY,
                                  ldy, d, dV, ldv, ws, ws_bytes, as_stream(stream));
}

}  // extern "C"
