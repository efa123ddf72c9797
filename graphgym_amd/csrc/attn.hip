// Per-edge attention pieces for the GAT layers (K12-K14): SDDMM scores and the softmax
// over each destination row's entries (the multi-head weighted aggregation is spmm.hip's).
//   dot-product form   gat_id                TfgIDLayer.py:297-355
//   additive form      GATIDConvLayer        idconv.py:317-332
//   segment softmax    SparseAdj.softmax     sparse_adj.py:136-151
// One wavefront owns one destination row: it keeps the row's query in registers,
// streams the neighbours' keys with coalesced row loads and reduces each head's
// dot product across its lanes with DPP/permute shuffles.
#include "common.h"
#include "vecio.h"

namespace mp {

__device__ __forceinline__ float wave_sum_seg(float v, int seg_lanes) {
  // sum within aligned groups of seg_lanes (power of two <= 64) lanes
  for (int off = seg_lanes >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  return v;
}

// s[e*H+h] = scale * <A[row, slice h], B[col, slice h]>
// Feature columns are walked in tiles of 64; head slices are dh = d / H wide.  When
// dh is a power of two <= 64 that divides 64 the per-head sums are wave-segment sums.
__global__ __launch_bounds__(kBlock) void sddmm_dot_kernel(const int32_t* __restrict__ rowptr,
                                                           const int32_t* __restrict__ col, int64_t N,
                                                           const float* __restrict__ A, int64_t lda,
                                                           const float* __restrict__ B, int64_t ldb,
                                                           int32_t d, int32_t heads, float scale,
                                                           float* s) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int dh = d / heads;
  for (int64_t r = (int64_t)blockIdx.x * kWavesPerBlock + wave; r < N;
       r += (int64_t)gridDim.x * kWavesPerBlock) {
    const int e0 = rowptr[r], e1 = rowptr[r + 1];
    for (int e = e0; e < e1; ++e) {
      const int c = col[e];
      // general path: each lane accumulates its columns per head, then a full wave sum per head
      for (int h = 0; h < heads; ++h) {
        float acc = 0.f;
        for (int k = lane; k < dh; k += kWave)
          acc = fmaf(A[r * lda + h * dh + k], B[(int64_t)c * ldb + h * dh + k], acc);
        acc = wave_sum_seg(acc, kWave);
        if (lane == 0) s[(int64_t)e * heads + h] = acc * scale;
      }
    }
  }
}


// Entry-balanced SDDMM: every wave owns kStream consecutive stored entries (no row ever makes a
// wave longer than another), reads 64 (row, col) pairs with coalesced loads, broadcasts them to
// SGPRs and issues two coalesced row loads per entry — A[row] (an L1/L2 hit while the row repeats)
// and B[col] — U entries in flight.  The per-head dot product is a wave-segment reduction
// (lanes of one head are contiguous); scores leave the wave as one coalesced store per 64 entries.
// MASK (the weight gradient of a weighted max, mp_spmm_heads_max_da_f32): a column's product enters entry e's sum only
// where e won that column of its row, argmax[row, c] == e — one more coalesced row load (argmax[row], beside A[row]).
constexpr int kStream = 256;

template <int W, int U, bool MASK>
__global__ __launch_bounds__(kBlock) void sddmm_stream_kernel(const int32_t* __restrict__ row_of,
                                                              const int32_t* __restrict__ col, int64_t nnz,
                                                              const float* __restrict__ A, int64_t lda,
                                                              const float* __restrict__ B, int64_t ldb,
                                                              int32_t d, int32_t heads, float scale, float* s,
                                                              const int32_t* __restrict__ argmax, int64_t ldm) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t w0 = ((int64_t)blockIdx.x * kWavesPerBlock + wave) * kStream;
  if (w0 >= nnz) return;
  const int64_t w1 = w0 + kStream < nnz ? w0 + kStream : nnz;
  const int tiles = (d + kWave * W - 1) / (kWave * W);
  const int gs = (d / heads) / W;        // lanes per head (heads > 1 implies tiles == 1, checked on the host)
  for (int64_t ec = w0; ec < w1; ec += kWave) {
    const int64_t me = ec + lane < w1 ? ec + lane : w1 - 1;
    const int rv = row_of[me];
    const int cv = col[me];
    const int n = (int)(w1 - ec < kWave ? w1 - ec : kWave);
    float res = 0.f;
    for (int jb = 0; jb < n; jb += U) {
      float acc[U];
      int rj[U], cj[U];
#pragma unroll
      for (int j = 0; j < U; ++j) {
        acc[j] = 0.f;
        rj[j] = bcast_i(rv, jb + j);
        cj[j] = bcast_i(cv, jb + j) & 0x7fffffff;
      }
      for (int t = 0; t < tiles; ++t) {
        const int c0 = (t * kWave + lane) * W;
        const bool on = c0 < d;
        const int c0ld = on ? c0 : 0;
        float a[U][W], b[U][W];
        int m[MASK ? U : 1][W];
#pragma unroll
        for (int j = 0; j < U; ++j) {
          load_vec<W>(A + (int64_t)rj[j] * lda + c0ld, a[j]);
          load_vec<W>(B + (int64_t)cj[j] * ldb + c0ld, b[j]);
          if constexpr (MASK) load_i32<W>(argmax + (int64_t)rj[j] * ldm + c0ld, m[j]);
        }
#pragma unroll
        for (int j = 0; j < U; ++j) {
          if (on) {
            const int e = (int)(ec + jb + j);
#pragma unroll
            for (int k = 0; k < W; ++k) {
              if constexpr (MASK) acc[j] = m[j][k] == e ? fmaf(a[j][k], b[j][k], acc[j]) : acc[j];
              else acc[j] = fmaf(a[j][k], b[j][k], acc[j]);
            }
          }
        }
      }
      if (heads == 1) {
#pragma unroll
        for (int j = 0; j < U; ++j) {
          float t = acc[j];
          for (int off = 32; off > 0; off >>= 1) t += __shfl_xor(t, off, kWave);
          if (lane == jb + j) res = t;
        }
      } else {
#pragma unroll
        for (int j = 0; j < U; ++j) {
          float t = acc[j];
          for (int off = gs >> 1; off > 0; off >>= 1) t += __shfl_xor(t, off, kWave);
          const int64_t e = ec + jb + j;
          if (e < w1 && (lane % gs) == 0 && lane / gs < heads) s[e * heads + lane / gs] = t * scale;
        }
      }
    }
    if (heads == 1 && lane < n) s[ec + lane] = res * scale;
  }
}

__global__ __launch_bounds__(kBlock) void sddmm_add_kernel(const int32_t* __restrict__ rowptr,
                                                           const int32_t* __restrict__ col, int64_t N,
                                                           const float* __restrict__ ai,
                                                           const float* __restrict__ aj, float slope,
                                                           float* s) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  for (int64_t r = (int64_t)blockIdx.x * kWavesPerBlock + wave; r < N;
       r += (int64_t)gridDim.x * kWavesPerBlock) {
    const int e0 = rowptr[r], e1 = rowptr[r + 1];
    const float a_r = ai[r];
    for (int e = e0 + lane; e < e1; e += kWave) {
      const float x = a_r + aj[col[e]];
      s[e] = x > 0.f ? x : slope * x;  // F.leaky_relu, idconv.py:326
    }
  }
}

// softmax over a row's entries, in three tiers decided per row inside ONE launch (round 4; no row lists, no workspace):
//   short  (<= kSmShort = 16 entries — 90 % of the rows of a scale-free graph, 11 entries on average at m = 5): ONE lane
//          per row, the row's scores in registers — one load and one store per entry instead of three sweeps (the three
//          sweeps of rounds 1-3 were four dependent memory latencies per round of a workgroup: 1.86 ms at 10^7 rows
//          against 0.15 ms of traffic); adjacent lanes hold adjacent rows, so a wave reads one contiguous stretch
//   medium (<= kSmLong = 2048): a group of kSmLanes = 16 lanes, three sweeps, reductions inside the aligned group
//   long   the WHOLE workgroup (256 lanes, block-wide reductions): a hub row of 20 000 entries was 1 200 trips of its 16
//          lanes, one load in flight each
// The lanes of a workgroup vote per round through LDS: medium and long rows are queued there and worked off by groups /
// by everyone after the short rows.  Rows are dealt to workgroups in chunks of 16 (a hubs-first numbering does not put
// the 256 longest rows into workgroup 0).  Which queue slot a row gets does not enter its result: same bits every run.
constexpr int kSmLanes = 16;
constexpr int kSmShort = 16;
constexpr int kSmLong = 2048;

__device__ __forceinline__ float block_max_f32(float v, float* buf) {
  for (int off = kWave >> 1; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, kWave));
  if ((threadIdx.x & (kWave - 1)) == 0) buf[threadIdx.x / kWave] = v;
  __syncthreads();
  v = buf[0];
#pragma unroll
  for (int w = 1; w < kWavesPerBlock; ++w) v = fmaxf(v, buf[w]);
  __syncthreads();
  return v;
}

__device__ __forceinline__ float block_sum_f32(float v, float* buf) {
  for (int off = kWave >> 1; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0) buf[threadIdx.x / kWave] = v;
  __syncthreads();
  v = buf[0];
#pragma unroll
  for (int w = 1; w < kWavesPerBlock; ++w) v += buf[w];   // (wave order: the same bits every run)
  __syncthreads();
  return v;
}

// The row loop shared by the three kernels below.
//   short_row(r, e0, len): one lane, 0 < len <= short_max <= kSmShort (called divergently: no shuffles, no barriers
//                          inside); short_max = 0 sends every row to the groups
//   medium_rows(r, e0, e1, trips, sub): this 16-lane group's queued row (e0 == e1: none this trip; `trips` is the wave's
//                                       maximum, so the shuffles inside stay converged)
//   long_row(r, e0, e1, buf): the whole workgroup on one row (every thread calls it; buf: kWavesPerBlock floats)
template <class ShortRow, class MediumRows, class LongRow>
__device__ __forceinline__ void softmax_row_loop(const int32_t* __restrict__ rowptr, int64_t N, int short_max,
                                                 ShortRow short_row, MediumRows medium_rows, LongRow long_row) {
  __shared__ int med_s[kBlock], med_e0_s[kBlock], med_e1_s[kBlock];   // (row, first entry, end: no second trip to rowptr)
  __shared__ int long_s[kBlock];
  __shared__ int n_med_s, n_long_s;
  __shared__ float red_s[kWavesPerBlock];
  const int sub = threadIdx.x % kSmLanes, grp = threadIdx.x / kSmLanes;
  const int64_t per_round = (int64_t)gridDim.x * kBlock;
  const int64_t rounds = (N + per_round - 1) / per_round;   // the same for every lane: barriers and shuffles need everyone
  for (int64_t it = 0; it < rounds; ++it) {
    // chunks of 16 consecutive rows, dealt round-robin over the workgroups
    const int64_t r0 = it * per_round + ((int64_t)grp * gridDim.x + blockIdx.x) * kSmLanes + sub;
    const bool live = r0 < N;
    const int64_t r = live ? r0 : N - 1;
    const int e0 = live ? rowptr[r] : 0, e1 = live ? rowptr[r + 1] : 0;
    const int len = e1 - e0;
    if (threadIdx.x == 0) { n_med_s = 0; n_long_s = 0; }
    __syncthreads();
    if (len > kSmLong) long_s[atomicAdd(&n_long_s, 1)] = (int)r;
    else if (len > short_max) {
      const int slot = atomicAdd(&n_med_s, 1);
      med_s[slot] = (int)r; med_e0_s[slot] = e0; med_e1_s[slot] = e1;
    }
    __syncthreads();
    if (len > 0 && len <= short_max) short_row(r, e0, len);
    const int n_med = n_med_s, n_long = n_long_s;           // (block-uniform)
    for (int base = 0; base < n_med; base += kBlock / kSmLanes) {
      const int q = base + grp;
      const bool has = q < n_med;
      const int rm = has ? med_s[q] : 0;
      const int m0 = has ? med_e0_s[q] : 0, m1 = has ? med_e1_s[q] : 0;
      int trips = (m1 - m0 + kSmLanes - 1) / kSmLanes;
      for (int off = kSmLanes; off < kWave; off <<= 1) trips = max(trips, __shfl_xor(trips, off, kWave));
      medium_rows((int64_t)rm, m0, m1, trips, sub);
    }
    for (int q = 0; q < n_long; ++q) {
      const int rl = long_s[q];
      long_row((int64_t)rl, rowptr[rl], rowptr[rl + 1], red_s);
    }
    __syncthreads();                                        // the queues are rewritten by the next round
  }
}

__global__ __launch_bounds__(kBlock) void row_softmax_kernel(const int32_t* __restrict__ rowptr, int64_t N,
                                                             int32_t heads, const float* s, float* out) {
  softmax_row_loop(rowptr, N, kSmShort,
    [&](int64_t, int e0, int len) {
      for (int h = 0; h < heads; ++h) {
        float v[kSmShort];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < kSmShort; ++j) {
          v[j] = j < len ? s[(int64_t)(e0 + j) * heads + h] : -INFINITY;
          m = fmaxf(m, v[j]);
        }
        float z = 0.f;
#pragma unroll
        for (int j = 0; j < kSmShort; ++j) {
          v[j] = j < len ? expf(v[j] - m) : 0.f;
          z += v[j];
        }
#pragma unroll
        for (int j = 0; j < kSmShort; ++j)
          if (j < len) out[(int64_t)(e0 + j) * heads + h] = v[j] / z;
      }
    },
    [&](int64_t, int e0, int e1, int trips, int sub) {
      // the first kSmKeep trips (rows of up to 64 entries: 97 % of the medium rows) stay in registers — one load and one
      // store per entry; only the rest of a longer row is swept three times
      constexpr int kSmKeep = 4;
      for (int h = 0; h < heads; ++h) {
        float v[kSmKeep];
        float m = -INFINITY;
#pragma unroll
        for (int t = 0; t < kSmKeep; ++t) {
          const int e = e0 + t * kSmLanes + sub;
          v[t] = e < e1 ? s[(int64_t)e * heads + h] : -INFINITY;
          m = fmaxf(m, v[t]);
        }
        for (int t = kSmKeep; t < trips; ++t) {
          const int e = e0 + t * kSmLanes + sub;
          if (e < e1) m = fmaxf(m, s[(int64_t)e * heads + h]);
        }
        for (int off = kSmLanes >> 1; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, kWave));
        float z = 0.f;
#pragma unroll
        for (int t = 0; t < kSmKeep; ++t) {
          v[t] = e0 + t * kSmLanes + sub < e1 ? expf(v[t] - m) : 0.f;
          z += v[t];
        }
        for (int t = kSmKeep; t < trips; ++t) {
          const int e = e0 + t * kSmLanes + sub;
          if (e < e1) z += expf(s[(int64_t)e * heads + h] - m);
        }
        z = wave_sum_seg(z, kSmLanes);
#pragma unroll
        for (int t = 0; t < kSmKeep; ++t) {
          const int e = e0 + t * kSmLanes + sub;
          if (e < e1) out[(int64_t)e * heads + h] = v[t] / z;
        }
        for (int t = kSmKeep; t < trips; ++t) {
          const int e = e0 + t * kSmLanes + sub;
          if (e < e1) out[(int64_t)e * heads + h] = expf(s[(int64_t)e * heads + h] - m) / z;
        }
      }
    },
    [&](int64_t, int e0, int e1, float* buf) {
      for (int h = 0; h < heads; ++h) {
        float m = -INFINITY;
#pragma unroll 4
        for (int e = e0 + (int)threadIdx.x; e < e1; e += kBlock) m = fmaxf(m, s[(int64_t)e * heads + h]);
        m = block_max_f32(m, buf);
        float z = 0.f;
#pragma unroll 4
        for (int e = e0 + (int)threadIdx.x; e < e1; e += kBlock) z += expf(s[(int64_t)e * heads + h] - m);
        z = block_sum_f32(z, buf);
#pragma unroll 4
        for (int e = e0 + (int)threadIdx.x; e < e1; e += kBlock)
          out[(int64_t)e * heads + h] = expf(s[(int64_t)e * heads + h] - m) / z;
      }
    });
}

// Additive attention coefficients in one pass, all heads: alpha[e, h] = softmax over row r of
// leaky_relu(a_dst[r, h] + a_src[col[e], h])  (idconv.py:319-327; torch_geometric GATConv [3P]).  The scores are never
// stored: short rows compute them once into registers; the sweeps of the longer rows recompute them from the two
// per-node terms, which sit in L2.  Replaces one sddmm_add launch per head + a concatenation + the row softmax of round 1.
// EDGE (mp_edge_att_alpha_f32; attconv.py:342-357): the score has a third term a_edge[eid[e], h], one more scalar gather
// through the entry's input position, loaded next to col (eid < 0: no such term), and a_dst may be absent.
template <bool EDGE>
struct AlphaScore {
  const int32_t* __restrict__ col;
  const int32_t* __restrict__ eid;
  const float* __restrict__ a_dst;
  const float* __restrict__ a_src;
  const float* __restrict__ a_edge;
  int32_t heads;
  float slope;

  __device__ __forceinline__ float dst(int64_t r, int h) const {
    if constexpr (EDGE) return a_dst ? a_dst[r * heads + h] : 0.f;
    else return a_dst[r * heads + h];
  }
  // the pre-activation of an entry with source c and input position ei, then the leaky ReLU
  __device__ __forceinline__ float of(float ad, int c, int ei, int h) const {
    float v = ad + a_src[(int64_t)c * heads + h];
    if constexpr (EDGE) v += ei >= 0 ? a_edge[(int64_t)ei * heads + h] : 0.f;
    return v > 0.f ? v : slope * v;
  }
  __device__ __forceinline__ float at(float ad, int e, int h) const {
    if constexpr (EDGE) return of(ad, col[e], eid[e], h);
    else return of(ad, col[e], -1, h);
  }
};

template <bool EDGE>
__global__ __launch_bounds__(kBlock) void gat_alpha_kernel(const int32_t* __restrict__ rowptr, int64_t N,
                                                           AlphaScore<EDGE> sc, float* out) {
  const int heads = sc.heads;
  softmax_row_loop(rowptr, N, kSmShort,
    [&](int64_t r, int e0, int len) {
      int c[kSmShort];
      int ei[EDGE ? kSmShort : 1];
#pragma unroll
      for (int j = 0; j < kSmShort; ++j) {
        c[j] = j < len ? sc.col[e0 + j] : 0;
        if constexpr (EDGE) ei[j] = j < len ? sc.eid[e0 + j] : -1;
      }
      for (int h = 0; h < heads; ++h) {
        const float ad = sc.dst(r, h);
        float v[kSmShort];
        float m = -INFINITY;
#pragma unroll
        for (int j = 0; j < kSmShort; ++j) {
          int eij = -1;
          if constexpr (EDGE) eij = ei[j];
          const float t = sc.of(ad, c[j], eij, h);
          v[j] = j < len ? t : -INFINITY;
          m = fmaxf(m, v[j]);
        }
        float z = 0.f;
#pragma unroll
        for (int j = 0; j < kSmShort; ++j) {
          v[j] = j < len ? expf(v[j] - m) : 0.f;
          z += v[j];
        }
#pragma unroll
        for (int j = 0; j < kSmShort; ++j)
          if (j < len) out[(int64_t)(e0 + j) * heads + h] = v[j] / z;
      }
    },
    [&](int64_t r, int e0, int e1, int trips, int sub) {
      for (int h = 0; h < heads; ++h) {
        const float ad = sc.dst(r, h);
        float m = -INFINITY;
        for (int t = 0; t < trips; ++t) {
          const int e = e0 + t * kSmLanes + sub;
          if (e < e1) m = fmaxf(m, sc.at(ad, e, h));
        }
        for (int off = kSmLanes >> 1; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, kWave));
        float z = 0.f;
        for (int t = 0; t < trips; ++t) {
          const int e = e0 + t * kSmLanes + sub;
          if (e < e1) z += expf(sc.at(ad, e, h) - m);
        }
        z = wave_sum_seg(z, kSmLanes);
        for (int t = 0; t < trips; ++t) {
          const int e = e0 + t * kSmLanes + sub;
          if (e < e1) out[(int64_t)e * heads + h] = expf(sc.at(ad, e, h) - m) / z;
        }
      }
    },
    [&](int64_t r, int e0, int e1, float* buf) {
      for (int h = 0; h < heads; ++h) {
        const float ad = sc.dst(r, h);
        float m = -INFINITY;
#pragma unroll 4
        for (int e = e0 + (int)threadIdx.x; e < e1; e += kBlock) m = fmaxf(m, sc.at(ad, e, h));
        m = block_max_f32(m, buf);
        float z = 0.f;
#pragma unroll 4
        for (int e = e0 + (int)threadIdx.x; e < e1; e += kBlock) z += expf(sc.at(ad, e, h) - m);
        z = block_sum_f32(z, buf);
#pragma unroll 4
        for (int e = e0 + (int)threadIdx.x; e < e1; e += kBlock)
          out[(int64_t)e * heads + h] = expf(sc.at(ad, e, h) - m) / z;
      }
    });
}

// ds = p * (dp - sum_row(p * dp))
__global__ __launch_bounds__(kBlock) void row_softmax_bwd_kernel(const int32_t* __restrict__ rowptr,
                                                                 int64_t N, int32_t heads,
                                                                 const float* __restrict__ p,
                                                                 const float* __restrict__ dp, float* ds) {
  // (several heads: a lane per row walks its entries once per head with a stride of `heads` — 5.3 against 4.5 ms at four
  // heads; the groups take every row there)
  softmax_row_loop(rowptr, N, heads == 1 ? kSmShort : 0,
    [&](int64_t, int e0, int len) {
      for (int h = 0; h < heads; ++h) {
        float pv[kSmShort], dv[kSmShort];
        float t = 0.f;
#pragma unroll
        for (int j = 0; j < kSmShort; ++j) {
          pv[j] = j < len ? p[(int64_t)(e0 + j) * heads + h] : 0.f;
          dv[j] = j < len ? dp[(int64_t)(e0 + j) * heads + h] : 0.f;
          t = fmaf(pv[j], dv[j], t);
        }
#pragma unroll
        for (int j = 0; j < kSmShort; ++j)
          if (j < len) ds[(int64_t)(e0 + j) * heads + h] = pv[j] * (dv[j] - t);
      }
    },
    [&](int64_t, int e0, int e1, int trips, int sub) {
      for (int h = 0; h < heads; ++h) {
        float t = 0.f;
        for (int k = 0; k < trips; ++k) {
          const int e = e0 + k * kSmLanes + sub;
          if (e < e1) t = fmaf(p[(int64_t)e * heads + h], dp[(int64_t)e * heads + h], t);
        }
        t = wave_sum_seg(t, kSmLanes);
        for (int k = 0; k < trips; ++k) {
          const int e = e0 + k * kSmLanes + sub;
          if (e < e1) {
            const int64_t i = (int64_t)e * heads + h;
            ds[i] = p[i] * (dp[i] - t);
          }
        }
      }
    },
    [&](int64_t, int e0, int e1, float* buf) {
      for (int h = 0; h < heads; ++h) {
        float t = 0.f;
#pragma unroll 4
        for (int e = e0 + (int)threadIdx.x; e < e1; e += kBlock)
          t = fmaf(p[(int64_t)e * heads + h], dp[(int64_t)e * heads + h], t);
        t = block_sum_f32(t, buf);
#pragma unroll 4
        for (int e = e0 + (int)threadIdx.x; e < e1; e += kBlock) {
          const int64_t i = (int64_t)e * heads + h;
          ds[i] = p[i] * (dp[i] - t);
        }
      }
    });
}

static bool al(const void* p, size_t a) { return ((uintptr_t)p % a) == 0; }

// the entry-balanced launch of both forms: widest vector every operand allows, no wider than the row needs
template <bool MASK>
static int sddmm_stream_launch(const int32_t* row_of, const int32_t* col, int64_t nnz, const float* Am, int64_t lda,
                               const float* Bm, int64_t ldb, int32_t d, int32_t heads, float scale, float* s,
                               const int32_t* argmax, int64_t ldm, hipStream_t st) {
  const int dh = d / heads;
  int w = 4;
  auto ok = [&](int ww) {
    return d % ww == 0 && dh % ww == 0 && lda % ww == 0 && ldb % ww == 0 && al(Am, 4u * ww) && al(Bm, 4u * ww) &&
           (!MASK || (ldm % ww == 0 && al(argmax, 4u * ww)));
  };
  while (w > 1 && !ok(w)) w >>= 1;
  while (w > 1 && kWave * (w / 2) >= d) w >>= 1;
  if (heads > 1) {
    const int gs = dh / w;   // lanes per head must be a power of two inside one wave-wide tile
    if (d > kWave * w || gs < 1 || (gs & (gs - 1)) || kWave % gs) return MP_ERR_UNSUPPORTED;
  }
  const int64_t waves = ceil_div(nnz, kStream);
  dim3 grid((unsigned)ceil_div(waves, kWavesPerBlock));
  switch (w) {
    case 4: hipLaunchKernelGGL((sddmm_stream_kernel<4, 4, MASK>), grid, dim3(kBlock), 0, st, row_of, col, nnz, Am, lda, Bm, ldb, d, heads, scale, s, argmax, ldm); break;
    case 2: hipLaunchKernelGGL((sddmm_stream_kernel<2, 4, MASK>), grid, dim3(kBlock), 0, st, row_of, col, nnz, Am, lda, Bm, ldb, d, heads, scale, s, argmax, ldm); break;
    default: hipLaunchKernelGGL((sddmm_stream_kernel<1, 4, MASK>), grid, dim3(kBlock), 0, st, row_of, col, nnz, Am, lda, Bm, ldb, d, heads, scale, s, argmax, ldm); break;
  }
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // namespace mp

using namespace mp;

extern "C" {

int mp_sddmm_dot_f32(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, const float* Qm,
                     int64_t ldq, const float* Km, int64_t ldk, int32_t d, int32_t heads, float scale,
                     float* s, mp_stream_t stream) {
  if (!rowptr || N < 0 || nnz < 0 || d <= 0 || heads <= 0 || d % heads) return MP_ERR_INVALID_ARG;
  if (nnz > 0 && (!col || !Qm || !Km || !s)) return MP_ERR_INVALID_ARG;
  if (ldq < d || ldk < d) return MP_ERR_INVALID_ARG;
  if (N == 0 || nnz == 0) return MP_OK;
  hipLaunchKernelGGL(sddmm_dot_kernel, dim3(row_grid(N)), dim3(kBlock), 0, as_stream(stream), rowptr, col, N,
                     Qm, ldq, Km, ldk, d, heads, scale, s);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_sddmm_dot_stream_f32(const int32_t* row_of, const int32_t* col, int64_t nnz, const float* Am,
                            int64_t lda, const float* Bm, int64_t ldb, int32_t d, int32_t heads, float scale,
                            float* s, mp_stream_t stream) {
  if (nnz < 0 || d <= 0 || heads <= 0 || d % heads) return MP_ERR_INVALID_ARG;
  if (nnz == 0) return MP_OK;
  if (!row_of || !col || !Am || !Bm || !s || lda < d || ldb < d) return MP_ERR_INVALID_ARG;
  return sddmm_stream_launch<false>(row_of, col, nnz, Am, lda, Bm, ldb, d, heads, scale, s, nullptr, 0,
                                    as_stream(stream));
}

int mp_spmm_heads_max_da_f32(const int32_t* row_of, const int32_t* col, int64_t nnz, const int32_t* argmax,
                             int64_t ldm, const float* dY, int64_t ldy, const float* V, int64_t ldv, int32_t d,
                             int32_t heads, float* da, mp_stream_t stream) {
  if (nnz < 0 || d <= 0 || heads < 1 || d % heads) return MP_ERR_INVALID_ARG;
  if (ldm < d || ldy < d || ldv < d) return MP_ERR_INVALID_ARG;
  if (nnz >= INT32_MAX) return MP_ERR_UNSUPPORTED;
  if (nnz == 0) return MP_OK;         // no entry: the per-entry arrays (and those of an operator without rows) may be NULL
  if (!row_of || !col || !argmax || !dY || !V || !da) return MP_ERR_INVALID_ARG;
  return sddmm_stream_launch<true>(row_of, col, nnz, dY, ldy, V, ldv, d, heads, 1.0f, da, argmax, ldm,
                                   as_stream(stream));
}

int mp_sddmm_add_f32(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, const float* ai,
                     const float* aj, float slope, float* s, mp_stream_t stream) {
  if (!rowptr || N < 0 || nnz < 0) return MP_ERR_INVALID_ARG;
  if (nnz > 0 && (!col || !ai || !aj || !s)) return MP_ERR_INVALID_ARG;
  if (N == 0 || nnz == 0) return MP_OK;
  hipLaunchKernelGGL(sddmm_add_kernel, dim3(row_grid(N)), dim3(kBlock), 0, as_stream(stream), rowptr, col, N,
                     ai, aj, slope, s);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_csr_row_softmax_f32(const int32_t* rowptr, int64_t N, int32_t heads, const float* s, float* out,
                           mp_stream_t stream) {
  if (!rowptr || N < 0 || heads <= 0) return MP_ERR_INVALID_ARG;
  if (N == 0) return MP_OK;
  if (!s || !out) return MP_ERR_INVALID_ARG;
  hipLaunchKernelGGL(row_softmax_kernel, dim3(flat_grid(N)), dim3(kBlock), 0, as_stream(stream), rowptr, N,
                     heads, s, out);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_gat_alpha_f32(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, int32_t heads,
                     const float* a_dst, const float* a_src, float slope, float* alpha, mp_stream_t stream) {
  if (!rowptr || N < 0 || nnz < 0 || heads < 1 || (nnz > 0 && (!col || !a_dst || !a_src || !alpha)))
    return MP_ERR_INVALID_ARG;
  if (N == 0 || nnz == 0) return MP_OK;
  const AlphaScore<false> sc = {col, nullptr, a_dst, a_src, nullptr, heads, slope};
  hipLaunchKernelGGL(gat_alpha_kernel<false>, dim3(flat_grid(N)), dim3(kBlock), 0, as_stream(stream), rowptr, N, sc,
                     alpha);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_edge_att_alpha_f32(const int32_t* rowptr, const int32_t* col, const int32_t* eid, int64_t N, int64_t nnz,
                          int32_t heads, const float* a_dst, const float* a_src, const float* a_edge, float slope,
                          float* alpha, mp_stream_t stream) {
  if (!rowptr || N < 0 || nnz < 0 || heads < 1 || (nnz > 0 && (!col || !eid || !a_src || !a_edge || !alpha)))
    return MP_ERR_INVALID_ARG;
  if (N >= INT32_MAX || nnz >= INT32_MAX) return MP_ERR_UNSUPPORTED;
  if (N == 0 || nnz == 0) return MP_OK;
  const AlphaScore<true> sc = {col, eid, a_dst, a_src, a_edge, heads, slope};
  hipLaunchKernelGGL(gat_alpha_kernel<true>, dim3(flat_grid(N)), dim3(kBlock), 0, as_stream(stream), rowptr, N, sc,
                     alpha);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

int mp_csr_row_softmax_bwd_f32(const int32_t* rowptr, int64_t N, int32_t heads, const float* p,
                               const float* dp, float* ds, mp_stream_t stream) {
  if (!rowptr || N < 0 || heads <= 0) return MP_ERR_INVALID_ARG;
  if (N == 0) return MP_OK;
  if (!p || !dp || !ds) return MP_ERR_INVALID_ARG;
  hipLaunchKernelGGL(row_softmax_bwd_kernel, dim3(flat_grid(N)), dim3(kBlock), 0, as_stream(stream), rowptr, N,
                     heads, p, dp, ds);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // extern "C"
