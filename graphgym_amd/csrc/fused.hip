// Aggregate -> transform in one kernel:   out = act( (A X [+ s * S]) W + bias )
// i.e. SparseAdj.matmul followed by the layer's kernel product (TfgIDLayer.py:510-523 in the
// aggregate-first order, GIN's (1 + eps) x + sum -> first Linear, idconv.py:371-399) without the
// [N, F] intermediate making a round trip through HBM, and with the MFMA work of one row tile
// running while the other workgroups of the compute unit are still gathering theirs.
//
// Measured background (profiles/r01_overlap.log): the gather kernel reaches 88 % of its full-chip
// rate on half of the compute units — it is bound by HBM, not by issue slots — so the matrix cores
// of every CU are idle most of the time; a separate GEMM then needs its own 11 ms.  Here:
//   * a workgroup (4 waves) owns a tile of 32 consecutive destination rows;
//   * phase A: the tile's stored entries are split into four equal runs, one per wave (a row cut
//     by a run boundary is finished through a carry row, added in wave order => bitwise
//     reproducible); each wave walks its run exactly like the aggregation kernel (64 indices per
//     coalesced load, one v_readlane broadcast per entry, 1 KiB row loads, MP_FUSED_U in flight) and
//     leaves the reduced rows in LDS;
//   * phase B: the 32 x F tile in LDS times W on the matrix cores (v_mfma_f32_32x32x2_f32, exact
//     fp32 fma chain): each wave owns 64 output columns, B fragments come straight from W in L2
//     (256 KiB, resident in every XCD's L2) as 8-byte loads, bias + activation fused into the store.
// 36 KiB LDS per workgroup => 4 workgroups per CU: while one multiplies, three gather.
//
// F = 512 (config C5's width) runs as two K halves over the same 32-row tile: gather columns 0..255 of the
// neighbour rows, multiply by W[0:256], gather columns 256..511, multiply by W[256:512] into the same
// accumulators (the accumulators of all output column blocks stay in registers: d_out <= 512).
//
// The identity branch of the ID layers (out = A (X W + S X W_id), TfgIDLayer.py:510-517, idconv.py:150-177)
// needs no second tile here: A S X W_id = A_id Z with Z = X[id] W_id (n_id rows, a small product) and A_id the
// entries whose source is an identity node.  The main kernel leaves rows that own such an entry un-activated
// (`defer_act`), and id_fixup_kernel adds A_id Z to exactly those rows and applies the activation.
#include "fused_pc.h"
#include <map>
#include <mutex>
#include <utility>

namespace mp {

constexpr int kTileRows = 32;

// The one-role kernel: every wave of a workgroup gathers, then multiplies.  Since round 3 it serves the shapes the
// producer/consumer kernel (fused_pc.h) is not built for: see launch_fused.
// W: floats per lane of one K half (half width FH = 64 W); KH: K halves (F = KH * FH); NCB: output column blocks of
// 256 whose accumulators stay live across the halves (KH == 2 only; KH == 1 walks the blocks one after another);
// PF: W fragments fetched PF K-groups ahead
template <int W, bool WEIGHTED, int KH, int NCB, int PF, bool BF16X3>
__global__ __launch_bounds__(kBlock, KH == 2 ? 3 : 4) void agg_dense_kernel(FusedArgs a) {
  constexpr int FH = kWave * W;
  constexpr int LDT = FH + 4;   // row stride of the tile: 16-byte aligned rows, conflict-free b128 fragment reads
  __shared__ __attribute__((aligned(16))) float T[kTileRows][LDT];
  __shared__ __attribute__((aligned(16))) float carry[kWavesPerBlock - 1][FH];
  __shared__ int carry_row[kWavesPerBlock];
  __shared__ float inv_deg[kTileRows];
  __shared__ int defer_l[kTileRows];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // A workgroup walks tiles blockIdx.x, blockIdx.x + gridDim.x, ... (kFusedMaxGrid workgroups at most: ~5 tiles each at
  // 10^7 rows).  Fewer, longer-lived workgroups: -1.7 % (out only) / -4 % (aggregated rows kept) against one workgroup
  // per tile in an in-process A/B; a smaller grid loses to the hub tiles at the head of the matrix (1024 workgroups:
  // +14 %).  Tiles are independent and a tile's summation order does not depend on who computes it: same bits.
  // (KH == 2 — F = 512 — keeps one tile per workgroup: with the tile loop its 164 registers spill)
  for (int tile = blockIdx.x; (int64_t)tile * kTileRows < a.N; tile += gridDim.x) {
  const int R0 = tile * kTileRows;
  const int R1 = min(R0 + kTileRows, a.N);

  // ---- the wave's run of entries (the same for every K half) ----
  // lane i (<= 32) holds the start of tile row i (rows past the end of the matrix are empty)
  const int rp_v = lane <= kTileRows ? a.rowptr[min(R0 + lane, R1)] : INT_MAX;
  if (wave == 0) {   // 1 / (entries of the row): lane i sees the starts of rows i and i + 1
    const int nxt = __shfl_down(rp_v, 1, kWave);
    if (lane < kTileRows) {
      inv_deg[lane] = (a.mean && nxt > rp_v) ? 1.0f / (float)(nxt - rp_v) : (a.mean ? 0.f : 1.f);
      defer_l[lane] = (a.defer_act != nullptr && R0 + lane < R1) ? (int)a.defer_act[R0 + lane] : 0;
    }
  }
  const int E0 = bcast_i(rp_v, 0);
  const int E1 = bcast_i(rp_v, kTileRows);
  const int q = (E1 - E0 + kWavesPerBlock - 1) / kWavesPerBlock;
  const int es = min(E0 + wave * q, E1);
  const int ee = min(es + q, E1);
  int first_rl = -1;
  bool cont = false;
  if (es < ee) {
    const unsigned long long started = __ballot(lane >= 1 && lane <= kTileRows && rp_v <= es);
    first_rl = __builtin_amdgcn_readfirstlane((int)__popcll(started));
    cont = bcast_i(rp_v, first_rl) < es;
  }
  if (lane == 0) carry_row[wave] = cont ? first_rl : -1;

  const int fr = lane & 31, kk = lane >> 5;
  const int fr_c = fr, kk_c = kk;   // (for the epilogue: MP_DEFINE_STORE_BLOCK)
  f32x16 acc[KH == 2 ? NCB : 1][1][2];   // ([column block][one 32-row block][column tile]: the shape of mfma_rows*)
  if constexpr (KH == 2) {
#pragma unroll
    for (int b = 0; b < NCB; ++b)
#pragma unroll
      for (int r = 0; r < 16; ++r) { acc[b][0][0][r] = 0.f; acc[b][0][1][r] = 0.f; }
  }

  MP_DEFINE_STORE_BLOCK(inv_deg, defer_l, R0, R1);

#pragma unroll
  for (int kh = 0; kh < KH; ++kh) {
    const int k0 = kh * FH;   // first feature column of this half
    // ---- init: T = self_scale * S rows (or zeros; rows past N stay zero) ----
    {
      constexpr int VPR = FH / 4;                 // float4 per row
      for (int i = tid; i < kTileRows * VPR; i += kBlock) {
        const int m = i / VPR, c = (i % VPR) * 4;
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (a.S != nullptr && R0 + m < R1) {
          v = *reinterpret_cast<const f32x4*>(a.S + (int64_t)(R0 + m) * a.lds + k0 + c);
          v *= a.self_scale;
        }
        *reinterpret_cast<f32x4*>(&T[m][c]) = v;
      }
    }
    __syncthreads();   // T initialised (and carry_row / inv_deg / defer_l visible)

    // ---- phase A: this wave's run of entries, feature columns [k0, k0 + FH) ----
    if (es < ee) {
      const float* __restrict__ xlane = a.X + k0 + lane * W;
      int rl = first_rl;
      int rend = bcast_i(rp_v, rl + 1);
      float accr[W];
#pragma unroll
      for (int k = 0; k < W; ++k) accr[k] = 0.f;

      auto flush = [&]() {
        if (cont && rl == first_rl) {
          store_vec<W>(&carry[wave - 1][lane * W], accr);
        } else {
          float t[W];
          load_vec<W>(&T[rl][lane * W], t);
#pragma unroll
          for (int k = 0; k < W; ++k) t[k] += accr[k];
          store_vec<W>(&T[rl][lane * W], t);
        }
#pragma unroll
        for (int k = 0; k < W; ++k) accr[k] = 0.f;
      };

      for (int ec = es; ec < ee; ec += kWave) {
        const int me = min(ec + lane, ee - 1);
        const int cv = a.col[me] & 0x7fffffff;   // an identity mark (sign bit) is not part of the index
        float wv = 1.f;
        if (WEIGHTED) wv = a.val[me];
        const int n = min(kWave, ee - ec);
        for (int jb = 0; jb < n; jb += MP_FUSED_U) {
          float v[MP_FUSED_U][W];
#pragma unroll
          for (int j = 0; j < MP_FUSED_U; ++j) {
            const int c = bcast_i(cv, jb + j);
            load_vec<W>(xlane + (int64_t)c * a.ldx, v[j]);
          }
#pragma unroll
          for (int j = 0; j < MP_FUSED_U; ++j) {
            const int e = ec + jb + j;
            if (e < ee) {
              while (e >= rend) {
                flush();
                rl += 1;
                rend = bcast_i(rp_v, rl + 1);
              }
              const float w = WEIGHTED ? bcast_f(wv, jb + j) : 1.f;
#pragma unroll
              for (int k = 0; k < W; ++k) accr[k] = fmaf(w, v[j][k], accr[k]);
            }
          }
        }
      }
      flush();
    }
    __syncthreads();

    // ---- carries: a row cut by run boundaries gets its later parts in wave order ----
    if (tid < FH) {
#pragma unroll
      for (int w = 1; w < kWavesPerBlock; ++w) {
        const int cr = carry_row[w];
        if (cr >= 0) T[cr][tid] += carry[w - 1][tid];
      }
    }
    __syncthreads();

    if (a.P != nullptr) {   // the aggregated rows, kept for the weight gradient
      constexpr int VPR = FH / 4;
      for (int i = tid; i < kTileRows * VPR; i += kBlock) {
        const int m = i / VPR, c = (i % VPR) * 4;
        if (R0 + m < R1) {
          f32x4 v = *reinterpret_cast<const f32x4*>(&T[m][c]);
          v *= inv_deg[m];
          __builtin_nontemporal_store(v, reinterpret_cast<f32x4*>(a.P + (int64_t)(R0 + m) * a.ldp + k0 + c));
        }
      }
    }
    // ---- phase B: [32 x FH] tile x W[k0 : k0 + FH, :] on the matrix cores ----
    if constexpr (KH == 1) {
      for (int cb = 0; cb < a.dout; cb += 64 * kWavesPerBlock) {
        const int n0 = cb + wave * 64;
        if (n0 >= a.dout) break;                       // wave-uniform
        const int cpair = n0 + 2 * fr;
        const int ccol = cpair < a.dout ? cpair : a.dout - 2;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc[0][0][0][r] = 0.f; acc[0][0][1][r] = 0.f; }
        if constexpr (BF16X3) {
          const __bf16* w0 = a.Wsp + ((int64_t)kk * a.dout + ccol) * 8;
          mfma_rows_bf16x3<FH, 1, 1>(T, w0, 0, (int64_t)a.dout * 16, (int64_t)a.dout * a.ldws, acc, fr, kk);
        } else {
          const float* __restrict__ wp = a.Wm + (int64_t)(4 * kk) * a.ldw + ccol;
          mfma_rows<FH, PF, 1>(T, wp, a.ldw, acc[0], fr, kk);
        }
        store_block(acc[0][0][0], acc[0][0][1], n0, 0);
      }
    } else {
#pragma unroll
      for (int b = 0; b < NCB; ++b) {
        const int n0 = b * 64 * kWavesPerBlock + wave * 64;
        if (n0 < a.dout) {                             // wave-uniform
          const int cpair = n0 + 2 * fr;
          const int ccol = cpair < a.dout ? cpair : a.dout - 2;
          if constexpr (BF16X3) {
            const __bf16* w0 = a.Wsp + ((int64_t)(k0 / 8 + kk) * a.dout + ccol) * 8;
            f32x16 one[1][1][2] = {{{acc[b][0][0], acc[b][0][1]}}};   // (a copy in registers: a cast of acc[b] would put all of acc in scratch)
            mfma_rows_bf16x3<FH, 1, 1>(T, w0, 0, (int64_t)a.dout * 16, (int64_t)a.dout * a.ldws, one, fr, kk);
            acc[b][0][0] = one[0][0][0]; acc[b][0][1] = one[0][0][1];
          } else {
            const float* __restrict__ wp = a.Wm + (int64_t)(k0 + 4 * kk) * a.ldw + ccol;
            mfma_rows<FH, PF, 1>(T, wp, a.ldw, acc[b], fr, kk);
          }
        }
      }
      if (kh + 1 < KH) __syncthreads();   // every wave has read T before the next half re-initialises it
    }
  }
  if constexpr (KH == 2) {
#pragma unroll
    for (int b = 0; b < NCB; ++b) {
      const int n0 = b * 64 * kWavesPerBlock + wave * 64;
      if (n0 < a.dout) store_block(acc[b][0][0], acc[b][0][1], n0, 0);
    }
  }
  if constexpr (KH == 2) break;
  __syncthreads();   // every wave is done with T, carry_row, inv_deg before the next tile rewrites them
  }
}

__device__ unsigned int g_pc_tile_ctr[kPcSlots];

constexpr int kFusedMaxGrid = 65536;

template <int W, int KH, int NCB, int PF>
static int launch_fused_tiles(const FusedArgs& a, hipStream_t st) {   // one workgroup walks tiles b, b + grid, ... (round 2 form)
  const int64_t n_tiles = ceil_div(a.N, kTileRows);
  const dim3 grid((unsigned)(KH == 2 || n_tiles < kFusedMaxGrid ? n_tiles : kFusedMaxGrid)), block(kBlock);
  with_bools(a.val != nullptr, a.Wsp != nullptr, [&](auto weighted, auto bf16x3) {
    hipLaunchKernelGGL((agg_dense_kernel<W, decltype(weighted)::value, KH, NCB, PF, decltype(bf16x3)::value>), grid, block,
                       0, st, a);
  });
  MP_LAUNCH_CHECK();
  return MP_OK;
}

// (declared in fused_pc.h, with what a slot is)
int pc_counter(unsigned int** ctr, hipStream_t st) {
  static std::mutex mu;
  static unsigned int* base[kMaxDevPc] = {nullptr};
  static int next_slot[kMaxDevPc] = {0};
  static std::map<std::pair<int, hipStream_t>, int> slot_of;
  int dev = 0;
  MP_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= kMaxDevPc) return MP_ERR_UNSUPPORTED;
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  if (st != nullptr) MP_HIP(hipStreamIsCapturing(st, &cap));
  int slot = -1;
  {
    std::lock_guard<std::mutex> lock(mu);
    if (!base[dev]) {
      void* p = nullptr;
      MP_HIP(hipGetSymbolAddress(&p, HIP_SYMBOL(g_pc_tile_ctr)));
      base[dev] = reinterpret_cast<unsigned int*>(p);
    }
    if (cap == hipStreamCaptureStatusActive) {
      if (next_slot[dev] < kPcSlots) slot = next_slot[dev]++;
    } else {
      auto key = std::make_pair(dev, st);
      auto it = slot_of.find(key);
      if (it != slot_of.end()) {
        slot = it->second;
      } else if (next_slot[dev] < kPcSlots) {
        slot = next_slot[dev]++;
        slot_of[key] = slot;
      }
    }
  }
  if (slot < 0) return MP_ERR_UNSUPPORTED;
  *ctr = base[dev] + slot;
  MP_HIP(hipMemsetAsync(*ctr, 0, sizeof(unsigned int), st));
  return MP_OK;
}

template <int W, int KH, int NCB, int PF, int TR, int NP, int NC, bool HAS_S>
static int launch_fused_pc_s(const FusedArgs& a, hipStream_t st) {
  PcLaunch p;
  const int rc = pc_launch(a.N, TR, st, &p);
  if (rc != MP_OK) return rc;
  with_bools(a.val != nullptr, a.Wsp != nullptr, [&](auto weighted, auto bf16x3) {
    hipLaunchKernelGGL((agg_dense_pc_kernel<W, decltype(weighted)::value, KH, NCB, PF, decltype(bf16x3)::value, TR, NP, NC,
                                            HAS_S>),
                       p.grid, dim3((NP + NC) * kWave), 0, st, a, p.ctr, p.n_tiles);
  });
  MP_LAUNCH_CHECK();
  return MP_OK;
}

// SELF_OK: the self-term form of this shape is built (it holds TR / NP rows of S in registers: not every shape has them)
template <int W, int KH, int NCB, int PF, int TR, int NP, int NC, bool SELF_OK = false>
static int launch_fused_pc(const FusedArgs& a, hipStream_t st) {
  if (a.S == nullptr) return launch_fused_pc_s<W, KH, NCB, PF, TR, NP, NC, false>(a, st);
  if constexpr (SELF_OK) return launch_fused_pc_s<W, KH, NCB, PF, TR, NP, NC, true>(a, st);
  else return launch_fused_tiles<W, KH, NCB, PF>(a, st);
}

// Dispatch.  F >= 256: tiles of 64 rows, 4 gathering + 4 multiplying waves, one workgroup per CU.  In-process A/B at
// 10^7 rows, 1.1 x 10^8 entries (profiles/r03_fused_variants.json), out only / aggregated rows kept:
//   F = 256: one-role kernel 23.7 / 24.6 ms, 32 rows x 4 producers 22.5 / 24.3, 64 x 2 24.6 / 25.9, 64 x 4 20.97 / 22.98,
//            64 x 6 21.8 / 23.9, 64 x 8 22.0 / 24.6 (plain aggregation alone: 20.7);   F = 512: 57.4 / 56.3 (32 x 4) / 53.2.
// Narrower layers keep 32-row tiles: their buffers are small enough for two workgroups per CU either way.
template <int W, int KH, int NCB, int PF>
static int launch_fused(const FusedArgs& a, hipStream_t st) {
  if constexpr (W == 4) {
    if constexpr (KH == 1) {
      if (a.dout > 256 && a.S != nullptr) return launch_fused_tiles<W, KH, NCB, PF>(a, st);   // (no self-term form with 8 consumers)
      // small operators: 32-row tiles (twice the workgroups: 2 x 10^5 rows 0.57 vs 0.71 ms; 10^6 rows 2.13 vs 2.09)
      if (a.N < (1 << 19) && a.dout <= 256) return launch_fused_pc<W, KH, NCB, PF, 32, 4, 4, true>(a, st);
      if (a.dout > 256) return launch_fused_pc<W, KH, 1, PF, 64, 4, 8>(a, st);   // one column block per consumer wave
      return launch_fused_pc<W, KH, 1, PF, 64, 4, 4, true>(a, st);
    } else {
      // F = 512 -> 512: the accumulators live across the K halves.  Eight multiplying waves with one 64-column block each
      // (152 registers; 168 + 20 B of scratch with the self term) against four with two blocks walking K together
      // (rounds 2-3: the one-block form spilled then): 50.8 vs 51.6 ms, with the self term 52.1 vs 52.7 — round 4, same
      // process and buffers, same bits
      if (a.dout == 512) return launch_fused_pc<W, KH, 1, PF, 64, 4, 8, true>(a, st);
      if (a.dout > 256) return launch_fused_tiles<W, KH, NCB, PF>(a, st);   // (a ragged second block: the one-role kernel)
      return launch_fused_pc<W, KH, 1, PF, 64, 4, 4, true>(a, st);
    }
  } else {
    return launch_fused_pc<W, KH, NCB, PF, 32, 4, 4, true>(a, st);
  }
}

// out[rows[k], :] = act(out[rows[k], :] + sum_{e in [crp[k], crp[k+1])} val[e] * Z[slot[e], :]) — one wave per
// listed row (a few entries each), columns in 16-byte pieces where the alignment allows
// SET: out[rows[k], :] = the sum alone (the row's previous contents are not read)
template <int VW, bool SET = false>
__global__ __launch_bounds__(kBlock) void id_fixup_kernel(const int32_t* __restrict__ rows,
                                                          const int32_t* __restrict__ crp,
                                                          const int32_t* __restrict__ slot,
                                                          const float* __restrict__ val, int32_t n_rows,
                                                          const float* __restrict__ Z, int64_t ldz, float* out,
                                                          int64_t ldo, int32_t d, int32_t act) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (int k = blockIdx.x * kWavesPerBlock + wave; k < n_rows; k += gridDim.x * kWavesPerBlock) {
    const int r = rows[k];
    const int e0 = crp[k], e1 = crp[k + 1];
    for (int c0 = lane * VW; c0 < d; c0 += kWave * VW) {
      float acc[VW];
      if constexpr (SET) {
#pragma unroll
        for (int i = 0; i < VW; ++i) acc[i] = 0.f;
      } else {
        load_vec<VW>(out + (int64_t)r * ldo + c0, acc);
      }
      for (int e = e0; e < e1; ++e) {
        float z[VW];
        load_vec<VW>(Z + (int64_t)slot[e] * ldz + c0, z);
        const float w = val ? val[e] : 1.f;
#pragma unroll
        for (int i = 0; i < VW; ++i) acc[i] = fmaf(w, z[i], acc[i]);
      }
      if (act == MP_ACT_RELU) {
#pragma unroll
        for (int i = 0; i < VW; ++i) acc[i] = fmaxf(acc[i], 0.f);
      }
      store_vec<VW>(out + (int64_t)r * ldo + c0, acc);
    }
  }
}

// SET: the rows are written (mp_id_rows_f32, no activation); otherwise added to and activated (mp_id_fixup_f32)
template <bool SET>
static int launch_id_fixup(const int32_t* rows, const int32_t* crp, const int32_t* slot, const float* val, int64_t n_rows,
                           const float* Z, int64_t ldz, float* out, int64_t ldo, int32_t d, int act, hipStream_t st) {
  const int blocks = row_grid(n_rows);
  const bool v4 = d % 4 == 0 && ldz % 4 == 0 && ldo % 4 == 0 && ((uintptr_t)Z % 16) == 0 && ((uintptr_t)out % 16) == 0;
  if (v4)
    hipLaunchKernelGGL((id_fixup_kernel<4, SET>), dim3(blocks), dim3(kBlock), 0, st, rows, crp, slot, val,
                       (int32_t)n_rows, Z, ldz, out, ldo, d, (int32_t)act);
  else
    hipLaunchKernelGGL((id_fixup_kernel<1, SET>), dim3(blocks), dim3(kBlock), 0, st, rows, crp, slot, val,
                       (int32_t)n_rows, Z, ldz, out, ldo, d, (int32_t)act);
  MP_LAUNCH_CHECK();
  return MP_OK;
}

}  // namespace mp

using namespace mp;

extern "C" {

static int agg_dense_common(const int32_t* rowptr, const int32_t* col, const float* val, int64_t N, int reduce,
                            const float* X, int64_t ldx, int32_t F, const float* S, int64_t lds, float self_scale,
                            const float* W, int64_t ldw, int32_t d_out, const float* bias, int act,
                            const uint8_t* defer_act, float* P, int64_t ldp, float* out, int64_t ldo,
                            const void* W_split, const float* R, int64_t ldr, mp_stream_t stream) {
  if (!rowptr || !X || !W || !out || N < 0 || F <= 0 || d_out <= 0) return MP_ERR_INVALID_ARG;
  if (W_split && ((uintptr_t)W_split % 16)) return MP_ERR_ALIGNMENT;
  if (ldx < F || ldw < d_out || ldo < d_out || (S && lds < F) || (P && ldp < F) || (R && ldr < d_out))
    return MP_ERR_INVALID_ARG;
  if (act != MP_ACT_NONE && act != MP_ACT_RELU) return MP_ERR_INVALID_ARG;
  if (reduce != MP_SUM && reduce != MP_MEAN) return MP_ERR_INVALID_ARG;
  if (reduce == MP_MEAN && S) return MP_ERR_INVALID_ARG;
  if (d_out % 2) return MP_ERR_UNSUPPORTED;
  if (F == 512 && d_out > 512) return MP_ERR_UNSUPPORTED;   // the accumulators of every column block stay in registers
  const int rc = check_shape(F, 64, N, kTileRows);
  if (rc != MP_OK) return rc;
  const int w = F == 512 ? 4 : F / kWave;
  if (mis(X, ldx, 4 * w) || (S && mis(S, lds, 16)) || (P && mis(P, ldp, 16)) || mis(W, ldw, 8) || mis(out, ldo, 8) ||
      (bias && ((uintptr_t)bias % 8)) || (R && mis(R, ldr, 8)))
    return MP_ERR_ALIGNMENT;
  if (N == 0) return MP_OK;
  if (!col) return MP_ERR_INVALID_ARG;
  FusedArgs a = fused_args(rowptr, col, val, N, reduce, X, ldx, F, out, ldo, d_out);
  a.S = S; a.lds = lds; a.self_scale = self_scale;
  a.Wm = W; a.ldw = ldw; a.Wsp = reinterpret_cast<const __bf16*>(W_split);
  a.bias = bias; a.act = act; a.defer_act = defer_act;
  a.P = P; a.ldp = ldp; a.R = R; a.ldr = ldr;
  hipStream_t st = as_stream(stream);
  if (F == 512) return launch_fused<4, 2, 2, 2>(a, st);   // (the one-block instantiation spills: the compiler's choice)
  switch (w) {
    case 4: return launch_fused<4, 1, 1, 2>(a, st);
    case 2: return launch_fused<2, 1, 1, 1>(a, st);
    default: return launch_fused<1, 1, 1, 1>(a, st);
  }
}

int mp_agg_rows_tiles_f32(const int32_t* rowptr, const int32_t* col, const float* val, int64_t N, int reduce,
                          const float* X, int64_t ldx, int32_t F, const float* S, int64_t lds, float self_scale,
                          float* out, int64_t ldo, mp_stream_t stream) {
  return agg_rows_tiles<false>(rowptr, col, val, N, reduce, X, ldx, F, S, lds, self_scale, out, ldo, stream);
}

int mp_idgnn_agg_tiles_f32(const int32_t* rowptr, const int32_t* col, const float* val, int64_t N, const float* X,
                           int64_t ldx, int32_t F, const uint8_t* id_rows, const int32_t* rows, const int32_t* crp,
                           const int32_t* slot, const float* val_id, int64_t n_rows, const float* Z, int64_t ldz, float* P,
                           int64_t ldp, float* Q, int64_t ldq, mp_stream_t stream) {
  if (!Q || n_rows < 0) return MP_ERR_INVALID_ARG;
  if (n_rows > 0 && (!id_rows || !rows || !crp || !slot || !Z || ldz < F)) return MP_ERR_INVALID_ARG;
  // the main branch's rows P and the zero rows of Q on the tile kernel (every other argument is checked there) ...
  const int rc = agg_rows_tiles<false>(rowptr, col, val, N, MP_SUM, X, ldx, F, nullptr, 0, 0.f, P, ldp, stream, Q, ldq,
                                       n_rows > 0 ? id_rows : nullptr);
  if (rc != MP_OK || n_rows == 0 || N == 0) return rc;
  // ... and the rows of Q next to an identity node from their few identity entries
  // (run BESIDE the tile kernel on a second stream — the rows are disjoint — it gains nothing: 21.74-21.77 ms against
  // 21.77 in line, same box; the zero rows of Q, 10 GB of stores, are what the second branch costs)
  return launch_id_fixup<true>(rows, crp, slot, val_id, n_rows, Z, ldz, Q, ldq, F, MP_ACT_NONE, as_stream(stream));
}

int mp_agg_dense_f32(const int32_t* rowptr, const int32_t* col, const float* val, int64_t N, int reduce,
                     const float* X, int64_t ldx, int32_t F, const float* S, int64_t lds, float self_scale, const float* W,
                     int64_t ldw, int32_t d_out, const float* bias, int act, const uint8_t* defer_act, float* P,
                     int64_t ldp, float* out, int64_t ldo, const void* W_split, mp_stream_t stream) {
  return agg_dense_common(rowptr, col, val, N, reduce, X, ldx, F, S, lds, self_scale, W, ldw, d_out, bias, act, defer_act,
                          P, ldp, out, ldo, W_split, nullptr, 0, stream);
}

int mp_agg_dense_add_f32(const int32_t* rowptr, const int32_t* col, const float* val, int64_t N, int reduce,
                         const float* X, int64_t ldx, int32_t F, const float* S, int64_t lds, float self_scale,
                         const float* W, int64_t ldw, int32_t d_out, const float* bias, int act,
                         const uint8_t* defer_act, float* P, int64_t ldp, float* out, int64_t ldo, const void* W_split,
                         const float* R, int64_t ldr, mp_stream_t stream) {
  if (!R) return MP_ERR_INVALID_ARG;
  return agg_dense_common(rowptr, col, val, N, reduce, X, ldx, F, S, lds, self_scale, W, ldw, d_out, bias, act, defer_act,
                          P, ldp, out, ldo, W_split, R, ldr, stream);
}

int mp_id_fixup_f32(const int32_t* rows, const int32_t* crp, const int32_t* slot, const float* val, int64_t n_rows,
                    const float* Z, int64_t ldz, float* out, int64_t ldo, int32_t d, int act, mp_stream_t stream) {
  if (n_rows < 0 || d <= 0 || (n_rows > 0 && (!rows || !crp || !slot || !Z || !out))) return MP_ERR_INVALID_ARG;
  if (act != MP_ACT_NONE && act != MP_ACT_RELU) return MP_ERR_INVALID_ARG;
  if (ldz < d || ldo < d || n_rows >= INT32_MAX) return MP_ERR_INVALID_ARG;
  if (n_rows == 0) return MP_OK;
  return launch_id_fixup<false>(rows, crp, slot, val, n_rows, Z, ldz, out, ldo, d, act, as_stream(stream));
}

int mp_id_rows_f32(const int32_t* rows, const int32_t* crp, const int32_t* slot, const float* val, int64_t n_rows,
                   const float* Z, int64_t ldz, float* out, int64_t ldo, int32_t d, mp_stream_t stream) {
  if (n_rows < 0 || d <= 0 || (n_rows > 0 && (!rows || !crp || !slot || !Z || !out))) return MP_ERR_INVALID_ARG;
  if (ldz < d || ldo < d || n_rows >= INT32_MAX) return MP_ERR_INVALID_ARG;
  if (n_rows == 0) return MP_OK;
  return launch_id_fixup<true>(rows, crp, slot, val, n_rows, Z, ldz, out, ldo, d, MP_ACT_NONE, as_stream(stream));
}

}  // extern "C"
