// The hot-column form of the tile aggregation, mp_agg_rows_tiles_hot_f32: agg_dense_pc_kernel<..., HOT = true> (fused_pc.h)
// in a translation unit of its own, so that the compiler flag it needs applies to these kernels and to no other.
//
// Per gathered row the producers branch on the row's tag (wave-uniform: a scalar branch) between a default-policy and a
// non-temporal load.  The CFG structurizer turns each such if / else into two one-sided regions, which leaves paths
// with zero or two loads; the wait counting then falls back to vmcnt(0) at every row a burst consumes.  build.py builds
// this file with -structurizecfg-skip-uniform-regions=true (uniform branches stay branches): the hot kernels then have
// the counted waits of the plain ones.  fused.hip itself is built without it.
#include "fused_pc.h"

extern "C" int mp_agg_rows_tiles_hot_f32(const int32_t* rowptr, const int32_t* col_hot, const float* val, int64_t N,
                                         int reduce, const float* X, int64_t ldx, int32_t F, const float* S, int64_t lds,
                                         float self_scale, float* out, int64_t ldo, mp_stream_t stream) {
  return mp::agg_rows_tiles<true>(rowptr, col_hot, val, N, reduce, X, ldx, F, S, lds, self_scale, out, ldo, stream);
}
