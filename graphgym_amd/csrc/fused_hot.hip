// The hot-column form of the tile aggregation, mp_agg_rows_tiles_hot_f32: agg_dense_pc_kernel<..., HOT = true> (fused.hip)
// in a translation unit of its own, so that the compiler flag it needs applies to these kernels and to no other.
//
// Per gathered row the producers branch on the row's tag (wave-uniform: a scalar branch) between a default-policy and a
// non-temporal load.  The CFG structurizer turns each such if / else into two one-sided regions, which leaves paths
// with zero or two loads; the wait counting then falls back to vmcnt(0) at every row a burst consumes.  build.py builds
// this file with -structurizecfg-skip-uniform-regions=true (uniform branches stay branches): the hot kernels then have
// the counted waits of the plain ones.  fused.hip itself is built without it.
#define MP_FUSED_HOT_TU 1
#include "fused.hip"
