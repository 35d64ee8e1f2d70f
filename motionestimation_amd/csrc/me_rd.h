// me_rd.h -- the rate-constrained search's internal interface (include/me.h
// "rate-constrained motion search"): what the host-only planner
// (me_rd_plan.cpp), the kernels (me_rd.hip; their launchers are declared in
// me_kernels.h) and the entry points share.  The fast kernel's tiling is
// me_tile_geom.h's.  No HIP dependency.  Not installed.
#pragma once
#include "me_tile_geom.h"

namespace me {

// dy rows per lane-task of the fast kernel, K = rd_fast_k(range).  4 * K <= 64:
// the lane key's index.
constexpr int RD_K_SMALL = 6, RD_K_LARGE = 10;

// The geometry and lambda rules of the search: ME_OK, or the status the entry
// points return with *why set to a static message.
me_status rd_check(int width, int height, int stride, int blk, int range, uint32_t lambda,
                   const char** why);

// A full tile has 4 G ceil((2S + 1) / K) lane-tasks of K dy rows each and runs
// them in rounds of TILE_THREADS: the K whose rounds x K is smaller (the tile's
// last round wastes less), the larger K on a tie (fewer window rows read per
// dy row).  DESIGN.md "Rate-constrained search".
ME_TILE_HD inline int rd_fast_k(int range) {
  const int per_chunk = TILE_TB * tile_groups(range);
  const int rs = (per_chunk * tile_chunks(range, RD_K_SMALL) + TILE_THREADS - 1) / TILE_THREADS * RD_K_SMALL;
  const int rl = (per_chunk * tile_chunks(range, RD_K_LARGE) + TILE_THREADS - 1) / TILE_THREADS * RD_K_LARGE;
  return rs < rl ? RD_K_SMALL : RD_K_LARGE;
}

// bits(v) = 2 floor(log2(2 |v| + 1)) + 1, |v| < 2^30.
ME_TILE_HD inline int rd_bits(int v) {
  const uint32_t u = 2u * (uint32_t)(v < 0 ? -v : v) + 1u;
  return 63 - 2 * __builtin_clz(u);
}

#ifdef __HIPCC__
// Saturating u32 add (v_add_u32 with clamp); me_rd.hip and me_partition.hip.
__device__ inline __attribute__((always_inline)) uint32_t add_sat(uint32_t a, uint32_t b) {
  return __builtin_elementwise_add_sat(a, b);
}
#endif

}  // namespace me
