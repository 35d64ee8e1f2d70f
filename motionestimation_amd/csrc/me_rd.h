// me_rd.h -- the rate-constrained search's internal interface (include/me.h
// "rate-constrained motion search"): what the host-only planner
// (me_rd_plan.cpp), the kernels (me_rd.hip; their launchers are declared in
// me_kernels.h) and the entry points share.  No HIP dependency.  Not installed.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "me.h"

#ifdef __HIPCC__
#define ME_RD_HD __host__ __device__
#else
#define ME_RD_HD
#endif

namespace me {

// Fast kernel geometry: a workgroup takes RD_TB full-size blocks of one block
// row; a lane owns 4 dx x K dy candidates of one of them, K = rd_fast_k(range).
// 4 * K <= 64: the lane key's index.
constexpr int RD_TB = 4;
constexpr int RD_K_SMALL = 6, RD_K_LARGE = 10;
constexpr int RD_FAST_MAX_RANGE = 64;
constexpr int RD_FAST_THREADS = 256;

// The geometry and lambda rules of the search: ME_OK, or the status the entry
// points return with *why set to a static message.
me_status rd_check(int width, int height, int stride, int blk, int range, uint32_t lambda,
                   const char** why);

// dx groups of 4 of a fast-kernel lane row: the 2S + 1 displacements plus the
// window's alignment slack a = (-S) mod 4 <= 3.
ME_RD_HD inline int rd_fast_groups(int range) { return (2 * range + 1 + 3 + 3) / 4; }
// dy rows per lane-task.  A full tile has 4 G ceil((2S + 1) / K) lane-tasks of
// K dy rows each and runs them in rounds of RD_FAST_THREADS: the K whose rounds
// x K is smaller (the tile's last round wastes less), the larger K on a tie
// (fewer window rows read per dy row).  DESIGN.md "Rate-constrained search".
ME_RD_HD inline int rd_fast_k(int range) {
  const int per_chunk = RD_TB * rd_fast_groups(range), n = 2 * range + 1;
  const int rs = (per_chunk * ((n + RD_K_SMALL - 1) / RD_K_SMALL) + RD_FAST_THREADS - 1) /
                 RD_FAST_THREADS * RD_K_SMALL;
  const int rl = (per_chunk * ((n + RD_K_LARGE - 1) / RD_K_LARGE) + RD_FAST_THREADS - 1) /
                 RD_FAST_THREADS * RD_K_LARGE;
  return rs < rl ? RD_K_SMALL : RD_K_LARGE;
}
// Row pitch (bytes) and rows of the fast kernel's LDS window.
ME_RD_HD inline int rd_fast_pitch(int range) { return 4 * (RD_TB * 4 + rd_fast_groups(range)); }
ME_RD_HD inline int rd_fast_rows(int range) {
  const int k = rd_fast_k(range), chunks = (2 * range + 1 + k - 1) / k;
  return chunks * k + 15;
}

// bits(v) = 2 floor(log2(2 |v| + 1)) + 1, |v| < 2^30.
ME_RD_HD inline int rd_bits(int v) {
  const uint32_t u = 2u * (uint32_t)(v < 0 ? -v : v) + 1u;
  return 63 - 2 * __builtin_clz(u);
}

#ifdef __HIPCC__
// Saturating u32 add (v_add_u32 with clamp); me_rd.hip and me_partition_rd.hip.
__device__ inline __attribute__((always_inline)) uint32_t add_sat(uint32_t a, uint32_t b) {
  return __builtin_elementwise_add_sat(a, b);
}
#endif

}  // namespace me
