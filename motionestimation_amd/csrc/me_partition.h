// me_partition.h -- the partition search's internal interface (include/me.h
// "partition search"): what the host-only planner (me_partition_plan.cpp), the
// kernels (me_partition.hip; their launchers are declared in me_kernels.h) and
// the entry points share.  No HIP dependency (the kernels' shared device code is
// me_partition_lane.h).  Not installed.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "me.h"

#ifdef __HIPCC__
#define ME_PART_HD __host__ __device__
#else
#define ME_PART_HD
#endif

namespace me {

// Fast kernel geometry: a workgroup takes PART_TB full-size macroblocks of one
// macroblock row; a lane owns 4 dx x PART_K dy candidates of one of them.
constexpr int PART_TB = 4;
constexpr int PART_K = 6;
constexpr int PART_FAST_MAX_RANGE = 64;
constexpr int PART_FAST_THREADS = 256;

// The geometry rules of the search (B, S, plane size): ME_OK, or the status
// the entry points return with *why set to a static message.
me_status partition_check(int width, int height, int stride, int blk, int range,
                          const char** why);

// dx groups of 4 of a fast-kernel lane row: the 2S + 1 displacements plus the
// window's alignment slack a = (-S) mod 4 <= 3.
ME_PART_HD inline int partition_fast_groups(int range) { return (2 * range + 1 + 3 + 3) / 4; }
// Row pitch (bytes) and rows of the fast kernel's LDS window.
ME_PART_HD inline int partition_fast_pitch(int range) { return 4 * (PART_TB * 4 + partition_fast_groups(range)); }
ME_PART_HD inline int partition_fast_rows(int range) {
  const int chunks = (2 * range + 1 + PART_K - 1) / PART_K;
  return chunks * PART_K + 15;
}

// The rate-constrained fast kernel (me_partition_rd.hip) shares the geometry;
// its dy rows per lane-task (DESIGN.md "Rate-constrained partition search").
constexpr int PART_RD_K = 6;
ME_PART_HD inline int partition_rd_fast_rows(int range) {
  const int chunks = (2 * range + 1 + PART_RD_K - 1) / PART_RD_K;
  return chunks * PART_RD_K + 15;
}

}  // namespace me
