// me_partition.h -- the partition searches' internal interface (include/me.h
// "partition search", "rate-constrained partition search"): what the host-only
// planner (me_partition_plan.cpp), the kernels (me_partition.hip; their
// launchers are declared in me_kernels.h) and the entry points share.  The
// fast kernels' tiling is me_tile_geom.h's.  No HIP dependency (the kernels'
// shared device code is me_tile_search.h).  Not installed.
#pragma once
#include "me_tile_geom.h"

namespace me {

// dy rows per lane-task of the fast kernels: the plain search's and the
// rate-constrained one's (DESIGN.md "Rate-constrained partition search").
constexpr int PART_K = 6;
constexpr int PART_RD_K = 6;

// The geometry rules of the search (B, S, plane size): ME_OK, or the status
// the entry points return with *why set to a static message.
me_status partition_check(int width, int height, int stride, int blk, int range,
                          const char** why);

}  // namespace me
