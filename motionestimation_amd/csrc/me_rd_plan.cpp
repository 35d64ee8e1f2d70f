// me_rd_plan.cpp -- host-only side of the rate-constrained search (include/me.h
// "rate-constrained motion search"): argument rules, the code length of a
// vector component, and which kernel takes a frame's full-size blocks.  Plain
// C++ with no HIP dependency, like the other planners.
#include <stdint.h>

#include "me.h"
#include "me_rd.h"

namespace me {

me_status rd_check(int width, int height, int stride, int blk, int range, uint32_t lambda,
                   const char** why) {
  const char* dummy;
  if (!why) why = &dummy;
  if (const me_status s = frame_check(width, height, stride, why)) return s;
  if (blk < 1 || blk > ME_MAX_BLOCK) return *why = "block_size", ME_EINVAL;
  if (range < 0) return *why = NEGATIVE_RANGE, ME_EINVAL;
  if (lambda > ME_RD_MAX_LAMBDA) return *why = "lambda above ME_RD_MAX_LAMBDA", ME_EINVAL;
  if (range > ME_RD_MAX_RANGE)
    return *why = "rate-constrained search_range above ME_RD_MAX_RANGE", ME_EUNSUPPORTED;
  return plane_check(stride, height, why);
}

}  // namespace me

extern "C" {

int me_mv_bits(int v) {
  // 2 |v| + 1 in 64 bits: any int
  const uint64_t u = 2 * (uint64_t)(v < 0 ? -(int64_t)v : (int64_t)v) + 1;
  return 2 * (63 - __builtin_clzll(u)) + 1;
}

int me_rd_kernel_variant(int width, int height, int stride, int blk, int range, uint32_t lambda) {
  if (me::rd_check(width, height, stride, blk, range, lambda, nullptr) != ME_OK) return -1;
  // The fast kernel holds a candidate's J in 26 bits of a 32-bit key.
  const bool fast = me::tile_fast_shape(width, height, stride, blk, range) &&
                    lambda <= ME_RD_FAST_MAX_LAMBDA;
  return fast ? ME_RD_KERNEL_FAST : ME_RD_KERNEL_GENERIC;
}

}  // extern "C"
