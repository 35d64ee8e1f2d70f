// me_partition_plan.cpp -- host-only side of the partition search (include/me.h
// "partition search"): argument rules, grid counts, which kernel takes a
// frame's full-size macroblocks, and the leaf field on the host.  Plain C++
// with no HIP dependency, like the other planners.
#include <stdint.h>

#include "me.h"
#include "me_partition.h"

namespace me {

me_status partition_check(int width, int height, int stride, int blk, int range,
                          const char** why) {
  const char* dummy;
  if (!why) why = &dummy;
  if (const me_status s = frame_check(width, height, stride, why)) return s;
  if (range < 0) return *why = NEGATIVE_RANGE, ME_EINVAL;
  if (blk != 8 && blk != 16 && blk != 32)
    return *why = "partition search takes block_size 8, 16 or 32", ME_EUNSUPPORTED;
  if (range > ME_PART_MAX_RANGE)
    return *why = "partition search_range above ME_PART_MAX_RANGE", ME_EUNSUPPORTED;
  return plane_check(stride, height, why);
}

}  // namespace me

extern "C" {

me_status me_partition_counts(int width, int height, int blk, int counts[4]) {
  if (!counts || width <= 0 || height <= 0 || blk < 2 || blk % 2) return ME_EINVAL;
  const int h = blk / 2;
  const int64_t nbx = ((int64_t)width + blk - 1) / blk, nby = ((int64_t)height + blk - 1) / blk;
  const int64_t nhx = ((int64_t)width + h - 1) / h, nhy = ((int64_t)height + h - 1) / h;
  if (nhx * nhy > INT32_MAX) return ME_EINVAL;
  counts[0] = (int)(nbx * nby);
  counts[1] = (int)(nbx * nhy);
  counts[2] = (int)(nhx * nby);
  counts[3] = (int)(nhx * nhy);
  return ME_OK;
}

int me_partition_kernel_variant(int width, int height, int stride, int blk, int range) {
  if (me::partition_check(width, height, stride, blk, range, nullptr) != ME_OK) return -1;
  return me::tile_fast_shape(width, height, stride, blk, range) ? ME_PART_KERNEL_FAST
                                                                : ME_PART_KERNEL_GENERIC;
}

int me_partition_rd_kernel_variant(int width, int height, int stride, int blk, int range,
                                   uint32_t lambda) {
  if (lambda > ME_PART_RD_MAX_LAMBDA) return -1;
  const int v = me_partition_kernel_variant(width, height, stride, blk, range);
  // The fast kernel holds a candidate's J in 26 bits of a 32-bit key, like
  // me_rd_fast_kernel.
  if (v == ME_PART_KERNEL_FAST && lambda > ME_RD_FAST_MAX_LAMBDA) return ME_PART_KERNEL_GENERIC;
  return v;
}

me_status me_partition_leaf_field(int width, int height, int blk, const me_part_fields* in,
                                  int16_t* leaf) {
  int n[4];
  if (!in || !leaf || !in->mv_2nx2n || !in->mv_2nxn || !in->mv_nx2n || !in->mv_nxn || !in->mode)
    return ME_EINVAL;
  if (me_partition_counts(width, height, blk, n) != ME_OK) return ME_EINVAL;
  const int h = blk / 2;
  const int nbx = (width + blk - 1) / blk, nhx = (width + h - 1) / h, nhy = (height + h - 1) / h;
  for (int i = 0; i < n[0]; i++)
    if (in->mode[i] > ME_PART_NxN) return ME_EINVAL;
  for (int hy = 0; hy < nhy; hy++) {
    for (int hx = 0; hx < nhx; hx++) {
      const int bx = hx / 2, by = hy / 2;
      const int16_t* v;
      switch (in->mode[by * nbx + bx]) {
        case ME_PART_2Nx2N: v = in->mv_2nx2n + 2 * ((size_t)by * nbx + bx); break;
        case ME_PART_2NxN: v = in->mv_2nxn + 2 * ((size_t)hy * nbx + bx); break;
        case ME_PART_Nx2N: v = in->mv_nx2n + 2 * ((size_t)by * nhx + hx); break;
        default: v = in->mv_nxn + 2 * ((size_t)hy * nhx + hx); break;
      }
      leaf[2 * ((size_t)hy * nhx + hx)] = v[0];
      leaf[2 * ((size_t)hy * nhx + hx) + 1] = v[1];
    }
  }
  return ME_OK;
}

}  // extern "C"
