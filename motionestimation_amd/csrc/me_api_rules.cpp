// me_api_rules.cpp -- the C ABI's argument rules and record layouts
// (me_api_rules.h).  Plain C++ with no HIP dependency, like the planners.
#include "me_api_rules.h"

#include <stdarg.h>
#include <stdio.h>

#include "me_partition.h"
#include "me_rd.h"

namespace me {
namespace rules {
me_status fail(char* err, size_t n, me_status s, const char* fmt, ...) {
  if (err && n) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(err, n, fmt, ap);
    va_end(ap);
  }
  return s;
}

namespace {

// Append a region of `bytes` bytes of `elem`-byte elements to L.
void add(Layout* L, size_t bytes, size_t elem) {
  L->off[L->n] = L->total;
  L->bytes[L->n] = bytes;
  L->elem[L->n++] = elem;
  L->total += bytes;
}
bool valid_cost(int cost) {
  return cost == ME_COST_SSD || cost == ME_COST_SAD || cost == ME_COST_SSIM || cost == ME_COST_SATD;
}

}  // namespace

me_status one_device(int n_devs, const char* what, char* err, size_t n) {
  if (n_devs > 1)
    return fail(err, n, ME_EUNSUPPORTED, "%s on %zu devices (one device only)", what, (size_t)n_devs);
  return ME_OK;
}

me_status args(const void* ref, const void* cur, int width, int height, int stride, int blk,
               int range, int cost, const void* mv, char* err, size_t n) {
  if (!ref || !cur || !mv) return fail(err, n, ME_EINVAL, "null plane or output pointer");
  if (width <= 0 || height <= 0) return fail(err, n, ME_EINVAL, "frame %dx%d", width, height);
  if (stride < width) return fail(err, n, ME_EINVAL, "stride %d < width %d", stride, width);
  if (blk < 1 || blk > ME_MAX_BLOCK) return fail(err, n, ME_EINVAL, "block_size %d", blk);
  if (range < 0 || range > ME_MAX_RANGE) return fail(err, n, ME_EINVAL, "search_range %d", range);
  if (!valid_cost(cost)) return fail(err, n, ME_EINVAL, "cost %d", cost);
  // An integer search asked for SATD is a valid request this build does not
  // serve (the sub-pel entry points pass search_cost(cost): it never arrives
  // from them).
  if (cost == ME_COST_SATD)
    return fail(err, n, ME_EUNSUPPORTED,
                "integer searches have no SATD cost (quarter-pel refinement and bi-prediction only)");
  // Buffer descriptors carry 32-bit byte ranges: planes stay below 2 GiB.
  if ((long long)stride * height >= (1LL << 31))
    return fail(err, n, ME_EUNSUPPORTED, "plane of %lld bytes (limit 2 GiB)",
                (long long)stride * height);
  return ME_OK;
}

me_status stripe(int nby, int blk, int range, int r0, int r1, int ref_row0, int cur_row0, int job,
                 char* err, size_t n) {
  const long long cur0 = (long long)r0 * blk, need_ref0 = cur0 - range > 0 ? cur0 - range : 0;
  const bool rows = r0 < 0 || r1 > nby || r0 > r1;
  const bool ref = ref_row0 < 0 || ref_row0 > need_ref0, cur = cur_row0 < 0 || cur_row0 > cur0;
  if (!rows && !ref && !cur) return ME_OK;
  char pre[24] = "";
  if (job >= 0) snprintf(pre, sizeof pre, "job %d: ", job);
  if (rows) return fail(err, n, ME_EINVAL, "%sblock rows [%d, %d)", pre, r0, r1);
  if (ref) return fail(err, n, ME_EINVAL, "%sref_row0 %d", pre, ref_row0);
  return fail(err, n, ME_EINVAL, "%scur_row0 %d", pre, cur_row0);
}

me_status frame_batch(int n_frames, const FramePlane* planes, int n_planes, char* err, size_t n) {
  if (n_frames < 1 || n_frames > 4096) return fail(err, n, ME_EINVAL, "n_frames %d", n_frames);
  for (int k = 0; k < n_planes; k++)
    if (n_frames > 1 && planes[k].frame_stride < planes[k].frame_bytes)
      return fail(err, n, ME_EINVAL, "frame stride %zu below a frame's %llu bytes",
                  planes[k].frame_stride, planes[k].frame_bytes);
  for (int k = 0; k < n_planes; k++) {
    // (a stride of 2 GiB or more is past the limit by itself: the sum below never
    // wraps, where (n_frames - 1) * SIZE_MAX would come out small)
    const unsigned long long fs = n_frames > 1 ? planes[k].frame_stride : 0;
    if (fs >= (1ull << 31))
      return fail(err, n, ME_EUNSUPPORTED, "frame stride of %llu bytes (limit 2 GiB)", fs);
    const unsigned long long stack = (unsigned long long)(n_frames - 1) * fs + planes[k].frame_bytes;
    if (stack >= (1ull << 31))
      return fail(err, n, ME_EUNSUPPORTED, "batch of %llu bytes (limit 2 GiB)", stack);
  }
  return ME_OK;
}

me_status qpel(int cost, const void* mv_q, char* err, size_t n) {
  if (!mv_q) return fail(err, n, ME_EINVAL, "null quarter-pel output");
  if (cost == ME_COST_SSIM)
    return fail(err, n, ME_EUNSUPPORTED,
                "quarter-pel refinement has no SSIM cost (SAD, SSD or SATD)");
  return ME_OK;
}

me_status bipred(int cost, const void* ref1, const void* q1, const void* out0, const void* out1,
                 const void* mode, char* err, size_t n) {
  if (!ref1 || !q1 || !out0 || !out1 || !mode)
    return fail(err, n, ME_EINVAL, "null bi-prediction plane, field or mode pointer");
  if (cost == ME_COST_SSIM)
    return fail(err, n, ME_EUNSUPPORTED, "bi-prediction has no SSIM cost (SAD, SSD or SATD)");
  return ME_OK;
}

me_status partition(int n_devs, const void* ref, const void* cur, int width, int height, int stride,
                    int blk, int range, int cost, uint32_t lambda, const me_part_fields* out,
                    int counts[4], char* err, size_t n) {
  if (!ref || !cur || !out) return fail(err, n, ME_EINVAL, "null plane or field pointer");
  if (!out->mv_2nx2n || !out->mv_2nxn || !out->mv_nx2n || !out->mv_nxn || !out->mode)
    return fail(err, n, ME_EINVAL, "null partition vector field or mode array");
  if (!valid_cost(cost)) return fail(err, n, ME_EINVAL, "cost %d", cost);
  const char* why = "";
  const me_status s = partition_check(width, height, stride, blk, range, &why);
  if (s != ME_OK)
    return fail(err, n, s, "%s (%dx%d pitch %d, B %d, S %d)", why, width, height, stride, blk, range);
  if (cost != ME_COST_SAD) return fail(err, n, ME_EUNSUPPORTED, "partition search costs SAD only");
  if (lambda > ME_PART_MAX_LAMBDA)
    return fail(err, n, ME_EINVAL, "lambda %u above ME_PART_MAX_LAMBDA", lambda);
  if (n_devs > 1) return one_device(n_devs, "partition search", err, n);
  if (me_partition_counts(width, height, blk, counts) != ME_OK)
    return fail(err, n, ME_EINVAL, "frame %dx%d", width, height);
  return ME_OK;
}

me_status partition_rd(int n_devs, const void* ref, const void* cur, int width, int height,
                       int stride, int blk, int range, int cost, uint32_t lambda,
                       const me_part_rd_fields* out, int counts[4], char* err, size_t n) {
  if (!out) return fail(err, n, ME_EINVAL, "null plane or field pointer");
  const me_status s =
      partition(n_devs, ref, cur, width, height, stride, blk, range, cost, 0, &out->f, counts, err, n);
  if (s != ME_OK) return s;
  if (lambda > ME_PART_RD_MAX_LAMBDA)
    return fail(err, n, ME_EINVAL, "lambda %u above ME_PART_RD_MAX_LAMBDA", lambda);
  return ME_OK;
}

me_status partition_qpel(int n_devs, const void* ref, const void* cur, int width, int height,
                         int stride, int blk, int cost, uint32_t lambda, const me_part_fields* in,
                         const me_part_rd_fields* out, int counts[4], char* err, size_t n) {
  if (!ref || !cur || !in || !out) return fail(err, n, ME_EINVAL, "null plane or field pointer");
  if (!in->mv_2nx2n || !in->mv_2nxn || !in->mv_nx2n || !in->mv_nxn)
    return fail(err, n, ME_EINVAL, "null integer partition vector field");
  if (!out->f.mv_2nx2n || !out->f.mv_2nxn || !out->f.mv_nx2n || !out->f.mv_nxn || !out->f.mode)
    return fail(err, n, ME_EINVAL, "null partition vector field or mode array");
  if (!valid_cost(cost)) return fail(err, n, ME_EINVAL, "cost %d", cost);
  const char* why = "";
  const me_status s = partition_check(width, height, stride, blk, 0, &why);
  if (s != ME_OK)
    return fail(err, n, s, "%s (%dx%d pitch %d, B %d)", why, width, height, stride, blk);
  if (cost == ME_COST_SSIM)
    return fail(err, n, ME_EUNSUPPORTED,
                "partition-wise refinement has no SSIM cost (SAD, SSD or SATD)");
  if (lambda > ME_PART_RD_MAX_LAMBDA)
    return fail(err, n, ME_EINVAL, "lambda %u above ME_PART_RD_MAX_LAMBDA", lambda);
  if (n_devs > 1) return one_device(n_devs, "partition-wise refinement", err, n);
  if (me_partition_counts(width, height, blk, counts) != ME_OK)
    return fail(err, n, ME_EINVAL, "frame %dx%d", width, height);
  return ME_OK;
}

me_status partition_leaf(int n_devs, int width, int height, int blk, int n_frames,
                         const me_part_fields* in, const void* leaf, char* err, size_t n) {
  me_status s = frame_batch(n_frames, nullptr, 0, err, n);
  if (s != ME_OK) return s;
  if (!in || !leaf || !in->mv_2nx2n || !in->mv_2nxn || !in->mv_nx2n || !in->mv_nxn || !in->mode)
    return fail(err, n, ME_EINVAL, "null partition vector field, mode array or leaf field");
  const char* why = "";
  if ((s = partition_check(width, height, width, blk, 0, &why)) != ME_OK)
    return fail(err, n, s, "%s (%dx%d, B %d)", why, width, height, blk);
  return one_device(n_devs, "partition leaf field", err, n);
}

me_status rd_ctx(int n_devs, uint32_t lambda, const char* what, char* err, size_t n) {
  if (lambda > ME_RD_MAX_LAMBDA)
    return fail(err, n, ME_EINVAL, "lambda %u above ME_RD_MAX_LAMBDA", lambda);
  return one_device(n_devs, what, err, n);
}

me_status rd(int n_devs, const void* ref, const void* cur, int width, int height, int stride,
             int blk, int range, int cost, uint32_t lambda, const void* mv, const void* block_cost,
             char* err, size_t n) {
  if (!ref || !cur || !mv || !block_cost)
    return fail(err, n, ME_EINVAL, "null plane, vector or cost pointer");
  if (!valid_cost(cost)) return fail(err, n, ME_EINVAL, "cost %d", cost);
  const char* why = "";
  const me_status s = rd_check(width, height, stride, blk, range, lambda, &why);
  if (s != ME_OK)
    return fail(err, n, s, "%s (%dx%d pitch %d, B %d, S %d, lambda %u)", why, width, height, stride,
                blk, range, lambda);
  if (cost != ME_COST_SAD)
    return fail(err, n, ME_EUNSUPPORTED, "rate-constrained search costs SAD only");
  return rd_ctx(n_devs, lambda, "rate-constrained search", err, n);
}

me_status vectors(const int16_t* const* fields, int n_fields, size_t n_blocks, int max,
                  const char* max_name, char* err, size_t n) {
  for (size_t i = 0; i < 2 * n_blocks; i++)
    for (int f = 0; f < n_fields; f++)
      if (fields[f][i] > max || fields[f][i] < -max)
        return fail(err, n, ME_EINVAL, "block %zu: vector component %d beyond %s (%d)", i / 2,
                    (int)fields[f][i], max_name, max);
  return ME_OK;
}

me_status pred_modes(const uint8_t* mode, size_t n_blocks, char* err, size_t n) {
  for (size_t i = 0; i < n_blocks; i++)
    if (mode[i] > ME_PRED_BI)
      return fail(err, n, ME_EINVAL, "block %zu: mode %d (0, 1 or 2)", i, (int)mode[i]);
  return ME_OK;
}

me_status pixels(const int* ref, const int* cur, size_t count, uint8_t* ref8, uint8_t* cur8, char* err,
                 size_t n) {
  // the planes came from 8-bit files: anything else would be searched as its
  // low byte and give a field the reference would not
  for (size_t i = 0; i < count; i++) {
    if ((unsigned)ref[i] > 255u || (unsigned)cur[i] > 255u)
      return fail(err, n, ME_EINVAL, "pixel %zu (%d, %d) outside [0, 255]", i, ref[i], cur[i]);
    ref8[i] = (uint8_t)ref[i];
    cur8[i] = (uint8_t)cur[i];
  }
  return ME_OK;
}

Layout layout_mv_cost(size_t nb) {
  Layout L{};
  add(&L, 4 * nb, 2), add(&L, 4 * nb, 4);
  return L;
}

Layout layout_bipred(size_t nb) {
  Layout L{};
  add(&L, 4 * nb, 2), add(&L, 4 * nb, 2), add(&L, 4 * nb, 4), add(&L, 12 * nb, 4), add(&L, nb, 1);
  L.total = 28 * nb;  // (what the entry points ask for: mode as if 4 bytes per block)
  return L;
}

Layout layout_rd(size_t nb) {
  Layout L{};
  add(&L, 4 * nb, 2), add(&L, 4 * nb, 2), add(&L, 4 * nb, 4), add(&L, 4 * nb, 4), add(&L, nb, 1);
  L.total = (L.total + 7) / 8 * 8;
  return L;
}

// The four vector grids, then the four cost grids, the mode costs and the modes.
Layout layout_partition(const int c[4]) {
  Layout L{};
  for (int g = 0; g < 4; g++) add(&L, 4 * (size_t)c[g], 2);
  for (int g = 0; g < 4; g++) add(&L, 4 * (size_t)c[g], 4);
  add(&L, 4 * (size_t)c[0], 4), add(&L, (size_t)c[0], 1);
  L.total = (L.total + 7) / 8 * 8;
  return L;
}

// The predictors, the vector, cost and distortion grids, the mode costs, the
// rate grids and the modes.
Layout layout_partition_rd(const int c[4]) {
  Layout L{};
  add(&L, 4 * (size_t)c[0], 2);
  for (int g = 0; g < 4; g++) add(&L, 4 * (size_t)c[g], 2);
  for (int g = 0; g < 8; g++) add(&L, 4 * (size_t)c[g % 4], 4);
  add(&L, 4 * (size_t)c[0], 4);
  for (int g = 0; g < 4; g++) add(&L, (size_t)c[g], 1);
  add(&L, (size_t)c[0], 1);
  L.total = (L.total + 7) / 8 * 8;
  return L;
}

}  // namespace rules
}  // namespace me
