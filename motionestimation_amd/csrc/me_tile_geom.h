// me_tile_geom.h -- geometry and argument rules the tile searches share (the
// partition, rate-constrained and rate-constrained partition searches:
// me_partition.h, me_rd.h): one fast-kernel tiling, one fast-shape predicate,
// the check rules they have in common.  Host and device, no HIP dependency (the
// kernels' shared device code is me_tile_search.h).  Not installed.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "me.h"

#ifdef __HIPCC__
#define ME_TILE_HD __host__ __device__
#else
#define ME_TILE_HD
#endif

namespace me {

// Fast kernel geometry: a workgroup of TILE_THREADS takes TILE_TB full-size
// 16 x 16 blocks of one block row; a lane owns 4 dx x K dy candidates of one of
// them (K: PART_K, PART_RD_K, rd_fast_k).
constexpr int TILE_TB = 4;
constexpr int TILE_THREADS = 256;
constexpr int TILE_MAX_RANGE = 64;

// dx groups of 4 of a fast-kernel lane row: the 2S + 1 displacements plus the
// window's alignment slack a = (-S) mod 4 <= 3.
ME_TILE_HD inline int tile_groups(int range) { return (2 * range + 1 + 3 + 3) / 4; }
// Row pitch (bytes) and rows of the fast kernel's LDS window; the dy rows go in
// chunks of k.
ME_TILE_HD inline int tile_pitch(int range) { return 4 * (TILE_TB * 4 + tile_groups(range)); }
ME_TILE_HD inline int tile_chunks(int range, int k) { return (2 * range + 1 + k - 1) / k; }
ME_TILE_HD inline int tile_rows(int range, int k) { return tile_chunks(range, k) * k + 15; }
// Dynamic LDS of a fast kernel: the window, the tile's current blocks (256
// bytes each), `keys` u64 keys per block, then with `rate` the rate tables
// (4 G + rows - 15 words per block).
inline size_t tile_lds_bytes(int range, int k, int keys, bool rate) {
  const int rows = tile_rows(range, k);
  return (size_t)((rows * tile_pitch(range) + 15) & ~15) + TILE_TB * 256 + (size_t)TILE_TB * keys * 8 +
         (rate ? (size_t)TILE_TB * 4 * (4 * tile_groups(range) + rows - 15) : 0);
}

// The shapes whose full-size blocks a fast kernel takes: it stages its window
// with 4-byte LDS DMA granules (none may straddle a row's end: width and pitch
// multiples of 4) and holds a 16 x 16 block's SADs in packed u16.
inline bool tile_fast_shape(int width, int height, int stride, int blk, int range) {
  return blk == 16 && range <= TILE_MAX_RANGE && width % 4 == 0 && stride % 4 == 0 && width >= 16 &&
         height >= 16;
}

// The check rules every tile search has: the first two of a check function,
// and its last.  ME_OK, or the status with *why set to a static message.
inline me_status frame_check(int width, int height, int stride, const char** why) {
  if (width <= 0 || height <= 0) return *why = "frame size", ME_EINVAL;
  if (stride < width) return *why = "stride below width", ME_EINVAL;
  return ME_OK;
}
inline me_status plane_check(int stride, int height, const char** why) {
  if ((long long)stride * height >= (1LL << 31))
    return *why = "plane of 2 GiB or more", ME_EUNSUPPORTED;
  return ME_OK;
}
// The message of the negative-range rule, which sits among a search's own rules.
inline constexpr const char* NEGATIVE_RANGE = "negative search_range";

}  // namespace me
