// me_rd.hip -- rate-constrained integer search, J = SAD + lambda * R (include/
// me.h "rate-constrained motion search"; DESIGN.md "Rate-constrained search").
// No reference counterpart: the reference minimises distortion alone.
//
// R(d) = bits(4 dx - px) + bits(4 dy - py) against the block's quarter-pel
// predictor p, bits(v) = 63 - 2 clz(2 |v| + 1) (rd_bits of me_rd.h).  The
// running minimum uses the packed key of me_kernels.h on J,
//     key = J << 32 | (dy + 32768) << 16 | (dx + 32768),
// whose unsigned minimum is the smallest J and, among equal J, the first
// displacement in raster order.  The thread that writes a block's record
// recomputes R from the winning displacement; the distortion is J - lambda R.
//
// Kernels (the building blocks are me_tile_search.h's):
//   me_rd_fast_kernel<K>  B = 16, full-size blocks, S <= 64, rows a multiple of
//                         4 bytes, lambda <= ME_RD_FAST_MAX_LAMBDA; K = 6 or 10
//                         by the range (rd_fast_k).  A workgroup takes TILE_TB
//                         blocks of one row, their union window is staged once
//                         in LDS by LDS DMA, a lane holds its block in 64 VGPRs
//                         and owns 4 dx x K dy candidates, walking the K + 15
//                         window rows with v_qsad_pk_u16_u8 into one packed-u16
//                         accumulator per dy row (tile_lane<K, 1>).  The rate
//                         is separable: the workgroup tabulates lambda
//                         bits(4 dx - px) per window column and lambda
//                         bits(4 dy - py) per row in LDS (~0 for a column or
//                         row that is no candidate), a lane reads its 4 + K
//                         entries; J is a 32-bit saturating sum per candidate,
//                         the lane key J << 6 | 4 j + i.
//   me_tile_generic_kernel<1, true, RdOut, rd_store>
//                         B in [1, 64], any S <= 128, clipped blocks, any pitch
//                         and lambda: one workgroup per block, one candidate
//                         per lane per step, v_sad_u8 into a u32 sum.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "me.h"
#include "me_kernels.h"
#include "me_rd.h"
#include "me_tile_search.h"

namespace me {
namespace {

struct RdOut {
  const int16_t* pred;  // null: all zero
  int16_t* mv;
  uint32_t* cost;
  uint32_t* dist;  // may be null
  uint8_t* bits;   // may be null
  int nbx, nby;
  uint32_t lambda;
};

// The record of block (bx, by) of frame f from its winning key and predictor.
__device__ __forceinline__ void rd_store(const RdOut& o, int f, int bx, int by, const uint64_t* k,
                                         int px, int py) {
  const size_t rec = (size_t)f * o.nbx * o.nby + (size_t)by * o.nbx + bx;
  const uint64_t key = *k;
  const int dx = (int)(key & 0xFFFF) - 32768, dy = (int)((key >> 16) & 0xFFFF) - 32768;
  const uint32_t r = (uint32_t)(rd_bits(4 * dx - px) + rd_bits(4 * dy - py));
  const uint32_t j = (uint32_t)(key >> 32);
  store_mv(o.mv + 2 * rec, 0, key);
  o.cost[rec] = j;
  if (o.dist) o.dist[rec] = j - o.lambda * r;
  if (o.bits) o.bits[rec] = (uint8_t)r;
}

// The lane's best 32-bit key J << 6 | 4 j + i, ordered like (J, dy, dx) within
// the lane.  rx[i] = lambda bits(4 dx_i - px) << 6 | i and ry[j] = lambda
// bits(4 dy_j - py) << 6 | 4 j come from the workgroup's rate tables: the sum
// with sad << 6 carries nothing between the fields (4 j + i < 64, J < 2^26) and
// stays below 2^32 - 1.  A column or row outside the block's candidates has
// ~0 in its table entry, and both adds saturate, so its key is ~0, above every
// valid one: no compare, mask or branch per candidate.
template <int K>
__device__ __forceinline__ uint32_t rd_lane_key(const uint64_t (&acc)[K][1], const uint32_t (&rx)[4],
                                                const uint32_t* ry) {
  uint32_t best = ~0u;
#pragma unroll
  for (int j = 0; j < K; j++) {
    const uint32_t lo = (uint32_t)acc[j][0], hi = (uint32_t)(acc[j][0] >> 32), r = ry[j];
    const uint32_t k0 = add_sat((lo & 0xFFFFu) << 6, add_sat(rx[0], r));
    const uint32_t k1 = add_sat((lo >> 16) << 6, add_sat(rx[1], r));
    const uint32_t k2 = add_sat((hi & 0xFFFFu) << 6, add_sat(rx[2], r));
    const uint32_t k3 = add_sat((hi >> 16) << 6, add_sat(rx[3], r));
    best = min(min(best, k0), min(k1, min(k2, k3)));
  }
  return best;
}

// Dynamic LDS: FastTile's (one key per block), then the rate tables with the
// lane key's index bits (fill_rate_x / fill_rate_y, INDEX).
template <int K>
__global__ __launch_bounds__(TILE_THREADS) void me_rd_fast_kernel(
    const uint8_t* __restrict__ ref, size_t ref_frame_stride, const uint8_t* __restrict__ cur,
    size_t cur_frame_stride, int width, int height, int stride, int S, int nbx_full, RdOut o) {
  extern __shared__ __align__(16) uint8_t smem[];
  const int tid = threadIdx.x;
  const FastTile t = fast_tile<K>(smem, S, nbx_full, height);
  uint32_t* const rxt = reinterpret_cast<uint32_t*>(t.keys + TILE_TB);
  uint32_t* const ryt = rxt + TILE_TB * 4 * t.G;
  const size_t rec0 = (size_t)t.f * o.nbx * o.nby + (size_t)t.by * o.nbx + t.bx0;

  fast_stage(t, smem, ref, ref_frame_stride, cur, cur_frame_stride, width, height, stride, S);
  if (tid < TILE_TB) t.keys[tid] = ~0ull;
  fill_rate_x<true>(rxt, t, S, width, o.pred, rec0, o.lambda);
  fill_rate_y<K, true>(ryt, t, S, o.pred, rec0, o.lambda);
  fast_stage_wait();

  const int T = fast_tasks(t);
  for (int i = tid; i < T; i += TILE_THREADS) {
    const FastTask k = fast_task<K>(t, i);
    uint32_t c[16][4];
    load_block(t.cur_lds, k.b, c);
    uint64_t acc[K][1];
    tile_lane<K, 1>(fast_task_at(smem, t, k), t.pitch, c, acc);

    const int dxg = 4 * k.gi - S - t.a;  // dx of the lane's first candidate
    const uint4 rv = reinterpret_cast<const uint4*>(rxt)[k.b * t.G + k.gi];
    const uint32_t rx[4] = {rv.x, rv.y, rv.z, rv.w};
    const uint32_t best = rd_lane_key<K>(acc, rx, ryt + k.b * t.chunks * K + k.d0);
    if (best != ~0u) {
      const int idx = (int)(best & 63u);
      merge_key(&t.keys[k.b], make_key(best >> 6, dxg + (idx & 3), k.d0 + (idx >> 2) - S));
    }
  }
  __syncthreads();
  if (tid < t.nb)
    rd_store(o, t.f, t.bx0 + tid, t.by, t.keys + tid, pred_at(o.pred, rec0 + tid, 0),
             pred_at(o.pred, rec0 + tid, 1));
}

}  // namespace

hipError_t launch_rd_search(const FrameBatch& b, int range, uint32_t lambda, bool fast,
                            const int16_t* pred, int16_t* mv, uint32_t* cost, uint32_t* dist,
                            uint8_t* bits, hipStream_t stream) {
  const RdOut o{pred, mv, cost, dist, bits, (b.width + b.blk - 1) / b.blk, (b.height + b.blk - 1) / b.blk,
                lambda};
  const int k = rd_fast_k(range);
  return launch_tile_search<RdOut>(
      b, range, fast, k == RD_K_SMALL ? me_rd_fast_kernel<RD_K_SMALL> : me_rd_fast_kernel<RD_K_LARGE>,
      tile_lds_bytes(range, k, 1, true), me_tile_generic_kernel<1, true, RdOut, rd_store>, o, stream);
}

}  // namespace me
