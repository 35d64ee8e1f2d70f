// me_partition.hip -- variable-block-size partition search with mode decision,
// plain and rate-constrained (include/me.h "partition search", "rate-constrained
// partition search"; DESIGN.md under the same names).  No reference
// counterpart: the reference searches one block size per run.
//
// For every candidate displacement of a B x B macroblock the SADs of its four
// h x h quadrants (h = B / 2) are formed once; the halves and the whole are
// sums of them.  Nine running minima per macroblock (whole, top, bottom, left,
// right, four quarters) use the packed key of me_kernels.h,
//     key = cost << 32 | (dy + 32768) << 16 | (dx + 32768),
// whose unsigned minimum is the smallest cost and, among equal costs, the
// first displacement in raster order.  The mode decision runs in the same
// launch, by the thread that writes a macroblock's records.
//
// The rate-constrained search has J_p(d) = SAD_p(d) + lambda R(d) in the nine
// minima, R(d) = bits(4 dx - px) + bits(4 dy - py) against the macroblock's
// quarter-pel predictor (rd_bits of me_rd.h): one rate per displacement, shared
// by the nine partitions.  The writing thread recomputes R from each winning
// displacement (dist = J - lambda R) and decides the mode on sum J_p + lambda
// mbits(m), mbits = (1, 3, 3, 5) against the plain search's (1, 2, 2, 4).
//
// Kernels (the building blocks are me_tile_search.h's):
//   me_part_fast_kernel<K>     B = 16, full-size macroblocks, S <= 64, rows a
//                              multiple of 4 bytes.  A workgroup takes TILE_TB
//                              macroblocks of one row, their union window is
//                              staged once in LDS by LDS DMA, a lane holds its
//                              macroblock in 64 VGPRs and owns 4 dx x K dy
//                              candidates, walking the K + 15 window rows with
//                              v_qsad_pk_u16_u8 into four packed-u16 quadrant
//                              accumulators per dy row (tile_lane<K, 4>): 8
//                              VGPRs, the same 64 qsads as a plain 16 x 16
//                              search.  Candidates outside the frame are masked.
//   me_part_rd_fast_kernel<K>  the same, lambda <= ME_RD_FAST_MAX_LAMBDA, with
//                              me_rd_fast_kernel's rate tables in LDS: lambda
//                              bits(4 dx - px) per window column and lambda
//                              bits(4 dy - py) per row of every macroblock, ~0
//                              where the column or row is no candidate.  Per dy
//                              row and dx one saturating r = rx + ry, then per
//                              partition one saturating J = sad + r and the
//                              lane key J << 6 | 4 j + i: an invalid
//                              candidate's J is ~0, its key at least
//                              0xFFFFFFC0, above every valid one (J < 2^26 -
//                              1); no compare, mask or branch per candidate.
//   me_tile_generic_kernel<4, false, PartOut, part_store> and
//   me_tile_generic_kernel<4, true, PartRdOut, part_rd_store>
//                              B in {8, 16, 32}, any S <= 128, clipped
//                              macroblocks, any pitch (and lambda): one
//                              workgroup per macroblock, one candidate per lane
//                              per step, v_sad_u8 into u32 quadrant sums, R per
//                              candidate.
//   me_part_leaf_kernel        the leaf field from the four fields and the modes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "me.h"
#include "me_kernels.h"
#include "me_partition.h"
#include "me_rd.h"
#include "me_tile_search.h"

namespace me {
namespace {

struct PartOut {
  me_part_fields f;
  int nbx, nby, nhx, nhy;
  uint32_t lambda;
};

struct PartRdOut {
  me_part_rd_fields f;
  const int16_t* pred;  // null: all zero
  int nbx, nby, nhx, nhy;
  uint32_t lambda;
};

// The nine cells of macroblock (bx, by) of frame f in their grids (2Nx2N, 2NxN,
// Nx2N, NxN: grid_of).  A partition exists iff its cell is inside its grid.
struct PartCells {
  size_t at[P_N];
  bool there[P_N];
};
__device__ __forceinline__ constexpr int grid_of(int p) {
  return p == P_FULL ? 0 : p <= P_BOT ? 1 : p <= P_RIGHT ? 2 : 3;
}
template <typename Out>
__device__ __forceinline__ PartCells part_cells(const Out& o, int f, int bx, int by) {
  const size_t f0 = (size_t)f * o.nbx * o.nby, f1 = (size_t)f * o.nbx * o.nhy;
  const size_t f2 = (size_t)f * o.nhx * o.nby, f3 = (size_t)f * o.nhx * o.nhy;
  const bool right = 2 * bx + 1 < o.nhx, bottom = 2 * by + 1 < o.nhy;
  const size_t q = f3 + (size_t)(2 * by) * o.nhx + 2 * bx;
  return {{f0 + (size_t)by * o.nbx + bx, f1 + (size_t)(2 * by) * o.nbx + bx,
           f1 + (size_t)(2 * by + 1) * o.nbx + bx, f2 + (size_t)by * o.nhx + 2 * bx,
           f2 + (size_t)by * o.nhx + 2 * bx + 1, q, q + 1, q + o.nhx, q + o.nhx + 1},
          {true, true, bottom, true, right, true, right, bottom, right && bottom}};
}

// Macroblock mb's mode from its partitions' costs j (0 for the missing ones, so
// the sums need no special case) and the modes' penalties lambda x (1, half,
// half, quarter).
__device__ __forceinline__ void part_mode(const me_part_fields& F, size_t mb, const uint32_t (&j)[P_N],
                                          uint32_t lambda, uint32_t half, uint32_t quarter) {
  const uint32_t j1 = j[P_TOP] + j[P_BOT] + half * lambda;
  const uint32_t j2 = j[P_LEFT] + j[P_RIGHT] + half * lambda;
  const uint32_t j3 = j[P_TL] + j[P_TR] + j[P_BL] + j[P_BR] + quarter * lambda;
  uint32_t best = j[P_FULL] + lambda;
  int mode = ME_PART_2Nx2N;
  if (j1 < best) best = j1, mode = ME_PART_2NxN;
  if (j2 < best) best = j2, mode = ME_PART_Nx2N;
  if (j3 < best) best = j3, mode = ME_PART_NxN;
  F.mode[mb] = (uint8_t)mode;
  if (F.mode_cost) F.mode_cost[mb] = best;
}

// Records and mode of macroblock (bx, by) of frame f from its nine keys
// (make_key / store_mv of me_kernels.h).
__device__ __forceinline__ void part_store(const PartOut& o, int f, int bx, int by,
                                           const uint64_t* k) {
  const PartCells c = part_cells(o, f, bx, by);
  int16_t* const mv[4] = {o.f.mv_2nx2n, o.f.mv_2nxn, o.f.mv_nx2n, o.f.mv_nxn};
  uint32_t* const cost[4] = {o.f.cost_2nx2n, o.f.cost_2nxn, o.f.cost_nx2n, o.f.cost_nxn};
  uint32_t j[P_N];
#pragma unroll
  for (int p = 0; p < P_N; p++) {
    j[p] = 0;
    if (c.there[p]) {
      j[p] = (uint32_t)(k[p] >> 32);
      store_mv(mv[grid_of(p)] + 2 * c.at[p], 0, k[p]);
      if (cost[grid_of(p)]) cost[grid_of(p)][c.at[p]] = j[p];
    }
  }
  part_mode(o.f, c.at[P_FULL], j, o.lambda, 2, 4);
}

// ... with the rate: R from each winning displacement and the macroblock's
// predictor (px, py), J in cost and J - lambda R in dist.
__device__ __forceinline__ void part_rd_store(const PartRdOut& o, int f, int bx, int by,
                                              const uint64_t* k, int px, int py) {
  const PartCells c = part_cells(o, f, bx, by);
  const me_part_rd_fields& F = o.f;
  int16_t* const mv[4] = {F.f.mv_2nx2n, F.f.mv_2nxn, F.f.mv_nx2n, F.f.mv_nxn};
  uint32_t* const cost[4] = {F.f.cost_2nx2n, F.f.cost_2nxn, F.f.cost_nx2n, F.f.cost_nxn};
  uint32_t* const dist[4] = {F.dist_2nx2n, F.dist_2nxn, F.dist_nx2n, F.dist_nxn};
  uint8_t* const bits[4] = {F.bits_2nx2n, F.bits_2nxn, F.bits_nx2n, F.bits_nxn};
  uint32_t j[P_N];
#pragma unroll
  for (int p = 0; p < P_N; p++) {
    j[p] = 0;
    if (c.there[p]) {
      const int g = grid_of(p);
      const int dx = (int)(k[p] & 0xFFFF) - 32768, dy = (int)((k[p] >> 16) & 0xFFFF) - 32768;
      const uint32_t r = (uint32_t)(rd_bits(4 * dx - px) + rd_bits(4 * dy - py));
      j[p] = (uint32_t)(k[p] >> 32);
      store_mv(mv[g] + 2 * c.at[p], 0, k[p]);
      if (cost[g]) cost[g][c.at[p]] = j[p];
      if (dist[g]) dist[g][c.at[p]] = j[p] - o.lambda * r;
      if (bits[g]) bits[g][c.at[p]] = (uint8_t)r;
    }
  }
  part_mode(F.f, c.at[P_FULL], j, o.lambda, 3, 5);
}

// --------------------------------------------------------------------- fast
// The lane's nine 32-bit keys (sad << 16 | 4 j + i), ordered like (cost, dy,
// dx) within the lane; an invalid candidate's sad is forced to 0xFFFF (above
// any valid one: 65,280).  MASK = false where every candidate of the wave is
// valid (uniform).
template <int K, bool MASK>
__device__ __forceinline__ void part_lane_keys(const uint64_t (&acc)[K][4], uint32_t mlo,
                                               uint32_t mhi, int jlo, int jhi,
                                               uint32_t (&best)[P_N]) {
#pragma unroll
  for (int p = 0; p < P_N; p++) best[p] = ~0u;
#pragma unroll
  for (int j = 0; j < K; j++) {
    uint32_t lo[P_N], hi[P_N];
    nine_sums(acc[j], lo, hi);
    const bool jv = j >= jlo && j <= jhi;
#pragma unroll
    for (int p = 0; p < P_N; p++) {
      uint32_t l = lo[p], h = hi[p];
      if (MASK) {
        l = jv ? l | mlo : ~0u;
        h = jv ? h | mhi : ~0u;
      }
      const uint32_t k0 = (l << 16) | (uint32_t)(4 * j);
      const uint32_t k1 = (l & 0xFFFF0000u) | (uint32_t)(4 * j + 1);
      const uint32_t k2 = (h << 16) | (uint32_t)(4 * j + 2);
      const uint32_t k3 = (h & 0xFFFF0000u) | (uint32_t)(4 * j + 3);
      best[p] = min(min(best[p], k0), min(k1, min(k2, k3)));
    }
  }
}

// Dynamic LDS: FastTile's, with 9 keys per macroblock.  This kernel keeps its
// geometry, staging, task decode and block load written out (they say what
// fast_tile, fast_stage, fast_task and load_block of me_tile_search.h say):
// built from those it measured 0.4 % slower at 4K +-64, twice, with a
// lane-task's listing all but equal to this one's (profiles/README.md).  It
// shares the row walk, nine_sums, merge_key and the record writer.
template <int K>
__global__ __launch_bounds__(TILE_THREADS) void me_part_fast_kernel(
    const uint8_t* __restrict__ ref, size_t ref_frame_stride, const uint8_t* __restrict__ cur,
    size_t cur_frame_stride, int width, int height, int stride, int S, int nbx_full, PartOut o) {
  extern __shared__ __align__(16) uint8_t smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = TILE_THREADS / 64;
  const int bx0 = (int)blockIdx.x * TILE_TB, by = blockIdx.y, f = blockIdx.z;
  const int nb = min(TILE_TB, nbx_full - bx0);
  const int G = tile_groups(S), pitch = tile_pitch(S);
  const int chunks = (2 * S + 1 + K - 1) / K, rows = chunks * K + 15;
  uint8_t* const cur_lds = smem + ((rows * pitch + 15) & ~15);
  uint64_t* const keys = reinterpret_cast<uint64_t*>(cur_lds + TILE_TB * 256);
  const int y0 = by * 16;
  const int a = ((bx0 * 16 - S) % 4 + 4) % 4;
  const int X0 = bx0 * 16 - S - a;

  // plane bytes of one frame: granules (4 bytes, 4-aligned: width and pitch
  // are multiples of 4) wholly inside or wholly outside
  const uint32_t plane = (uint32_t)(stride * (height - 1) + width);
  const __amdgpu_buffer_rsrc_t rref = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(ref + (size_t)f * ref_frame_stride), (short)0, plane, 0x00020000);
  const __amdgpu_buffer_rsrc_t rcur = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(cur + (size_t)f * cur_frame_stride), (short)0, plane, 0x00020000);
  // window row r <- frame row y0 - S + r, one DMA step per row (pitch <= 256);
  // offsets before the plane wrap to huge ones: the range check returns zeros
  // (unsigned arithmetic: a wrapped offset is in range or zeroed, never a fault)
  for (int r = wave; r < rows; r += NW) {
    if (4 * lane < pitch)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rref, (__attribute__((address_space(3))) void*)(smem + r * pitch), 4,
          (uint32_t)(y0 - S + r) * (uint32_t)stride + (uint32_t)(X0 + 4 * lane), 0, 0, 0);
  }
  // current block b, row y -> LDS bytes (b * 16 + y) * 16: one block (64
  // granules, 256 bytes) per DMA step
  for (int b = wave; b < nb; b += NW) {
    const int y = lane >> 2, xw = (lane & 3) * 4;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(
        rcur, (__attribute__((address_space(3))) void*)(cur_lds + b * 256), 4,
        (uint32_t)((y0 + y) * stride + (bx0 + b) * 16 + xw), 0, 0, 0);
  }
  if (tid < TILE_TB * P_N) keys[tid] = ~0ull;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // valid displacement rows of the macroblock row; chunks wholly outside are
  // skipped (tasks are chunk-major)
  const int dymin = max(-S, -y0), dymax = min(S, height - 16 - y0);
  const int lc0 = (dymin + S) / K, lc1 = (dymax + S) / K + 1;
  const int per_chunk = nb * G, T = (lc1 - lc0) * per_chunk;
  const uint32_t lds0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) const uint8_t*)smem);
  for (int t = tid; t < T; t += TILE_THREADS) {
    const int lcr = t / per_chunk, rem = t - lcr * per_chunk;
    const int b = rem / G, gi = rem - b * G;
    const int d0 = (lc0 + lcr) * K;  // first dy row of the task, as dy + S
    const int x0 = (bx0 + b) * 16;
    uint32_t c[16][4];
#pragma unroll
    for (int y = 0; y < 16; y++) {
      const uint4 v = reinterpret_cast<const uint4*>(cur_lds)[b * 16 + y];
      c[y][0] = v.x, c[y][1] = v.y, c[y][2] = v.z, c[y][3] = v.w;
    }
    uint64_t acc[K][4];
    tile_lane<K, 4>(lds0 + (uint32_t)(d0 * pitch + 4 * (b * 4 + gi)), pitch, c, acc);

    const int dxmin = max(-S, -x0), dxmax = min(S, width - 16 - x0);
    const int jlo = dymin + S - d0, jhi = dymax + S - d0;
    const int dxg = 4 * gi - S - a;  // dx of the lane's first candidate
    const bool edge = dxg < dxmin || dxg + 3 > dxmax || jlo > 0 || jhi < K - 1;
    uint32_t best[P_N];
    if (__builtin_amdgcn_ballot_w64(edge) == 0) {
      part_lane_keys<K, false>(acc, 0u, 0u, jlo, jhi, best);
    } else {
      uint32_t mlo = 0, mhi = 0;
#pragma unroll
      for (int i = 0; i < 4; i++) {
        const int dx = dxg + i;
        const uint32_t msk = (dx < dxmin || dx > dxmax) ? 0xFFFFu : 0u;
        if (i < 2) mlo |= msk << (16 * i);
        else mhi |= msk << (16 * (i - 2));
      }
      part_lane_keys<K, true>(acc, mlo, mhi, jlo, jhi, best);
    }
#pragma unroll
    for (int p = 0; p < P_N; p++) {
      if (best[p] < 0xFFFF0000u) {
        const int idx = (int)(best[p] & 0xFFFFu);
        const uint64_t key = make_key(best[p] >> 16, dxg + (idx & 3), d0 + (idx >> 2) - S);
        merge_key(&keys[b * P_N + p], key);
      }
    }
  }
  __syncthreads();
  if (tid < nb) part_store(o, f, bx0 + tid, by, keys + tid * P_N);
}

// Every lane key of a valid rate-constrained candidate is below this one
// (J < 2^26 - 1).
constexpr uint32_t LANE_KEY_INVALID = 0xFFFFFFC0u;

// The lane's nine 32-bit keys J << 6 | 4 j + i, ordered like (J, dy, dx) within
// the lane.  rx[i] = lambda bits(4 dx_i - px) and ry[j] = lambda bits(4 dy_j -
// py) come from the workgroup's rate tables, ~0 for a column or row outside
// the macroblock's candidates: r = rx + ry saturates to ~0 there, and so does
// every J = sad + r, whose key is then at least LANE_KEY_INVALID.  A valid J is
// below 2^26 - 1 (65,280 + 66 lambda, lambda <= ME_RD_FAST_MAX_LAMBDA), so the
// shift loses nothing.
template <int K>
__device__ __forceinline__ void part_rd_lane_keys(const uint64_t (&acc)[K][4],
                                                  const uint32_t (&rx)[4], const uint32_t* ry,
                                                  uint32_t (&best)[P_N]) {
#pragma unroll
  for (int p = 0; p < P_N; p++) best[p] = ~0u;
#pragma unroll
  for (int j = 0; j < K; j++) {
    uint32_t lo[P_N], hi[P_N];
    nine_sums(acc[j], lo, hi);
    const uint32_t rj = ry[j];
    const uint32_t r0 = add_sat(rx[0], rj), r1 = add_sat(rx[1], rj);
    const uint32_t r2 = add_sat(rx[2], rj), r3 = add_sat(rx[3], rj);
#pragma unroll
    for (int p = 0; p < P_N; p++) {
      const uint32_t k0 = (add_sat(lo[p] & 0xFFFFu, r0) << 6) | (uint32_t)(4 * j);
      const uint32_t k1 = (add_sat(lo[p] >> 16, r1) << 6) | (uint32_t)(4 * j + 1);
      const uint32_t k2 = (add_sat(hi[p] & 0xFFFFu, r2) << 6) | (uint32_t)(4 * j + 2);
      const uint32_t k3 = (add_sat(hi[p] >> 16, r3) << 6) | (uint32_t)(4 * j + 3);
      best[p] = min(min(best[p], k0), min(k1, min(k2, k3)));
    }
  }
}

// Dynamic LDS: FastTile's, with 9 keys per macroblock, then the rate tables
// without index bits (fill_rate_x / fill_rate_y).
template <int K>
__global__ __launch_bounds__(TILE_THREADS) void me_part_rd_fast_kernel(
    const uint8_t* __restrict__ ref, size_t ref_frame_stride, const uint8_t* __restrict__ cur,
    size_t cur_frame_stride, int width, int height, int stride, int S, int nbx_full,
    PartRdOut o) {
  extern __shared__ __align__(16) uint8_t smem[];
  const int tid = threadIdx.x;
  const FastTile t = fast_tile<K>(smem, S, nbx_full, height);
  uint32_t* const rxt = reinterpret_cast<uint32_t*>(t.keys + TILE_TB * P_N);
  uint32_t* const ryt = rxt + TILE_TB * 4 * t.G;
  const size_t mb0 = (size_t)t.f * o.nbx * o.nby + (size_t)t.by * o.nbx + t.bx0;

  fast_stage(t, smem, ref, ref_frame_stride, cur, cur_frame_stride, width, height, stride, S);
  if (tid < TILE_TB * P_N) t.keys[tid] = ~0ull;
  fill_rate_x<false>(rxt, t, S, width, o.pred, mb0, o.lambda);
  fill_rate_y<K, false>(ryt, t, S, o.pred, mb0, o.lambda);
  fast_stage_wait();

  const int T = fast_tasks(t);
  for (int i = tid; i < T; i += TILE_THREADS) {
    const FastTask k = fast_task<K>(t, i);
    uint32_t c[16][4];
    load_block(t.cur_lds, k.b, c);
    uint64_t acc[K][4];
    tile_lane<K, 4>(fast_task_at(smem, t, k), t.pitch, c, acc);

    const int dxg = 4 * k.gi - S - t.a;  // dx of the lane's first candidate
    const uint4 rv = reinterpret_cast<const uint4*>(rxt)[k.b * t.G + k.gi];
    const uint32_t rx[4] = {rv.x, rv.y, rv.z, rv.w};
    uint32_t best[P_N];
    part_rd_lane_keys<K>(acc, rx, ryt + k.b * t.chunks * K + k.d0, best);
#pragma unroll
    for (int p = 0; p < P_N; p++) {
      if (best[p] < LANE_KEY_INVALID) {
        const int idx = (int)(best[p] & 63u);
        merge_key(&t.keys[k.b * P_N + p],
                  make_key(best[p] >> 6, dxg + (idx & 3), k.d0 + (idx >> 2) - S));
      }
    }
  }
  __syncthreads();
  if (tid < t.nb)
    part_rd_store(o, t.f, t.bx0 + tid, t.by, t.keys + tid * P_N, pred_at(o.pred, mb0 + tid, 0),
                  pred_at(o.pred, mb0 + tid, 1));
}

// One thread per cell of the NxN grid (blockIdx.y: the frame).
__global__ __launch_bounds__(256) void me_part_leaf_kernel(PartOut o, int16_t* __restrict__ leaf) {
  const int i = blockIdx.x * 256 + threadIdx.x, f = blockIdx.y;
  if (i >= o.nhx * o.nhy) return;
  const int hx = i % o.nhx, hy = i / o.nhx, bx = hx / 2, by = hy / 2;
  const size_t f0 = (size_t)f * o.nbx * o.nby, f1 = (size_t)f * o.nbx * o.nhy;
  const size_t f2 = (size_t)f * o.nhx * o.nby, f3 = (size_t)f * o.nhx * o.nhy;
  const int16_t* v;
  switch (o.f.mode[f0 + (size_t)by * o.nbx + bx]) {
    case ME_PART_2Nx2N: v = o.f.mv_2nx2n + 2 * (f0 + (size_t)by * o.nbx + bx); break;
    case ME_PART_2NxN: v = o.f.mv_2nxn + 2 * (f1 + (size_t)hy * o.nbx + bx); break;
    case ME_PART_Nx2N: v = o.f.mv_nx2n + 2 * (f2 + (size_t)by * o.nhx + hx); break;
    default: v = o.f.mv_nxn + 2 * (f3 + (size_t)hy * o.nhx + hx); break;
  }
  leaf[2 * (f3 + i)] = v[0];
  leaf[2 * (f3 + i) + 1] = v[1];
}

PartOut part_out(const me_part_fields& f, int width, int height, int blk, uint32_t lambda) {
  const int h = blk / 2;
  return PartOut{f, (width + blk - 1) / blk, (height + blk - 1) / blk, (width + h - 1) / h,
                 (height + h - 1) / h, lambda};
}

}  // namespace

hipError_t launch_partition_search(const FrameBatch& b, int range, uint32_t lambda, bool fast,
                                   const me_part_fields& out, hipStream_t stream) {
  return launch_tile_search<PartOut>(b, range, fast, me_part_fast_kernel<PART_K>,
                                     tile_lds_bytes(range, PART_K, P_N, false),
                                     me_tile_generic_kernel<4, false, PartOut, part_store>,
                                     part_out(out, b.width, b.height, b.blk, lambda), stream);
}

hipError_t launch_partition_rd_search(const FrameBatch& b, int range, uint32_t lambda, bool fast,
                                      const int16_t* pred, const me_part_rd_fields& out,
                                      hipStream_t stream) {
  const PartOut g = part_out(out.f, b.width, b.height, b.blk, lambda);
  return launch_tile_search<PartRdOut>(b, range, fast, me_part_rd_fast_kernel<PART_RD_K>,
                                       tile_lds_bytes(range, PART_RD_K, P_N, true),
                                       me_tile_generic_kernel<4, true, PartRdOut, part_rd_store>,
                                       PartRdOut{out, pred, g.nbx, g.nby, g.nhx, g.nhy, lambda}, stream);
}

hipError_t launch_partition_leaf(int width, int height, int blk, int n_frames,
                                 const me_part_fields& in, int16_t* leaf, hipStream_t stream) {
  const PartOut o = part_out(in, width, height, blk, 0);
  hipLaunchKernelGGL(me_part_leaf_kernel, dim3((unsigned)((o.nhx * o.nhy + 255) / 256), (unsigned)n_frames),
                     dim3(256), 0, stream, o, leaf);
  return hipGetLastError();
}

}  // namespace me
