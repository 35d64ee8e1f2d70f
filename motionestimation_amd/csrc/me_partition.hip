// me_partition.hip -- variable-block-size partition search with mode decision
// (include/me.h "partition search"; DESIGN.md "Partition search").  No
// reference counterpart: the reference searches one block size per run.
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
// Kernels:
//   me_part_fast_kernel<K>  B = 16, full-size macroblocks, S <= 64, rows a
//                           multiple of 4 bytes.  The me_fast_kernel scheme:
//                           a workgroup takes PART_TB macroblocks of one row,
//                           their union window is staged once in LDS by LDS
//                           DMA, a lane holds its macroblock in 64 VGPRs and
//                           owns 4 dx x K dy candidates, walking the K + 15
//                           window rows with v_qsad_pk_u16_u8.  Per dy row four
//                           packed-u16 quadrant accumulators (segments 0-1 /
//                           2-3 of a row are left / right, rows 0-7 / 8-15 top
//                           / bottom): 8 VGPRs, the same 64 qsads as a plain
//                           16 x 16 search.  (The row walk, part_lane, lives in
//                           me_partition_lane.h: me_partition_rd.hip shares it.)
//   me_part_generic_kernel  B in {8, 16, 32}, any S <= 128, clipped
//                           macroblocks, any pitch: one workgroup per
//                           macroblock, one candidate per lane per step,
//                           v_sad_u8 into u32 quadrant sums.
//   me_part_leaf_kernel     the leaf field from the four fields and the modes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "me.h"
#include "me_kernels.h"
#include "me_partition.h"
#include "me_partition_lane.h"

namespace me {
namespace {

struct PartOut {
  me_part_fields f;
  int nbx, nby, nhx, nhy;
  uint32_t lambda;
};

// A cell's record from its key (make_key / store_mv of me_kernels.h).
__device__ __forceinline__ void store_rec(int16_t* mv, uint32_t* cost, size_t at, uint64_t key) {
  store_mv(mv + 2 * at, 0, key);
  if (cost) cost[at] = (uint32_t)(key >> 32);
}

// Records and mode of macroblock (bx, by) of frame f from its nine keys.  A
// partition exists iff its cell is inside its grid; the quadrant sums of the
// missing ones are 0, so the mode costs need no special case.
__device__ __forceinline__ void part_store(const PartOut& o, int f, int bx, int by,
                                           const uint64_t* k) {
  const size_t f0 = (size_t)f * o.nbx * o.nby, f1 = (size_t)f * o.nbx * o.nhy;
  const size_t f2 = (size_t)f * o.nhx * o.nby, f3 = (size_t)f * o.nhx * o.nhy;
  const bool right = 2 * bx + 1 < o.nhx, bottom = 2 * by + 1 < o.nhy;
  const size_t mb = f0 + (size_t)by * o.nbx + bx;
  store_rec(o.f.mv_2nx2n, o.f.cost_2nx2n, mb, k[P_FULL]);
  store_rec(o.f.mv_2nxn, o.f.cost_2nxn, f1 + (size_t)(2 * by) * o.nbx + bx, k[P_TOP]);
  if (bottom)
    store_rec(o.f.mv_2nxn, o.f.cost_2nxn, f1 + (size_t)(2 * by + 1) * o.nbx + bx, k[P_BOT]);
  store_rec(o.f.mv_nx2n, o.f.cost_nx2n, f2 + (size_t)by * o.nhx + 2 * bx, k[P_LEFT]);
  if (right) store_rec(o.f.mv_nx2n, o.f.cost_nx2n, f2 + (size_t)by * o.nhx + 2 * bx + 1, k[P_RIGHT]);
  const size_t q = f3 + (size_t)(2 * by) * o.nhx + 2 * bx;
  store_rec(o.f.mv_nxn, o.f.cost_nxn, q, k[P_TL]);
  if (right) store_rec(o.f.mv_nxn, o.f.cost_nxn, q + 1, k[P_TR]);
  if (bottom) store_rec(o.f.mv_nxn, o.f.cost_nxn, q + o.nhx, k[P_BL]);
  if (right && bottom) store_rec(o.f.mv_nxn, o.f.cost_nxn, q + o.nhx + 1, k[P_BR]);

  auto c = [&](int p, bool there) { return there ? (uint32_t)(k[p] >> 32) : 0u; };
  const uint32_t j0 = c(P_FULL, true) + o.lambda;
  const uint32_t j1 = c(P_TOP, true) + c(P_BOT, bottom) + 2 * o.lambda;
  const uint32_t j2 = c(P_LEFT, true) + c(P_RIGHT, right) + 2 * o.lambda;
  const uint32_t j3 = c(P_TL, true) + c(P_TR, right) + c(P_BL, bottom) + c(P_BR, right && bottom) +
                      4 * o.lambda;
  uint32_t best = j0;
  int mode = ME_PART_2Nx2N;
  if (j1 < best) best = j1, mode = ME_PART_2NxN;
  if (j2 < best) best = j2, mode = ME_PART_Nx2N;
  if (j3 < best) best = j3, mode = ME_PART_NxN;
  o.f.mode[mb] = (uint8_t)mode;
  if (o.f.mode_cost) o.f.mode_cost[mb] = best;
}

// ------------------------------------------------------------------ generic
constexpr int GEN_THREADS = 256;

// One workgroup per macroblock (blockIdx.x) and frame (blockIdx.y).  The
// current block sits in LDS as rows of B bytes, zero beyond the clipped size;
// the reference is read from memory, bytes beyond the clipped block never.
// nbx_skip x nby_skip: the full-size macroblocks the fast kernel took (0 x 0:
// none); the grid then counts the rim only, the right columns of every
// macroblock row first, then the bottom rows' other macroblocks.
__global__ __launch_bounds__(GEN_THREADS) void me_part_generic_kernel(
    const uint8_t* __restrict__ ref, size_t ref_frame_stride, const uint8_t* __restrict__ cur,
    size_t cur_frame_stride, int width, int height, int stride, int B, int S, int nbx_skip,
    int nby_skip, PartOut o) {
  __shared__ uint32_t cblk[32 * 8];
  __shared__ uint64_t red[GEN_THREADS / 64][P_N];
  const int tid = threadIdx.x, f = blockIdx.y;
  int bx = (int)blockIdx.x % o.nbx, by = (int)blockIdx.x / o.nbx;
  if (nbx_skip > 0) {
    const int right = o.nbx - nbx_skip, i = (int)blockIdx.x - right * o.nby;
    if (i < 0) {
      bx = nbx_skip + (int)blockIdx.x % right, by = (int)blockIdx.x / right;
    } else {
      bx = i % nbx_skip, by = nby_skip + i / nbx_skip;
    }
  }
  const int x0 = bx * B, y0 = by * B, h = B / 2, CW = B / 4;
  const int bw = min(B, width - x0), bh = min(B, height - y0);
  ref += (size_t)f * ref_frame_stride;
  cur += (size_t)f * cur_frame_stride;

  for (int i = tid; i < B * CW; i += GEN_THREADS) {
    const int y = i / CW, xw = (i % CW) * 4;
    uint32_t w = 0;
    for (int e = 0; e < 4; e++)
      if (y < bh && xw + e < bw) w |= (uint32_t)cur[(size_t)(y0 + y) * stride + x0 + xw + e] << (8 * e);
    cblk[i] = w;
  }
  __syncthreads();

  const int cx0 = max(0, x0 - S), cx1 = min(width, x0 + bw + S) - bw;
  const int cy0 = max(0, y0 - S), cy1 = min(height, y0 + bh + S) - bh;
  const int ncx = cx1 - cx0 + 1, ncand = ncx * (cy1 - cy0 + 1);
  uint64_t best[P_N];
#pragma unroll
  for (int p = 0; p < P_N; p++) best[p] = ~0ull;
  for (int t = tid; t < ncand; t += GEN_THREADS) {
    const int cy = cy0 + t / ncx, cx = cx0 + t % ncx;
    uint32_t q[4] = {0, 0, 0, 0};  // TL, TR, BL, BR
    for (int y = 0; y < bh; y++) {
      const uint8_t* r = ref + (size_t)(cy + y) * stride + cx;
      for (int k = 0; k < CW; k++) {
        const int xw = 4 * k;
        if (xw >= bw) break;
        uint32_t w = 0;
        for (int e = 0; e < 4; e++)
          if (xw + e < bw) w |= (uint32_t)r[xw + e] << (8 * e);
        const int qi = (y >= h ? 2 : 0) + (xw >= h ? 1 : 0);  // (h is a multiple of 4)
        q[qi] = __builtin_amdgcn_sad_u8(w, cblk[y * CW + k], q[qi]);
      }
    }
    const int dx = cx - x0, dy = cy - y0;
    const uint32_t c9[P_N] = {q[0] + q[1] + q[2] + q[3], q[0] + q[1], q[2] + q[3], q[0] + q[2],
                              q[1] + q[3], q[0], q[1], q[2], q[3]};
#pragma unroll
    for (int p = 0; p < P_N; p++) {
      const uint64_t key = make_key(c9[p], dx, dy);
      best[p] = key < best[p] ? key : best[p];
    }
  }
#pragma unroll
  for (int p = 0; p < P_N; p++) {
    uint64_t v = best[p];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const uint64_t u = __shfl_xor(v, off, 64);
      v = u < v ? u : v;
    }
    if ((tid & 63) == 0) red[tid >> 6][p] = v;
  }
  __syncthreads();
  if (tid == 0) {
    uint64_t k[P_N];
#pragma unroll
    for (int p = 0; p < P_N; p++) {
      uint64_t v = red[0][p];
#pragma unroll
      for (int w = 1; w < GEN_THREADS / 64; w++) v = red[w][p] < v ? red[w][p] : v;
      k[p] = v;
    }
    part_store(o, f, bx, by, k);
  }
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
#pragma unroll
    for (int q = 0; q < 4; q++) {
      lo[P_TL + q] = (uint32_t)acc[j][q];
      hi[P_TL + q] = (uint32_t)(acc[j][q] >> 32);
    }
    auto sum = [&](int d, int a, int b) {
      lo[d] = pk_add(lo[a], lo[b]);
      hi[d] = pk_add(hi[a], hi[b]);
    };
    sum(P_TOP, P_TL, P_TR);
    sum(P_BOT, P_BL, P_BR);
    sum(P_LEFT, P_TL, P_BL);
    sum(P_RIGHT, P_TR, P_BR);
    sum(P_FULL, P_TOP, P_BOT);
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

// Workgroup (blockIdx.x, blockIdx.y, blockIdx.z) = (tile of PART_TB full-size
// macroblocks, macroblock row, frame).  Dynamic LDS: the window (rows x pitch,
// frame rows y0 - S .., columns X0 .., X0 = tile x - S - a a multiple of 4;
// zeros outside the plane's bytes, whatever the neighbouring rows hold beyond
// the frame's sides -- those candidates are masked), the tile's current blocks
// (256 bytes each), then the 9 keys per macroblock.
template <int K>
__global__ __launch_bounds__(PART_FAST_THREADS) void me_part_fast_kernel(
    const uint8_t* __restrict__ ref, size_t ref_frame_stride, const uint8_t* __restrict__ cur,
    size_t cur_frame_stride, int width, int height, int stride, int S, int nbx_full, PartOut o) {
  extern __shared__ __align__(16) uint8_t smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = PART_FAST_THREADS / 64;
  const int bx0 = (int)blockIdx.x * PART_TB, by = blockIdx.y, f = blockIdx.z;
  const int nb = min(PART_TB, nbx_full - bx0);
  const int G = partition_fast_groups(S), pitch = partition_fast_pitch(S);
  const int chunks = (2 * S + 1 + K - 1) / K, rows = chunks * K + 15;
  uint8_t* const cur_lds = smem + ((rows * pitch + 15) & ~15);
  uint64_t* const keys = reinterpret_cast<uint64_t*>(cur_lds + PART_TB * 256);
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
  if (tid < PART_TB * P_N) keys[tid] = ~0ull;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // valid displacement rows of the macroblock row; chunks wholly outside are
  // skipped (tasks are chunk-major)
  const int dymin = max(-S, -y0), dymax = min(S, height - 16 - y0);
  const int lc0 = (dymin + S) / K, lc1 = (dymax + S) / K + 1;
  const int per_chunk = nb * G, T = (lc1 - lc0) * per_chunk;
  const uint32_t lds0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) const uint8_t*)smem);
  for (int t = tid; t < T; t += PART_FAST_THREADS) {
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
    part_lane<K>(lds0 + (uint32_t)(d0 * pitch + 4 * (b * 4 + gi)), pitch, c, acc);

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
        // most lanes lose to a key already there: read before the atomic
        if (key < keys[b * P_N + p])
          atomicMin(reinterpret_cast<unsigned long long*>(&keys[b * P_N + p]),
                    (unsigned long long)key);
      }
    }
  }
  __syncthreads();
  if (tid < nb) part_store(o, f, bx0 + tid, by, keys + tid * P_N);
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
  const PartOut o = part_out(out, b.width, b.height, b.blk, lambda);
  const int nbx_full = b.width / b.blk, nby_full = b.height / b.blk;
  if (fast) {
    const int rows = partition_fast_rows(range), pitch = partition_fast_pitch(range);
    const size_t lds = (size_t)((rows * pitch + 15) & ~15) + PART_TB * 256 + PART_TB * P_N * 8;
    const dim3 grid((unsigned)((nbx_full + PART_TB - 1) / PART_TB), (unsigned)nby_full,
                    (unsigned)b.n_frames);
    hipLaunchKernelGGL(me_part_fast_kernel<PART_K>, grid, dim3(PART_FAST_THREADS), lds, stream, b.ref,
                       b.ref_frame_stride, b.cur, b.cur_frame_stride, b.width, b.height, b.stride, range,
                       nbx_full, o);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  // every macroblock, or the rim the fast kernel left: (nbx - nbx_full) right
  // columns of all rows, then nbx_full macroblocks of each clipped bottom row
  const int sx = fast ? nbx_full : 0, sy = fast ? nby_full : 0;
  const int n = fast ? (o.nbx - sx) * o.nby + sx * (o.nby - sy) : o.nbx * o.nby;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(me_part_generic_kernel, dim3((unsigned)n, (unsigned)b.n_frames),
                     dim3(GEN_THREADS), 0, stream, b.ref, b.ref_frame_stride, b.cur, b.cur_frame_stride,
                     b.width, b.height, b.stride, b.blk, range, sx, sy, o);
  return hipGetLastError();
}

hipError_t launch_partition_leaf(int width, int height, int blk, int n_frames,
                                 const me_part_fields& in, int16_t* leaf, hipStream_t stream) {
  const PartOut o = part_out(in, width, height, blk, 0);
  hipLaunchKernelGGL(me_part_leaf_kernel, dim3((unsigned)((o.nhx * o.nhy + 255) / 256), (unsigned)n_frames),
                     dim3(256), 0, stream, o, leaf);
  return hipGetLastError();
}

}  // namespace me
