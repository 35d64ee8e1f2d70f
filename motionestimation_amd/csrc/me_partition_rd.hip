// me_partition_rd.hip -- rate-constrained partition search (include/me.h
// "rate-constrained partition search"; DESIGN.md "Rate-constrained partition
// search").  No reference counterpart.
//
// The partition search of me_partition.hip with J_p(d) = SAD_p(d) + lambda R(d)
// in the nine running minima, R(d) = bits(4 dx - px) + bits(4 dy - py) against
// the macroblock's quarter-pel predictor (rd_bits of me_rd.h): one rate per
// displacement, shared by the nine partitions.  The minima use the packed key
// of me_kernels.h on J_p,
//     key = J << 32 | (dy + 32768) << 16 | (dx + 32768),
// so the unsigned minimum is the smallest J and, among equal J, the first
// displacement in raster order.  The thread that writes a macroblock's records
// recomputes R from each winning displacement (dist = J - lambda R) and decides
// the mode on sum J_p + lambda mbits(m), mbits = (1, 3, 3, 5).
//
// Kernels:
//   me_part_rd_fast_kernel<K>  B = 16, full-size macroblocks, S <= 64, rows a
//                              multiple of 4 bytes, lambda <=
//                              ME_RD_FAST_MAX_LAMBDA.  me_part_fast_kernel's
//                              staging, tiling and row walk (part_lane of
//                              me_partition_lane.h: four packed-u16 quadrant
//                              accumulators per dy row) with me_rd_fast_kernel's
//                              rate tables in LDS: lambda bits(4 dx - px) per
//                              window column and lambda bits(4 dy - py) per row
//                              of every macroblock, ~0 where the column or row
//                              is no candidate.  Per dy row and dx one
//                              saturating r = rx + ry, then per partition one
//                              saturating J = sad + r and the lane key
//                              J << 6 | 4 j + i: an invalid candidate's J is
//                              ~0, its key at least 0xFFFFFFC0, above every
//                              valid one (J < 2^26 - 1); no compare, mask or
//                              branch per candidate.
//   me_part_rd_generic_kernel  B in {8, 16, 32}, any S <= 128, clipped
//                              macroblocks, any pitch and lambda: one
//                              workgroup per macroblock, one candidate per lane
//                              per step, v_sad_u8 into u32 quadrant sums, R per
//                              candidate.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "me.h"
#include "me_kernels.h"
#include "me_partition.h"
#include "me_partition_lane.h"
#include "me_rd.h"

namespace me {
namespace {

struct PartRdOut {
  me_part_rd_fields f;
  const int16_t* pred;  // null: all zero
  int nbx, nby, nhx, nhy;
  uint32_t lambda;
};

// Every lane key of a valid candidate is below this one (J < 2^26 - 1).
constexpr uint32_t LANE_KEY_INVALID = 0xFFFFFFC0u;

// A cell's record from its key and the macroblock's predictor; returns J.
__device__ __forceinline__ uint32_t store_rd_rec(int16_t* mv, uint32_t* cost, uint32_t* dist,
                                                 uint8_t* bits, size_t at, uint64_t key,
                                                 uint32_t lambda, int px, int py) {
  const int dx = (int)(key & 0xFFFF) - 32768, dy = (int)((key >> 16) & 0xFFFF) - 32768;
  const uint32_t r = (uint32_t)(rd_bits(4 * dx - px) + rd_bits(4 * dy - py));
  const uint32_t j = (uint32_t)(key >> 32);
  store_mv(mv + 2 * at, 0, key);
  if (cost) cost[at] = j;
  if (dist) dist[at] = j - lambda * r;
  if (bits) bits[at] = (uint8_t)r;
  return j;
}

// Records and mode of macroblock (bx, by) of frame f from its nine keys.  A
// partition exists iff its cell is inside its grid; the missing ones add
// nothing to a mode's J.
__device__ __forceinline__ void part_rd_store(const PartRdOut& o, int f, int bx, int by,
                                              const uint64_t* k) {
  const size_t f0 = (size_t)f * o.nbx * o.nby, f1 = (size_t)f * o.nbx * o.nhy;
  const size_t f2 = (size_t)f * o.nhx * o.nby, f3 = (size_t)f * o.nhx * o.nhy;
  const bool right = 2 * bx + 1 < o.nhx, bottom = 2 * by + 1 < o.nhy;
  const size_t mb = f0 + (size_t)by * o.nbx + bx;
  const int px = o.pred ? o.pred[2 * mb] : 0, py = o.pred ? o.pred[2 * mb + 1] : 0;
  const me_part_rd_fields& F = o.f;
  auto g0 = [&](size_t at, int p) {
    return store_rd_rec(F.f.mv_2nx2n, F.f.cost_2nx2n, F.dist_2nx2n, F.bits_2nx2n, at, k[p],
                        o.lambda, px, py);
  };
  auto g1 = [&](size_t at, int p) {
    return store_rd_rec(F.f.mv_2nxn, F.f.cost_2nxn, F.dist_2nxn, F.bits_2nxn, at, k[p], o.lambda,
                        px, py);
  };
  auto g2 = [&](size_t at, int p) {
    return store_rd_rec(F.f.mv_nx2n, F.f.cost_nx2n, F.dist_nx2n, F.bits_nx2n, at, k[p], o.lambda,
                        px, py);
  };
  auto g3 = [&](size_t at, int p) {
    return store_rd_rec(F.f.mv_nxn, F.f.cost_nxn, F.dist_nxn, F.bits_nxn, at, k[p], o.lambda, px,
                        py);
  };
  const uint32_t j0 = g0(mb, P_FULL) + o.lambda;
  uint32_t j1 = g1(f1 + (size_t)(2 * by) * o.nbx + bx, P_TOP) + 3 * o.lambda;
  if (bottom) j1 += g1(f1 + (size_t)(2 * by + 1) * o.nbx + bx, P_BOT);
  uint32_t j2 = g2(f2 + (size_t)by * o.nhx + 2 * bx, P_LEFT) + 3 * o.lambda;
  if (right) j2 += g2(f2 + (size_t)by * o.nhx + 2 * bx + 1, P_RIGHT);
  const size_t q = f3 + (size_t)(2 * by) * o.nhx + 2 * bx;
  uint32_t j3 = g3(q, P_TL) + 5 * o.lambda;
  if (right) j3 += g3(q + 1, P_TR);
  if (bottom) j3 += g3(q + o.nhx, P_BL);
  if (right && bottom) j3 += g3(q + o.nhx + 1, P_BR);

  uint32_t best = j0;
  int mode = ME_PART_2Nx2N;
  if (j1 < best) best = j1, mode = ME_PART_2NxN;
  if (j2 < best) best = j2, mode = ME_PART_Nx2N;
  if (j3 < best) best = j3, mode = ME_PART_NxN;
  F.f.mode[mb] = (uint8_t)mode;
  if (F.f.mode_cost) F.f.mode_cost[mb] = best;
}

// ------------------------------------------------------------------ generic
constexpr int GEN_THREADS = 256;

// me_part_generic_kernel with the rate in the keys.  One workgroup per
// macroblock (blockIdx.x) and frame (blockIdx.y).  The current block sits in
// LDS as rows of B bytes, zero beyond the clipped size; the reference is read
// from memory, bytes beyond the clipped block never.  nbx_skip x nby_skip: the
// full-size macroblocks the fast kernel took (0 x 0: none); the grid then
// counts the rim only, the right columns of every macroblock row first, then
// the bottom rows' other macroblocks.
__global__ __launch_bounds__(GEN_THREADS) void me_part_rd_generic_kernel(
    const uint8_t* __restrict__ ref, size_t ref_frame_stride, const uint8_t* __restrict__ cur,
    size_t cur_frame_stride, int width, int height, int stride, int B, int S, int nbx_skip,
    int nby_skip, PartRdOut o) {
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
  const size_t mb = (size_t)f * o.nbx * o.nby + (size_t)by * o.nbx + bx;
  const int px = o.pred ? o.pred[2 * mb] : 0, py = o.pred ? o.pred[2 * mb + 1] : 0;
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
    // B = 32, lambda = 2^23: 261,120 + 66 * 2^23 < 2^32
    const uint32_t lr = o.lambda * (uint32_t)(rd_bits(4 * dx - px) + rd_bits(4 * dy - py));
    const uint32_t c9[P_N] = {q[0] + q[1] + q[2] + q[3], q[0] + q[1], q[2] + q[3], q[0] + q[2],
                              q[1] + q[3], q[0], q[1], q[2], q[3]};
#pragma unroll
    for (int p = 0; p < P_N; p++) {
      const uint64_t key = make_key(c9[p] + lr, dx, dy);
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
    part_rd_store(o, f, bx, by, k);
  }
}

// --------------------------------------------------------------------- fast
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

// Workgroup (blockIdx.x, blockIdx.y, blockIdx.z) = (tile of PART_TB full-size
// macroblocks, macroblock row, frame).  Dynamic LDS: me_part_fast_kernel's
// (the window, rows x pitch, frame rows y0 - S .., columns X0 .., X0 = tile x -
// S - a a multiple of 4, zeros outside the plane's bytes; the tile's current
// blocks, 256 bytes each; the 9 keys per macroblock), then the rate tables of
// me_rd_fast_kernel without the index bits: per macroblock 4 G words
// lambda bits(4 dx - px) for the window columns q = dx + S + a and chunks * K
// words lambda bits(4 dy - py) for the rows d = dy + S; ~0 where dx or dy is
// not among the macroblock's candidates (whatever the window holds there).
template <int K>
__global__ __launch_bounds__(PART_FAST_THREADS) void me_part_rd_fast_kernel(
    const uint8_t* __restrict__ ref, size_t ref_frame_stride, const uint8_t* __restrict__ cur,
    size_t cur_frame_stride, int width, int height, int stride, int S, int nbx_full,
    PartRdOut o) {
  extern __shared__ __align__(16) uint8_t smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = PART_FAST_THREADS / 64;
  const int bx0 = (int)blockIdx.x * PART_TB, by = blockIdx.y, f = blockIdx.z;
  const int nb = min(PART_TB, nbx_full - bx0);
  const int G = partition_fast_groups(S), pitch = partition_fast_pitch(S);
  const int chunks = (2 * S + 1 + K - 1) / K, rows = chunks * K + 15;
  uint8_t* const cur_lds = smem + ((rows * pitch + 15) & ~15);
  uint64_t* const keys = reinterpret_cast<uint64_t*>(cur_lds + PART_TB * 256);
  uint32_t* const rxt = reinterpret_cast<uint32_t*>(keys + PART_TB * P_N);
  uint32_t* const ryt = rxt + PART_TB * 4 * G;
  const int y0 = by * 16;
  const int a = ((bx0 * 16 - S) % 4 + 4) % 4;
  const int X0 = bx0 * 16 - S - a;
  const size_t mb0 = (size_t)f * o.nbx * o.nby + (size_t)by * o.nbx + bx0;

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
  // valid displacement rows of the macroblock row
  const int dymin = max(-S, -y0), dymax = min(S, height - 16 - y0);
  for (int i = tid; i < nb * 4 * G; i += PART_FAST_THREADS) {
    const int b = i / (4 * G), q = i - b * 4 * G, dx = q - S - a, x0 = (bx0 + b) * 16;
    const int px = o.pred ? o.pred[2 * (mb0 + b)] : 0;
    const bool ok = dx >= max(-S, -x0) && dx <= min(S, width - 16 - x0);
    rxt[i] = ok ? o.lambda * (uint32_t)rd_bits(4 * dx - px) : ~0u;
  }
  for (int i = tid; i < nb * chunks * K; i += PART_FAST_THREADS) {
    const int b = i / (chunks * K), d = i - b * chunks * K, dy = d - S;
    const int py = o.pred ? o.pred[2 * (mb0 + b) + 1] : 0;
    const bool ok = dy >= dymin && dy <= dymax;
    ryt[i] = ok ? o.lambda * (uint32_t)rd_bits(4 * dy - py) : ~0u;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // chunks wholly outside the valid rows are skipped (tasks are chunk-major)
  const int lc0 = (dymin + S) / K, lc1 = (dymax + S) / K + 1;
  const int per_chunk = nb * G, T = (lc1 - lc0) * per_chunk;
  const uint32_t lds0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) const uint8_t*)smem);
  for (int t = tid; t < T; t += PART_FAST_THREADS) {
    const int lcr = t / per_chunk, rem = t - lcr * per_chunk;
    const int b = rem / G, gi = rem - b * G;
    const int d0 = (lc0 + lcr) * K;  // first dy row of the task, as dy + S
    uint32_t c[16][4];
#pragma unroll
    for (int y = 0; y < 16; y++) {
      const uint4 v = reinterpret_cast<const uint4*>(cur_lds)[b * 16 + y];
      c[y][0] = v.x, c[y][1] = v.y, c[y][2] = v.z, c[y][3] = v.w;
    }
    uint64_t acc[K][4];
    part_lane<K>(lds0 + (uint32_t)(d0 * pitch + 4 * (b * 4 + gi)), pitch, c, acc);

    const int dxg = 4 * gi - S - a;  // dx of the lane's first candidate
    const uint4 rv = reinterpret_cast<const uint4*>(rxt)[b * G + gi];
    const uint32_t rx[4] = {rv.x, rv.y, rv.z, rv.w};
    uint32_t best[P_N];
    part_rd_lane_keys<K>(acc, rx, ryt + b * chunks * K + d0, best);
#pragma unroll
    for (int p = 0; p < P_N; p++) {
      if (best[p] < LANE_KEY_INVALID) {
        const int idx = (int)(best[p] & 63u);
        const uint64_t key = make_key(best[p] >> 6, dxg + (idx & 3), d0 + (idx >> 2) - S);
        // most lanes lose to a key already there: read before the atomic
        if (key < keys[b * P_N + p])
          atomicMin(reinterpret_cast<unsigned long long*>(&keys[b * P_N + p]),
                    (unsigned long long)key);
      }
    }
  }
  __syncthreads();
  if (tid < nb) part_rd_store(o, f, bx0 + tid, by, keys + tid * P_N);
}

}  // namespace

hipError_t launch_partition_rd_search(const FrameBatch& b, int range, uint32_t lambda, bool fast,
                                      const int16_t* pred, const me_part_rd_fields& out,
                                      hipStream_t stream) {
  const int h = b.blk / 2;
  const PartRdOut o{out, pred, (b.width + b.blk - 1) / b.blk, (b.height + b.blk - 1) / b.blk,
                    (b.width + h - 1) / h, (b.height + h - 1) / h, lambda};
  const int nbx_full = b.width / b.blk, nby_full = b.height / b.blk;
  if (fast) {
    const int rows = partition_rd_fast_rows(range), pitch = partition_fast_pitch(range);
    // window, current blocks, keys, then the rate tables (4 G + rows - 15 words
    // per macroblock)
    const size_t lds = (size_t)((rows * pitch + 15) & ~15) + PART_TB * 256 + PART_TB * P_N * 8 +
                       (size_t)PART_TB * 4 * (4 * partition_fast_groups(range) + rows - 15);
    const dim3 grid((unsigned)((nbx_full + PART_TB - 1) / PART_TB), (unsigned)nby_full,
                    (unsigned)b.n_frames);
    hipLaunchKernelGGL(me_part_rd_fast_kernel<PART_RD_K>, grid, dim3(PART_FAST_THREADS), lds,
                       stream, b.ref, b.ref_frame_stride, b.cur, b.cur_frame_stride, b.width, b.height, b.stride,
                       range, nbx_full, o);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  // every macroblock, or the rim the fast kernel left: (nbx - nbx_full) right
  // columns of all rows, then nbx_full macroblocks of each clipped bottom row
  const int sx = fast ? nbx_full : 0, sy = fast ? nby_full : 0;
  const int n = fast ? (o.nbx - sx) * o.nby + sx * (o.nby - sy) : o.nbx * o.nby;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(me_part_rd_generic_kernel, dim3((unsigned)n, (unsigned)b.n_frames),
                     dim3(GEN_THREADS), 0, stream, b.ref, b.ref_frame_stride, b.cur, b.cur_frame_stride,
                     b.width, b.height, b.stride, b.blk, range, sx, sy, o);
  return hipGetLastError();
}

}  // namespace me
