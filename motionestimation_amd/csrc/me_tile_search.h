// me_tile_search.h -- device side of the tile searches: the building blocks the
// kernels of me_partition.hip and me_rd.hip are made of (geometry in
// me_tile_geom.h).  Plain inline functions and small structs, one generic
// kernel template, and the host helper that launches a search's two kernels.
// HIP translation units only.
//
//   generic   me_tile_generic_kernel<NQ, RATE, Out, STORE>: one workgroup per
//             block, one candidate per lane per step, v_sad_u8 into NQ u32 sums
//             (1: the block; 4: its quadrants, nine keys), lambda R added to
//             the cost with RATE.  Pieces: rim_block, stage_block, cand_rect,
//             wg_min_keys.
//   fast      a search's own __global__ function reads: fast_tile, fast_stage,
//             (fill_rate_x / fill_rate_y,) fast_stage_wait, then per lane-task
//             fast_task, load_block, tile_lane<K, NQ>, its keys, merge_key.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "me_kernels.h"
#include "me_rd.h"
#include "me_tile_geom.h"

namespace me {

// Key index of a macroblock's nine partitions.
enum { P_FULL = 0, P_TOP, P_BOT, P_LEFT, P_RIGHT, P_TL, P_TR, P_BL, P_BR, P_N };

typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));

// Per 16-bit half a + b (v_pk_add_u16): quadrant, half and full SADs of a
// 16 x 16 block all fit u16 (16,320 / 32,640 / 65,280).
__device__ __forceinline__ uint32_t pk_add(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, (u16x2)(__builtin_bit_cast(u16x2, a) + __builtin_bit_cast(u16x2, b)));
}

// The nine packed sums of a dy row from its quadrant accumulators q = TL, TR,
// BL, BR (four packed u16 SADs, dx 0..3, each): lo = dx 0-1, hi = dx 2-3.
__device__ __forceinline__ void nine_sums(const uint64_t (&q)[4], uint32_t (&lo)[P_N],
                                          uint32_t (&hi)[P_N]) {
#pragma unroll
  for (int i = 0; i < 4; i++) {
    lo[P_TL + i] = (uint32_t)q[i];
    hi[P_TL + i] = (uint32_t)(q[i] >> 32);
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
}

// Block `rec`'s quarter-pel predictor component c (0: x, 1: y); null: all zero.
__device__ __forceinline__ int pred_at(const int16_t* pred, size_t rec, int c) {
  return pred ? pred[2 * rec + c] : 0;
}

// ------------------------------------------------------------------ generic
constexpr int GEN_THREADS = 256;

struct BlockXY {
  int bx, by;
};

// Block i of a generic launch over an nbx x nby grid.  nbx_skip x nby_skip:
// the full-size blocks the fast kernel took (0 x 0: none); the launch then
// counts the rim only, the right columns of every block row first, then the
// bottom rows' other blocks.
__device__ __forceinline__ BlockXY rim_block(int i, int nbx, int nby, int nbx_skip, int nby_skip) {
  if (nbx_skip > 0) {
    const int right = nbx - nbx_skip, r = i - right * nby;
    if (r < 0) return {nbx_skip + i % right, i / right};
    return {r % nbx_skip, nby_skip + r / nbx_skip};
  }
  return {i % nbx, i / nbx};
}

// The block at (x0, y0) clipped to bw x bh into cblk as B rows of CW words,
// zero beyond the clipped size; ends in a barrier.
__device__ __forceinline__ void stage_block(uint32_t* cblk, const uint8_t* cur, int stride, int x0,
                                            int y0, int bw, int bh, int B, int CW) {
  for (int i = threadIdx.x; i < B * CW; i += GEN_THREADS) {
    const int y = i / CW, xw = (i % CW) * 4;
    uint32_t w = 0;
    for (int e = 0; e < 4; e++)
      if (y < bh && xw + e < bw) w |= (uint32_t)cur[(size_t)(y0 + y) * stride + x0 + xw + e] << (8 * e);
    cblk[i] = w;
  }
  __syncthreads();
}

// Top-left corners of the block's candidates, raster order: the search square
// clipped to the frame.
struct CandRect {
  int cx0, cy0, ncx, ncand;
};
__device__ __forceinline__ CandRect cand_rect(int width, int height, int x0, int y0, int bw, int bh,
                                              int S) {
  const int cx0 = max(0, x0 - S), cx1 = min(width, x0 + bw + S) - bw;
  const int cy0 = max(0, y0 - S), cy1 = min(height, y0 + bh + S) - bh;
  const int ncx = cx1 - cx0 + 1;
  return {cx0, cy0, ncx, ncx * (cy1 - cy0 + 1)};
}

// The workgroup's minimum of each of the lanes' NK keys, left in thread 0's
// best: wave shuffle-min, then the waves' minima through red.
template <int NK>
__device__ __forceinline__ void wg_min_keys(uint64_t (&best)[NK], uint64_t (*red)[NK]) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int p = 0; p < NK; p++) {
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
#pragma unroll
    for (int p = 0; p < NK; p++) {
      uint64_t v = red[0][p];
#pragma unroll
      for (int w = 1; w < GEN_THREADS / 64; w++) v = red[w][p] < v ? red[w][p] : v;
      best[p] = v;
    }
  }
}

// One workgroup per block (blockIdx.x, by rim_block) and frame (blockIdx.y).
// NQ = 1: B in [1, 64], one key; NQ = 4: B in {8, 16, 32}, quadrant sums and
// the nine keys of P_*.  RATE: cost + lambda (bits(4 dx - px) + bits(4 dy -
// py)) against the block's predictor o.pred (B = 32, lambda = 2^23: 261,120 +
// 66 * 2^23 < 2^32).  The current block sits in LDS; the reference is read
// from memory, bytes beyond the clipped block never.  Out: nbx, nby, lambda
// (and pred); STORE(o, f, bx, by, keys), with RATE STORE(o, f, bx, by, keys,
// px, py), writes the block's records.
template <int NQ, bool RATE, typename Out, auto STORE>
__global__ __launch_bounds__(GEN_THREADS) void me_tile_generic_kernel(
    const uint8_t* __restrict__ ref, size_t ref_frame_stride, const uint8_t* __restrict__ cur,
    size_t cur_frame_stride, int width, int height, int stride, int B, int S, int nbx_skip,
    int nby_skip, Out o) {
  static_assert(NQ == 1 || NQ == 4, "a block's sum or its quadrants'");
  constexpr int NK = NQ == 4 ? P_N : 1;
  __shared__ uint32_t cblk[NQ == 4 ? 32 * 8 : ME_MAX_BLOCK * ME_MAX_BLOCK / 4];
  __shared__ uint64_t red[GEN_THREADS / 64][NK];
  const int tid = threadIdx.x, f = blockIdx.y;
  const BlockXY m = rim_block((int)blockIdx.x, o.nbx, o.nby, nbx_skip, nby_skip);
  const int x0 = m.bx * B, y0 = m.by * B, h = B / 2, CW = (B + 3) / 4;
  const int bw = min(B, width - x0), bh = min(B, height - y0);
  int px = 0, py = 0;
  if constexpr (RATE) {
    const size_t rec = (size_t)f * o.nbx * o.nby + (size_t)m.by * o.nbx + m.bx;
    px = pred_at(o.pred, rec, 0), py = pred_at(o.pred, rec, 1);
  }
  ref += (size_t)f * ref_frame_stride;
  cur += (size_t)f * cur_frame_stride;
  stage_block(cblk, cur, stride, x0, y0, bw, bh, B, CW);

  const CandRect r = cand_rect(width, height, x0, y0, bw, bh, S);
  uint64_t best[NK];
#pragma unroll
  for (int p = 0; p < NK; p++) best[p] = ~0ull;
  for (int t = tid; t < r.ncand; t += GEN_THREADS) {
    const int cy = r.cy0 + t / r.ncx, cx = r.cx0 + t % r.ncx;
    uint32_t q[NQ] = {};  // the block, or TL, TR, BL, BR
    for (int y = 0; y < bh; y++) {
      const uint8_t* rr = ref + (size_t)(cy + y) * stride + cx;
      for (int k = 0; k < CW; k++) {
        const int xw = 4 * k;
        if (xw >= bw) break;
        uint32_t w = 0;
        for (int e = 0; e < 4; e++)
          if (xw + e < bw) w |= (uint32_t)rr[xw + e] << (8 * e);
        const int qi = NQ == 4 ? (y >= h ? 2 : 0) + (xw >= h ? 1 : 0) : 0;  // (h is a multiple of 4)
        q[qi] = __builtin_amdgcn_sad_u8(w, cblk[y * CW + k], q[qi]);
      }
    }
    const int dx = cx - x0, dy = cy - y0;
    uint32_t lr = 0;
    if constexpr (RATE) lr = o.lambda * (uint32_t)(rd_bits(4 * dx - px) + rd_bits(4 * dy - py));
    uint32_t c[NK] = {q[0]};
    if constexpr (NQ == 4) {
      c[P_FULL] = q[0] + q[1] + q[2] + q[3];
      c[P_TOP] = q[0] + q[1], c[P_BOT] = q[2] + q[3], c[P_LEFT] = q[0] + q[2], c[P_RIGHT] = q[1] + q[3];
#pragma unroll
      for (int i = 0; i < 4; i++) c[P_TL + i] = q[i];
    }
#pragma unroll
    for (int p = 0; p < NK; p++) {
      const uint64_t key = make_key(c[p] + lr, dx, dy);
      best[p] = key < best[p] ? key : best[p];
    }
  }
  wg_min_keys(best, red);
  if (tid == 0) {
    if constexpr (RATE) STORE(o, f, m.bx, m.by, best, px, py);
    else STORE(o, f, m.bx, m.by, best);
  }
}

// --------------------------------------------------------------------- fast
// A fast kernel's workgroup: (blockIdx.x, blockIdx.y, blockIdx.z) = (tile of
// TILE_TB full-size blocks, block row, frame).  Its dynamic LDS opens with the
// window (rows x pitch: frame rows y0 - S .., columns X0 .., X0 = tile x - S -
// a a multiple of 4; zeros outside the plane's bytes, whatever the neighbouring
// rows hold beyond the frame's sides -- those candidates are no candidates),
// then the tile's current blocks (256 bytes each) and the search's keys; what
// follows is the search's own.
struct FastTile {
  int bx0, by, f, nb;        // first block, block row, frame, blocks (short at the row's end)
  int G, pitch, chunks, rows;
  int y0, a, X0;
  int dymin, dymax;          // valid displacement rows of the block row
  int lc0, lc1;              // its dy chunks: those wholly outside are skipped
  uint8_t* cur_lds;
  uint64_t* keys;
};

template <int K>
__device__ __forceinline__ FastTile fast_tile(uint8_t* smem, int S, int nbx_full, int height) {
  FastTile t;
  t.bx0 = (int)blockIdx.x * TILE_TB, t.by = blockIdx.y, t.f = blockIdx.z;
  t.nb = min(TILE_TB, nbx_full - t.bx0);
  t.G = tile_groups(S), t.pitch = tile_pitch(S);
  t.chunks = tile_chunks(S, K), t.rows = t.chunks * K + 15;
  t.y0 = t.by * 16;
  t.a = ((t.bx0 * 16 - S) % 4 + 4) % 4;
  t.X0 = t.bx0 * 16 - S - t.a;
  t.dymin = max(-S, -t.y0), t.dymax = min(S, height - 16 - t.y0);
  t.lc0 = (t.dymin + S) / K, t.lc1 = (t.dymax + S) / K + 1;
  t.cur_lds = smem + ((t.rows * t.pitch + 15) & ~15);
  t.keys = reinterpret_cast<uint64_t*>(t.cur_lds + TILE_TB * 256);
  return t;
}

// Starts the LDS DMA of the window and the tile's current blocks;
// fast_stage_wait ends it.
__device__ __forceinline__ void fast_stage(const FastTile& t, uint8_t* smem, const uint8_t* ref,
                                           size_t ref_frame_stride, const uint8_t* cur,
                                           size_t cur_frame_stride, int width, int height,
                                           int stride, int S) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int NW = TILE_THREADS / 64;
  // plane bytes of one frame: granules (4 bytes, 4-aligned: width and pitch
  // are multiples of 4) wholly inside or wholly outside
  const uint32_t plane = (uint32_t)(stride * (height - 1) + width);
  const __amdgpu_buffer_rsrc_t rref = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(ref + (size_t)t.f * ref_frame_stride), (short)0, plane, 0x00020000);
  const __amdgpu_buffer_rsrc_t rcur = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(cur + (size_t)t.f * cur_frame_stride), (short)0, plane, 0x00020000);
  // window row r <- frame row y0 - S + r, one DMA step per row (pitch <= 256);
  // offsets before the plane wrap to huge ones: the range check returns zeros
  // (unsigned arithmetic: a wrapped offset is in range or zeroed, never a fault)
  for (int r = wave; r < t.rows; r += NW) {
    if (4 * lane < t.pitch)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rref, (__attribute__((address_space(3))) void*)(smem + r * t.pitch), 4,
          (uint32_t)(t.y0 - S + r) * (uint32_t)stride + (uint32_t)(t.X0 + 4 * lane), 0, 0, 0);
  }
  // current block b, row y -> LDS bytes (b * 16 + y) * 16: one block (64
  // granules, 256 bytes) per DMA step
  for (int b = wave; b < t.nb; b += NW) {
    const int y = lane >> 2, xw = (lane & 3) * 4;
    __builtin_amdgcn_raw_ptr_buffer_load_lds(
        rcur, (__attribute__((address_space(3))) void*)(t.cur_lds + b * 256), 4,
        (uint32_t)((t.y0 + y) * stride + (t.bx0 + b) * 16 + xw), 0, 0, 0);
  }
}
__device__ __forceinline__ void fast_stage_wait() {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
}

// The rate tables of a tile whose first block's record is rec0 (the rate is
// separable, so a lane reads 4 + K words per task): per block 4 G words
// lambda bits(4 dx - px) for the window columns q = dx + S + a (fill_rate_x),
// and chunks * K words lambda bits(4 dy - py) for the rows d = dy + S
// (fill_rate_y); ~0 where dx or dy is not among the block's candidates
// (whatever the window holds there).  INDEX: the entry << 6 | the lane key's
// index bits, q & 3 and 4 (d % K).
template <bool INDEX>
__device__ __forceinline__ void fill_rate_x(uint32_t* rxt, const FastTile& t, int S, int width,
                                            const int16_t* pred, size_t rec0, uint32_t lambda) {
  for (int i = threadIdx.x; i < t.nb * 4 * t.G; i += TILE_THREADS) {
    const int b = i / (4 * t.G), q = i - b * 4 * t.G, dx = q - S - t.a, x0 = (t.bx0 + b) * 16;
    const bool ok = dx >= max(-S, -x0) && dx <= min(S, width - 16 - x0);
    const uint32_t lr = lambda * (uint32_t)rd_bits(4 * dx - pred_at(pred, rec0 + b, 0));
    rxt[i] = !ok ? ~0u : INDEX ? (lr << 6) + (uint32_t)(q & 3) : lr;
  }
}
template <int K, bool INDEX>
__device__ __forceinline__ void fill_rate_y(uint32_t* ryt, const FastTile& t, int S,
                                            const int16_t* pred, size_t rec0, uint32_t lambda) {
  for (int i = threadIdx.x; i < t.nb * t.chunks * K; i += TILE_THREADS) {
    const int b = i / (t.chunks * K), d = i - b * t.chunks * K, dy = d - S;
    const bool ok = dy >= t.dymin && dy <= t.dymax;
    const uint32_t lr = lambda * (uint32_t)rd_bits(4 * dy - pred_at(pred, rec0 + b, 1));
    ryt[i] = !ok ? ~0u : INDEX ? (lr << 6) + (uint32_t)(4 * (d % K)) : lr;
  }
}

// Lane-task i of the tile's fast_tasks (chunk-major): block b of the tile, dx
// group gi, first dy row d0 (as dy + S).
struct FastTask {
  int b, gi, d0;
};
__device__ __forceinline__ int fast_tasks(const FastTile& t) { return (t.lc1 - t.lc0) * t.nb * t.G; }
template <int K>
__device__ __forceinline__ FastTask fast_task(const FastTile& t, int i) {
  const int per_chunk = t.nb * t.G;
  const int lcr = i / per_chunk, rem = i - lcr * per_chunk;
  const int b = rem / t.G;
  return {b, rem - b * t.G, (t.lc0 + lcr) * K};
}
// LDS byte address of the task's first window row and the word of its first dx.
__device__ __forceinline__ uint32_t fast_task_at(const uint8_t* smem, const FastTile& t,
                                                 const FastTask& k) {
  const uint32_t lds0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) const uint8_t*)smem);
  return lds0 + (uint32_t)(k.d0 * t.pitch + 4 * (k.b * 4 + k.gi));
}

// Current block b of the tile into 64 VGPRs.
__device__ __forceinline__ void load_block(const uint8_t* cur_lds, int b, uint32_t (&c)[16][4]) {
#pragma unroll
  for (int y = 0; y < 16; y++) {
    const uint4 v = reinterpret_cast<const uint4*>(cur_lds)[b * 16 + y];
    c[y][0] = v.x, c[y][1] = v.y, c[y][2] = v.z, c[y][3] = v.w;
  }
}

// A lane's key into its block's LDS slot.  Most lanes lose to a key already
// there: read before the atomic.
__device__ __forceinline__ void merge_key(uint64_t* slot, uint64_t key) {
  if (key < *slot) atomicMin(reinterpret_cast<unsigned long long*>(slot), (unsigned long long)key);
}

// Orders row YY's qsads before the next row's (volatile) address step: see
// pin_rows of me_kernels.hip.
template <int J, int K, int NQ, int YY>
__device__ __forceinline__ void pin_rows(uint64_t (&acc)[K][NQ]) {
  if constexpr (J < K) {
    if constexpr (YY - J >= 0 && YY - J < 16) {
      if constexpr (NQ == 4)
        asm volatile("" : "+v"(acc[J][(YY - J) >= 8 ? 2 : 0]), "+v"(acc[J][(YY - J) >= 8 ? 3 : 1]));
      else
        asm volatile("" : "+v"(acc[J][0]));
    }
    pin_rows<J + 1, K, NQ, YY>(acc);
  }
}

// The lane's 4 dx x K dy candidates of a 16 x 16 block c: LDS byte address
// `at` is window row (first dy row) and the word of the lane's first dx.
// acc[j][q]: four packed u16 SADs (dx 0..3) of dy row j; NQ = 1: the block's,
// NQ = 4: q = TL, TR, BL, BR (segments 0-1 / 2-3 of a row are left / right,
// rows 0-7 / 8-15 top / bottom), the same 64 qsads either way.  The row walk is
// qsad_lane's of me_kernels.hip (one segment per window row: the next row's
// four ds_read2_b32, then this row's qsads).
template <int K, int NQ>
__device__ __forceinline__ void tile_lane(uint32_t at, int pitch, const uint32_t (&c)[16][4],
                                          uint64_t (&acc)[K][NQ]) {
  static_assert(NQ == 1 || NQ == 4, "a block's sum or its quadrants'");
  constexpr int NR = K + 15;
  uint32_t oe = at, oo = at + 4;
  asm volatile("" : "+v"(oo));
#pragma unroll
  for (int j = 0; j < K; j++)
#pragma unroll
    for (int q = 0; q < NQ; q++) acc[j][q] = 0;
  typedef __attribute__((address_space(3))) const uint32_t lds_u32;
  auto load = [&](uint64_t (&dst)[4]) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      lds_u32* w = reinterpret_cast<lds_u32*>((uintptr_t)((k & 1) ? oo : oe)) + 2 * (k >> 1);
      dst[k] = ((uint64_t)w[1] << 32) | w[0];
    }
  };
  uint64_t pr[4], nx[4];
  load(pr);
  static_for<0, NR>([&](auto YY) {
    constexpr int yy = decltype(YY)::value;
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (yy + 1 < NR) {
      oe += pitch;
      oo += pitch;
      asm volatile("" : "+v"(oe), "+v"(oo));
      load(nx);
    }
    static_for<0, 4>([&](auto KK) {
      constexpr int k = decltype(KK)::value;
      static_for<0, K>([&](auto JJ) {
        constexpr int j = decltype(JJ)::value;
        constexpr int y = yy - j;
        if constexpr (y >= 0 && y < 16) {
          constexpr int q = NQ == 4 ? (y >= 8 ? 2 : 0) + (k >= 2 ? 1 : 0) : 0;
          acc[j][q] = __builtin_amdgcn_qsad_pk_u16_u8(pr[k], c[y][k], acc[j][q]);
        }
      });
    });
    pin_rows<0, K, NQ, yy>(acc);
    if constexpr (yy + 1 < NR) {
#pragma unroll
      for (int k = 0; k < 4; k++) pr[k] = nx[k];
    }
  });
}

// ----------------------------------------------------------------- launcher
template <typename Out>
using FastKernel = void (*)(const uint8_t*, size_t, const uint8_t*, size_t, int, int, int, int, int, Out);
template <typename Out>
using GenericKernel = void (*)(const uint8_t*, size_t, const uint8_t*, size_t, int, int, int, int, int,
                               int, int, Out);

// A search over the batch's o.nbx x o.nby blocks: with `fast` the full-size
// blocks on fk (lds bytes of dynamic LDS) and the rim it leaves on gk -- the
// (nbx - nbx_full) right columns of all rows, then nbx_full blocks of each
// clipped bottom row (rim_block) -- else every block on gk.
template <typename Out>
hipError_t launch_tile_search(const FrameBatch& b, int range, bool fast, FastKernel<Out> fk,
                              size_t lds, GenericKernel<Out> gk, const Out& o, hipStream_t stream) {
  const int nbx = o.nbx, nby = o.nby, nbx_full = b.width / b.blk, nby_full = b.height / b.blk;
  if (fast) {
    const dim3 grid((unsigned)((nbx_full + TILE_TB - 1) / TILE_TB), (unsigned)nby_full,
                    (unsigned)b.n_frames);
    hipLaunchKernelGGL(fk, grid, dim3(TILE_THREADS), lds, stream, b.ref, b.ref_frame_stride, b.cur,
                       b.cur_frame_stride, b.width, b.height, b.stride, range, nbx_full, o);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  const int sx = fast ? nbx_full : 0, sy = fast ? nby_full : 0;
  const int n = fast ? (nbx - sx) * nby + sx * (nby - sy) : nbx * nby;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(gk, dim3((unsigned)n, (unsigned)b.n_frames), dim3(GEN_THREADS), 0, stream, b.ref,
                     b.ref_frame_stride, b.cur, b.cur_frame_stride, b.width, b.height, b.stride, b.blk,
                     range, sx, sy, o);
  return hipGetLastError();
}

}  // namespace me
