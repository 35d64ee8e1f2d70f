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
// Kernels:
//   me_rd_fast_kernel<K>  B = 16, full-size blocks, S <= 64, rows a multiple of
//                         4 bytes, lambda <= ME_RD_FAST_MAX_LAMBDA; K = 6 or 10
//                         by the range (rd_fast_k).  The me_part_fast_kernel
//                         scheme: a workgroup takes RD_TB blocks of one row,
//                         their union window is staged once in LDS by LDS DMA,
//                         a lane holds its block in 64 VGPRs and owns 4 dx x K
//                         dy candidates, walking the K + 15 window rows with
//                         v_qsad_pk_u16_u8 into one packed-u16 accumulator per
//                         dy row.  The rate is separable: the workgroup
//                         tabulates lambda bits(4 dx - px) per window column
//                         and lambda bits(4 dy - py) per row in LDS (~0 for a
//                         column or row that is no candidate), a lane reads its
//                         4 + K entries; J is a 32-bit saturating sum per
//                         candidate, the lane key J << 6 | 4 j + i.
//   me_rd_generic_kernel  B in [1, 64], any S <= 128, clipped blocks, any pitch
//                         and lambda: one workgroup per block, one candidate
//                         per lane per step, v_sad_u8 into a u32 sum.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "me.h"
#include "me_kernels.h"
#include "me_rd.h"

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

// Block `rec`'s record from its winning key and predictor.
__device__ __forceinline__ void rd_store(const RdOut& o, size_t rec, uint64_t key, int px, int py) {
  const int dx = (int)(key & 0xFFFF) - 32768, dy = (int)((key >> 16) & 0xFFFF) - 32768;
  const uint32_t r = (uint32_t)(rd_bits(4 * dx - px) + rd_bits(4 * dy - py));
  const uint32_t j = (uint32_t)(key >> 32);
  store_mv(o.mv + 2 * rec, 0, key);
  o.cost[rec] = j;
  if (o.dist) o.dist[rec] = j - o.lambda * r;
  if (o.bits) o.bits[rec] = (uint8_t)r;
}

// ------------------------------------------------------------------ generic
constexpr int GEN_THREADS = 256;

// One workgroup per block (blockIdx.x) and frame (blockIdx.y).  The current
// block sits in LDS as rows of CW words, zero beyond the clipped size; the
// reference is read from memory, bytes beyond the clipped block never.
// nbx_skip x nby_skip: the full-size blocks the fast kernel took (0 x 0: none);
// the grid then counts the rim only, the right columns of every block row
// first, then the bottom rows' other blocks.
__global__ __launch_bounds__(GEN_THREADS) void me_rd_generic_kernel(
    const uint8_t* __restrict__ ref, size_t ref_frame_stride, const uint8_t* __restrict__ cur,
    size_t cur_frame_stride, int width, int height, int stride, int B, int S, int nbx_skip,
    int nby_skip, RdOut o) {
  __shared__ uint32_t cblk[ME_MAX_BLOCK * ME_MAX_BLOCK / 4];
  __shared__ uint64_t red[GEN_THREADS / 64];
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
  const int x0 = bx * B, y0 = by * B, CW = (B + 3) / 4;
  const int bw = min(B, width - x0), bh = min(B, height - y0);
  const size_t rec = (size_t)f * o.nbx * o.nby + (size_t)by * o.nbx + bx;
  const int px = o.pred ? o.pred[2 * rec] : 0, py = o.pred ? o.pred[2 * rec + 1] : 0;
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
  uint64_t best = ~0ull;
  for (int t = tid; t < ncand; t += GEN_THREADS) {
    const int cy = cy0 + t / ncx, cx = cx0 + t % ncx;
    uint32_t sad = 0;
    for (int y = 0; y < bh; y++) {
      const uint8_t* r = ref + (size_t)(cy + y) * stride + cx;
      for (int k = 0; k < CW; k++) {
        const int xw = 4 * k;
        if (xw >= bw) break;
        uint32_t w = 0;
        for (int e = 0; e < 4; e++)
          if (xw + e < bw) w |= (uint32_t)r[xw + e] << (8 * e);
        sad = __builtin_amdgcn_sad_u8(w, cblk[y * CW + k], sad);
      }
    }
    const int dx = cx - x0, dy = cy - y0;
    const uint32_t r = (uint32_t)(rd_bits(4 * dx - px) + rd_bits(4 * dy - py));
    const uint64_t key = make_key(sad + o.lambda * r, dx, dy);
    best = key < best ? key : best;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint64_t u = __shfl_xor(best, off, 64);
    best = u < best ? u : best;
  }
  if ((tid & 63) == 0) red[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    uint64_t v = red[0];
#pragma unroll
    for (int w = 1; w < GEN_THREADS / 64; w++) v = red[w] < v ? red[w] : v;
    rd_store(o, rec, v, px, py);
  }
}

// --------------------------------------------------------------------- fast
// Orders row YY's qsads before the next row's (volatile) address step: see
// pin_rows of me_kernels.hip.
template <int J, int K, int YY>
__device__ __forceinline__ void rd_pin_rows(uint64_t (&acc)[K]) {
  if constexpr (J < K) {
    if constexpr (YY - J >= 0 && YY - J < 16) asm volatile("" : "+v"(acc[J]));
    rd_pin_rows<J + 1, K, YY>(acc);
  }
}

// The lane's 4 dx x K dy SADs of a 16 x 16 block c: LDS byte address `at` is
// window row (first dy row) and the word of the lane's first dx.  acc[j]: four
// packed u16 SADs (dx 0..3) of dy row j.  The row walk is qsad_lane's of
// me_kernels.hip (one segment per window row: the next row's four
// ds_read2_b32, then this row's qsads).
template <int K>
__device__ __forceinline__ void rd_lane(uint32_t at, int pitch, const uint32_t (&c)[16][4],
                                        uint64_t (&acc)[K]) {
  constexpr int NR = K + 15;
  uint32_t oe = at, oo = at + 4;
  asm volatile("" : "+v"(oo));
#pragma unroll
  for (int j = 0; j < K; j++) acc[j] = 0;
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
        if constexpr (y >= 0 && y < 16)
          acc[j] = __builtin_amdgcn_qsad_pk_u16_u8(pr[k], c[y][k], acc[j]);
      });
    });
    rd_pin_rows<0, K, yy>(acc);
    if constexpr (yy + 1 < NR) {
#pragma unroll
      for (int k = 0; k < 4; k++) pr[k] = nx[k];
    }
  });
}

// The lane's best 32-bit key J << 6 | 4 j + i, ordered like (J, dy, dx) within
// the lane.  rx[i] = lambda bits(4 dx_i - px) << 6 | i and ry[j] = lambda
// bits(4 dy_j - py) << 6 | 4 j come from the workgroup's rate tables: the sum
// with sad << 6 carries nothing between the fields (4 j + i < 64, J < 2^26) and
// stays below 2^32 - 1.  A column or row outside the block's candidates has
// ~0 in its table entry, and both adds saturate, so its key is ~0, above every
// valid one: no compare, mask or branch per candidate.
template <int K>
__device__ __forceinline__ uint32_t rd_lane_key(const uint64_t (&acc)[K], const uint32_t (&rx)[4],
                                                const uint32_t* ry) {
  uint32_t best = ~0u;
#pragma unroll
  for (int j = 0; j < K; j++) {
    const uint32_t lo = (uint32_t)acc[j], hi = (uint32_t)(acc[j] >> 32), r = ry[j];
    const uint32_t k0 = add_sat((lo & 0xFFFFu) << 6, add_sat(rx[0], r));
    const uint32_t k1 = add_sat((lo >> 16) << 6, add_sat(rx[1], r));
    const uint32_t k2 = add_sat((hi & 0xFFFFu) << 6, add_sat(rx[2], r));
    const uint32_t k3 = add_sat((hi >> 16) << 6, add_sat(rx[3], r));
    best = min(min(best, k0), min(k1, min(k2, k3)));
  }
  return best;
}

// Workgroup (blockIdx.x, blockIdx.y, blockIdx.z) = (tile of RD_TB full-size
// blocks, block row, frame).  Dynamic LDS: the window (rows x pitch, frame rows
// y0 - S .., columns X0 .., X0 = tile x - S - a a multiple of 4; zeros outside
// the plane's bytes, whatever the neighbouring rows hold beyond the frame's
// sides -- those candidates' keys saturate), the tile's current blocks (256 bytes
// each), one key per block, then the rate tables: per block 4 G words
// lambda bits(4 dx - px) << 6 | (q & 3) for the window columns q = dx + S + a,
// and chunks * K words lambda bits(4 dy - py) << 6 | 4 (d % K) for the rows
// d = dy + S (the rate is separable, so a lane reads 4 + K words per task);
// ~0 where dx or dy is not among the block's candidates.
template <int K>
__global__ __launch_bounds__(RD_FAST_THREADS) void me_rd_fast_kernel(
    const uint8_t* __restrict__ ref, size_t ref_frame_stride, const uint8_t* __restrict__ cur,
    size_t cur_frame_stride, int width, int height, int stride, int S, int nbx_full, RdOut o) {
  extern __shared__ __align__(16) uint8_t smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  constexpr int NW = RD_FAST_THREADS / 64;
  const int bx0 = (int)blockIdx.x * RD_TB, by = blockIdx.y, f = blockIdx.z;
  const int nb = min(RD_TB, nbx_full - bx0);
  const int G = rd_fast_groups(S), pitch = rd_fast_pitch(S);
  const int chunks = (2 * S + 1 + K - 1) / K, rows = chunks * K + 15;
  uint8_t* const cur_lds = smem + ((rows * pitch + 15) & ~15);
  uint64_t* const keys = reinterpret_cast<uint64_t*>(cur_lds + RD_TB * 256);
  uint32_t* const rxt = reinterpret_cast<uint32_t*>(keys + RD_TB);
  uint32_t* const ryt = rxt + RD_TB * 4 * G;
  const int y0 = by * 16;
  const int a = ((bx0 * 16 - S) % 4 + 4) % 4;
  const int X0 = bx0 * 16 - S - a;
  const size_t rec0 = (size_t)f * o.nbx * o.nby + (size_t)by * o.nbx + bx0;

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
  if (tid < RD_TB) keys[tid] = ~0ull;
  // valid displacement rows of the block row
  const int dymin = max(-S, -y0), dymax = min(S, height - 16 - y0);
  for (int i = tid; i < nb * 4 * G; i += RD_FAST_THREADS) {
    const int b = i / (4 * G), q = i - b * 4 * G, dx = q - S - a, x0 = (bx0 + b) * 16;
    const int px = o.pred ? o.pred[2 * (rec0 + b)] : 0;
    const bool ok = dx >= max(-S, -x0) && dx <= min(S, width - 16 - x0);
    rxt[i] = ok ? ((o.lambda * (uint32_t)rd_bits(4 * dx - px)) << 6) + (uint32_t)(q & 3) : ~0u;
  }
  for (int i = tid; i < nb * chunks * K; i += RD_FAST_THREADS) {
    const int b = i / (chunks * K), d = i - b * chunks * K, dy = d - S;
    const int py = o.pred ? o.pred[2 * (rec0 + b) + 1] : 0;
    const bool ok = dy >= dymin && dy <= dymax;
    ryt[i] = ok ? ((o.lambda * (uint32_t)rd_bits(4 * dy - py)) << 6) + (uint32_t)(4 * (d % K)) : ~0u;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();

  // chunks wholly outside the valid rows are skipped (tasks are chunk-major)
  const int lc0 = (dymin + S) / K, lc1 = (dymax + S) / K + 1;
  const int per_chunk = nb * G, T = (lc1 - lc0) * per_chunk;
  const uint32_t lds0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) const uint8_t*)smem);
  for (int t = tid; t < T; t += RD_FAST_THREADS) {
    const int lcr = t / per_chunk, rem = t - lcr * per_chunk;
    const int b = rem / G, gi = rem - b * G;
    const int d0 = (lc0 + lcr) * K;  // first dy row of the task, as dy + S
    uint32_t c[16][4];
#pragma unroll
    for (int y = 0; y < 16; y++) {
      const uint4 v = reinterpret_cast<const uint4*>(cur_lds)[b * 16 + y];
      c[y][0] = v.x, c[y][1] = v.y, c[y][2] = v.z, c[y][3] = v.w;
    }
    uint64_t acc[K];
    rd_lane<K>(lds0 + (uint32_t)(d0 * pitch + 4 * (b * 4 + gi)), pitch, c, acc);

    const int dxg = 4 * gi - S - a;  // dx of the lane's first candidate
    const uint4 rv = reinterpret_cast<const uint4*>(rxt)[b * G + gi];
    const uint32_t rx[4] = {rv.x, rv.y, rv.z, rv.w};
    const uint32_t best = rd_lane_key<K>(acc, rx, ryt + b * chunks * K + d0);
    if (best != ~0u) {
      const int idx = (int)(best & 63u);
      const uint64_t key = make_key(best >> 6, dxg + (idx & 3), d0 + (idx >> 2) - S);
      // most lanes lose to a key already there: read before the atomic
      if (key < keys[b])
        atomicMin(reinterpret_cast<unsigned long long*>(&keys[b]), (unsigned long long)key);
    }
  }
  __syncthreads();
  if (tid < nb) {
    const size_t rec = rec0 + tid;
    rd_store(o, rec, keys[tid], o.pred ? o.pred[2 * rec] : 0, o.pred ? o.pred[2 * rec + 1] : 0);
  }
}

}  // namespace

hipError_t launch_rd_search(const FrameBatch& b, int range, uint32_t lambda, bool fast,
                            const int16_t* pred, int16_t* mv, uint32_t* cost, uint32_t* dist,
                            uint8_t* bits, hipStream_t stream) {
  const RdOut o{pred, mv, cost, dist, bits, (b.width + b.blk - 1) / b.blk, (b.height + b.blk - 1) / b.blk,
                lambda};
  const int nbx_full = b.width / b.blk, nby_full = b.height / b.blk;
  if (fast) {
    const int rows = rd_fast_rows(range), pitch = rd_fast_pitch(range);
    // window, current blocks, keys, then the rate tables (4 G + rows - 15 words per block)
    const size_t lds = (size_t)((rows * pitch + 15) & ~15) + RD_TB * 256 + RD_TB * 8 +
                       (size_t)RD_TB * 4 * (4 * rd_fast_groups(range) + rows - 15);
    const dim3 grid((unsigned)((nbx_full + RD_TB - 1) / RD_TB), (unsigned)nby_full,
                    (unsigned)b.n_frames);
    if (rd_fast_k(range) == RD_K_SMALL)
      hipLaunchKernelGGL(me_rd_fast_kernel<RD_K_SMALL>, grid, dim3(RD_FAST_THREADS), lds, stream,
                         b.ref, b.ref_frame_stride, b.cur, b.cur_frame_stride, b.width, b.height, b.stride,
                         range, nbx_full, o);
    else
      hipLaunchKernelGGL(me_rd_fast_kernel<RD_K_LARGE>, grid, dim3(RD_FAST_THREADS), lds, stream,
                         b.ref, b.ref_frame_stride, b.cur, b.cur_frame_stride, b.width, b.height, b.stride,
                         range, nbx_full, o);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  // every block, or the rim the fast kernel left: (nbx - nbx_full) right
  // columns of all rows, then nbx_full blocks of each clipped bottom row
  const int sx = fast ? nbx_full : 0, sy = fast ? nby_full : 0;
  const int n = fast ? (o.nbx - sx) * o.nby + sx * (o.nby - sy) : o.nbx * o.nby;
  if (n == 0) return hipSuccess;
  hipLaunchKernelGGL(me_rd_generic_kernel, dim3((unsigned)n, (unsigned)b.n_frames),
                     dim3(GEN_THREADS), 0, stream, b.ref, b.ref_frame_stride, b.cur, b.cur_frame_stride,
                     b.width, b.height, b.stride, b.blk, range, sx, sy, o);
  return hipGetLastError();
}

}  // namespace me
