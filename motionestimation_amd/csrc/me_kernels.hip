// me_kernels.hip -- CDNA4 (gfx950) full-search block-matching kernels.
//
// Semantics follow the reference CPU search exactly (souravBhat/MotionEstimation
// src/cpu/main.c:39-82): frame-clamped window (:73-76), candidates whose whole
// block fits the window (:53-54), the first minimum in raster order wins
// (:53-60, strict <).  Ties are made order-independent by reducing packed keys
//     key = cost << 32 | (dy + 32768) << 16 | (dx + 32768)
// with an unsigned min: the smallest key is the smallest cost and, among equal
// costs, the smallest (dy, dx) -- the reference's raster-first choice.
//
// Kernels (the matrix-core SSD kernels are in me_mfma.hip, SSIM in me_ssim.hip):
//   me_fast_kernel<COST, B, K, PC>
//                          SAD (qsad) or SSD (dot4), B in {8, 16}, full-width
//                          blocks.  Persistent and double-buffered: an item is
//                          (tile of TB blocks of one block row, pass of dy
//                          chunks); the union search window of the tile is
//                          staged once in LDS by LDS DMA; each SAD lane owns 4
//                          horizontal x K vertical candidates of one block and
//                          walks the window rows, 16 |a-b| per v_qsad_pk_u16_u8
//                          with the cur block held in VGPRs.
//   me_flow_kernel<B, K, PC>, me_flow_chain_kernel<B, K> (me_flow_kernel.inc,
//                          compiled twice; the second: pruning launches with box-sum planes)
//                          SAD, 16x16, S = 32 on frames with >= 2 tiles per CU
//                          (the 1080p headline): one 1,024-thread workgroup
//                          per CU, a ring of LDS slots, waves pulling 64-lane
//                          wave-tasks from one LDS counter (no item barriers).
//   me_generic_kernel      any B <= 64, any S, SSD or SAD, partial blocks; one
//                          workgroup per block, one candidate per lane.  SSD on
//                          blocks with w*h > 256 replays the reference's float
//                          accumulation (main.c:19-27) so the argmin is identical
//                          even when the float sum rounds.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <mutex>
#include <type_traits>
#include <vector>

#include "me_kernels.h"
#include "me_tuning.h"


namespace me {

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    uint64_t o = __shfl_xor(v, off, 64);
    v = o < v ? o : v;
  }
  return v;
}

__device__ __forceinline__ const uint8_t* row_ptr(const SearchArgs& p, const uint8_t* base,
                                                  int row0, int y) {
  return base + (ptrdiff_t)(y - row0) * p.stride;
}

// ------------------------------------------------------------------ generic
// One workgroup per block, GENERIC_THREADS lanes, one candidate per lane per
// step.  Window staged in LDS when it fits (win_lds_bytes > 0), else read from
// global memory.
template <int COST>
__global__ __launch_bounds__(GENERIC_THREADS) void me_generic_kernel(SearchArgs p, int bx0,
                                                                     int nbx_range, int row0,
                                                                     int win_lds_bytes) {
  extern __shared__ __align__(16) uint8_t smem[];
  __shared__ uint64_t red[GENERIC_THREADS / 64];
  const int tid = threadIdx.x;
  const int bx = bx0 + (int)(blockIdx.x % nbx_range);
  const int by = row0 + (int)(blockIdx.x / nbx_range);
  const int B = p.blk, S = p.range;
  const int tlx = bx * B, tly = by * B;
  const int w = min(B, p.width - tlx), h = min(B, p.height - tly);
  const int wx0 = max(tlx - S, 0), wy0 = max(tly - S, 0);
  const int wx1 = min(tlx + w - 1 + S, p.width - 1), wy1 = min(tly + h - 1 + S, p.height - 1);
  const int ncx = wx1 - w + 1 - wx0 + 1, ncy = wy1 - h + 1 - wy0 + 1;
  const int ww = wx1 - wx0 + 1, wh = wy1 - wy0 + 1;

  uint8_t* cblk = smem;                       // w*h bytes
  uint8_t* win = smem + ((B * B + 15) & ~15); // ww*wh bytes when staged
  const bool staged = win_lds_bytes >= ww * wh;
  for (int i = tid; i < w * h; i += GENERIC_THREADS) {
    int oy = i / w, ox = i % w;
    cblk[i] = row_ptr(p, p.cur, p.cur_row0, tly + oy)[tlx + ox];
  }
  if (staged)
    for (int i = tid; i < ww * wh; i += GENERIC_THREADS) {
      int oy = i / ww, ox = i % ww;
      win[i] = row_ptr(p, p.ref, p.ref_row0, wy0 + oy)[wx0 + ox];
    }
  __syncthreads();

  // SSD on large blocks: key on the float MSE exactly as the reference rounds it.
  const bool float_key = (COST == COST_SSD) && (w * h > 256);
  uint64_t best = ~0ull;
  const int ncand = ncx * ncy;
  for (int t = tid; t < ncand; t += GENERIC_THREADS) {
    const int cy = t / ncx, cx = t % ncx;
    uint32_t acc = 0;
    float facc = 0.f;
    for (int oy = 0; oy < h; oy++) {
      const uint8_t* r = staged ? win + (cy + oy) * ww + cx
                                : row_ptr(p, p.ref, p.ref_row0, wy0 + cy + oy) + wx0 + cx;
      const uint8_t* c = cblk + oy * w;
      for (int ox = 0; ox < w; ox++) {
        int d = (int)c[ox] - (int)r[ox];
        if (COST == COST_SAD) {
          acc += (uint32_t)abs(d);
        } else if (float_key) {
          facc = __fadd_rn(facc, (float)(d * d));  // main.c:24, float += int
        } else {
          acc += (uint32_t)(d * d);
        }
      }
    }
    uint32_t k32 = acc;
    if (float_key) k32 = __float_as_uint(__fdiv_rn(facc, (float)(w * h)));  // main.c:27
    const int dx = wx0 + cx - tlx, dy = wy0 + cy - tly;
    uint64_t key = make_key(k32, dx, dy);
    best = key < best ? key : best;
  }
  best = wave_min_u64(best);
  if ((tid & 63) == 0) red[tid >> 6] = best;
  __syncthreads();
  if (tid == 0) {
    uint64_t b = red[0];
#pragma unroll
    for (int i = 1; i < GENERIC_THREADS / 64; i++) b = red[i] < b ? red[i] : b;
    const int dx = (int)(b & 0xFFFF) - 32768, dy = (int)((b >> 16) & 0xFFFF) - 32768;
    uint32_t cost = (uint32_t)(b >> 32);
    if (float_key) {  // report the integer SSD of the chosen vector
      cost = 0;
      for (int oy = 0; oy < h; oy++) {
        const uint8_t* r = row_ptr(p, p.ref, p.ref_row0, tly + dy + oy) + tlx + dx;
        for (int ox = 0; ox < w; ox++) {
          int d = (int)cblk[oy * w + ox] - (int)r[ox];
          cost += (uint32_t)(d * d);
        }
      }
    }
    const int out = (by - p.block_row_begin) * p.nbx + bx;
    p.mv[2 * out] = (int16_t)dx;
    p.mv[2 * out + 1] = (int16_t)dy;
    if (p.cost) p.cost[out] = cost;
  }
}

// --------------------------------------------------------------- qsad (SAD)
// Workgroup = TB consecutive full-width blocks of one block row; the union of
// their search windows is staged ONCE in LDS:
//   frame rows [Y0, Y0 + rows_alloc) x columns [X0, X0 + pitch), Y0 = tly - S,
//   X0 = tlx(b0) - S - a rounded down to a multiple of 4 (a = (tlx - S) mod 4),
//   zeros outside the frame (those candidates are masked).
// Each tile row is stored twice, the second copy shifted left by 4 bytes, so
// every 8-byte qsad operand (ref words w, w+1) is one aligned ds_read_b64 from
// one copy or the other -- gfx950 needs even-aligned VGPR pairs and unaligned
// overlapping pairs would cost a v_mov per qsad.
// Task t of the workgroup -> (dy chunk, block, dx group): the lane owns dx
// offsets q = 4g..4g+3 (dx = q - S - a) and dy offsets d = chunk*K .. +K-1
// (dy = d - S); it walks the K + H - 1 window rows once, each row feeding up
// to K accumulators (u16x4 packed, SAD <= 65280 fits) against the cur block
// held in VGPRs.
// Empty volatile asm on the accumulators row YY touched: orders that row's
// qsads before the next row's (volatile) address step.
template <int J, int K, int YY, int H>
__device__ __forceinline__ void pin_rows(uint64_t (&acc)[K]) {
  if constexpr (J < K) {
    if constexpr (YY - J >= 0 && YY - J < H) asm volatile("" : "+v"(acc[J]));
    pin_rows<J + 1, K, YY, H>(acc);
  }
}

template <int J, int K, int YY, int H>
__device__ __forceinline__ void pin_rows32(uint32_t (&acc)[K]) {
  if constexpr (J < K) {
    if constexpr (YY - J >= 0 && YY - J < H) asm volatile("" : "+v"(acc[J]));
    pin_rows32<J + 1, K, YY, H>(acc);
  }
}

// PC > 0: the pitch is that compile-time constant, and the rows of a group of
// RG share one base address (the row offset goes into the ds_read2 offset
// fields, <= 1020 bytes): one address add per group instead of per row.
// HK > 0: hook() runs at the start of every HK-th window row (the flow kernel's
// issue-priority check).
struct NoHook {
  __device__ void operator()() const {}
};
template <int B, int K, int H, int PC = 0, int HK = 0, typename Hook = NoHook>
__device__ __forceinline__ void qsad_lane(const uint8_t* __restrict__ tile, int pitch,
                                          uint32_t buf_off, int lrow, int w0,
                                          const uint32_t (&c)[B][B / 4], uint64_t (&acc)[K],
                                          Hook hook = Hook{}) {
  constexpr int CW = B / 4;
  constexpr int NR = K + H - 1;
  constexpr int RG = PC > 0 ? ((1020 - 4 * CW) / PC + 1 < 8 ? (1020 - 4 * CW) / PC + 1 : 8) : 1;
  // Operand pair k = ref words (w0 + k, w0 + k + 1) of the current row: one
  // ds_read2_b32 straight into an aligned VGPR pair.  Pairs 0, 2 come from
  // byte offset oe = 4*w0, pairs 1, 3 from oo = oe + 4; both advance through
  // an opaque asm, so the compiler neither hoists every row's address (spills)
  // nor merges the overlapping words of adjacent pairs (v_mov per qsad).
  const uint32_t lds0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) const uint8_t*)tile);
  uint32_t oe = lds0 + buf_off + (uint32_t)(lrow * pitch + 4 * w0);
  uint32_t oo = oe + 4;
  asm volatile("" : "+v"(oo));

#pragma unroll
  for (int j = 0; j < K; j++) acc[j] = 0;

  // LDS addresses as plain integers (address space 3, base folded into oe/oo
  // once) so no per-row add of the dynamic-LDS symbol survives.
  typedef __attribute__((address_space(3))) const uint32_t lds_u32;
  auto load = [&](uint64_t (&dst)[CW], uint32_t ro) {
#pragma unroll
    for (int k = 0; k < CW; k++) {
      lds_u32* w = reinterpret_cast<lds_u32*>((uintptr_t)(((k & 1) ? oo : oe) + ro)) + 2 * (k >> 1);
      dst[k] = ((uint64_t)w[1] << 32) | w[0];
    }
  };
  uint64_t pr[CW], nx[CW];
  load(pr, 0);
  static_for<0, NR>([&](auto YY) {
    constexpr int yy = decltype(YY)::value;
    // one segment per window row: next row's loads, then this row's qsads.
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (HK > 0 && yy > 0 && yy % HK == 0) {
      hook();
      __builtin_amdgcn_sched_barrier(0);
    }
    if constexpr (yy + 1 < NR) {
      if constexpr (PC > 0) {
        constexpr int nr = yy + 1;
        if constexpr (nr % RG == 0) {
          oe += RG * PC;
          oo += RG * PC;
          asm volatile("" : "+v"(oe), "+v"(oo));
        }
        load(nx, (uint32_t)((nr % RG) * PC));
      } else {
        oe += pitch;
        oo += pitch;
        asm volatile("" : "+v"(oe), "+v"(oo));
        load(nx, 0);
      }
    }
    static_for<0, CW>([&](auto KK) {
      constexpr int k = decltype(KK)::value;
      static_for<0, K>([&](auto JJ) {
        constexpr int j = decltype(JJ)::value;
        constexpr int y = yy - j;
        if constexpr (y >= 0 && y < H)
          acc[j] = __builtin_amdgcn_qsad_pk_u16_u8(pr[k], c[y][k], acc[j]);
      });
    });
    // Pin this row's qsads inside its segment (readnone intrinsics are not
    // ordered by sched_barrier; the DAG would otherwise sink them past every
    // later row's loads and spill the loaded rows).
    pin_rows<0, K, yy, H>(acc);
    if constexpr (yy + 1 < NR) {
#pragma unroll
      for (int k = 0; k < CW; k++) pr[k] = nx[k];
    }
  });
}

#ifdef ME_STAMPS
// Diagnostic build only (-DME_STAMPS): per-workgroup s_memtime stamps
// [start, staged, computed, end, hw_id, xcc_id] for tools/stamps.py.
__device__ unsigned long long g_stamps[8 << 16];
#define ME_STAMP(slot, v) do { if (threadIdx.x == 0 && wid < (1 << 16)) g_stamps[8 * wid + (slot)] = (v); } while (0)
// ... and per wave of me_fast_kernel: [start, first item staged, last task
// loop done, end, hw_id, xcc_id, realtime start, realtime end] (tools/wave_stamps.py)
__device__ unsigned long long g_wstamps[8 << 14];
// The flow kernel's bound phase per wave (refills only), cycles summed: [cur q
// and minlb init, step 2's chunks, chunks run, the fold column, step 3, step 4,
// items bounded, step 3's wait for the window DMA] (tools/flow_stamps.py).
__device__ unsigned long long g_bstamps[16 << 14];
// ... words 8, 9: cycles from a slot's publish (the release store of `ready`)
// to the start of the first executed wave-task of its item, summed over the
// items this wave completed, and their count.  g_pub / g_first: per workgroup
// and slot, the publish time and the earliest executed task's start.
__device__ unsigned long long g_pub[16 << 12], g_first[16 << 12];
#define ME_BSTAMP(i) do { if (bs) { const unsigned long long bnow = __builtin_amdgcn_s_memtime(); bs[i] += bnow - bt; bt = bnow; } } while (0)
#define ME_WSTAMP(slot, v) do { if ((threadIdx.x & 63) == 0 && wwid < (1 << 14)) g_wstamps[8 * wwid + (slot)] = (v); } while (0)
#else
#define ME_WSTAMP(slot, v) do { } while (0)
#define ME_STAMP(slot, v) do { } while (0)
#define ME_BSTAMP(i) do { } while (0)
#endif

// 32-bit lane keys (sad << 16 | j*5 + i) ordered like (cost, dy, dx); i = 4 is
// the fold's dx = +S column (after every group dx of the same dy).  j*5 + i <=
// 64 for K <= 13 keeps every index an inline constant (VOP3 on gfx950 takes
// no literals: larger ones would each pin a VGPR and spill); invalid
// candidates forced to sad 0xFFFF (> any valid SAD: B*B*255 <= 65280).
// MASKJ = false on items whose whole dy range is valid (uniform per item).
// min(a, b, c) as one v_min3_u32 (ASM, K > 13: the 8x8 K = 26 lane-tasks):
// written as min(min(..)) the compiler reassociates the two key chains into
// trees of v_min + v_min3 (72 instead of 52 instructions for the 104 keys of
// an 8x8 lane-task).  The K <= 13 instances keep plain C: the asm operands
// pinned registers there and spilled 5 VGPRs of the 4K instance
// <SAD, 16, 13, 272> (24 bytes per lane of scratch, 32 MiB of writes per
// 16-frame launch; tests/test_kernel_resources.py guards it).
template <bool ASM>
__device__ __forceinline__ uint32_t min3u(uint32_t a, uint32_t b, uint32_t c) {
  if constexpr (ASM) {
    uint32_t r;
    asm("v_min3_u32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
  } else {
    return min(min(a, b), c);
  }
}

template <int K, int J0, int J1, bool MASKJ>
__device__ __forceinline__ uint32_t lane_best_rows(const uint64_t (&acc)[K], uint32_t mlo,
                                                   uint32_t mhi, int jlo, int jhi) {
  // Two independent min3 chains (i = 0,1 and i = 2,3): the epilogues of all
  // waves on a SIMD tend to coincide (item barriers), so a single 2K-deep
  // dependent chain would run at VALU latency, not issue rate.
  uint32_t b01 = ~0u, b23 = ~0u;
#pragma unroll
  for (int j = J0; j < J1; j++) {
    uint32_t lo = (uint32_t)acc[j] | mlo, hi = (uint32_t)(acc[j] >> 32) | mhi;
    if (MASKJ) {
      const bool jv = j >= jlo && j <= jhi;
      lo = jv ? lo : ~0u;
      hi = jv ? hi : ~0u;
    }
    const uint32_t k0 = (lo << 16) | (uint32_t)(5 * (j - J0));
    const uint32_t k1 = (lo & 0xFFFF0000u) | (uint32_t)(5 * (j - J0) + 1);
    const uint32_t k2 = (hi << 16) | (uint32_t)(5 * (j - J0) + 2);
    const uint32_t k3 = (hi & 0xFFFF0000u) | (uint32_t)(5 * (j - J0) + 3);
    b01 = min3u<(K > 13)>(b01, k0, k1);
    b23 = min3u<(K > 13)>(b23, k2, k3);
  }
  return min(b01, b23);
}

// K > 13 (26: 8x8 SAD): two runs of 13 rows, each with inline-constant
// indices; the second's keys move past the first's (+ 5 * 13), so the min
// still orders by (sad, j, i).  A lane key's index is 5 j + i for every K.
template <int K, bool MASKJ>
__device__ __forceinline__ uint32_t lane_best(const uint64_t (&acc)[K], uint32_t mlo,
                                              uint32_t mhi, int jlo, int jhi) {
  if constexpr (K <= 13) {
    return lane_best_rows<K, 0, K, MASKJ>(acc, mlo, mhi, jlo, jhi);
  } else {
    const uint32_t a = lane_best_rows<K, 0, 13, MASKJ>(acc, mlo, mhi, jlo, jhi);
    uint32_t b = lane_best_rows<K, 13, K, MASKJ>(acc, mlo, mhi, jlo, jhi);
    b = b < 0xFFFF0000u ? b + 65u : b;  // (an all-masked run stays ~0)
    return min(a, b);
  }
}

// Fold column: SAD of the lane's one dx = +S candidate (window rows row..row+H-1,
// B bytes at byte offset `off` of the tile row, B-aligned) with v_sad_u8.
template <int B, int H>
__device__ __forceinline__ uint32_t tail_sad(const uint8_t* __restrict__ tile, int pitch,
                                             uint32_t off, const uint32_t (&c)[B][B / 4]) {
  const uint32_t lds0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) const uint8_t*)tile);
  uint32_t o = lds0 + off;
  uint32_t sad = 0;
#pragma unroll
  for (int y = 0; y < H; y++) {
    if constexpr (B == 16) {
      typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
      typedef __attribute__((address_space(3))) const u32x4 lds_v4;
      const u32x4 w = *reinterpret_cast<lds_v4*>((uintptr_t)o);
      sad = __builtin_amdgcn_sad_u8(w[0], c[y][0], sad);
      sad = __builtin_amdgcn_sad_u8(w[1], c[y][1], sad);
      sad = __builtin_amdgcn_sad_u8(w[2], c[y][2], sad);
      sad = __builtin_amdgcn_sad_u8(w[3], c[y][3], sad);
    } else {
      typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
      typedef __attribute__((address_space(3))) const u32x2 lds_v2;
      const u32x2 w = *reinterpret_cast<lds_v2*>((uintptr_t)o);
      sad = __builtin_amdgcn_sad_u8(w[0], c[y][0], sad);
      sad = __builtin_amdgcn_sad_u8(w[1], c[y][1], sad);
    }
    o += pitch;
  }
  return sad;
}

// --------------------------------------------------------------- dot4 (SSD)
// SSD of one dx and K dy candidates, exactly: SSD = sum c^2 + sum r^2 - 2 sum c*r
// in u32.  sum c*r: v_dot4_u32_u8 of the cur words with the ref words realigned
// to this lane's dx (v_alignbyte, shift sh); sum r^2: a running prefix P over
// the window rows (4 more dot4 per row), snapshotted when candidate j's first
// row arrives (pst[j] = P(j-1)) and closed after its last (pst[j] = P - pst[j]).
// Returns out[j] = sum r^2 - 2 sum c*r (mod 2^32; the caller adds sum c^2).
template <int B, int K, int H>
__device__ __forceinline__ void ssd_lane(const uint8_t* __restrict__ tile, int pitch,
                                         uint32_t buf_off, int lrow, int wb, int sh,
                                         const uint32_t (&c)[B][B / 4], uint32_t (&out)[K]) {
  constexpr int CW = B / 4;
  constexpr int NR = K + H - 1;
  const uint32_t lds0 = (uint32_t)(uintptr_t)((__attribute__((address_space(3))) const uint8_t*)tile);
  uint32_t o = lds0 + buf_off + (uint32_t)(lrow * pitch + 4 * wb);
  typedef __attribute__((address_space(3))) const uint32_t lds_u32;
  auto load = [&](uint32_t (&dst)[CW + 1]) {
    lds_u32* w = reinterpret_cast<lds_u32*>((uintptr_t)o);
#pragma unroll
    for (int k = 0; k <= CW; k++) dst[k] = w[k];
  };
  uint32_t acc[K], pst[K];
#pragma unroll
  for (int j = 0; j < K; j++) { acc[j] = 0; pst[j] = 0; }
  uint32_t P = 0;
  uint32_t w[CW + 1], nw[CW + 1];
  load(w);
  static_for<0, NR>([&](auto YY) {
    constexpr int yy = decltype(YY)::value;
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (yy + 1 < NR) {
      o += pitch;
      asm volatile("" : "+v"(o));
      load(nw);
    }
    uint32_t al[CW];
#pragma unroll
    for (int k = 0; k < CW; k++) al[k] = __builtin_amdgcn_alignbyte(w[k + 1], w[k], sh);
    uint32_t rs = 0;
#pragma unroll
    for (int k = 0; k < CW; k++) rs = __builtin_amdgcn_udot4(al[k], al[k], rs, false);
    P += rs;
    static_for<0, CW>([&](auto KK) {
      constexpr int k = decltype(KK)::value;
      static_for<0, K>([&](auto JJ) {
        constexpr int j = decltype(JJ)::value;
        constexpr int y = yy - j;
        if constexpr (y >= 0 && y < H) acc[j] = __builtin_amdgcn_udot4(al[k], c[y][k], acc[j], false);
      });
    });
    if constexpr (yy + 1 < K) pst[yy + 1] = P;          // P(j - 1) for j = yy + 1
    if constexpr (yy - H + 1 >= 0 && yy - H + 1 < K)    // last row of j = yy - H + 1
      pst[yy - H + 1] = P - pst[yy - H + 1];
    pin_rows32<0, K, yy, H>(acc);
    if constexpr (yy + 1 < NR) {
#pragma unroll
      for (int k = 0; k <= CW; k++) w[k] = nw[k];
    }
  });
#pragma unroll
  for (int j = 0; j < K; j++) out[j] = pst[j] - 2u * acc[j];
}

// Lane key ((v + SSD_BIAS) << 5 | j) with v = sum r^2 - 2 sum c*r: SSD = v +
// sum c^2, and sum c^2 is the same for every candidate of a block, so v ranks
// them exactly; v >= -sum c^2 > -2^24 (B <= 16), so v + SSD_BIAS lies in
// [0, 2^25) and the key below 2^30 (j < 32).  Block costs get sum c^2 back
// once per block at output.
constexpr uint32_t SSD_BIAS = 1u << 24;

template <int K, bool MASKJ>
__device__ __forceinline__ uint32_t lane_best_ssd(const uint32_t (&v)[K], int jlo, int jhi) {
  static_assert(K < 32, "j field is 5 bits");
  uint32_t b0 = ~0u, b1 = ~0u;  // two chains (see lane_best)
#pragma unroll
  for (int j = 0; j < K; j++) {
    uint32_t key = ((v[j] + SSD_BIAS) << 5) | (uint32_t)j;
    if (MASKJ) key = (j >= jlo && j <= jhi) ? key : ~0u;
    if (j & 1) b1 = min(b1, key);
    else b0 = min(b0, key);
  }
  return min(b0, b1);
}

// LDS DMA of `bytes` (multiple of 16) into lds_dst: 16 bytes per lane, lane i
// of DMA step s covers bytes [1024 s + 16 i, +16) of the destination; src_off
// maps such a destination byte offset to the buffer offset (any uint32: the
// descriptor's range check returns zeros for offsets past the resident rows,
// including negative ones, which wrap).
// Lane index recomputed per call: an opaque copy of threadIdx.x keeps the
// compiler from hoisting lane-derived staging addresses out of the item loop,
// where they would stay live across the 128-VGPR task loop and spill.
__device__ __forceinline__ int fresh_tid() {
  int t = (int)threadIdx.x;
  asm volatile("" : "+v"(t));
  return t;
}

template <typename F>
__device__ __forceinline__ void dma16(__amdgpu_buffer_rsrc_t rs, uint8_t* lds_dst, int bytes,
                                      F src_off) {
  const int tid = fresh_tid();
  const int lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  for (int s0 = wave * 1024; s0 < bytes; s0 += nw * 1024) {
    const int d = s0 + 16 * lane;
    // lanes past the end must not execute: an out-of-range lane would still
    // write (zeros) to its LDS slot.
    if (d < bytes)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rs, (__attribute__((address_space(3))) void*)(lds_dst + s0), 16, src_off(d), 0, 0, 0);
  }
}

// LDS DMA with 4-byte granules (256 bytes per wave step): used for the ref
// tile, whose left/top edges hang off the frame.  X0 is 4-aligned, so no
// granule straddles x = 0 or x = W (W % 4 == 0 on this path): every granule is
// either all in-frame or all masked, and the range check zeroes out-of-range
// ones (a 16-byte granule straddling x = 0 on row 0 would be zeroed whole).
template <typename F>
__device__ __forceinline__ void dma4(__amdgpu_buffer_rsrc_t rs, uint8_t* lds_dst, int bytes,
                                     F src_off) {
  const int tid = fresh_tid();
  const int lane = tid & 63, wave = tid >> 6, nw = blockDim.x >> 6;
  for (int s0 = wave * 256; s0 < bytes; s0 += nw * 256) {
    const int d = s0 + 4 * lane;
    if (d < bytes)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rs, (__attribute__((address_space(3))) void*)(lds_dst + s0), 4, src_off(d), 0, 0, 0);
  }
}

// One work item (Item, me_geom.h) = (tile of TB blocks, dy pass).
template <int B, int K>
__device__ __forceinline__ Item item_of(const SearchArgs& p, const QsadGeom& g, int tile,
                                        int pass) {
  Item it;
  it.j = 0;
  if (g.strip_w > 0) {
    // strip-major: strip s holds tile columns [s * sw, s * sw + its width),
    // walked row by row (the last strip may be narrower)
    const int sw = g.strip_w, per = sw * g.nrows;
    const int s = tile / per, r = tile - s * per;
    const int w = min(sw, g.wg_per_row - s * sw);
    const int row = r / w;
    it.bx0 = (s * sw + (r - row * w)) * g.tb;
    it.by = g.row0 + row;
  } else {
    // row-major; the division by a multiply-high (scalar) where the host
    // verified the magic: a VALU integer division here ran twice per item
    const int row = g.magic_wpr ? (int)__umulhi((uint32_t)tile, g.magic_wpr) : tile / g.wg_per_row;
    it.bx0 = (tile - row * g.wg_per_row) * g.tb;
    it.by = g.row0 + row;
  }
  it.nb = min(g.tb, g.nbx_full - it.bx0);
  it.tly = it.by * B;
  it.h = min(B, p.height - it.tly);
  it.a = ((it.bx0 * B - p.range) % 4 + 4) % 4;
  it.X0 = it.bx0 * B - p.range - it.a;
  it.c0 = pass * g.cpp;
  it.nch = min(g.cpp, g.chunks - it.c0);
  it.prow0 = it.tly - p.range + it.c0 * K;  // frame row of tile row 0
  it.prows = it.nch * K + B - 1;            // rows this item touches
  return it;
}

// Tile of a launch over a job table -> (job, tile of that job's rows): jobs
// are consecutive tile ranges (jb.tile_pre), every job the same frame
// geometry; a job's planes and records are its own.
// job_item_at: j is the tile's job (flow_job_from / flow_job_find of me_geom.h).
template <int B, int K>
__device__ __forceinline__ Item job_item_at(const SearchArgs& p, const QsadGeom& g,
                                            const FlowJobs& jb, int tile, int pass, int j) {
  QsadGeom gj = g;
  gj.row0 = jb.r0[j];
  if (g.strip_w > 0) gj.nrows = (jb.tile_pre[j + 1] - jb.tile_pre[j]) / g.wg_per_row;  // strip walk
  Item it = item_of<B, K>(p, gj, tile - jb.tile_pre[j], pass);
  it.j = j;
  return it;
}
// The item kernel claims its tiles dynamically and in no order: the scan from
// job 0.  (flow_job_from's loop and job_item_at's body written out: through
// either helper every me_fast_kernel instance allocated its registers anew,
// and its items are long enough to hide the scan.)
template <int B, int K>
__device__ __forceinline__ Item job_item(const SearchArgs& p, const QsadGeom& g,
                                         const FlowJobs& jb, int tile, int pass) {
  int j = 0;
  while (j + 1 < jb.n && jb.tile_pre[j + 1] <= tile) j++;
  QsadGeom gj = g;
  gj.row0 = jb.r0[j];
  if (g.strip_w > 0) gj.nrows = (jb.tile_pre[j + 1] - jb.tile_pre[j]) / g.wg_per_row;  // strip walk
  Item it = item_of<B, K>(p, gj, tile - jb.tile_pre[j], pass);
  it.j = j;
  return it;
}

// Issue the staging of one item into an LDS buffer from its job's planes:
// asynchronous LDS DMA on the aligned path (no VGPR round trip, completes
// under the previous item's compute), synchronous byte copies otherwise.
template <int B>
__device__ __forceinline__ void stage_item(const SearchArgs& p, const QsadGeom& g, const Item& it,
                                           uint8_t* buf, const FlowJobs& jb) {
  uint8_t* tile = buf;
  uint8_t* cur = buf + g.tile_bytes;
  const int pitch = g.pitch, stride = p.stride;
  const int tid = fresh_tid(), nthr = blockDim.x;
  const int ref_row0 = jb.ref_row0[it.j], cur_row0 = jb.cur_row0[it.j];
  if (g.aligned) {
    const __amdgpu_buffer_rsrc_t rref = __builtin_amdgcn_make_buffer_rsrc(
        (void*)jb.ref[it.j], (short)0, jb.ref_bytes[it.j], 0x00020000);
    const __amdgpu_buffer_rsrc_t rcur = __builtin_amdgcn_make_buffer_rsrc(
        (void*)jb.cur[it.j], (short)0, jb.cur_bytes[it.j], 0x00020000);
    // tile byte (r, x) <- ref(prow0 + r, X0 + x); zeros outside the resident rows.
    const int base = (it.prow0 - ref_row0) * stride + it.X0;
    auto src = [&](int d) {
      const int r = (int)__umulhi((uint32_t)d, g.pitch_magic), x = d - r * pitch;
      return (uint32_t)(base + r * stride + x);
    };
    // 16-byte granules when X0, the frame width and the rows are 16-aligned:
    // no granule straddles x = 0 or x = W, and a quarter of the DMA steps.
    if (g.tile16)
      dma16(rref, tile, it.prows * pitch, src);
    else
      dma4(rref, tile, it.prows * pitch, src);
    // cur block b, row oy -> LDS bytes (b * B + oy) * B
    const int cbase = (it.tly - cur_row0) * stride + it.bx0 * B;
    if constexpr (B == 16) {
      dma16(rcur, cur, it.nb * B * B, [&](int d) {
        return (uint32_t)(cbase + ((d >> 4) & 15) * stride + (d >> 8) * B);
      });
    } else {
      dma4(rcur, cur, it.nb * B * B, [&](int d) {
        return (uint32_t)(cbase + ((d >> 3) & 7) * stride + (d >> 6) * B + (d & 4));
      });
    }
  } else {
    for (int i = tid; i < it.prows * pitch; i += nthr) {
      const int r = i / pitch, x = i - r * pitch;
      const int y = it.prow0 + r, xx = it.X0 + x;
      tile[i] = (y >= 0 && y < p.height && xx >= 0 && xx < p.width)
                    ? row_ptr(p, jb.ref[it.j], ref_row0, y)[xx] : 0;
    }
    for (int i = tid; i < it.nb * B * B; i += nthr) {
      const int b = i / (B * B), rem = i - b * B * B, oy = rem / B, x = rem - oy * B;
      cur[i] = oy < it.h ? row_ptr(p, jb.cur[it.j], cur_row0, it.tly + oy)[(it.bx0 + b) * B + x] : 0;
    }
  }
}

// Persistent, double-buffered search over a job table (one frame, or the
// frames / stripes of a batch: every job's tiles, job-major).  The grid is
// sized to what fits on the chip at once; workgroups sharing an XCD (bid % 8,
// a speed heuristic only) walk one contiguous band of tiles, so each XCD's L2
// holds one band of rows.  Item k of a workgroup = (its k / passes-th tile,
// pass k % passes); while item k is computed from LDS buffer k & 1, item k + 1
// streams into the other.
template <int COST, int B, int K, int PC = 0>
__global__ __launch_bounds__(1024) void me_fast_kernel(SearchArgs p, QsadGeom g, FlowJobs jb) {
  constexpr int CW = B / 4;
  extern __shared__ __align__(16) uint8_t smem[];
  const int buf_bytes = g.tile_bytes + g.tb * B * B;
  uint64_t* keys = reinterpret_cast<uint64_t*>(smem + 2 * buf_bytes);
  const int tid = threadIdx.x, nthr = blockDim.x;
  const int S = p.range;

  // Tiles of this workgroup come from the band of its XCD group x (bid % 8,
  // a speed heuristic only).  Dynamic (p.sched != null): the group's
  // workgroups pull whole tiles from one agent-scope counter, so faster CUs
  // take more; tile ids are pulled two tiles ahead into an LDS ring so the
  // double-buffered staging always knows its next item.  Static otherwise:
  // member m of n_x takes band tiles m, m + n_x, ...
  const int ntiles = jb.tile_pre[jb.n];
  const int nwg = (int)gridDim.x, bid = (int)blockIdx.x;
  const int ng = nwg < 8 ? nwg : 8;  // XCD groups that have workgroups
  const int x = bid % ng, m = bid / ng;
  const int n_x = nwg / ng + (x < nwg % ng ? 1 : 0);
  const int band0 = (int)((long)ntiles * x / ng), band1 = (int)((long)ntiles * (x + 1) / ng);
  const int passes = (g.chunks + g.cpp - 1) / g.cpp;
  // Dynamic only with enough tiles per workgroup (g.dyn_tiles, see plan_fast):
  // with few, the item-start pulls of all workgroups coincide and serialise.
  const bool dyn = p.sched != nullptr && g.dyn_tiles > 0 && ntiles >= g.dyn_tiles * nwg;
  int* tq = reinterpret_cast<int*>(smem + 2 * buf_bytes + 128);  // 4-slot ring of tile ids
#ifdef ME_STAMPS
  const int wid = bid;
  const int wwid = bid * (int)(blockDim.x >> 6) + (int)(threadIdx.x >> 6);
#endif
  ME_STAMP(0, __builtin_amdgcn_s_memtime());
  ME_STAMP(6, __builtin_amdgcn_s_memrealtime());
  ME_WSTAMP(0, __builtin_amdgcn_s_memtime());
  ME_WSTAMP(6, __builtin_amdgcn_s_memrealtime());
  // Staging at raised issue priority: the SIMD arbiter otherwise favours the
  // oldest waves, so the co-resident workgroups already computing starve a
  // later one's staging address math and it gets its first item late (the
  // small-stripe "staircase" of DESIGN.md (e): per-wave stamps
  // profiles/r03c_wave_stamps.txt).
  if (g.prio) __builtin_amdgcn_s_setprio(3);
  // Dynamic: each workgroup's first two tiles are its static ones (no atomic
  // storm at launch); band y's tiles past its first 2 * n_y are claimed from a
  // two-ended u64 counter: its own workgroups from the front (low half), once
  // their band is exhausted other XCD groups' workgroups from the back (high
  // half; clocks differ by several % between XCDs, so bands finish unevenly).
  // One atomic add per claim and the claim is valid iff lo + hi < avail of the
  // returned old value, so every tile is claimed once.  Thieves take the band's
  // LAST rows, contiguously, where front steals each re-read a whole window
  // (2S + B rows) on the thief's XCD for B rows of output; at 4K +-64 steals
  // are few and both measured alike (365 vs 368 MB per 16-frame launch,
  // profiles/r04i_*, r04j_*: the excess there was the claim distance, below).
  auto pull = [&]() -> int {
    for (int d = 0; d < ng; d++) {
      const int y = x + d < ng ? x + d : x + d - ng;
      const int b0 = (int)((long)ntiles * y / ng), b1 = (int)((long)ntiles * (y + 1) / ng);
      const int n_y = nwg / ng + (y < nwg % ng ? 1 : 0);
      const int first = min(b1 - b0, 2 * n_y), avail = b1 - b0 - first;
      if (avail <= 0) continue;
      const uint64_t o = __hip_atomic_fetch_add(reinterpret_cast<uint64_t*>(p.sched) + y,
                                                d == 0 ? 1ull : (1ull << 32), __ATOMIC_RELAXED,
                                                __HIP_MEMORY_SCOPE_AGENT);
      const int lo = (int)(uint32_t)o, hi = (int)(o >> 32);
      if (lo + hi < avail) return d == 0 ? b0 + first + lo : b1 - 1 - hi;
    }
    return -1;
  };
  auto static_tile = [&](int i) -> int {  // i-th static tile of this workgroup
    const int t = band0 + m + i * n_x;
    return t < band1 ? t : -1;
  };
  auto tile_at = [&](int i) -> int {  // i-th tile of this workgroup, -1 = none
    return dyn ? tq[i & 3] : static_tile(i);
  };
  auto claim = [&](int i) -> int {  // tile i of this workgroup (dynamic)
    if (i < 2) {
      const int t = static_tile(i);
      if (t >= 0) return t;
    }
    return pull();
  };
  const int ahead = g.pull_ahead;
  if (dyn && tid == 0) {
    tq[0] = claim(0);
    if (ahead == 2) tq[1] = tq[0] >= 0 ? claim(1) : -1;
  }
  if (tid < g.tb) keys[tid] = ~0ull;
  __syncthreads();

  int ti = 0, pass = 0;
  int rot = bid % (nthr >> 6);
#ifdef ME_STAMPS
  int nitems = 0;
#endif
  int tile = tile_at(0);
  if (tile >= 0) stage_item<B>(p, g, job_item<B, K>(p, g, jb, tile, 0), smem, jb);
  const int G = g.groups;
  for (int k = 0; tile >= 0; k++) {
    const Item it = job_item<B, K>(p, g, jb, tile, pass);
    uint8_t* buf = smem + (k & 1) * buf_bytes;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();  // item k staged by every wave; item k-1 fully consumed
    if (k == 0) ME_STAMP(2, __builtin_amdgcn_s_memtime());  // first item staged
    if (k == 0) ME_WSTAMP(1, __builtin_amdgcn_s_memtime());
    if (dyn && pass == 0 && tid == 0) {  // starting tile ti: claim tile ti + ahead
      const int prev = tq[(ti + ahead - 1) & 3];
      tq[(ti + ahead) & 3] = prev >= 0 ? claim(ti + ahead) : -1;
    }
    {
      const int ntile = pass + 1 < passes ? tile : tile_at(ti + 1);
      const int npass = pass + 1 < passes ? pass + 1 : 0;
      if (g.prio) __builtin_amdgcn_s_setprio(3);
      if (ntile >= 0)
        stage_item<B>(p, g, job_item<B, K>(p, g, jb, ntile, npass),
                      smem + ((k + 1) & 1) * buf_bytes, jb);
      if (g.prio) __builtin_amdgcn_s_setprio(0);
    }
#ifdef ME_STAMPS
    nitems++;
#endif
    const uint32_t* cur_lds = reinterpret_cast<const uint32_t*>(buf + g.tile_bytes);
    const uint32_t tile_off = (uint32_t)((k & 1) * buf_bytes);
    const int dymin = max(-S, -it.tly), dymax = min(S, p.height - it.h - it.tly);
    // Chunks whose dy range lies wholly outside [dymin, dymax] (top / bottom
    // block rows) are skipped: tasks are chunk-major, so whole waves drop out.
    const int lc0 = max(0, (dymin + S) / K - it.c0);
    const int lc1 = min(it.nch, (dymax + S) / K + 1 - it.c0);
    // Every candidate row of this item valid -> no per-row masks (uniform).
    const bool full_rows = dymin + S <= it.c0 * K && dymax + S >= (it.c0 + it.nch) * K - 1;
    const int per_chunk = it.nb * G;
    const int T = (lc1 - lc0) * per_chunk;
    // task t -> (chunk, block, group) by multiply-high: t / G with the host's
    // verified magic, then / nb with a per-item magic (nb <= 16).
    const uint32_t magic_nb = it.nb == g.tb ? g.magic_tb : 0xFFFFFFFFu / (uint32_t)it.nb + 1u;
    // When T is not a multiple of the workgroup size the last round falls to
    // the first waves; rotate which wave that is from item to item so no SIMD
    // takes every extra round (rot == (bid + k) % waves, kept as a counter).
    int vt = fresh_tid() - 64 * rot;
    if (vt < 0) vt += nthr;
    rot = rot + 1 == (nthr >> 6) ? 0 : rot + 1;
    for (int t = vt; t < T; t += nthr) {
      const int bg = (int)__umulhi((uint32_t)t, g.magic_groups);  // t / G
      const int gi = t - bg * G;
      const int lcr = it.nb == 1 ? bg : (int)__umulhi((uint32_t)bg, magic_nb);  // bg / nb
      const int b = bg - lcr * it.nb;
      const int lc = lc0 + lcr;
      const int d0 = (it.c0 + lc) * K;
      const int tlx = (it.bx0 + b) * B;

      uint32_t c[B][CW];
#pragma unroll
      for (int y = 0; y < B; y++) {
        if constexpr (CW == 4) {
          const uint4 v = reinterpret_cast<const uint4*>(cur_lds)[b * B + y];
          c[y][0] = v.x; c[y][1] = v.y; c[y][2] = v.z; c[y][3] = v.w;
        } else {
          const uint2 v = reinterpret_cast<const uint2*>(cur_lds)[b * B + y];
          c[y][0] = v.x; c[y][1] = v.y;
        }
      }
      // Valid candidate ranges of this block (main.c:73-76 in closed form).
      const int dxmin = max(-S, -tlx), dxmax = min(S, p.width - B - tlx);
      const int jlo = dymin + S - d0, jhi = dymax + S - d0;
      if constexpr (COST == COST_SSD) {
        // lane = one dx (gi = dx + S); its column starts at tile byte b*B + a + gi
        const int q = b * B + it.a + gi, dx = gi - S;
        uint32_t v[K];
        if (it.h == B)
          ssd_lane<B, K, B>(smem, g.pitch, tile_off, lc * K, q >> 2, q & 3, c, v);
        else
          ssd_lane<B, K, B / 2>(smem, g.pitch, tile_off, lc * K, q >> 2, q & 3, c, v);
        uint32_t best = full_rows ? lane_best_ssd<K, false>(v, jlo, jhi)
                                  : lane_best_ssd<K, true>(v, jlo, jhi);
        if (dx < dxmin || dx > dxmax) best = ~0u;
        if (best != ~0u) {
          const int dy = d0 + (int)(best & 31u) - S;
          atomicMin(reinterpret_cast<unsigned long long*>(&keys[b]),
                    (unsigned long long)make_key(best >> 5, dx, dy));
        }
        continue;
      }
      const int w0 = (b * B) / 4 + gi;
      uint64_t acc[K];
      // fold: lane gi < K also owns candidate (dx = +S, dy index jt = gi)
      const int jt = gi < K ? gi : K - 1;
      const uint32_t toff = tile_off + (uint32_t)((lc * K + jt) * g.pitch + b * B + 2 * S);
      uint32_t tsad = 0;
      if (it.h == B) {
        qsad_lane<B, K, B, PC>(smem, g.pitch, tile_off, lc * K, w0, c, acc);
        if (g.fold) tsad = tail_sad<B, B>(smem, g.pitch, toff, c);
      } else {
        qsad_lane<B, K, B / 2, PC>(smem, g.pitch, tile_off, lc * K, w0, c, acc);
        if (g.fold) tsad = tail_sad<B, B / 2>(smem, g.pitch, toff, c);
      }
      // Waves with no frame-edge candidate (most of them) take the unmasked
      // epilogue: the test is wave-uniform, so there is no divergence.
      const int dxg = 4 * gi - S - it.a;  // dx of this lane's first candidate
      const bool edge = dxg < dxmin || dxg + 3 > dxmax;
      uint32_t best;
      const bool no_edge = __builtin_amdgcn_ballot_w64(edge) == 0;
      const int sjlo = __builtin_amdgcn_readfirstlane(jlo), sjhi = __builtin_amdgcn_readfirstlane(jhi);
      if (no_edge && (full_rows || __builtin_amdgcn_ballot_w64(jlo != sjlo || jhi != sjhi) == 0)) {
        // Rows partial only (the last dy chunk, the top and bottom block rows)
        // with one row range for the wave: park the invalid rows at SAD 0xFFFF
        // (scalar tests, a move only where a row is out) and take the unmasked
        // epilogue; the masked one tests every row of every lane.  (Testing
        // the row range only on partial-row tasks measured 0.7 % slower at 8K:
        // 271.7 vs 269.7 ms, profiles/r04y_ab.txt.)
        if (!full_rows) {
#pragma unroll
          for (int j = 0; j < K; j++)
            if (j < sjlo || j > sjhi) acc[j] = ~0ull;
        }
        best = lane_best<K, false>(acc, 0u, 0u, jlo, jhi);
      } else {
        uint32_t mlo = 0, mhi = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int dx = dxg + i;
          const uint32_t msk = (dx < dxmin || dx > dxmax) ? 0xFFFFu : 0u;
          if (i < 2) mlo |= msk << (16 * i);
          else mhi |= msk << (16 * (i - 2));
        }
        best = lane_best<K, true>(acc, mlo, mhi, jlo, jhi);
      }
      if (g.fold) {
        const bool tv = gi < K && jt >= jlo && jt <= jhi && S <= dxmax;
        best = min(best, tv ? (tsad << 16) | (uint32_t)(5 * jt + 4) : ~0u);
      }
      if (best < 0xFFFF0000u) {
        const int idx = (int)(best & 0xFFFFu), jj = idx / 5, i = idx - 5 * jj;
        const int dy = d0 + jj - S, dx = i == 4 ? S : 4 * gi + i - S - it.a;
        atomicMin(reinterpret_cast<unsigned long long*>(&keys[b]),
                  (unsigned long long)make_key(best >> 16, dx, dy));
      }
    }
    ME_WSTAMP(2, __builtin_amdgcn_s_memtime());  // this wave's tasks of item k done
    if (pass == passes - 1) {
      __syncthreads();  // every task of the tile has folded its key
      if (tid < it.nb) {
        const uint64_t kk = keys[tid];
        uint64_t none = ~0ull;  // materialised here, not kept live (it spilled)
        asm volatile("" : "+v"(none));
        keys[tid] = none;  // ready for this workgroup's next tile
        const int out = (it.by - jb.r0[it.j]) * p.nbx + it.bx0 + tid;
        int16_t* mv = jb.mv[it.j];
        store_mv(mv, out, kk);
        uint32_t cost = (uint32_t)(kk >> 32);
        if constexpr (COST == COST_SSD) {  // biased v -> SSD: + sum c^2 of the block
          const uint32_t* cb = reinterpret_cast<const uint32_t*>(buf + g.tile_bytes) + tid * B * CW;
          uint32_t csq = 0;
#pragma unroll 4
          for (int i = 0; i < B * CW; i++) csq = __builtin_amdgcn_udot4(cb[i], cb[i], csq, false);
          cost = cost - SSD_BIAS + csq;
        }
        if (jb.cost[it.j]) jb.cost[it.j][out] = cost;
      }
      ti++;
      pass = 0;
      tile = tile_at(ti);  // written >= one barrier ago
    } else {
      pass++;
    }
  }
  ME_STAMP(1, (unsigned long long)nitems);
#ifdef ME_STAMPS
  if ((threadIdx.x & 63) == 0 && wwid < (1 << 14)) {
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    g_wstamps[8 * wwid + 3] = __builtin_amdgcn_s_memtime();
    g_wstamps[8 * wwid + 4] = hw;
    g_wstamps[8 * wwid + 5] = xcc;
    g_wstamps[8 * wwid + 7] = __builtin_amdgcn_s_memrealtime();
  }
#endif
  if (dyn && tid == 0) {
    // The last workgroup out re-zeroes the counters for the next launch on
    // this stream (every other workgroup's final pull precedes its arrival).
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    const uint32_t d = __hip_atomic_fetch_add(p.sched + SCHED_ARRIVE, 1u, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
    if (d == (uint32_t)nwg - 1) {
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
#pragma unroll
      for (int i = 0; i <= SCHED_ARRIVE; i++)
        __hip_atomic_store(p.sched + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
#ifdef ME_STAMPS
  if (tid == 0 && wid < (1 << 16)) {
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    g_stamps[8 * wid + 3] = __builtin_amdgcn_s_memtime();
    g_stamps[8 * wid + 4] = hw;
    g_stamps[8 * wid + 5] = xcc;
    g_stamps[8 * wid + 7] = __builtin_amdgcn_s_memrealtime();
  }
#endif
}

// --------------------------------------------------------------- flow (SAD)
// One workgroup per CU, 16 waves, no barriers after the start.  The
// workgroup's items (tiles of tb blocks with ALL their dy chunks) sit in a
// ring of NB LDS slots; the waves pull wave-tasks (64 consecutive lane-tasks
// of one item) from one LDS counter, so the 4 waves of every SIMD keep taking
// work until the workgroup's list is empty: no item barrier, no per-item
// partial last round of the workgroup (tb * G * chunks is a multiple of 64 on
// the shapes the planner gives this kernel: 1080p +-32 tb = 4 -> 320 lanes).
// The wave that finishes an item's last wave-task writes its blocks' vectors,
// then refills the slot with item k + NB (LDS DMA, its own vmcnt wait) and
// publishes it; a wave that pulls a task of an unpublished item sleeps on the
// slot's ready word.  Pulls are in order, so the items < k are all pulled
// before a wave waits on item k: the last of them to finish refills slot k % NB.
struct FlowCtl {
  uint32_t next;       // wave-tasks handed out
  uint32_t ready[16];  // item index + 1 published in the slot
  uint32_t done[16];   // wave-tasks of the slot's item finished
  // The pruning switches (PF_*), copied here once: read from LDS where they
  // are used, they occupy no SGPRs across the task loop (kernel arguments would).
  uint32_t pflags;
  uint32_t run;        // items in a row the bound could not thin (bypass)
  // pruning launches only (the plain launch's LDS ends above)
  uint32_t live[16];   // live lane-tasks of the slot's item (its list's length)
  uint32_t stats[4];   // tuning build: live, all lane-tasks, bypassed items, items (flushed at the end)
  uint32_t split[3];   // tuning build: executed wave-tasks run whole, with 2 and with 4 or more lanes per list entry
  uint32_t hist_off;   // tuning build (PF_HIST): bytes from this block to the launch's 64 counters of executed wave-tasks of
                       // h = B items by list entries held (sched[SCHED_SPLIT_HIST ..])
  uint32_t pre[3];     // tuning build, chain kernel: items pre-bound, post-bounds that met BUSY, items that fell back (a bounded
                       // item of a slot's second or later turn whose marker named no pre-bound: it ran the whole bound)
};
// PF_PLANES: the launch has box-sum planes (FlowJobs::planes): flow_bound skips
// its step 1 and loads the plane rows of step 2 from them (the slim scratch).
// PF_SPLIT: a pruned item's wave-task of <= 32 list entries is split by rows
// (flow_split_task below); PF_SPLIT_124: by the earlier rule of 1, 2 or 4 lanes
// per entry (the tuning build's A/B).
// PF_TABLE: the workgroup's items are decoded in the LDS item table behind this
// block (me_geom.h FlowEntry).  PF_EARLY: a slot's fill issues the window DMA
// last and starts the bound under it (flow_fill below).  PF_PRE: the wave that
// publishes an item forms the bound's minlb of the slot's next item behind the
// publish (the pre-bound, flow_fill below); PF_PRE_PRIO: its issue priority.
enum { PF_ON = 1, PF_VERIFY = 2, PF_BYPASS = 4, PF_STATS = 8, PF_PLANES = 16, PF_SPLIT = 32, PF_TABLE = 64,
       PF_EARLY = 128, PF_PRE = 256, PF_PRE_PRIO_SHIFT = 9, PF_PRE_PRIO = 3 << PF_PRE_PRIO_SHIFT,
       PF_SPLIT_124 = 2048, PF_HIST = 4096 };  // (PF_HIST: QsadGeom::prune_stats == 2)
static_assert(sizeof(FlowCtl) <= FLOW_CTL_BYTES, "control block of the pruning launch");

// Tile of the flow kernel's launch -> its item (all dy chunks: one pass).  A
// workgroup's tiles only grow (band0 + m + k n_x), so an item's job is found
// from the job jprev of an earlier item of the workgroup; the first lookup of
// a wave (jprev < 0) bisects the table.  The scan from job 0 this replaces made
// one scalar-memory round trip per job in front of the tile, at every advance
// and in front of every refill's DMA.
template <int B, int K>
__device__ __forceinline__ Item flow_item(const SearchArgs& p, const QsadGeom& g,
                                          const FlowJobs& jb, int tile, int jprev) {
  const int j = jprev < 0 ? flow_job_find(jb, tile) : flow_job_from(jb, tile, jprev);
  return job_item_at<B, K>(p, g, jb, tile, 0, j);
}

// Single-wave LDS DMA of one flow item (the aligned path): tile rows and cur
// blocks, from its job's planes, under the caller's one vmcnt wait.  (The
// job's box-sum planes are not staged: the bound phase loads what it reads of
// them into registers, flow_plane_fetch below.)
template <int B>
__device__ __forceinline__ void stage_item_wave(const SearchArgs& p, const QsadGeom& g, const Item& it,
                                                uint8_t* buf, const FlowJobs& jb) {
  const __amdgpu_buffer_rsrc_t rref =
      __builtin_amdgcn_make_buffer_rsrc((void*)jb.ref[it.j], (short)0, jb.ref_bytes[it.j], 0x00020000);
  const __amdgpu_buffer_rsrc_t rcur =
      __builtin_amdgcn_make_buffer_rsrc((void*)jb.cur[it.j], (short)0, jb.cur_bytes[it.j], 0x00020000);
  // lane recomputed per call (fresh_tid): hoisted lane-derived offsets spilled
  const int lane = fresh_tid() & 63;
  uint8_t* tile = buf;
  uint8_t* cur = buf + g.tile_bytes;
  const int pitch = g.pitch, stride = p.stride;
  const uint32_t base = (uint32_t)((it.prow0 - jb.ref_row0[it.j]) * stride + it.X0);
  const int bytes = it.prows * pitch;
  for (int s0 = 0; s0 < bytes; s0 += 1024) {  // 16-byte granules (g.tile16)
    const int d = s0 + 16 * lane;
    const int r = (int)__umulhi((uint32_t)d, g.pitch_magic), x = d - r * pitch;
    if (d < bytes)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rref, (__attribute__((address_space(3))) void*)(tile + s0), 16,
          base + (uint32_t)(r * stride + x), 0, 0, 0);
  }
  const uint32_t cbase = (uint32_t)((it.tly - jb.cur_row0[it.j]) * stride + it.bx0 * B);
  const int cb = it.nb * B * B;
  for (int s0 = 0; s0 < cb; s0 += 1024) {
    const int d = s0 + 16 * lane;
    if (d < cb)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(
          rcur, (__attribute__((address_space(3))) void*)(cur + s0), 16,
          cbase + (uint32_t)(((d >> 4) & 15) * stride + (d >> 8) * B), 0, 0, 0);
  }
}

// The chain kernel stages an item in parts (flow_fill): stage_item_wave's two loops apart.
// WHAT: bit 0 the window, bit 1 the cur blocks (window first where both).
// STEPS > 0: the window in exactly STEPS DMA instructions (the caller checked
// that the item's bytes end in the last of them), so that a vmcnt(STEPS) behind
// them waits for everything issued in front and for nothing of the window.
constexpr int FLOW_STAGE_WIN = 1, FLOW_STAGE_CUR = 2;
template <int B, int WHAT, int STEPS = 0>
__device__ __forceinline__ void stage_item_part(const SearchArgs& p, const QsadGeom& g, const Item& it,
                                                uint8_t* buf, const FlowJobs& jb) {
  const __amdgpu_buffer_rsrc_t rref =
      __builtin_amdgcn_make_buffer_rsrc((void*)jb.ref[it.j], (short)0, jb.ref_bytes[it.j], 0x00020000);
  const __amdgpu_buffer_rsrc_t rcur =
      __builtin_amdgcn_make_buffer_rsrc((void*)jb.cur[it.j], (short)0, jb.cur_bytes[it.j], 0x00020000);
  // lane recomputed per call (fresh_tid): hoisted lane-derived offsets spilled
  const int lane = fresh_tid() & 63;
  uint8_t* tile = buf;
  uint8_t* cur = buf + g.tile_bytes;
  const int pitch = g.pitch, stride = p.stride;
  if constexpr ((WHAT & FLOW_STAGE_WIN) != 0) {
    const uint32_t base = (uint32_t)((it.prow0 - jb.ref_row0[it.j]) * stride + it.X0);
    const int bytes = it.prows * pitch;
    auto step = [&](int s0) {  // 16-byte granules (g.tile16)
      const int d = s0 + 16 * lane;
      const int r = (int)__umulhi((uint32_t)d, g.pitch_magic), x = d - r * pitch;
      if (d < bytes)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            rref, (__attribute__((address_space(3))) void*)(tile + s0), 16,
            base + (uint32_t)(r * stride + x), 0, 0, 0);
    };
    if constexpr (STEPS > 0) {
#pragma unroll
      for (int i = 0; i < STEPS; i++) step(1024 * i);
    } else {
      for (int s0 = 0; s0 < bytes; s0 += 1024) step(s0);
    }
  }
  if constexpr ((WHAT & FLOW_STAGE_CUR) != 0) {
    const uint32_t cbase = (uint32_t)((it.tly - jb.cur_row0[it.j]) * stride + it.bx0 * B);
    const int cb = it.nb * B * B;
    for (int s0 = 0; s0 < cb; s0 += 1024) {
      const int d = s0 + 16 * lane;
      if (d < cb)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(
            rcur, (__attribute__((address_space(3))) void*)(cur + s0), 16,
            cbase + (uint32_t)(((d >> 4) & 15) * stride + (d >> 8) * B), 0, 0, 0);
    }
  }
}

// Wave-tasks of one item: its lane-tasks (valid chunks x blocks x groups) / 64, rounded up.
template <int B, int K>
__device__ __forceinline__ int flow_tasks(const SearchArgs& p, const QsadGeom& g, const Item& it,
                                          int* lc0_out) {
  // (flow_item_tasks of me_geom.h, the item table's count, is this rule: tests/test_flow_item_table.py)
  const int S = p.range;
  const int dymin = max(-S, -it.tly), dymax = min(S, p.height - it.h - it.tly);
  const int lc0 = max(0, (dymin + S) / K), lc1 = min(it.nch, (dymax + S) / K + 1);
  *lc0_out = lc0;
  return ((lc1 - lc0) * it.nb * g.groups + 63) >> 6;
}

// ------------------------------------------------------ flow: the bound phase
// Pruning by an exact lower bound.  Let q(.) be the 4x4 box sum >> 4; a 16x16
// block has 16 sub-blocks sb.  By the triangle inequality per sub-block, and
// with at most 15 lost to each of the 16 shifts,
//     SAD(c, r) >= sum_sb |sum c_sb - sum r_sb| >= 16 * sum_sb |q(c_sb) - q(r_sb)| - 240 = LB.
// The wave that staged an item runs this before it publishes the slot:
//   1. q of the whole staged window as four byte planes by x phase (plane k
//      holds columns = k mod 4), and q of the cur blocks' 16 sub-blocks;
//   2. sum_sb |..| of every VALID candidate, 4 candidates per qsad (4 qsads per
//      candidate row: one per sub-block row), min-reduced into minlb[lc][b][gi]
//      per lane-task, the fold column (dx = +S) into the lane-task that owns it;
//   3. the exact SAD of two seeds per block, (0, 0) and the candidate of the
//      smallest bound, merged into the slot's keys like any lane-task's result;
//      U_b = the seeded key's cost;
//   4. the list of the lane-tasks with 16 * minlb - 240 <= U_b (signed), in
//      index order (so a full list is the identity).
// Exactness: a lane-task is left out only if every valid candidate in it has
// LB > U_b; U_b is the exact SAD of a valid candidate of block b already in
// keys; LB <= SAD, so every skipped candidate has SAD > U_b and can neither
// win nor tie.  Equality is never pruned.  Invalid (clamped-out) candidates
// enter no minimum: they never seed and never keep a lane-task alive.
// Items of the h = B/2 bottom row are not bounded: all their lane-tasks live.
// Entry of minlb: q-sum << 7 | dy index in the chunk << 3 | x phase (4: fold).
typedef unsigned short flow_us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_key(uint32_t a, uint32_t j) {  // per u16: a * 16 + j
  const flow_us2 v = __builtin_bit_cast(flow_us2, a) * (flow_us2)(16) + (flow_us2)((unsigned short)j);
  return __builtin_bit_cast(uint32_t, v);
}
__device__ __forceinline__ uint32_t pk_min(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(flow_us2, a),
                                                                __builtin_bit_cast(flow_us2, b)));
}
// Lane l's value of lane l ^ X (X < 32) by ds_swizzle: needs no lane id, which
// the compiler would keep in a VGPR across the 128-VGPR task loop.
template <int X>
__device__ __forceinline__ uint32_t swz_xor(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_ds_swizzle((int)v, (X << 10) | 0x1F);
}
__device__ __forceinline__ void lds_fence() {  // this wave's LDS writes before its later reads
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

// ---- the bound's plane rows, from the job's box-sum planes (PF_PLANES) ----
// In a launch with planes step 2 reads them from global memory (L2 / Infinity
// Cache resident: the prepass wrote them in front of this launch), not from a
// copy in the slot: lane (block b, phase k, dx groups 4m .. 4m + 3) loads the 8
// bytes flow_plane_byte(.., yp, k, 4 b + 4 m) of every window row yp its
// chunks read, each row once per item: a K = 13 row chunk reads the 25 rows
// lc K .. lc K + 24, the next one carries the last 12 over and loads 13.  The
// fold column's lane (block b, dy mod 16 = y) reads 4 bytes of phase 0 of the
// rows y + 4 n.  The descriptor holds exactly the job's plane bytes: rows
// above or below the job's resident ones read 0 and are masked like the
// window's (no load straddles the end: flow_plane_loads_fit, host-checked).
constexpr int FLOW_PLN_ROWS = 25, FLOW_PLN_FOLD = 20;
#ifdef ME_FLOW_STREAM  // the A/B build of the chain kernel's streamed step 2 (Makefile `stream`)
constexpr bool FLOW_STREAM = true;
#else
constexpr bool FLOW_STREAM = false;
#endif
struct FlowPlaneRegs {
  uint32_t lo[FLOW_PLN_ROWS], hi[FLOW_PLN_ROWS];  // the chunk's rows, bytes 0-3 and 4-7
  uint32_t f[FLOW_PLN_FOLD];                      // the fold column's rows y + 4 n
};
typedef uint32_t flow_u2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t flow_plane_rsrc(const FlowJobs& jb, int j) {
  return __builtin_amdgcn_make_buffer_rsrc((void*)(jb.planes + ((size_t)jb.plane_off64[j] << 6)), (short)0,
                                           jb.plane_rows[j] * 4 * jb.plane_pitch, 0x00020000);
}
// N window rows from y0 on of the lane's phase k at `byte`
template <int N, bool CHAIN = false>
__device__ __forceinline__ void flow_plane_rows_load(__amdgpu_buffer_rsrc_t rs, int pp, int rel, int X0, int y0,
                                                     int k, int byte, uint32_t (&lo)[N], uint32_t (&hi)[N],
                                                     int at = 0) {
  // The lane's part in one VGPR, the row's in an SGPR the compiler cannot
  // follow: it otherwise keeps all N row offsets in VGPRs across the chunk loop.
  // (The chain kernel: the lane's part opaque as well, else lane part + row
  // step, which no chunk changes, is hoisted out of its chunk loop as N more VGPRs.)
  uint32_t lv = flow_plane_lane_byte(pp, k, byte);
  uint32_t sr = flow_plane_row_byte(pp, rel, X0, y0);
  asm volatile("" : "+s"(sr));
  if constexpr (CHAIN) asm volatile("" : "+v"(lv));
#pragma unroll
  for (int r = 0; r < N; r++) {
    const flow_u2 v = __builtin_bit_cast(
        flow_u2, __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(lv + sr + (uint32_t)(4 * r * pp)), 0, 0));
    lo[at + r] = v.x;
    hi[at + r] = v.y;
  }
}
__device__ __forceinline__ void flow_plane_fold_load(__amdgpu_buffer_rsrc_t rs, int pp, int rel, int X0, int lane,
                                                     FlowPlaneRegs& R) {
  const uint32_t lv = flow_plane_lane_byte(pp, 0, 4 * (lane >> 4) + 16) + (uint32_t)(4 * (lane & 15) * pp);
  uint32_t sr = flow_plane_row_byte(pp, rel, X0, 0);
  asm volatile("" : "+s"(sr));
#pragma unroll
  for (int n = 0; n < FLOW_PLN_FOLD; n++)  // window row (lane & 15) + 4 n
    R.f[n] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rs, (int)(lv + sr + (uint32_t)(16 * n * pp)), 0, 0);
}
// Whether the staging wave issues the item's first plane loads with its window
// DMA (so both land under the one vmcnt wait): not for an item the bound will
// not look at (no planes in the launch, an h = B/2 item, the bypass state).
// The bypass state may end between here and the bound, which then loads them.
template <int B>
__device__ __forceinline__ bool flow_plane_wanted(const Item& it, FlowCtl* ctl) {
  const int pf = __builtin_amdgcn_readfirstlane((int)ctl->pflags);
  if (!(pf & PF_PLANES) || it.h != B) return false;
  return !((pf & PF_BYPASS) &&
           __builtin_amdgcn_readfirstlane(
               (int)__hip_atomic_load(&ctl->run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) >= 4);
}
// The first chunk's 25 rows.
template <int B, int K, bool CHAIN = false>
__device__ __forceinline__ void flow_plane_fetch(const Item& it, const FlowJobs& jb, FlowPlaneRegs& R) {
  constexpr int S = 32;
  static_assert(FLOW_PLN_ROWS == K + 12 && 4 * (FLOW_PLN_FOLD - 1) == 2 * S + 12, "rows a chunk, the fold column read");
  const int lane = fresh_tid() & 63;
  const int b = lane >> 4, k = (lane >> 2) & 3, m = lane & 3;
  const int lc0 = max(0, (max(-S, -it.tly) + S) / K);
  const __amdgpu_buffer_rsrc_t rs = flow_plane_rsrc(jb, it.j);
  const int pp = jb.plane_pitch, rel = it.prow0 - jb.ref_row0[it.j];
  flow_plane_rows_load<FLOW_PLN_ROWS, CHAIN>(rs, pp, rel, it.X0, lc0 * K, k, 4 * b + 4 * m, R.lo, R.hi);
}
__device__ __forceinline__ void flow_plane_zero(FlowPlaneRegs& R) {
#pragma unroll
  for (int r = 0; r < FLOW_PLN_ROWS; r++) R.lo[r] = R.hi[r] = 0;
#pragma unroll
  for (int n = 0; n < FLOW_PLN_FOLD; n++) R.f[n] = 0;
}

// R: the item's first plane rows where `fetched` (flow_plane_fetch, issued by
// the caller in front of its wait for the window); else loaded here if the
// launch has planes.
// The chain kernel runs the bound in two parts where it can (flow_fill below):
// PRE: the pre-bound alone, that is the init, step 2 and the fold column of an
// h = B item of a launch with planes, whose slot still holds the item in front:
// it reads the cur blocks from global memory (flow_qcur_byte), writes minlb and
// qcur and nothing else, and takes no part in the bypass accounting.  mark
// (not PRE): the slot's marker says that this item's pre-bound ran or is
// running, so the bound waits for its DONE (bounded; *expired) and then runs
// steps 3 and 4 alone, unless the bypass state gives the item its full list.
template <int B, int K, bool CHAIN = false, bool PRE = false>
__device__ __forceinline__ void flow_bound(const SearchArgs& p, const QsadGeom& g, const Item& it,
                                           uint8_t* buf, uint64_t* keys, FlowCtl* ctl, int slot,
                                           const FlowJobs& jb, FlowPlaneRegs& R, bool fetched,
                                           unsigned long long* bs = nullptr, const uint32_t* mark = nullptr,
                                           int kitem = 0, bool* expired = nullptr) {
  static_assert(CHAIN || !PRE, "the pre-bound is the chain kernel's");
  constexpr int S = 32, G = 16, TB = 4, P = 144;
#ifdef ME_STAMPS
  unsigned long long bt = __builtin_amdgcn_s_memtime();  // (bs: the stamps build's split of a refill's bound)
#endif
  static_assert(B == 16 && K == 13, "bound scratch layout");
  const int lane = fresh_tid() & 63;
  const int pf = __builtin_amdgcn_readfirstlane((int)ctl->pflags);
  const bool planes = (pf & PF_PLANES) != 0;  // the slim scratch: no planes in the slot
  uint8_t* pr = buf + g.tile_bytes + TB * B * B;
  uint16_t* list = reinterpret_cast<uint16_t*>(pr);  // (overlays the slot's planes, dead by then)
  uint32_t* minlb = reinterpret_cast<uint32_t*>(pr + (planes ? FLOW_SLIM_MINLB : FLOW_PRUNE_MINLB));
  uint32_t* qcur = reinterpret_cast<uint32_t*>(pr + (planes ? FLOW_SLIM_QCUR : FLOW_PRUNE_QCUR));
  const uint32_t* cur = reinterpret_cast<const uint32_t*>(buf + g.tile_bytes);
  const int dymin = max(-S, -it.tly), dymax = min(S, p.height - it.h - it.tly);
  const int lc0 = max(0, (dymin + S) / K), lc1 = min(it.nch, (dymax + S) / K + 1);
  const int valid_lanes = (lc1 - lc0) * it.nb * G;
  const int nw = (valid_lanes + 63) >> 6;
  const bool verify = (pf & PF_VERIFY) != 0, stats = (pf & PF_STATS) != 0;
  uint8_t* dead = pr + FLOW_PRUNE_DEAD;                            // verify: [320] flags
  uint32_t* ub = reinterpret_cast<uint32_t*>(pr + FLOW_PRUNE_UB);  // verify: U_b

  // Bypass: after 4 items in a row that stayed more than 3/4 live the bound is
  // skipped for 96 items, then ONE item probes again (run 3 -> 4 by
  // compare-and-swap: the bound phases of the other slots keep bypassing).
  int run = 0;
  bool prober = false;
  if (!PRE && (pf & PF_BYPASS)) {
    run = __builtin_amdgcn_readfirstlane(
        (int)__hip_atomic_load(&ctl->run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    if (run == 3 && it.h == B) {
      uint32_t old = 3u;
      if (lane == 0)
        __hip_atomic_compare_exchange_strong(&ctl->run, &old, 4u, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_WORKGROUP);
      run = __builtin_amdgcn_readfirstlane((int)old);
      prober = run == 3;
    }
  }
  const bool bypass = it.h == B && run >= 4;
  // The pre-bound of this item, if the marker names it, must have ended before
  // anything else here: also on the bypass path, which ignores what it left but
  // publishes the item, and the next pre-bound of the slot writes the same minlb.
  // (a constant where there is no marker: the kernels without one compile the code they had)
  std::conditional_t<CHAIN && !PRE, bool, std::false_type> have_pre{};
  if constexpr (CHAIN && !PRE) {
    if (mark) {
#ifdef ME_STAMPS
      const unsigned long long wt0 = __builtin_amdgcn_s_memtime();
#endif
      int spins = 0;
      while (__hip_atomic_load(mark, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != flow_mark_done(kitem) &&
             ++spins < (1 << 20))
        __builtin_amdgcn_s_sleep(2);
      if (spins >= (1 << 20)) {
        if (lane == 0 && p.sched)
          __hip_atomic_store(p.sched + SCHED_ERR, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *expired = true;
        return;
      }
#ifdef ME_STAMPS
      if (bs && spins) {
        bs[8] += __builtin_amdgcn_s_memtime() - wt0;
        bs[9]++;
        bt = __builtin_amdgcn_s_memtime();
      }
#endif
      if (stats && lane == 0 && spins) atomicAdd(&ctl->pre[1], 1u);
      have_pre = !bypass;
    } else if (stats && lane == 0 && kitem >= 0 && it.h == B && !bypass) {
      // fell back: a bounded item of a slot's later turn (kitem >= 0: its marker was written) found no pre-bound
      atomicAdd(&ctl->pre[2], 1u);
    }
  }
  if (!PRE && (it.h != B || bypass)) {
    for (int r = 0; r < nw; r++) {
      const int idx = 64 * r + lane;
      if (idx < valid_lanes) list[idx] = (uint16_t)idx;
      if (verify && idx < valid_lanes) dead[idx] = 0;
    }
    if (lane == 0) {
      ctl->live[slot] = (uint32_t)valid_lanes;
      if (bypass &&
          __hip_atomic_fetch_add(&ctl->run, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) + 1u >= 100u)
        __hip_atomic_store(&ctl->run, 3u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      if (stats) {
        atomicAdd(&ctl->stats[0], (uint32_t)valid_lanes);
        atomicAdd(&ctl->stats[1], (uint32_t)valid_lanes);
        if (bypass) atomicAdd(&ctl->stats[2], 1u);
        atomicAdd(&ctl->stats[3], 1u);
      }
    }
    return;
  }

  // 1. box sums: the lane owns window columns x0, x0 + 1 and walks the 80 rows
  // with a sliding 4-row sum of the packed horizontal 4-sums.  (Not in a
  // launch with planes: the same bytes wherever a valid candidate reads them.)
  if (!have_pre) {
  [[maybe_unused]] uint32_t cg[4];  // PRE: the lane's four cur dwords (issued in front of the plane rows: they return first)
  if constexpr (PRE) {
    const __amdgpu_buffer_rsrc_t rcur =
        __builtin_amdgcn_make_buffer_rsrc((void*)jb.cur[it.j], (short)0, jb.cur_bytes[it.j], 0x00020000);
#pragma unroll
    for (int r = 0; r < 4; r++) {
      // (a block past the tile's last: an offset no descriptor holds, the load returns 0)
      const uint32_t off = (lane >> 4) < it.nb ? flow_qcur_byte(jb.cur_row0[it.j], p.stride, it.tly, it.bx0, lane, r)
                                               : 0x80000000u;
      cg[r] = (uint32_t)__builtin_amdgcn_raw_buffer_load_b32(rcur, (int)off, 0, 0);
    }
  }
  if (planes) {
    if (!fetched) flow_plane_fetch<B, K, CHAIN>(it, jb, R);
  } else {
    const int x0 = 2 * lane, sh = x0 & 3;
    const uint8_t* src = buf + (x0 & ~3);
    uint8_t* dst = pr + sh * FLOW_PRUNE_PLANE + (x0 >> 2);  // planes sh and sh + 1
    uint32_t h1 = 0, h2 = 0, h3 = 0;
#pragma unroll 8
    for (int r = 0; r < K * 5 + B - 1; r++) {
      const uint32_t* w = reinterpret_cast<const uint32_t*>(src + r * P);
      const uint32_t w0 = w[0], w1 = w[1];
      const uint32_t a0 = __builtin_amdgcn_alignbyte(w1, w0, sh);
      const uint32_t a1 = __builtin_amdgcn_alignbyte(w1, w0, sh + 1);
      const uint32_t h0 = __builtin_amdgcn_sad_u8(a0, 0u, 0u) | (__builtin_amdgcn_sad_u8(a1, 0u, 0u) << 16);
      const uint32_t v = h0 + h1 + h2 + h3;  // two sums <= 4080: no carry between the halves
      h3 = h2; h2 = h1; h1 = h0;
      if (r >= 3) {
        dst[(r - 3) * 32] = (uint8_t)((v & 0xFFFFu) >> 4);
        dst[(r - 3) * 32 + FLOW_PRUNE_PLANE] = (uint8_t)(v >> 20);
      }
    }
  }
  {
    // q of the cur blocks: lane = (block, sub-block row, sub-block column)
    const uint32_t* cw = cur + ((lane >> 4) * B + 4 * ((lane >> 2) & 3)) * 4 + (lane & 3);
    uint32_t sum = 0;
    if constexpr (PRE) {
#pragma unroll
      for (int r = 0; r < 4; r++) sum = __builtin_amdgcn_sad_u8(cg[r], 0u, sum);
    } else {
#pragma unroll
    for (int r = 0; r < 4; r++) sum = __builtin_amdgcn_sad_u8(cw[4 * r], 0u, sum);
    }
    reinterpret_cast<uint8_t*>(qcur)[lane] = (uint8_t)(sum >> 4);
#pragma unroll
    for (int r = 0; r < 5; r++) minlb[64 * r + lane] = ~0u;
  }
  lds_fence();
  ME_BSTAMP(0);
  }

  const int b = lane >> 4;
  const int dxmin = max(-S, -(it.bx0 + b) * B), dxmax = min(S, p.width - B - (it.bx0 + b) * B);
  const int Ylo = dymin + S, Yhi = dymax + S;
  // 2. bounds: lane = (block, x phase k, 4 dx groups 4m..4m+3); u16 t of a qsad
  // is the candidate dx + S = 4 (4m + t) + k.
  if (!have_pre) {
    uint32_t qc[4];
#pragma unroll
    for (int sy = 0; sy < 4; sy++) qc[sy] = qcur[b * 4 + sy];
    const int k = (lane >> 2) & 3, m = lane & 3;
    uint32_t mlo = 0, mhi = 0;
#pragma unroll
    for (int t = 0; t < 4; t++) {
      const int dx = 4 * (4 * m + t) + k - S;
      const uint32_t msk = (dx < dxmin || dx > dxmax) ? 0xFFFFu : 0u;
      if (t < 2) mlo |= msk << (16 * t);
      else mhi |= msk << (16 * (t - 2));
    }
    // One chunk: row(r, lo, hi) gives the lane's 8 bytes of window row lc K + r.
    auto chunk = [&](int lc, auto row) {
      uint32_t clo = ~0u, chi = ~0u;
#pragma unroll
      for (int j = 0; j < K; j++) {
        // No branch on the row's validity (a scalar mask instead): the chunk
        // is straight-line code, so the plane reads run ahead of the qsads.
        // Rows past the valid range are real plane rows (Y <= 64), only masked.
        const int Y = lc * K + j;
        const uint32_t my = (Y >= Ylo && Y <= Yhi) ? 0u : ~0u;
        uint64_t acc = 0;
#pragma unroll
        for (int sy = 0; sy < 4; sy++) {
          uint32_t lo, hi;
          row(j + 4 * sy, lo, hi);
          acc = __builtin_amdgcn_qsad_pk_u16_u8(((uint64_t)hi << 32) | lo, qc[sy], acc);
        }
        clo = pk_min(clo, pk_key((uint32_t)acc, (uint32_t)j) | mlo | my);
        chi = pk_min(chi, pk_key((uint32_t)(acc >> 32), (uint32_t)j) | mhi | my);
      }
#pragma unroll
      for (int t = 0; t < 4; t++) {
        const uint32_t e = ((t < 2 ? clo : chi) >> (16 * (t & 1))) & 0xFFFFu;
        if (e != 0xFFFFu)
          atomicMin(&minlb[(lc * TB + b) * G + 4 * m + t], ((e >> 4) << 7) | ((e & 15u) << 3) | (uint32_t)k);
      }
    };
    if (planes) {
      // R holds the chunk's 25 rows.  The next chunk's 13 new rows are issued
      // in front of this chunk's qsads and waited for behind them.
      const __amdgpu_buffer_rsrc_t rs = flow_plane_rsrc(jb, it.j);
      const int pp = jb.plane_pitch, rel = it.prow0 - jb.ref_row0[it.j];
      if constexpr (CHAIN && FLOW_STREAM) {
        // Step 2 streamed: the -DME_FLOW_STREAM A/B build (Makefile `stream`;
        // DESIGN.md, the item-chain paragraph), not the product.  A plane row is
        // used by its four qsads as it lands and its registers take the row two
        // 13-row groups ahead.  Row r adds qsad(row r, qc[sy]) to candidate row
        // dy = r - 4 sy: a ring of 13 packed accumulators, dy complete at row
        // dy + 12 and merged like a chunk's row j = dy mod 13 (same keys, same
        // entries).  The fold column is loaded behind the groups.
        uint32_t alo[K], ahi[K], nlo[K], nhi[K];
#pragma unroll
        for (int r = 0; r < K; r++) {
          alo[r] = R.lo[r];
          ahi[r] = R.hi[r];
        }
#pragma unroll
        for (int r = 0; r < 12; r++) {
          nlo[r] = R.lo[K + r];
          nhi[r] = R.hi[K + r];
        }
        {
          uint32_t t1[1], t2[1];
          flow_plane_rows_load<1, true>(rs, pp, rel, it.X0, lc0 * K + 25, k, 4 * b + 4 * m, t1, t2);
          nlo[12] = t1[0];
          nhi[12] = t2[0];
        }
        uint64_t acc[K];
#pragma unroll
        for (int r = 0; r < K; r++) acc[r] = 0;
        uint32_t clo = ~0u, chi = ~0u;
        // one group: rows c K .. c K + 12 from (xlo, xhi), refilled with group c + 2's
        auto group = [&](int c, uint32_t (&xlo)[K], uint32_t (&xhi)[K]) {
          uint32_t lv = flow_plane_lane_byte(pp, k, 4 * b + 4 * m);
          // (past the last group: an offset no descriptor holds, the loads return 0)
          uint32_t sr = c + 2 <= lc1 ? flow_plane_row_byte(pp, rel, it.X0, (c + 2) * K) : 0x80000000u;
          asm volatile("" : "+s"(sr));
          asm volatile("" : "+v"(lv));
#pragma unroll
          for (int j = 0; j < K; j++) {
            const uint64_t row = ((uint64_t)xhi[j] << 32) | xlo[j];
            acc[j] = __builtin_amdgcn_qsad_pk_u16_u8(row, qc[0], 0);
            acc[(j + K - 4) % K] = __builtin_amdgcn_qsad_pk_u16_u8(row, qc[1], acc[(j + K - 4) % K]);
            acc[(j + K - 8) % K] = __builtin_amdgcn_qsad_pk_u16_u8(row, qc[2], acc[(j + K - 8) % K]);
            acc[(j + K - 12) % K] = __builtin_amdgcn_qsad_pk_u16_u8(row, qc[3], acc[(j + K - 12) % K]);
            {
              const flow_u2 v = __builtin_bit_cast(
                  flow_u2, __builtin_amdgcn_raw_buffer_load_b64(rs, (int)(lv + sr + (uint32_t)(4 * j * pp)), 0, 0));
              xlo[j] = v.x;
              xhi[j] = v.y;
            }
            // complete: dy = c K + j - 12, row idx of chunk cc
            const int cc = j == 12 ? c : c - 1, idx = j == 12 ? 0 : j + 1;
            const int Y = c * K + j - 12;
            const uint32_t my = (Y >= Ylo && Y <= Yhi) ? 0u : ~0u;
            const uint64_t a = acc[(j + K - 12) % K];
            clo = pk_min(clo, pk_key((uint32_t)a, (uint32_t)idx) | mlo | my);
            chi = pk_min(chi, pk_key((uint32_t)(a >> 32), (uint32_t)idx) | mhi | my);
            if (j == 11) {  // chunk c - 1 is complete
#pragma unroll
              for (int t = 0; t < 4; t++) {
                const uint32_t e = ((t < 2 ? clo : chi) >> (16 * (t & 1))) & 0xFFFFu;
                if (e != 0xFFFFu)
                  atomicMin(&minlb[(cc * TB + b) * G + 4 * m + t], ((e >> 4) << 7) | ((e & 15u) << 3) | (uint32_t)k);
              }
              clo = chi = ~0u;
            }
          }
        };
        // groups lc0 .. lc1: the last one completes chunk lc1 - 1 (its row 12
        // starts a chunk past the valid ones: masked)
#pragma unroll 1
        for (int c = lc0; c <= lc1; c += 2) {
          group(c, alo, ahi);
          if (c + 1 <= lc1) group(c + 1, nlo, nhi);
        }
        ME_BSTAMP(1);
#ifdef ME_STAMPS
        if (bs) bs[2] += (unsigned long long)(lc1 - lc0);
#endif
        flow_plane_fold_load(rs, pp, rel, it.X0, lane, R);
        if (S <= dxmax) {
#pragma unroll
          for (int rr = 0; rr < 5; rr++) {
            const int Y = (lane & 15) + 16 * rr;
            if (Y <= 2 * S && Y >= Ylo && Y <= Yhi) {
              uint32_t lb = 0;
#pragma unroll
              for (int sy = 0; sy < 4; sy++) lb = __builtin_amdgcn_sad_u8(R.f[4 * rr + sy], qc[sy], lb);
              const int lc = Y / K, j = Y - lc * K;
              atomicMin(&minlb[(lc * TB + b) * G + j], (lb << 7) | ((uint32_t)j << 3) | 4u);
            }
          }
        }
      } else {
      // (the chain kernel runs its last chunk apart from the loop, below)
#pragma unroll 1
      for (int lc = lc0; lc + (CHAIN ? 1 : 0) < lc1; lc++) {
        uint32_t nlo[K], nhi[K];
        if (CHAIN || lc + 1 < lc1) {
          flow_plane_rows_load<K, CHAIN>(rs, pp, rel, it.X0, (lc + 1) * K + 12, k, 4 * b + 4 * m, nlo, nhi);
        } else {
#pragma unroll
          for (int r = 0; r < K; r++) nlo[r] = nhi[r] = 0;
        }
        chunk(lc, [&](int r, uint32_t& lo, uint32_t& hi) {
          lo = R.lo[r];
          hi = R.hi[r];
        });
#pragma unroll
        for (int r = 0; r < 12; r++) {
          R.lo[r] = R.lo[K + r];
          R.hi[r] = R.hi[K + r];
        }
#pragma unroll
        for (int r = 0; r < K; r++) {
          R.lo[12 + r] = nlo[r];
          R.hi[12 + r] = nhi[r];
        }
      }
      // The chain kernel's last chunk has no rows to fetch ahead: the fold
      // column's 20 loads go out in their place, under its qsads.  (Issued
      // behind the chunks they cost a global load's latency of their own;
      // issued in front of them their registers, live across every chunk, spilled.)
      if constexpr (!CHAIN) ME_BSTAMP(1);
      flow_plane_fold_load(rs, pp, rel, it.X0, lane, R);
      if constexpr (CHAIN) {
        if (lc1 > lc0)
          chunk(lc1 - 1, [&](int r, uint32_t& lo, uint32_t& hi) {
            lo = R.lo[r];
            hi = R.hi[r];
          });
        ME_BSTAMP(1);
      }
#ifdef ME_STAMPS
      if (bs) bs[2] += (unsigned long long)(lc1 - lc0);
#endif
      // the fold column dx = +S (phase 0, byte 4b + 16 ..): lane = (block, dy mod 16)
      if (S <= dxmax) {
#pragma unroll
        for (int rr = 0; rr < 5; rr++) {
          const int Y = (lane & 15) + 16 * rr;
          if (Y <= 2 * S && Y >= Ylo && Y <= Yhi) {
            uint32_t lb = 0;
#pragma unroll
            for (int sy = 0; sy < 4; sy++) lb = __builtin_amdgcn_sad_u8(R.f[4 * rr + sy], qc[sy], lb);
            const int lc = Y / K, j = Y - lc * K;
            atomicMin(&minlb[(lc * TB + b) * G + j], (lb << 7) | ((uint32_t)j << 3) | 4u);
          }
        }
      }
      }
    } else {
    const uint8_t* pl = pr + k * FLOW_PRUNE_PLANE + 4 * b + 4 * m;
#pragma unroll 1
    for (int lc = lc0; lc < lc1; lc++)
      chunk(lc, [&](int r, uint32_t& lo, uint32_t& hi) {
        const uint32_t* rp = reinterpret_cast<const uint32_t*>(pl + (lc * K + r) * 32);
        lo = rp[0];
        hi = rp[1];
      });
    // the fold column dx = +S (plane 0, index 4b + 16 ..): lane = (block, dy mod 16)
    if (S <= dxmax) {
#pragma unroll 1
      for (int rr = 0; rr < 5; rr++) {
        const int Y = (lane & 15) + 16 * rr;
        if (Y <= 2 * S && Y >= Ylo && Y <= Yhi) {
          uint32_t lb = 0;
#pragma unroll
          for (int sy = 0; sy < 4; sy++)
            lb = __builtin_amdgcn_sad_u8(*reinterpret_cast<const uint32_t*>(pr + (Y + 4 * sy) * 32 + 4 * b + 16),
                                         qc[sy], lb);
          const int lc = Y / K, j = Y - lc * K;
          atomicMin(&minlb[(lc * TB + b) * G + j], (lb << 7) | ((uint32_t)j << 3) | 4u);
        }
      }
    }
    }
  }
  lds_fence();
  ME_BSTAMP(3);
  if constexpr (PRE) return;

  // 3. seeds: lane = (block, block row); e = the block's smallest entry with
  // its chunk and group appended.  The first read of the staged window: in the
  // chain kernel (a launch with planes: no step 1) its DMA may still have been
  // in flight under step 2 (flow_fill).
  if constexpr (CHAIN) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  ME_BSTAMP(7);
  {
    uint32_t e = ~0u;
    for (int lc = lc0; lc < lc1; lc++) {
      const uint32_t v = minlb[(lc * TB + b) * G + (lane & 15)];
      if (v != ~0u) e = min(e, (v << 7) | ((uint32_t)lc << 4) | (uint32_t)(lane & 15));
    }
    e = min(e, swz_xor<8>(e));
    e = min(e, swz_xor<4>(e));
    e = min(e, swz_xor<2>(e));
    e = min(e, swz_xor<1>(e));
#pragma unroll 1
    for (int sd = 0; sd < 2; sd++) {
      bool ok = b < it.nb;
      int Y = S, X = S;
      asm volatile("" : "+v"(Y), "+v"(X));  // no constant key words kept live in VGPRs
      if (sd == 1) {
        ok = ok && e != ~0u;
        const uint32_t ent = e >> 7;
        const int kk = (int)(ent & 7u);
        if (ok) {
          Y = K * (int)((e >> 4) & 7u) + (int)((ent >> 3) & 15u);
          X = kk == 4 ? 2 * S : 4 * (int)(e & 15u) + kk;
        }
      }
      const int y = lane & 15;
      const int off = (Y + y) * P + b * B + X;
      const uint32_t* w = reinterpret_cast<const uint32_t*>(buf + (off & ~3));
      const uint32_t* c = cur + (b * B + y) * 4;
      uint32_t sad = 0;
#pragma unroll
      for (int i = 0; i < 4; i++)
        sad = __builtin_amdgcn_sad_u8(__builtin_amdgcn_alignbyte(w[i + 1], w[i], off & 3), c[i], sad);
      sad += swz_xor<8>(sad);
      sad += swz_xor<4>(sad);
      sad += swz_xor<2>(sad);
      sad += swz_xor<1>(sad);
      if (ok && y == 0)
        atomicMin(reinterpret_cast<unsigned long long*>(&keys[b]),
                  (unsigned long long)make_key(sad, X - S, Y - S));
    }
  }
  lds_fence();
  ME_BSTAMP(4);

  // 4. the live list (the planes are dead: the list overlays them)
  int L = 0;
  const uint32_t magic_nb = 0xFFFFFFFFu / (uint32_t)it.nb + 1u;
  for (int r = 0; r < nw; r++) {
    const int idx = 64 * r + lane;
    const bool valid = idx < valid_lanes;
    const int ii = valid ? idx : 0;
    const int bg = ii >> 4, gi = ii & 15;
    const int lcr = it.nb == 1 ? bg : (int)__umulhi((uint32_t)bg, magic_nb);
    const int b2 = bg - lcr * it.nb;
    const uint32_t v = minlb[((lc0 + lcr) * TB + b2) * G + gi];
    const int U = (int)(uint32_t)(keys[b2] >> 32);
    const bool live = valid && v != ~0u && 16 * (int)(v >> 7) - 240 <= U;
    if (verify) {
      if (valid) {
        list[idx] = (uint16_t)idx;
        dead[idx] = live ? 0 : 1;
      }
      if (r == 0 && lane < TB) ub[lane] = (uint32_t)(keys[lane] >> 32);
    }
    const uint64_t bal = __builtin_amdgcn_ballot_w64(live);
    const int rank = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32),
                                                    __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
    if (live && !verify) list[L + rank] = (uint16_t)idx;
    L += (int)__builtin_popcountll(bal);
  }
  if (lane == 0) {
    ctl->live[slot] = (uint32_t)(verify ? valid_lanes : L);
    // (bound phases of several slots run at once: an add, not a store of run + 1)
    if (pf & PF_BYPASS) {
      if (4 * L > 3 * valid_lanes) {
        if (!prober) __hip_atomic_fetch_add(&ctl->run, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      } else
        __hip_atomic_store(&ctl->run, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    if (stats) {
      atomicAdd(&ctl->stats[0], (uint32_t)L);
      atomicAdd(&ctl->stats[1], (uint32_t)valid_lanes);
      atomicAdd(&ctl->stats[3], 1u);
    }
  }
  ME_BSTAMP(5);
#ifdef ME_STAMPS
  if (bs) bs[6]++;
#endif
}

// ------------------------------------------------ flow: the row-split wave-task
// Task t of a pruned h = B item whose list has n <= 32 entries left for it
// (almost every executed task of correlated content: 9 live lane-tasks of 320
// per item on the bench input) would issue all 64 lanes' 13 dy rows for n live
// ones.  Split by rows instead (me_geom.h flow_split_*): an instance per rows a
// lane takes, R = 1, 2, 3, 4 or 7, with P = ceil(13 / R) lanes per entry; lane l
// = entry l / P, part l % P, rows [j0, j0 + R) of the entry's chunk: an (R + 15)-row
// window walk of 64 R qsads instead of 28 rows and 832.  The parts' keys meet in
// the block's keys word like those of different lane-tasks; rows two parts
// share give the same key twice.  The fold column's candidate runs
// in part 0 (j0 = 0: its row index is the chunk's).  A lane past the entries
// repeats the last one (so it raises no edge mask of its own) and merges nothing.
// The whole body, list read to key merge, lives here: nothing of it is live
// across the unsplit task's K = 13 row loop.
template <int B, int K, int PC, int KP, typename Hook>
__device__ __forceinline__ void flow_split_task(const SearchArgs& p, const QsadGeom& g, const Item& it,
                                                const uint8_t* smem, const uint8_t* buf, uint32_t tile_off,
                                                uint64_t* keys, int t, int n, int lc0c, int pfl,
                                                Hook lag_check) {
  constexpr int CW = B / 4;
  static_assert(K == FLOW_SPLIT_K && CW == 4 && KP < K && flow_split_instance(KP), "the split's row rules");
  const int S = p.range, G = g.groups;
  const int lane = fresh_tid() & 63;
  const FlowSplitLane sl = flow_split_lane(KP, lane, n);
  const int j0 = sl.row0;  // (0 in part 0 alone: the fold candidate's lane)
  const bool live = sl.live;
  const uint8_t* pv = buf + g.tile_bytes + g.tb * B * B;
  const int i = (int)reinterpret_cast<const uint16_t*>(pv)[64 * t + sl.entry];
  const int bg = (int)__umulhi((uint32_t)i, g.magic_groups);  // i / G
  const int gi = i - bg * G;
  const uint32_t magic_nb = 0xFFFFFFFFu / (uint32_t)it.nb + 1u;
  const int lcr = it.nb == 1 ? bg : (int)__umulhi((uint32_t)bg, magic_nb);
  const int b = bg - lcr * it.nb;
  const int lc = lc0c + lcr;
  const int d0 = lc * K + j0;  // dy + S of the lane's first row
  const int tlx = (it.bx0 + b) * B;
  const uint32_t* cur_lds = reinterpret_cast<const uint32_t*>(buf + g.tile_bytes);
  uint32_t c[B][CW];
#pragma unroll
  for (int y = 0; y < B; y++) {
    const uint4 v = reinterpret_cast<const uint4*>(cur_lds)[b * B + y];
    c[y][0] = v.x; c[y][1] = v.y; c[y][2] = v.z; c[y][3] = v.w;
  }
  const int dymin = max(-S, -it.tly), dymax = min(S, p.height - it.h - it.tly);
  const int dxmin = max(-S, -tlx), dxmax = min(S, p.width - B - tlx);
  const int jlo = dymin + S - d0, jhi = dymax + S - d0;  // in the lane's rows
  const bool full_rows = dymin + S <= 0 && dymax + S >= it.nch * K - 1;
  const int w0 = (b * B) / 4 + gi;
  uint64_t acc[KP];
  const int jt = gi < K ? gi : K - 1;  // the fold candidate's row of the chunk
  const uint32_t toff = tile_off + (uint32_t)((lc * K + jt) * g.pitch + b * B + 2 * S);
  uint32_t tsad = 0;
  qsad_lane<B, KP, B, PC, 4>(smem, g.pitch, tile_off, d0, w0, c, acc, lag_check);
  if (g.fold) tsad = tail_sad<B, B>(smem, g.pitch, toff, c);
  const int dxg = 4 * gi - S - it.a;
  const bool edge = dxg < dxmin || dxg + 3 > dxmax;
  uint32_t best;
  if (full_rows && __builtin_amdgcn_ballot_w64(edge) == 0) {
    best = lane_best<KP, false>(acc, 0u, 0u, jlo, jhi);
  } else {
    uint32_t mlo = 0, mhi = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int dx = dxg + k;
      const uint32_t msk = (dx < dxmin || dx > dxmax) ? 0xFFFFu : 0u;
      if (k < 2) mlo |= msk << (16 * k);
      else mhi |= msk << (16 * (k - 2));
    }
    best = lane_best<KP, true>(acc, mlo, mhi, jlo, jhi);
  }
  if (g.fold) {
    const bool tv = j0 == 0 && gi < K && jt >= jlo && jt <= jhi && S <= dxmax;
    best = min(best, tv ? (tsad << 16) | (uint32_t)(5 * jt + 4) : ~0u);
  }
  if (live && best < 0xFFFF0000u) {
    const int idx = (int)(best & 0xFFFFu), jj = idx / 5, k5 = idx - 5 * jj;
    const int dy = d0 + jj - S, dx = k5 == 4 ? S : 4 * gi + k5 - S - it.a;
    atomicMin(reinterpret_cast<unsigned long long*>(&keys[b]),
              (unsigned long long)make_key(best >> 16, dx, dy));
    // Verify mode (see the unsplit task): per lane, by the entry's index.
    if ((pfl & PF_VERIFY) && pv[FLOW_PRUNE_DEAD + i] && (best >> 16) <= reinterpret_cast<const uint32_t*>(pv + FLOW_PRUNE_UB)[b] &&
        p.sched)
      __hip_atomic_store(p.sched + SCHED_ERR, 2u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// ------------------------------------------------------- flow: filling a slot
// One wave stages item `it` into the slot at buf and, in a pruning launch
// (pfl != 0), runs its bound; the caller publishes the slot.  In a launch with
// box-sum planes the bound needs the cur blocks and its plane registers at
// once but the window only in its step 3, so those are issued FIRST and the
// window's DMA last: VMEM loads return in order, and vmcnt(FLOW_WIN_STEPS)
// behind exactly that many window instructions waits for all that was issued
// in front of them and for none of them.  The window lands under the bound's
// steps 1 and 2; flow_bound waits for it in front of step 3, and the
// vmcnt(0) behind the bound covers the paths that return before step 3 (an
// h = B/2 item, the bypass state).  Any other launch, and one whose windows
// (rows_alloc rows, every item's) are not FLOW_WIN_STEPS instructions long,
// waits for everything as before (PF_EARLY is set at the kernel's start).
constexpr int FLOW_WIN_STEPS = 12;
static_assert((5 * 13 + 16 - 1) * 144 > (FLOW_WIN_STEPS - 1) * 1024 && (5 * 13 + 16 - 1) * 144 <= FLOW_WIN_STEPS * 1024,
              "80 rows x 144 bytes in 1,024-byte DMA steps");
//
// The pre-bound (PF_PRE).  Init, step 2 and the fold column of the bound, a
// third of a slot's item-to-item chain, read only the item's cur bytes, its
// plane rows and its geometry, and write only minlb and qcur, which are dead
// in the slot once the item in front has its list.  So the wave that publishes
// item kn runs them for item kn + NB behind the publish (flow_prebound), while
// kn's tasks wait for waves and execute, and the slot's marker word tells the
// wave that later fills the slot with kn + NB what it finds:
//   writer, about to publish kn:  marker = BUSY(kn + NB) if it will pre-bound
//     (PF_PRE, kn + NB < nitems, an h = B item, not the bypass state), else
//     NONE; the ready store (release); the pre-bound; marker = DONE(kn + NB)
//     (release).
//   reader, having run kn's last task (so it acquired kn's ready word and sees
//     the marker of this turn: NONE, BUSY or DONE of kn + NB, never an older
//     one): on BUSY / DONE of its item it issues no plane fetch, evaluates the
//     bypass state as ever, waits for DONE (flow_bound) and runs steps 3 and 4;
//     on anything else it runs the whole bound, the code it always ran.
// No deadlock: between BUSY and DONE the writer executes straight-line code
// whose only waits are for its own loads and LDS operations (vmcnt, lgkmcnt),
// so DONE follows BUSY whatever the other waves do; the reader can see BUSY
// only after kn's publish, which the writer has behind it; NONE and DONE are
// final for the turn.  The reader's wait is bounded like the ready wait.  The
// first NB items have no writer: their slots' marker bytes are whatever the LDS
// held, and kitem < NB reads none of them.
// Exactness: minlb is a function of the cur bytes, the plane bytes and the
// geometry alone, so the list is the one the whole bound builds.
template <int B>
__device__ __forceinline__ uint32_t* flow_mark_of(const QsadGeom& g, uint8_t* buf) {
  return reinterpret_cast<uint32_t*>(buf + g.tile_bytes + g.tb * B * B + FLOW_SLIM_MARK);
}
template <int B, int K>
__device__ __forceinline__ void flow_prebound(const SearchArgs& p, const QsadGeom& g, const Item& it, uint8_t* buf,
                                              uint64_t* keys, FlowCtl* ctl, int slot, const FlowJobs& jb) {
  FlowPlaneRegs R;
  flow_bound<B, K, true, true>(p, g, it, buf, keys, ctl, slot, jb, R, false);
}
// kitem: the item's index in the workgroup's walk; *expired: the wait for the
// item's pre-bound ran out (the error word is set: the caller leaves the task loop).
template <int B, int K>
__device__ __forceinline__ void flow_fill(const SearchArgs& p, const QsadGeom& g, const Item& it, uint8_t* buf,
                                          uint64_t* keys, FlowCtl* ctl, int slot, const FlowJobs& jb, int pfl,
                                          bool boost, int kitem, int nb_slots, bool* expired,
                                          unsigned long long* st_landed, unsigned long long* bs = nullptr) {
  FlowPlaneRegs R;
  const uint32_t* mark = nullptr;
  if ((pfl & PF_PRE) && kitem >= nb_slots) {
    const uint32_t* mk = flow_mark_of<B>(g, buf);
    const uint32_t v = (uint32_t)__builtin_amdgcn_readfirstlane(
        (int)__hip_atomic_load(mk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP));
    if ((v >> 1) == (uint32_t)kitem + 1u) mark = mk;
  }
  const bool pl = pfl && !mark && flow_plane_wanted<B>(it, ctl);
  stage_item_part<B, FLOW_STAGE_CUR>(p, g, it, buf, jb);
  // (the bound's first plane rows: issued here, landed by the same wait)
  if (pl) flow_plane_fetch<B, K, true>(it, jb, R);
  else flow_plane_zero(R);
  if (pfl & PF_EARLY) {
    stage_item_part<B, FLOW_STAGE_WIN, FLOW_WIN_STEPS>(p, g, it, buf, jb);
    if (g.prio) __builtin_amdgcn_s_setprio(0);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(FLOW_WIN_STEPS) : "memory");
  } else {
    stage_item_part<B, FLOW_STAGE_WIN>(p, g, it, buf, jb);
    if (g.prio) __builtin_amdgcn_s_setprio(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  }
#ifdef ME_STAMPS
  if (st_landed) *st_landed = __builtin_amdgcn_s_memtime();
#endif
  if (pfl) {
    // (a refill at raised issue priority: nothing of the item runs before its bound ends)
    if (boost) __builtin_amdgcn_s_setprio(3);
    // (kitem to the bound: -1 where the slot's marker is not this launch's, the first ring turn or no PF_PRE)
    flow_bound<B, K, true>(p, g, it, buf, keys, ctl, slot, jb, R, pl, bs, mark,
                           (pfl & PF_PRE) && kitem >= nb_slots ? kitem : -1, expired);
    if (boost) __builtin_amdgcn_s_setprio(0);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

#define ME_FLOW_CHAIN 0
#include "me_flow_kernel.inc"
#undef ME_FLOW_CHAIN
#define ME_FLOW_CHAIN 1
#include "me_flow_kernel.inc"
#undef ME_FLOW_CHAIN

// ------------------------------------------------- flow: the box-sum prepass
// q = (4x4 box sum) >> 4 of every job's resident reference rows, once per
// launch, as the x-phase planes of me_geom.h (flow_plane_pitch): the flow
// kernel's bound phase would otherwise form the same sums in every tile whose
// window holds the pixel, about ten times per frame.  Memory bound: a thread
// owns 16 consecutive x (one dword of each phase row: a wave stores 256
// contiguous bytes per phase) and PLANES_RPT rows, reading each of its
// PLANES_RPT + 3 input rows once as one 16-byte and one 4-byte load and
// keeping the last three rows' packed horizontal 4-sums (four v_qsad_pk_u16_u8
// per row and v_perm_b32 to sort the bytes by phase: 16.8 us per 16 1080p
// frames, 66 MB moved; with v_alignbyte + v_sad_u8 per x it took 21.2 us).
constexpr int PLANES_RPT = 8;
__global__ __launch_bounds__(256) void me_box_planes_kernel(FlowJobs jb, int width, int stride) {
  const int j = (int)blockIdx.z;
  const int pitch = jb.plane_pitch, rows = jb.plane_rows[j];
  const int t = (int)(blockIdx.x * 64 + threadIdx.x);  // dword of a phase row
  const int y0 = (int)(blockIdx.y * 4 + threadIdx.y) * PLANES_RPT;
  if (4 * t >= pitch || y0 >= rows) return;
  const int xb = 16 * t - 32;  // the thread's first x
  const bool inx = xb >= 0 && xb < width;  // (W % 16 == 0: all 16 inside or none)
  const uint8_t* src = jb.ref[j] + xb;
  uint8_t* dst = jb.planes + ((size_t)jb.plane_off64[j] << 6) + 4 * t;
  // Bytes of the thread's phase dwords that hold a valid x (<= W - 4): all of
  // them, but for the frame's last 16 columns (x = W - 3 .. W - 1 are out).
  uint32_t keep[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    keep[k] = 0;
#pragma unroll
    for (int i = 0; i < 4; i++)
      if (inx && xb + 4 * i + k <= width - 4) keep[k] |= 0xFFu << (8 * i);
  }
  // h[g]: the row's four horizontal 4-sums at x = 4 g .. 4 g + 3 as packed u16
  // (one v_qsad_pk_u16_u8 against zero), lo = x, x + 1; hi = x + 2, x + 3.
  uint32_t h1l[4], h1h[4], h2l[4], h2h[4], h3l[4], h3h[4];
#pragma unroll
  for (int g = 0; g < 4; g++) h1l[g] = h1h[g] = h2l[g] = h2h[g] = h3l[g] = h3h[g] = 0;
#pragma unroll
  for (int r = 0; r < PLANES_RPT + 3; r++) {
    const int y = y0 + r;
    uint32_t w[5] = {0, 0, 0, 0, 0};
    if (inx && y < rows) {
      const uint4 v = *reinterpret_cast<const uint4*>(src + (size_t)y * stride);
      w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
      if (xb + 16 < width) w[4] = *reinterpret_cast<const uint32_t*>(src + (size_t)y * stride + 16);
    }
    uint32_t h0l[4], h0h[4];
#pragma unroll
    for (int g = 0; g < 4; g++) {
      const uint64_t h = __builtin_amdgcn_qsad_pk_u16_u8(((uint64_t)w[g + 1] << 32) | w[g], 0u, 0ull);
      h0l[g] = (uint32_t)h;
      h0h[g] = (uint32_t)(h >> 32);
    }
    if (r >= 3) {
      const int yo = y - 3;  // the box's top row; its bottom row y is resident or q is 0
      if (yo < rows) {
        // q pairs: four row sums <= 1020 each, no carry between the u16 halves
        uint32_t ql[4], qh[4];
#pragma unroll
        for (int g = 0; g < 4; g++) {
          ql[g] = ((h0l[g] + h1l[g] + h2l[g] + h3l[g]) >> 4) & 0x00FF00FFu;  // q(4g) | q(4g + 1) << 16
          qh[g] = ((h0h[g] + h1h[g] + h2h[g] + h3h[g]) >> 4) & 0x00FF00FFu;  // q(4g + 2) | q(4g + 3) << 16
        }
        // phase k's dword = q(k), q(4 + k), q(8 + k), q(12 + k): byte 0 (k even)
        // or 2 (k odd) of the four groups' pairs (v_perm_b32: selector bytes 0-3
        // take the second operand's bytes, 4-7 the first's)
        const uint32_t l01 = __builtin_amdgcn_perm(ql[1], ql[0], 0x06020400u);
        const uint32_t l23 = __builtin_amdgcn_perm(ql[3], ql[2], 0x06020400u);
        const uint32_t u01 = __builtin_amdgcn_perm(qh[1], qh[0], 0x06020400u);
        const uint32_t u23 = __builtin_amdgcn_perm(qh[3], qh[2], 0x06020400u);
        uint32_t o[4];
        o[0] = __builtin_amdgcn_perm(l23, l01, 0x05040100u);
        o[1] = __builtin_amdgcn_perm(l23, l01, 0x07060302u);
        o[2] = __builtin_amdgcn_perm(u23, u01, 0x05040100u);
        o[3] = __builtin_amdgcn_perm(u23, u01, 0x07060302u);
#pragma unroll
        for (int k = 0; k < 4; k++)
          *reinterpret_cast<uint32_t*>(dst + ((size_t)yo * 4 + k) * pitch) = y < rows ? o[k] & keep[k] : 0u;
      }
    }
#pragma unroll
    for (int g = 0; g < 4; g++) {
      h3l[g] = h2l[g]; h3h[g] = h2h[g];
      h2l[g] = h1l[g]; h2h[g] = h1h[g];
      h1l[g] = h0l[g]; h1h[g] = h0h[g];
    }
  }
}

// ------------------------------------------------------------------ launch
static int generic_lds_bytes(const SearchArgs& p, int* win_bytes) {
  const int B = p.blk;
  long win = (long)(B + 2 * p.range) * (B + 2 * p.range);
  const int cur = (B * B + 15) & ~15;
  if (cur + win > GENERIC_LDS_BUDGET) win = 0;  // read the window from global memory
  *win_bytes = (int)win;
  return cur + (int)win;
}

hipError_t launch_generic(const SearchArgs& p, int bx0, int nbx_range, int row0, int nrows,
                          hipStream_t stream) {
  if (nbx_range <= 0 || nrows <= 0) return hipSuccess;
  int win = 0;
  const int lds = generic_lds_bytes(p, &win);
  dim3 grid((unsigned)(nbx_range * nrows)), block(GENERIC_THREADS);
  if (p.cost_kind == COST_SAD)
    hipLaunchKernelGGL(me_generic_kernel<COST_SAD>, grid, block, lds, stream, p, bx0, nbx_range,
                       row0, win);
  else
    hipLaunchKernelGGL(me_generic_kernel<COST_SSD>, grid, block, lds, stream, p, bx0, nbx_range,
                       row0, win);
  return hipGetLastError();
}

// Per-kernel launch facts, computed once per (kernel, device[, shape]) and
// shared by every host thread (a mutex-protected list: the per-device threads
// of multi_search and me_search_pairs plan and launch concurrently).  Setting
// the dynamic-LDS attribute and querying occupancy on every launch cost host
// time on the small-stripe step, which is host-bound.
namespace {
struct LaunchFact {
  const void* fn;
  int dev, threads, lds, value;  // threads == 0: the LDS attribute entry (value = max set)
};
std::mutex g_fact_mu;
std::vector<LaunchFact> g_facts;

int current_device() {
  int dev = 0;
  (void)hipGetDevice(&dev);
  return dev;
}
}  // namespace

hipError_t lds_attr(const void* fn, int lds) {
  if (lds <= 64 * 1024) return hipSuccess;
  const int dev = current_device();
  std::lock_guard<std::mutex> lk(g_fact_mu);
  for (LaunchFact& f : g_facts)
    if (f.fn == fn && f.dev == dev && f.threads == 0) {
      if (f.value >= lds) return hipSuccess;
      const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
      if (e == hipSuccess) f.value = lds;
      return e;
    }
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
  if (e == hipSuccess) g_facts.push_back({fn, dev, 0, 0, lds});
  return e;
}

// Resident workgroups per CU for this kernel / block / LDS.
static int resident_wgs(const void* fn, int threads, int lds) {
  const int dev = current_device();
  {
    std::lock_guard<std::mutex> lk(g_fact_mu);
    for (const LaunchFact& f : g_facts)
      if (f.fn == fn && f.dev == dev && f.threads == threads && f.lds == lds) return f.value;
  }
  int n = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, threads, lds) != hipSuccess || n < 1)
    n = 1;
  std::lock_guard<std::mutex> lk(g_fact_mu);
  g_facts.push_back({fn, dev, threads, lds, n});
  return n;
}

// CUs of the device (every device of a context is the same part): a C++11
// function-local static, initialised once and thread-safely (multi_search and
// me_search_pairs call the planners from one host thread per device).
int cu_count() {
  static const int cus = []() {
    int dev = 0, n = 0;
    (void)hipGetDevice(&dev);
    if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n < 1)
      n = 256;
    return n;
  }();
  return cus;
}

// One item-kernel launch over the job table jb (full-height rows and h = B/2
// bottom rows; every job the geometry g was planned for).
static hipError_t launch_fast(const SearchArgs& p, const QsadGeom& g, int K, const FlowJobs& jb,
                              hipStream_t stream) {
  const int ntiles = jb.tile_pre[jb.n];
  if (ntiles <= 0) return hipSuccess;
  dim3 block((unsigned)g.threads);
// PP > 0: the instance with that compile-time tile pitch (row addresses in the
// ds_read2 offset fields), taken when the plan has exactly that pitch.
#define ME_FAST_CASE_P(CC, BB, KK, PP)                                                     \
  if (p.cost_kind == CC && p.blk == BB && K == KK && (PP == 0 || g.pitch == PP)) {         \
    const void* fn = (const void*)me_fast_kernel<CC, BB, KK, PP>;                         \
    const hipError_t e_ = lds_attr(fn, g.lds);                                             \
    if (e_ != hipSuccess) return e_;                                                       \
    int res = resident_wgs(fn, g.threads, g.lds);                                          \
    if (tuning().fast_res > 0 && tuning().fast_res < res) res = tuning().fast_res;         \
    const int nwg = ntiles < res * cu_count() ? ntiles : res * cu_count();                 \
    hipLaunchKernelGGL((me_fast_kernel<CC, BB, KK, PP>), dim3((unsigned)nwg), block, g.lds, stream, p, g, jb); \
    return hipGetLastError();                                                              \
  }
#define ME_FAST_CASE(CC, BB, KK) ME_FAST_CASE_P(CC, BB, KK, 0)
  // the plans' pitches of 4K +-64 (tb 8: 272; 1.098 -> 1.085 ms) and 8K 8x8
  // +-128 (tb 8: 336; 18.59 -> 18.19 ms); the 1080p stripes' pitches (144,
  // 112) measured no better (profiles/r02ah_ab_item_pitch.txt)
  ME_FAST_CASE_P(COST_SAD, 16, 13, 272) ME_FAST_CASE_P(COST_SAD, 8, 13, 336)
  ME_FAST_CASE(COST_SAD, 16, 13) ME_FAST_CASE(COST_SAD, 16, 11) ME_FAST_CASE(COST_SAD, 16, 8)
  ME_FAST_CASE(COST_SAD, 16, 5)
  ME_FAST_CASE(COST_SAD, 8, 13) ME_FAST_CASE(COST_SAD, 8, 11) ME_FAST_CASE(COST_SAD, 8, 8)
  ME_FAST_CASE_P(COST_SAD, 8, 26, 336) ME_FAST_CASE(COST_SAD, 8, 26)
  ME_FAST_CASE(COST_SSD, 16, 13) ME_FAST_CASE(COST_SSD, 16, 11) ME_FAST_CASE(COST_SSD, 16, 8)
  ME_FAST_CASE(COST_SSD, 8, 13) ME_FAST_CASE(COST_SSD, 8, 11) ME_FAST_CASE(COST_SSD, 8, 8)
#undef ME_FAST_CASE
#undef ME_FAST_CASE_P
  return hipErrorInvalidValue;
}

// The job table of jobs [0, n) (n <= MAX_JOBS; rows [r0, r1) each, already
// cut to what the kernel takes), wg_per_row tiles per block row.
static FlowJobs job_table(const SearchArgs& p, int wg_per_row, const SearchJob* jobs, int n) {
  FlowJobs jb;
  jb.n = 0;
  jb.tile_pre[0] = 0;
  jb.planes = nullptr;  // (launch_flow binds the box-sum planes)
  jb.plane_pitch = 0;
  for (int i = 0; i < n; i++) {
    const SearchJob& J = jobs[i];
    if (J.r1 <= J.r0) continue;
    const int j = jb.n++;
    jb.r0[j] = J.r0;
    jb.ref_row0[j] = J.ref_row0;
    jb.cur_row0[j] = J.cur_row0;
    const SearchArgs q = job_args(p, J);
    jb.ref_bytes[j] = q.ref_bytes;
    jb.cur_bytes[j] = q.cur_bytes;
    jb.ref[j] = J.ref;
    jb.cur[j] = J.cur;
    jb.mv[j] = J.mv;
    jb.cost[j] = J.cost;
    jb.plane_off64[j] = 0;
    jb.plane_rows[j] = flow_plane_rows(J, p.blk, p.range, p.height);
    jb.tile_pre[j + 1] = jb.tile_pre[j] + wg_per_row * (J.r1 - J.r0);
  }
  return jb;
}

// The item-table entries of the process's last flow launch with planes (-1:
// none yet); the tuning build's me_debug_flow_table reads it.
static std::atomic<int> g_last_flow_table{-1};
int last_flow_table() { return g_last_flow_table.load(std::memory_order_relaxed); }

// One flow-kernel launch over jobs [0, n) (full-height rows and h = B/2
// bottom rows only; n <= MAX_JOBS).
static hipError_t launch_flow(const SearchArgs& p, const QsadGeom& plan, const SearchJob* jobs, int n,
                              hipStream_t stream) {
  QsadGeom g = plan;
  FlowJobs jb = job_table(p, g.wg_per_row, jobs, n);
  const int ntiles = jb.tile_pre[jb.n];
  if (ntiles <= 0) return hipSuccess;
  int nwg = ntiles > cu_count() ? cu_count() : ntiles;  // one per CU, at most one per tile
  // (tuning build: fewer workgroups, so that a small launch gives each a long walk)
  if (tuning().flow_wgs > 0 && tuning().flow_wgs < nwg) nwg = tuning().flow_wgs;
  // The pruning launch's box-sum planes, in the scratch the context lent the
  // search when it holds every job's (attach_scratch sized it with
  // flow_planes_need; a captured search that met a smaller one runs without):
  // the prepass goes in front on the same stream.
  if (g.pitch == 144 && g.prune && g.slim_slots && p.scratch && flow_planes_on(tuning(), jb.n)) {
    size_t off = 0;
    int max_rows = 0;
    bool ok = true;
    for (int j = 0; j < jb.n; j++) {
      const size_t b = flow_plane_job_bytes(p.width, jb.plane_rows[j]);
      jb.plane_off64[j] = (uint32_t)(off >> 6);
      off += b;
      ok = ok && b > 0 && b < (1u << 31);
      if (jb.plane_rows[j] > max_rows) max_rows = jb.plane_rows[j];
    }
    if (ok && off <= p.scratch_bytes) {
      jb.planes = p.scratch;
      jb.plane_pitch = flow_plane_pitch(p.width);
      const dim3 grid((unsigned)((jb.plane_pitch / 4 + 63) / 64),
                      (unsigned)((max_rows + 4 * PLANES_RPT - 1) / (4 * PLANES_RPT)), (unsigned)jb.n);
      hipLaunchKernelGGL(me_box_planes_kernel, grid, dim3(64, 4), 0, stream, jb, p.width, p.stride);
      const hipError_t e = hipGetLastError();
      if (e != hipSuccess) return e;
    }
  }
  // The launch with planes keeps its workgroups' item tables behind the slim
  // layout where the longest of them fits what the ring leaves of the LDS.
  int table = 0, table_bytes = 0;
  if (jb.planes && tuning().flow_table != 0) {
    int max_by = 0;
    for (int i = 0; i < n; i++)
      if (jobs[i].r1 > jobs[i].r0 && jobs[i].r1 - 1 > max_by) max_by = jobs[i].r1 - 1;
    table = flow_table_entries(g, ntiles, nwg, max_by, FLOW_LDS_BUDGET - g.slim_lds, tuning().flow_table_cap);
    table_bytes = table * FLOW_ENTRY_BYTES;
  }
  if (jb.planes) g_last_flow_table.store(table, std::memory_order_relaxed);
  // Tuning build: the counting launch keeps its histogram of executed wave-tasks
  // (SCHED_SPLIT_HIST) in 64 words of LDS behind all that, where they fit, and
  // says so in prune_stats.
  int hist_bytes = 0;
  if (g.pitch == 144 && g.prune && g.prune_stats &&
      (jb.planes ? g.slim_lds + table_bytes : g.prune_lds) + FLOW_HIST_BYTES <= FLOW_LDS_BUDGET) {
    hist_bytes = FLOW_HIST_BYTES;
    g.prune_stats = 2;
  }
  // The pre-bound (flow_fill) and its issue priority: on in every launch with planes.
  const int pre = tuning().flow_pre != 0 ? 1 | (tuning().flow_pre_prio & 3) << 1 : 0;
  // 144: the pitch of the 4-block tiles 1080p +-32 gets (row addresses in
  // the ds_read2 offsets); any other pitch takes the runtime-pitch body
#define ME_FLOW_CASE(PP)                                                                        \
  if (PP == 0 || g.pitch == PP) {                                                               \
    const int lds = !(PP == 144 && g.prune) ? g.lds : (jb.planes ? g.slim_lds + table_bytes : g.prune_lds) + hist_bytes; \
    const void* fn = PP == 144 && g.prune && jb.planes ? (const void*)me_flow_chain_kernel<16, 13> \
                                                       : (const void*)me_flow_kernel<16, 13, PP>; \
    const hipError_t e = lds_attr(fn, lds);                                                     \
    if (e != hipSuccess) return e;                                                              \
    if (PP == 144 && g.prune && jb.planes)                                                      \
      hipLaunchKernelGGL((me_flow_chain_kernel<16, 13>), dim3((unsigned)nwg), dim3(1024), lds,  \
                         stream, p, g, jb, table, pre);                                         \
    else                                                                                        \
      hipLaunchKernelGGL((me_flow_kernel<16, 13, PP>), dim3((unsigned)nwg), dim3(1024), lds,    \
                         stream, p, g, jb);                                                     \
    return hipGetLastError();                                                                   \
  }
  ME_FLOW_CASE(144) ME_FLOW_CASE(0)
#undef ME_FLOW_CASE
  return hipErrorInvalidValue;
}

size_t flow_planes_need(const SearchArgs& base, const SearchJob* jobs, int n) {
  const PlanShape s{base.width, base.height, base.stride, base.blk, base.range, base.cost_kind, 0, 0};
  return flow_planes_scratch(s, cu_count(), tuning(), jobs, n);
}

size_t merge_tiles_needed(const SearchArgs& p) {
  if (p.block_row_end <= p.block_row_begin) return 0;
  return p.cost_kind == COST_SSD ? mfma_merge_tiles(p) : 0;
}

// One launch of the dispatcher's list (me_dispatch.h).
static hipError_t run_launch(const SearchArgs& base, const SearchJob* jobs, const Launch& l,
                             hipStream_t stream) {
  if (l.path) note_path(l.path);
  const SearchJob& J = jobs[l.job0];
  switch (l.kind) {
    case LAUNCH_GENERIC:
      return launch_generic(job_args(base, J), l.bx0, l.bx1 - l.bx0, launch_r0(l, J),
                            launch_r1(l, J) - launch_r0(l, J), stream);
    case LAUNCH_SSIM:
      return launch_ssim(job_args(base, J), stream);
    case LAUNCH_MFMA:
      return launch_mfma(base, &J, l.njobs, l.mg, l.scratch_stride, stream);
  }
  // ITEM, FLOW: the launch's rows of every job, its records from their first row
  SearchJob fj[MAX_JOBS];
  for (int i = 0; i < l.njobs; i++) {
    fj[i] = jobs[l.job0 + i];
    const int skip = launch_r0(l, fj[i]) - fj[i].r0;
    fj[i].r0 += skip;
    fj[i].r1 = launch_r1(l, fj[i]);
    fj[i].mv += 2 * (size_t)skip * base.nbx;
    if (fj[i].cost) fj[i].cost += (size_t)skip * base.nbx;
  }
  if (l.kind == LAUNCH_FLOW) return launch_flow(base, l.g, fj, l.njobs, stream);
  return launch_fast(base, l.g, l.K, job_table(base, l.g.wg_per_row, fj, l.njobs), stream);
}

hipError_t launch_jobs(const SearchArgs& base, const SearchJob* jobs, int n, hipStream_t stream) {
  const SearchShape s{base.width, base.height, base.stride, base.blk, base.range, base.cost_kind,
                      base.mkeys && base.mcnt ? base.merge_tiles : 0,
                      base.scratch ? base.scratch_bytes : 0};
  constexpr int CAP = 64;  // (longer batch lists come in windows)
  static_assert(CAP >= DISPATCH_JOB_MAX, "a job's launches fit the array");
  Launch list[CAP];
  auto run = [&](int count) {
    hipError_t e = hipSuccess;
    for (int i = 0; i < count && e == hipSuccess; i++) e = run_launch(base, jobs, list[i], stream);
    return e;
  };
  for (int skip = 0;; skip += CAP) {
    const int total = dispatch_batch(s, jobs, n, kernel_path(), cu_count(), tuning(), skip, list, CAP);
    if (total < 0) break;  // job by job
    const hipError_t e = run(total - skip < CAP ? total - skip : CAP);
    if (e != hipSuccess || total - skip <= CAP) return e;
  }
  for (int j = 0; j < n; j++) {
    const hipError_t e = run(dispatch_job(s, jobs, j, kernel_path(), cu_count(), tuning(), list));
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace me

#ifdef ME_STAMPS
// Diagnostic build only: copy the per-workgroup stamps to the host.
extern "C" int me_debug_wave_stamps(unsigned long long* out, int n_words) {
  if (n_words > (8 << 14)) n_words = 8 << 14;
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(me::g_wstamps), (size_t)n_words * 8, 0,
                                  hipMemcpyDeviceToHost);
}
extern "C" int me_debug_bound_stamps(unsigned long long* out, int n_words) {
  if (n_words > (16 << 14)) n_words = 16 << 14;
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(me::g_bstamps), (size_t)n_words * 8, 0,
                                  hipMemcpyDeviceToHost);
}
extern "C" int me_debug_stamps(unsigned long long* out, int n_words) {
  if (n_words > (8 << 16)) n_words = 8 << 16;
  return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(me::g_stamps), (size_t)n_words * 8, 0,
                                  hipMemcpyDeviceToHost);
}
#endif
