// me_partition_lane.h -- device side of the partition searches: what the fast
// kernels of me_partition.hip and me_partition_rd.hip share (the key index of
// the nine partitions and the lane's row walk).  HIP translation units only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "me_kernels.h"

namespace me {

// Key index of a macroblock's nine partitions.
enum { P_FULL = 0, P_TOP, P_BOT, P_LEFT, P_RIGHT, P_TL, P_TR, P_BL, P_BR, P_N };

typedef uint16_t u16x2 __attribute__((ext_vector_type(2)));

// Per 16-bit half a + b (v_pk_add_u16): quadrant, half and full SADs of a
// 16 x 16 block all fit u16 (16,320 / 32,640 / 65,280).
__device__ __forceinline__ uint32_t pk_add(uint32_t a, uint32_t b) {
  return __builtin_bit_cast(uint32_t, (u16x2)(__builtin_bit_cast(u16x2, a) + __builtin_bit_cast(u16x2, b)));
}

// Orders row YY's qsads before the next row's (volatile) address step: see
// pin_rows of me_kernels.hip.
template <int J, int K, int YY>
__device__ __forceinline__ void pin_rows(uint64_t (&acc)[K][4]) {
  if constexpr (J < K) {
    if constexpr (YY - J >= 0 && YY - J < 16)
      asm volatile("" : "+v"(acc[J][(YY - J) >= 8 ? 2 : 0]), "+v"(acc[J][(YY - J) >= 8 ? 3 : 1]));
    pin_rows<J + 1, K, YY>(acc);
  }
}

// The lane's 4 dx x K dy candidates of a 16 x 16 block c: LDS byte address
// `at` is window row (first dy row) and the word of the lane's first dx.
// acc[j][q], q = TL, TR, BL, BR: four packed u16 SADs (dx 0..3) each.  The
// row walk is qsad_lane's of me_kernels.hip (one segment per window row: the
// next row's four ds_read2_b32, then this row's qsads), with the accumulator
// chosen by the segment and the block row.
template <int K>
__device__ __forceinline__ void part_lane(uint32_t at, int pitch, const uint32_t (&c)[16][4],
                                          uint64_t (&acc)[K][4]) {
  constexpr int NR = K + 15;
  uint32_t oe = at, oo = at + 4;
  asm volatile("" : "+v"(oo));
#pragma unroll
  for (int j = 0; j < K; j++)
#pragma unroll
    for (int q = 0; q < 4; q++) acc[j][q] = 0;
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
          constexpr int q = (y >= 8 ? 2 : 0) + (k >= 2 ? 1 : 0);
          acc[j][q] = __builtin_amdgcn_qsad_pk_u16_u8(pr[k], c[y][k], acc[j][q]);
        }
      });
    });
    pin_rows<0, K, yy>(acc);
    if constexpr (yy + 1 < NR) {
#pragma unroll
      for (int k = 0; k < 4; k++) pr[k] = nx[k];
    }
  });
}

}  // namespace me
