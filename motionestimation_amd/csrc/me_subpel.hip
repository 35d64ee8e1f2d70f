// me_subpel.hip -- quarter-pel refinement of an integer MV field, sub-pel
// motion compensation, the bi-predictive mode decision over two quarter-pel
// fields with its compensation, and the partition-wise refinement of a
// partition search's four grids with its mode decision (include/me.h
// "quarter-pel", "bi-predictive" and "partition-wise quarter-pel refinement";
// DESIGN.md has the definitions and the LDS layouts).  No reference
// counterpart: the reference stops at integer vectors.
//
// Sample definition (H.264 luma, exact integers): reference samples are edge
// replicated, half samples are the 6-tap (1,-5,20,20,-5,1) filter rounded
// (+16)>>5, the centre half sample filters the unrounded horizontal
// intermediates and rounds (+512)>>10, quarter samples average two half-grid
// neighbours with (+1)>>1.  Every kernel here forms samples through
// qpel_stage / qpel_half_grid / qpel_taps / qpel_pred4: one definition of a
// sample.
//
// One workgroup per block, everything in LDS, each plane read once:
//   r   u8   (TB+6)^2  clamped reference window around the block at its
//                      integer vector: pixels [bx-3, bx+bw+3) x [by-3, by+bh+3)
//   b1  i16  (TB+6) rows x (TB+1) columns of unrounded horizontal half samples
//   hg  u8   the half-pel grid of the block +- 1 pixel, (2TB+3)^2 samples:
//            sample (X, Y) is P2(2bx-2+X, 2by-2+Y).  Stored as two planes by
//            the parity of X (plane X & 1, row Y, column X >> 1, pitch TB+8),
//            so the samples of horizontally adjacent pixels (X stride 2) are
//            adjacent bytes: a lane takes 4 pixels of a candidate as two
//            aligned dwords and one v_alignbyte, and costs them with one
//            v_sad_u8 (SAD) or two v_dot4_u32_u8 (SSD = sum p^2 - 2 sum pc +
//            sum c^2); for SATD the 4 pixels are one row of a 4x4 Hadamard tile
//            (satd4 below).
// A candidate (or the compensated block) is, per pixel, the rounded average of
// two hg samples at offsets that are uniform over the block.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "me.h"
#include "me_kernels.h"
#include "me_tile_search.h"
#include "me_rd.h"

namespace me {
namespace {

template <int TB>
struct QpelGeom {
  static constexpr int NT = TB >= 32 ? 256 : 64;  // threads per block (workgroup)
  static constexpr int NW = NT / 64;
  static constexpr int GW = TB / 4;                                  // 4-pixel groups per row
  static constexpr int GPL = GW * TB / NT < 1 ? 1 : GW * TB / NT;    // groups per lane
  static constexpr int RW = TB + 6, RP = TB + 8;
  static constexpr int BW = TB + 1, BP = TB + 2;
  static constexpr int HG = 2 * TB + 3;  // half-grid rows (and samples per row)
  // plane row pitch: TB + 2 columns, and the dword after a group's last
  // aligned one is read too (then shifted out)
  static constexpr int EP = TB + 8;
  static constexpr int PLANE = HG * EP;
};

template <int TB>
struct QpelLds {
  using G = QpelGeom<TB>;
  uint8_t r[G::RW * G::RP];
  int16_t b1[G::RW * G::BP];
  alignas(4) uint8_t hg[2 * G::PLANE];
  uint32_t red[G::NW * 9];
};

__device__ __forceinline__ int clip255(int v) { return min(max(v, 0), 255); }

// Clamped reference window of the bw x bh block whose integer position is
// (bx, by): any int32 position reads inside the plane.
template <int TB>
__device__ __forceinline__ void qpel_stage(QpelLds<TB>& s, const uint8_t* __restrict__ ref,
                                           int width, int height, int stride, int bx, int by,
                                           int bw, int bh) {
  using G = QpelGeom<TB>;
  for (int i = threadIdx.x; i < G::RW * G::RW; i += G::NT) {
    const int ry = i / G::RW, rx = i % G::RW;
    if (rx < bw + 6 && ry < bh + 6) {
      const int gx = min(max(bx - 3 + rx, 0), width - 1);
      const int gy = min(max(by - 3 + ry, 0), height - 1);
      s.r[ry * G::RP + rx] = ref[(size_t)gy * stride + gx];
    }
  }
}

__device__ __forceinline__ int tap6(int a, int b, int c, int d, int e, int f) {
  return a + f - 5 * (b + e) + 20 * (c + d);
}

// r -> b1 -> hg (barriers inside: every thread of the block calls it, after
// qpel_stage; hg is complete on return).  hg is s.hg, or a second grid of the
// same layout (the bi-prediction kernel keeps one per reference).
template <int TB>
__device__ __forceinline__ void qpel_half_grid(QpelLds<TB>& s, uint8_t* hg, int bw, int bh) {
  using G = QpelGeom<TB>;
  uint8_t* const he = hg;             // even X: column X / 2
  uint8_t* const ho = hg + G::PLANE;  // odd X: column (X - 1) / 2
  __syncthreads();
  // b1 column c is the half sample between pixels bx-1+c and bx+c
  for (int i = threadIdx.x; i < G::RW * G::BW; i += G::NT) {
    const int ry = i / G::BW, c = i % G::BW;
    if (c < bw + 1 && ry < bh + 6) {
      const uint8_t* p = &s.r[ry * G::RP + c];
      s.b1[ry * G::BP + c] = (int16_t)tap6(p[0], p[1], p[2], p[3], p[4], p[5]);
    }
  }
  __syncthreads();
  // X even, Y even: the pixels bx-1 .. bx+bw, by-1 .. by+bh
  for (int i = threadIdx.x; i < (TB + 2) * (TB + 2); i += G::NT) {
    const int j = i / (TB + 2), k = i % (TB + 2);
    if (k < bw + 2 && j < bh + 2) he[2 * j * G::EP + k] = s.r[(j + 2) * G::RP + k + 2];
  }
  // X odd, Y even
  for (int i = threadIdx.x; i < (TB + 2) * (TB + 1); i += G::NT) {
    const int j = i / (TB + 1), k = i % (TB + 1);
    if (k < bw + 1 && j < bh + 2)
      ho[2 * j * G::EP + k] = (uint8_t)clip255((s.b1[(j + 2) * G::BP + k] + 16) >> 5);
  }
  // X even, Y odd: the filter runs down the window's column
  for (int i = threadIdx.x; i < (TB + 1) * (TB + 2); i += G::NT) {
    const int j = i / (TB + 2), k = i % (TB + 2);
    if (k < bw + 2 && j < bh + 1) {
      const uint8_t* p = &s.r[j * G::RP + k + 2];
      const int h1 = tap6(p[0], p[G::RP], p[2 * G::RP], p[3 * G::RP], p[4 * G::RP], p[5 * G::RP]);
      he[(2 * j + 1) * G::EP + k] = (uint8_t)clip255((h1 + 16) >> 5);
    }
  }
  // X odd, Y odd: the filter runs down the unrounded b1 column (32 bits)
  for (int i = threadIdx.x; i < (TB + 1) * (TB + 1); i += G::NT) {
    const int j = i / (TB + 1), k = i % (TB + 1);
    if (k < bw + 1 && j < bh + 1) {
      const int16_t* p = &s.b1[j * G::BP + k];
      const int j1 = tap6(p[0], p[G::BP], p[2 * G::BP], p[3 * G::BP], p[4 * G::BP], p[5 * G::BP]);
      ho[(2 * j + 1) * G::EP + k] = (uint8_t)clip255((j1 + 512) >> 10);
    }
  }
  __syncthreads();
}
template <int TB>
__device__ __forceinline__ void qpel_half_grid(QpelLds<TB>& s, int bw, int bh) {
  qpel_half_grid<TB>(s, s.hg, bw, bh);
}

// The two half-grid samples whose rounded average is the prediction sample at
// quarter offset (ox, oy), |ox|, |oy| <= 3, from the block's integer position,
// as half-pel offsets (tx, ty) from the pixel's own sample.  A sample on the
// half grid is both taps.  hg's origin 2bx-2 is even, so the parity of the
// absolute half coordinates is the parity of the relative ones.
struct QpelTaps {
  int tx0, ty0, tx1, ty1;
};
__device__ __forceinline__ QpelTaps qpel_taps(int ox, int oy) {
  const int hx = ox >> 1, hy = oy >> 1;  // floor
  const int xo = ox & 1, yo = oy & 1;
  if (xo & yo) {
    // the two corners with an odd coordinate sum: the horizontal and the
    // vertical half sample, never the pixel or the centre
    if ((hx + hy) & 1) return {hx, hy, hx + 1, hy + 1};
    return {hx + 1, hy, hx, hy + 1};
  }
  return {hx, hy, hx + xo, hy + yo};
}

// hg samples at half-pel offset (tx, ty), tx in [-2, 2], of the 4 pixels
// (px0 .. px0 + 3, py) of the block, px0 a multiple of 4: bytes 0..3.
template <int TB>
__device__ __forceinline__ uint32_t qpel_load4(const uint8_t* hg, int px0, int py, int tx,
                                               int ty) {
  using G = QpelGeom<TB>;
  // sample X = 2 px + 2 + tx: plane tx & 1, column px + 1 + (tx >> 1)
  const int at = (tx & 1) * G::PLANE + (2 * py + 2 + ty) * G::EP + px0;
  const uint32_t lo = *reinterpret_cast<const uint32_t*>(&hg[at]);
  const uint32_t hi = *reinterpret_cast<const uint32_t*>(&hg[at + 4]);
  return __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)(1 + (tx >> 1)));
}

// Per byte (a + b + 1) >> 1.
__device__ __forceinline__ uint32_t avg4(uint32_t a, uint32_t b) {
  return (a | b) - (((a ^ b) >> 1) & 0x7F7F7F7Fu);
}

// Prediction samples of 4 adjacent pixels from the half grid hg.
template <int TB>
__device__ __forceinline__ uint32_t qpel_pred4(const uint8_t* hg, int px0, int py,
                                               const QpelTaps& t) {
  const uint32_t a = qpel_load4<TB>(hg, px0, py, t.tx0, t.ty0);
  if (t.tx0 == t.tx1 && t.ty0 == t.ty1) return a;  // uniform over the block
  return avg4(a, qpel_load4<TB>(hg, px0, py, t.tx1, t.ty1));
}
template <int TB>
__device__ __forceinline__ uint32_t qpel_pred4(const QpelLds<TB>& s, int px0, int py,
                                               const QpelTaps& t) {
  return qpel_pred4<TB>(s.hg, px0, py, t);
}

// Sum over the wave, the same (scalar) value in every lane.
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
  int x = (int)v;
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, false);  // row_shr:1
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, false);  // row_shr:2
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, false);  // row_shr:4
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, false);  // row_shr:8
  // lane 15 of each row of 16 holds the row's sum
  return (uint32_t)(__builtin_amdgcn_readlane(x, 15) + __builtin_amdgcn_readlane(x, 31) +
                    __builtin_amdgcn_readlane(x, 47) + __builtin_amdgcn_readlane(x, 63));
}

// A lane's pixels: GPL groups of 4 adjacent pixels; cur bytes and the mask of
// the bytes inside the (partial) block, 0 for a group outside it.
template <int TB>
struct QpelPix {
  int px0[QpelGeom<TB>::GPL], py[QpelGeom<TB>::GPL];
  uint32_t cur[QpelGeom<TB>::GPL], mask[QpelGeom<TB>::GPL];
};

// ---- SATD (include/me.h "SATD cost"; DESIGN.md "SATD cost") ----
//
// A lane's group of 4 adjacent pixels is one row of a 4x4 tile anchored at the
// block's top-left, and the tile's other rows are the groups of the lanes
// lane ^ GW and lane ^ 2 GW (group g is row g / GW; with GPL > 1 group k of a
// lane is NT / GW rows, a multiple of 4, further down: tiles of its own).  The
// transform is four butterfly stages that commute: two over the row's pixels
// inside the lane, two over the tile's rows across lanes, on packed int16
// (|T| <= 16 * 255).  The fourth stage is never formed: |a + b| + |a - b| =
// 2 max(|a|, |b|), so sum max(|a|, |b|) over the pairs is sum |T| / 2, the
// satd itself with its shift.  Bytes outside a partial block are 0 on both
// sides (QpelPix::mask): the zero padding of the definition.  Every lane of
// the wave calls this, the lanes without pixels included (they hold zeros).
typedef short s16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ s16x2 as_s16x2(uint32_t v) { return __builtin_bit_cast(s16x2, v); }

// Lane ^ M's v.  Inside a row of 16 lanes a DPP move: a quad permutation for
// M = 1, 2; row_ror:8 is the exchange itself for M = 8; for M = 4 row_ror:4
// serves the lanes whose bit 2 is set (banks 1 and 3) and row_ror:12 the
// others.  Across rows the LDS crossbar.  Every lane of the wave is active.
template <int M>
__device__ __forceinline__ uint32_t lane_xor(uint32_t v) {
  const int x = (int)v;
  if (M == 1) return (uint32_t)__builtin_amdgcn_update_dpp(0, x, 0xB1, 0xF, 0xF, false);
  if (M == 2) return (uint32_t)__builtin_amdgcn_update_dpp(0, x, 0x4E, 0xF, 0xF, false);
  if (M == 4) {
    const int t = __builtin_amdgcn_update_dpp(0, x, 0x124, 0xF, 0xA, false);  // row_ror:4
    return (uint32_t)__builtin_amdgcn_update_dpp(t, x, 0x12C, 0xF, 0x5, false);  // row_ror:12
  }
  if (M == 8) return (uint32_t)__builtin_amdgcn_update_dpp(0, x, 0x128, 0xF, 0xF, false);
  return (uint32_t)__shfl_xor(x, M, 64);
}

// v + partner in the lane whose bit M is clear, partner - v in lane ^ M.
template <int M>
__device__ __forceinline__ s16x2 satd_rows(s16x2 v) {
  const s16x2 partner = as_s16x2(lane_xor<M>(__builtin_bit_cast(uint32_t, v)));
  const short sg = (threadIdx.x & M) ? -1 : 1;
  return v * s16x2{sg, sg} + partner;
}

// The lane's share of the satd of prediction bytes p against cur bytes c.
template <int TB>
__device__ __forceinline__ uint32_t satd4(uint32_t p, uint32_t c) {
  constexpr int GW = QpelGeom<TB>::GW;
  // residuals of pixels (0, 2) and (1, 3)
  s16x2 e = as_s16x2(p & 0x00FF00FFu) - as_s16x2(c & 0x00FF00FFu);
  s16x2 o = as_s16x2((p >> 8) & 0x00FF00FFu) - as_s16x2((c >> 8) & 0x00FF00FFu);
  // (x, y) -> (x + y, x - y): pixels 0 with 2, 1 with 3
  e = e * s16x2{1, -1} + e.yx;
  o = o * s16x2{1, -1} + o.yx;
  e = satd_rows<GW>(e);
  o = satd_rows<GW>(o);
  e = satd_rows<2 * GW>(e);
  o = satd_rows<2 * GW>(o);
  // pixels (0, 2) with (1, 3): the stage that is not formed
  const s16x2 m = __builtin_elementwise_max(__builtin_elementwise_abs(e),
                                            __builtin_elementwise_abs(o));
  return (uint32_t)m.x + (uint32_t)m.y;
}

// Costs of the candidates centre + step * (dx, dy), dx, dy in {-1, 0, 1}, in
// raster order into out[0..9) (out[4], the centre, only when CENTRE), summed
// over the block: every thread returns the same nine numbers.
template <int TB, int COST, bool CENTRE>
__device__ __forceinline__ void qpel_costs(QpelLds<TB>& s, const QpelPix<TB>& P, uint32_t cc,
                                           int cx, int cy, int step, uint32_t (&out)[9]) {
  using G = QpelGeom<TB>;
  constexpr bool SSD = COST == ME_COST_SSD;
  uint32_t acc[9];
#pragma unroll
  for (int n = 0; n < 9; n++) {
    acc[n] = 0;
    if (n == 4 && !CENTRE) continue;
    const QpelTaps t = qpel_taps(cx + step * (n % 3 - 1), cy + step * (n / 3 - 1));
    uint32_t pp = 0, pc = 0;
#pragma unroll
    for (int k = 0; k < G::GPL; k++) {
      // bytes outside a partial block are 0 on both sides and cost nothing
      const uint32_t p = qpel_pred4<TB>(s, P.px0[k], P.py[k], t) & P.mask[k];
      if (COST == ME_COST_SATD) {
        pp += satd4<TB>(p, P.cur[k]);
      } else if (SSD) {
        pp = __builtin_amdgcn_udot4(p, p, pp, false);
        pc = __builtin_amdgcn_udot4(p, P.cur[k], pc, false);
      } else {
        pp = __builtin_amdgcn_sad_u8(p, P.cur[k], pp);
      }
    }
    // sum (p - c)^2 = sum p^2 - 2 sum pc + sum c^2 (cc: the lane's sum c^2)
    acc[n] = wave_sum(SSD ? pp + cc - 2 * pc : pp);
  }
  if (G::NW > 1) {
    __syncthreads();  // the previous stage's sums have been read
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int n = 0; n < 9; n++) s.red[(threadIdx.x >> 6) * 9 + n] = acc[n];
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < 9; n++) {
      acc[n] = 0;
      for (int w = 0; w < G::NW; w++) acc[n] += s.red[w * 9 + n];
    }
  }
#pragma unroll
  for (int n = 0; n < 9; n++)
    if (n != 4 || CENTRE) out[n] = acc[n];
}

// The lane's 4-pixel groups of the bw x bh block; cur (null: no cur bytes) is
// the block's top-left pixel, row pitch stride.
template <int TB>
__device__ __forceinline__ void qpel_pixels(QpelPix<TB>& P, const uint8_t* __restrict__ cur,
                                            int stride, int bw, int bh) {
  using G = QpelGeom<TB>;
#pragma unroll
  for (int k = 0; k < G::GPL; k++) {
    const int g = threadIdx.x + k * G::NT;
    const int py = g / G::GW, px0 = (g % G::GW) * 4;
    const bool row = py < bh;  // (bh <= TB also bounds g)
    P.px0[k] = row ? px0 : 0;
    P.py[k] = row ? py : 0;
    uint32_t c = 0, m = 0;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      if (row && px0 + e < bw) {
        m |= 0xFFu << (8 * e);
        if (cur) c |= (uint32_t)cur[(size_t)py * stride + px0 + e] << (8 * e);
      }
    }
    P.cur[k] = c;
    P.mask[k] = m;
  }
}

// One block (workgroup) per macroblock, the frame in blockIdx.y.  mv_in and
// mv_out may be the same array: a block reads its own record before its first
// barrier and writes it after its last.
template <int TB, int COST>
__global__ __launch_bounds__(QpelGeom<TB>::NT) void me_qpel_refine_kernel(
    const uint8_t* __restrict__ ref, size_t ref_frame_stride, const uint8_t* __restrict__ cur,
    size_t cur_frame_stride, int width, int height, int stride, int blk, int nbx, int nblk,
    const int16_t* mv_in, int16_t* mv_out, uint32_t* cost_out) {
  using G = QpelGeom<TB>;
  constexpr bool SSD = COST == ME_COST_SSD;
  __shared__ QpelLds<TB> s;
  const int b = blockIdx.x, f = blockIdx.y;
  const size_t rec = (size_t)f * nblk + b;
  const int x0 = (b % nbx) * blk, y0 = (b / nbx) * blk;
  const int bw = min(blk, width - x0), bh = min(blk, height - y0);
  const int mx = mv_in[2 * rec], my = mv_in[2 * rec + 1];
  ref += (size_t)f * ref_frame_stride;
  cur += (size_t)f * cur_frame_stride;

  QpelPix<TB> P;
  qpel_pixels<TB>(P, cur + (size_t)y0 * stride + x0, stride, bw, bh);
  uint32_t cc = 0;
  if (SSD) {
#pragma unroll
    for (int k = 0; k < G::GPL; k++) cc = __builtin_amdgcn_udot4(P.cur[k], P.cur[k], cc, false);
  }
  qpel_stage<TB>(s, ref, width, height, stride, x0 + mx, y0 + my, bw, bh);
  qpel_half_grid<TB>(s, bw, bh);

  uint32_t c9[9];
  int ox = 0, oy = 0;  // quarter offset of the best candidate from 4 * m
  uint32_t best;
  qpel_costs<TB, COST, true>(s, P, cc, 0, 0, 2, c9);
  best = c9[4];
#pragma unroll
  for (int n = 0; n < 9; n++) {
    if (n != 4 && c9[n] < best) {
      best = c9[n];
      ox = 2 * (n % 3 - 1);
      oy = 2 * (n / 3 - 1);
    }
  }
  const int cx = ox, cy = oy;
  qpel_costs<TB, COST, false>(s, P, cc, cx, cy, 1, c9);
#pragma unroll
  for (int n = 0; n < 9; n++) {
    if (n != 4 && c9[n] < best) {
      best = c9[n];
      ox = cx + n % 3 - 1;
      oy = cy + n / 3 - 1;
    }
  }
  if (threadIdx.x == 0) {
    mv_out[2 * rec] = (int16_t)(4 * mx + ox);
    mv_out[2 * rec + 1] = (int16_t)(4 * my + oy);
    if (cost_out) cost_out[rec] = best;
  }
}

// me_qpel_refine_kernel on Jq(q) = cost(P(q)) + lambda (bits(qx - px) +
// bits(qy - py)) against the block's quarter-pel predictor (include/me.h
// "rate-constrained motion search"): the same stages, candidate order, carried
// centre and strict <.  A kernel of its own, so the plain refinement's code and
// registers stay as they are.  pred null: all zero; cost_out (Jq) and dist_out
// (the cost at the result) may be null.
template <int TB, int COST>
__global__ __launch_bounds__(QpelGeom<TB>::NT) void me_qpel_refine_rd_kernel(
    const uint8_t* __restrict__ ref, size_t ref_frame_stride, const uint8_t* __restrict__ cur,
    size_t cur_frame_stride, int width, int height, int stride, int blk, int nbx, int nblk,
    uint32_t lambda, const int16_t* pred, const int16_t* mv_in, int16_t* mv_out,
    uint32_t* cost_out, uint32_t* dist_out) {
  using G = QpelGeom<TB>;
  constexpr bool SSD = COST == ME_COST_SSD;
  __shared__ QpelLds<TB> s;
  const int b = blockIdx.x, f = blockIdx.y;
  const size_t rec = (size_t)f * nblk + b;
  const int x0 = (b % nbx) * blk, y0 = (b / nbx) * blk;
  const int bw = min(blk, width - x0), bh = min(blk, height - y0);
  const int mx = mv_in[2 * rec], my = mv_in[2 * rec + 1];
  // the centre relative to the predictor, in quarter units
  const int ex = 4 * mx - (pred ? pred[2 * rec] : 0), ey = 4 * my - (pred ? pred[2 * rec + 1] : 0);
  ref += (size_t)f * ref_frame_stride;
  cur += (size_t)f * cur_frame_stride;

  QpelPix<TB> P;
  qpel_pixels<TB>(P, cur + (size_t)y0 * stride + x0, stride, bw, bh);
  uint32_t cc = 0;
  if (SSD) {
#pragma unroll
    for (int k = 0; k < G::GPL; k++) cc = __builtin_amdgcn_udot4(P.cur[k], P.cur[k], cc, false);
  }
  qpel_stage<TB>(s, ref, width, height, stride, x0 + mx, y0 + my, bw, bh);
  qpel_half_grid<TB>(s, bw, bh);

  auto rate = [&](int ox, int oy) {
    return lambda * (uint32_t)(rd_bits(ex + ox) + rd_bits(ey + oy));
  };
  uint32_t c9[9];
  int ox = 0, oy = 0;  // quarter offset of the best candidate from 4 * m
  qpel_costs<TB, COST, true>(s, P, cc, 0, 0, 2, c9);
  uint32_t dist = c9[4], best = dist + rate(0, 0);
#pragma unroll
  for (int n = 0; n < 9; n++) {
    const uint32_t j = c9[n] + rate(2 * (n % 3 - 1), 2 * (n / 3 - 1));
    if (n != 4 && j < best) {
      best = j;
      dist = c9[n];
      ox = 2 * (n % 3 - 1);
      oy = 2 * (n / 3 - 1);
    }
  }
  const int cx = ox, cy = oy;
  qpel_costs<TB, COST, false>(s, P, cc, cx, cy, 1, c9);
#pragma unroll
  for (int n = 0; n < 9; n++) {
    if (n == 4) continue;
    const uint32_t j = c9[n] + rate(cx + n % 3 - 1, cy + n / 3 - 1);
    if (j < best) {
      best = j;
      dist = c9[n];
      ox = cx + n % 3 - 1;
      oy = cy + n / 3 - 1;
    }
  }
  if (threadIdx.x == 0) {
    mv_out[2 * rec] = (int16_t)(4 * mx + ox);
    mv_out[2 * rec + 1] = (int16_t)(4 * my + oy);
    if (cost_out) cost_out[rec] = best;
    if (dist_out) dist_out[rec] = dist;
  }
}

// Sub-pel me_compensate_kernel, one block (workgroup) per macroblock: packed
// planes (pitch = width), outputs and stats as me_post.hip's kernel.
template <int TB>
__global__ __launch_bounds__(QpelGeom<TB>::NT) void me_qpel_compensate_kernel(
    const uint8_t* __restrict__ ref, const uint8_t* __restrict__ cur, int width, int height,
    int blk, int nbx, const int16_t* __restrict__ mvq, uint8_t* __restrict__ out5,
    int write_planes, unsigned long long* stats) {
  using G = QpelGeom<TB>;
  __shared__ QpelLds<TB> s;
  const int b = blockIdx.x;
  const int x0 = (b % nbx) * blk, y0 = (b / nbx) * blk;
  const int bw = min(blk, width - x0), bh = min(blk, height - y0);
  const int qx = mvq[2 * b], qy = mvq[2 * b + 1];
  QpelPix<TB> P;
  qpel_pixels<TB>(P, nullptr, 0, bw, bh);
  qpel_stage<TB>(s, ref, width, height, width, x0 + (qx >> 2), y0 + (qy >> 2), bw, bh);
  qpel_half_grid<TB>(s, bw, bh);
  const QpelTaps t = qpel_taps(qx & 3, qy & 3);

  const size_t n = (size_t)width * height;
  unsigned long long sq = 0;
  uint32_t mxv = 0;
#pragma unroll
  for (int k = 0; k < G::GPL; k++) {
    const uint32_t p4 = qpel_pred4<TB>(s, P.px0[k], P.py[k], t);
#pragma unroll
    for (int e = 0; e < 4; e++) {
      if (P.mask[k] >> (8 * e) & 1) {
        const size_t i = (size_t)(y0 + P.py[k]) * width + x0 + P.px0[k] + e;
        const int m = (int)(p4 >> (8 * e) & 0xFF);
        const int r = ref[i], c = cur[i];
        const int d = m - c;
        sq += (unsigned long long)(d * d);
        mxv = max(mxv, (uint32_t)max(m, c));
        if (write_planes) {
          out5[i] = (uint8_t)r;
          out5[n + i] = (uint8_t)c;
          out5[2 * n + i] = (uint8_t)m;
          out5[3 * n + i] = (uint8_t)abs(r - c);
          out5[4 * n + i] = (uint8_t)abs(d);
        } else {
          out5[i] = (uint8_t)m;
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sq += __shfl_xor(sq, off, 64);
    mxv = max(mxv, (uint32_t)__shfl_xor((int)mxv, off, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&stats[0], sq);
    atomicMax(&stats[1], (unsigned long long)mxv);
  }
}

// ---- bi-prediction (include/me.h "bi-prediction"; DESIGN.md "Bi-prediction") ----
//
// The window r and the intermediates b1 are staged for ref0 and turned into
// the half grid hg (of QpelLds), then reused for ref1 -> hg1: only the half
// grid is doubled.  Each window sits at its vector's nearest integer position
// (q + 2) >> 2, so the vector's own quarter offset is in [-2, 1] and its eight
// quarter-step neighbours are in [-3, 2]: inside the +-3 the half grid covers.
template <int TB>
struct BipredLds : QpelLds<TB> {
  alignas(4) uint8_t hg1[2 * QpelGeom<TB>::PLANE];
};

// Adds the cost terms of 4 (masked) prediction bytes p against cur bytes c.
template <int TB, int COST>
__device__ __forceinline__ void cost4(uint32_t p, uint32_t c, uint32_t& pp, uint32_t& pc) {
  if (COST == ME_COST_SATD) {
    pp += satd4<TB>(p, c);
  } else if (COST == ME_COST_SSD) {
    pp = __builtin_amdgcn_udot4(p, p, pp, false);
    pc = __builtin_amdgcn_udot4(p, c, pc, false);
  } else {
    pp = __builtin_amdgcn_sad_u8(p, c, pp);
  }
}

// v[0..N) summed over the block, N <= 9: every thread returns the same numbers.
template <int TB, int N>
__device__ __forceinline__ void block_sums(QpelLds<TB>& s, uint32_t (&v)[N]) {
  using G = QpelGeom<TB>;
#pragma unroll
  for (int n = 0; n < N; n++) v[n] = wave_sum(v[n]);
  if (G::NW > 1) {
    __syncthreads();  // the previous sums have been read
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int n = 0; n < N; n++) s.red[(threadIdx.x >> 6) * 9 + n] = v[n];
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < N; n++) {
      v[n] = 0;
      for (int w = 0; w < G::NW; w++) v[n] += s.red[w * 9 + n];
    }
  }
}

// One pass of the joint refinement: the eight quarter-step neighbours of
// (cx, cy) on the half grid hg, each averaged with the other reference's
// prediction held in registers, in raster order; a candidate replaces
// (best, bx, by) only with a strictly smaller cost.
template <int TB, int COST>
__device__ __forceinline__ void bipred_pass(QpelLds<TB>& s, const QpelPix<TB>& P, uint32_t cc,
                                            const uint32_t (&held)[QpelGeom<TB>::GPL],
                                            const uint8_t* hg, int cx, int cy, uint32_t& best,
                                            int& bx, int& by) {
  using G = QpelGeom<TB>;
  constexpr bool SSD = COST == ME_COST_SSD;
  uint32_t v[8];
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int n = j < 4 ? j : j + 1;  // raster index without the centre
    const QpelTaps t = qpel_taps(cx + n % 3 - 1, cy + n / 3 - 1);
    uint32_t pp = 0, pc = 0;
#pragma unroll
    for (int k = 0; k < G::GPL; k++) {
      const uint32_t p = avg4(held[k], qpel_pred4<TB>(hg, P.px0[k], P.py[k], t)) & P.mask[k];
      cost4<TB, COST>(p, P.cur[k], pp, pc);
    }
    v[j] = SSD ? pp + cc - 2 * pc : pp;
  }
  block_sums<TB, 8>(s, v);
#pragma unroll
  for (int j = 0; j < 8; j++) {
    const int n = j < 4 ? j : j + 1;
    if (v[j] < best) {
      best = v[j];
      bx = cx + n % 3 - 1;
      by = cy + n / 3 - 1;
    }
  }
}

// One block (workgroup) per macroblock, the frame in blockIdx.y.  The outputs
// may be the inputs: a block reads its own records before its first barrier
// and writes them after its last.
template <int TB, int COST>
__global__ __launch_bounds__(QpelGeom<TB>::NT) void me_bipred_kernel(
    const uint8_t* __restrict__ ref0, size_t ref0_frame_stride, const uint8_t* __restrict__ ref1,
    size_t ref1_frame_stride, const uint8_t* __restrict__ cur, size_t cur_frame_stride, int width,
    int height, int stride, int blk, int nbx, int nblk, int refine, const int16_t* q0_in,
    const int16_t* q1_in, int16_t* q0_out, int16_t* q1_out, uint8_t* mode_out, uint32_t* cost_out,
    uint32_t* cost3_out) {
  using G = QpelGeom<TB>;
  constexpr bool SSD = COST == ME_COST_SSD;
  __shared__ BipredLds<TB> s;
  const int b = blockIdx.x, f = blockIdx.y;
  const size_t rec = (size_t)f * nblk + b;
  const int x0 = (b % nbx) * blk, y0 = (b / nbx) * blk;
  const int bw = min(blk, width - x0), bh = min(blk, height - y0);
  const int q0x = q0_in[2 * rec], q0y = q0_in[2 * rec + 1];
  const int q1x = q1_in[2 * rec], q1y = q1_in[2 * rec + 1];
  // integer window positions and the vectors' quarter offsets from them
  const int i0x = (q0x + 2) >> 2, i0y = (q0y + 2) >> 2;
  const int i1x = (q1x + 2) >> 2, i1y = (q1y + 2) >> 2;
  ref0 += (size_t)f * ref0_frame_stride;
  ref1 += (size_t)f * ref1_frame_stride;
  cur += (size_t)f * cur_frame_stride;

  QpelPix<TB> P;
  qpel_pixels<TB>(P, cur + (size_t)y0 * stride + x0, stride, bw, bh);
  uint32_t cc = 0;
  if (SSD) {
#pragma unroll
    for (int k = 0; k < G::GPL; k++) cc = __builtin_amdgcn_udot4(P.cur[k], P.cur[k], cc, false);
  }
  qpel_stage<TB>(s, ref0, width, height, stride, x0 + i0x, y0 + i0y, bw, bh);
  qpel_half_grid<TB>(s, s.hg, bw, bh);
  // hg is complete and r / b1 are free again (qpel_half_grid ends on a barrier)
  qpel_stage<TB>(s, ref1, width, height, stride, x0 + i1x, y0 + i1y, bw, bh);
  qpel_half_grid<TB>(s, s.hg1, bw, bh);

  int o0x = q0x - 4 * i0x, o0y = q0y - 4 * i0y;  // b0 - 4 * i0, in [-2, 1]
  int o1x = q1x - 4 * i1x, o1y = q1y - 4 * i1y;
  uint32_t held[G::GPL];  // the prediction that stays while the other one moves
  uint32_t c3[3];
  {
    const QpelTaps t0 = qpel_taps(o0x, o0y), t1 = qpel_taps(o1x, o1y);
    uint32_t pp[3] = {0, 0, 0}, pc[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < G::GPL; k++) {
      const uint32_t a = qpel_pred4<TB>(s.hg, P.px0[k], P.py[k], t0);
      const uint32_t c = qpel_pred4<TB>(s.hg1, P.px0[k], P.py[k], t1);
      held[k] = a;
      cost4<TB, COST>(a & P.mask[k], P.cur[k], pp[0], pc[0]);
      cost4<TB, COST>(c & P.mask[k], P.cur[k], pp[1], pc[1]);
      cost4<TB, COST>(avg4(a, c) & P.mask[k], P.cur[k], pp[2], pc[2]);
    }
#pragma unroll
    for (int n = 0; n < 3; n++) c3[n] = SSD ? pp[n] + cc - 2 * pc[n] : pp[n];
    block_sums<TB, 3>(s, c3);
  }
  if (refine) {  // uniform over the grid
    bipred_pass<TB, COST>(s, P, cc, held, s.hg1, o1x, o1y, c3[2], o1x, o1y);
    const QpelTaps t1 = qpel_taps(o1x, o1y);
#pragma unroll
    for (int k = 0; k < G::GPL; k++) held[k] = qpel_pred4<TB>(s.hg1, P.px0[k], P.py[k], t1);
    bipred_pass<TB, COST>(s, P, cc, held, s.hg, o0x, o0y, c3[2], o0x, o0y);
  }
  if (threadIdx.x == 0) {
    // L0, L1, BI in that order, a later mode only with a strictly smaller cost
    uint32_t best = c3[0];
    int mode = ME_PRED_L0;
    if (c3[1] < best) best = c3[1], mode = ME_PRED_L1;
    if (c3[2] < best) best = c3[2], mode = ME_PRED_BI;
    const bool bi = mode == ME_PRED_BI;
    q0_out[2 * rec] = (int16_t)(bi ? 4 * i0x + o0x : q0x);
    q0_out[2 * rec + 1] = (int16_t)(bi ? 4 * i0y + o0y : q0y);
    q1_out[2 * rec] = (int16_t)(bi ? 4 * i1x + o1x : q1x);
    q1_out[2 * rec + 1] = (int16_t)(bi ? 4 * i1y + o1y : q1y);
    mode_out[rec] = (uint8_t)mode;
    if (cost_out) cost_out[rec] = best;
    if (cost3_out) {
      cost3_out[3 * rec] = c3[0];
      cost3_out[3 * rec + 1] = c3[1];
      cost3_out[3 * rec + 2] = c3[2];
    }
  }
}

// me_qpel_compensate_kernel with a mode per block: the block is P0(v0), P1(v1)
// or their rounded average.  One half grid: a reference's samples are in
// registers before the next one is staged.  Plane 0 and |ref - cur| are ref0's.
template <int TB>
__global__ __launch_bounds__(QpelGeom<TB>::NT) void me_bipred_compensate_kernel(
    const uint8_t* __restrict__ ref0, const uint8_t* __restrict__ ref1,
    const uint8_t* __restrict__ cur, int width, int height, int blk, int nbx,
    const int16_t* __restrict__ mv0, const int16_t* __restrict__ mv1,
    const uint8_t* __restrict__ mode, uint8_t* __restrict__ out5, int write_planes,
    unsigned long long* stats) {
  using G = QpelGeom<TB>;
  __shared__ QpelLds<TB> s;
  const int b = blockIdx.x;
  const int x0 = (b % nbx) * blk, y0 = (b / nbx) * blk;
  const int bw = min(blk, width - x0), bh = min(blk, height - y0);
  const int md = mode[b];  // uniform over the block (the host rejects md > 2)
  QpelPix<TB> P;
  qpel_pixels<TB>(P, nullptr, 0, bw, bh);
  uint32_t p4[G::GPL] = {};
  if (md != ME_PRED_L1) {
    const int qx = mv0[2 * b], qy = mv0[2 * b + 1];
    qpel_stage<TB>(s, ref0, width, height, width, x0 + (qx >> 2), y0 + (qy >> 2), bw, bh);
    qpel_half_grid<TB>(s, bw, bh);
    const QpelTaps t = qpel_taps(qx & 3, qy & 3);
#pragma unroll
    for (int k = 0; k < G::GPL; k++) p4[k] = qpel_pred4<TB>(s, P.px0[k], P.py[k], t);
  }
  if (md != ME_PRED_L0) {
    const int qx = mv1[2 * b], qy = mv1[2 * b + 1];
    // the reads of hg above precede the first barrier of this qpel_half_grid,
    // its writes to hg follow the second
    qpel_stage<TB>(s, ref1, width, height, width, x0 + (qx >> 2), y0 + (qy >> 2), bw, bh);
    qpel_half_grid<TB>(s, bw, bh);
    const QpelTaps t = qpel_taps(qx & 3, qy & 3);
#pragma unroll
    for (int k = 0; k < G::GPL; k++) {
      const uint32_t c = qpel_pred4<TB>(s, P.px0[k], P.py[k], t);
      p4[k] = md == ME_PRED_L1 ? c : avg4(p4[k], c);
    }
  }

  const size_t n = (size_t)width * height;
  unsigned long long sq = 0;
  uint32_t mxv = 0;
#pragma unroll
  for (int k = 0; k < G::GPL; k++) {
#pragma unroll
    for (int e = 0; e < 4; e++) {
      if (P.mask[k] >> (8 * e) & 1) {
        const size_t i = (size_t)(y0 + P.py[k]) * width + x0 + P.px0[k] + e;
        const int m = (int)(p4[k] >> (8 * e) & 0xFF);
        const int r = ref0[i], c = cur[i];
        const int d = m - c;
        sq += (unsigned long long)(d * d);
        mxv = max(mxv, (uint32_t)max(m, c));
        if (write_planes) {
          out5[i] = (uint8_t)r;
          out5[n + i] = (uint8_t)c;
          out5[2 * n + i] = (uint8_t)m;
          out5[3 * n + i] = (uint8_t)abs(r - c);
          out5[4 * n + i] = (uint8_t)abs(d);
        } else {
          out5[i] = (uint8_t)m;
        }
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    sq += __shfl_xor(sq, off, 64);
    mxv = max(mxv, (uint32_t)__shfl_xor((int)mxv, off, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(&stats[0], sq);
    atomicMax(&stats[1], (unsigned long long)mxv);
  }
}

// ---- partition-wise quarter-pel refinement (include/me.h "partition-wise
// quarter-pel refinement"; DESIGN.md has the layout and the counts) ----
//
// One workgroup per macroblock refines its nine partitions (P_FULL .. P_BR of
// me_tile_search.h's order: the macroblock, top, bottom, left, right, and
// the quarters TL, TR, BL, BR).  The lanes keep qpel_pixels' layout of the
// whole macroblock, one 4-pixel group each (GPL = 1 for B in {8, 16, 32}); a
// group lies in exactly one quarter, so a candidate is costed once per lane
// and reduced per quarter: every partition's cost is a sum of quarter sums
// (SATD too: its tiles are anchored at multiples of 4 and the quarters at
// multiples of h >= 4).
//
// Partitions are grouped by integer vector.  The window is staged and the half
// grid built once per distinct vector, over the bounding rectangle of the
// partitions that hold it; stage 1's nine candidates are the same positions
// for all of them.  Stage 2 then runs once per distinct stage-1 centre within
// the group, on the same half grid.  Everything a decision depends on is
// uniform over the workgroup, so the loops and branches are too.
// Per partition: its quarters (bit k: TL, TR, BL, BR), its grid, and its cell's
// offset in the macroblock.
__host__ __device__ constexpr int pq_quads(int p) {
  return (int)(0x8421A5C3Full >> (4 * p)) & 15;  // 15, 3, 12, 5, 10, 1, 2, 4, 8
}
__host__ __device__ constexpr int pq_grid(int p) { return p == 0 ? 0 : p < 3 ? 1 : p < 5 ? 2 : 3; }
__host__ __device__ constexpr int pq_i(int p) { return p == P_RIGHT || p == P_TR || p == P_BR; }
__host__ __device__ constexpr int pq_j(int p) { return p == P_BOT || p == P_BL || p == P_BR; }

struct PartQpelIO {
  const int16_t* in[4];  // integer grids
  int16_t* mv[4];
  uint32_t* cost[4];  // each may be null
  uint32_t* dist[4];
  uint8_t* bits[4];
  uint8_t* mode;
  uint32_t* mode_cost;  // may be null
  const int16_t* pred;  // null: all zero
  int nx[4], ny[4];     // the four grids
  uint32_t lambda;
};

template <int TB>
struct PartQpelLds : QpelLds<TB> {
  uint32_t qred[QpelGeom<TB>::NW * 9 * 2];  // per wave and candidate: left, right
};

// Sums over each row of 16 lanes, in the row's lane 15.
__device__ __forceinline__ int row_sum(uint32_t v) {
  int x = (int)v;
  x += __builtin_amdgcn_update_dpp(0, x, 0x111, 0xF, 0xF, false);  // row_shr:1
  x += __builtin_amdgcn_update_dpp(0, x, 0x112, 0xF, 0xF, false);  // row_shr:2
  x += __builtin_amdgcn_update_dpp(0, x, 0x114, 0xF, 0xF, false);  // row_shr:4
  x += __builtin_amdgcn_update_dpp(0, x, 0x118, 0xF, 0xF, false);  // row_shr:8
  return x;
}

// A partition's cost from the quarter sums (quads: its quarters).
__device__ __forceinline__ uint32_t part_sum(const uint32_t (&q)[4], int quads) {
  uint32_t c = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) c += quads >> k & 1 ? q[k] : 0;
  return c;
}

// v[n] summed over the lanes of each quarter (qi: the lane's), and from the
// quarter sums c[n]: the cost of the partition whose quarters are `quads` (the
// lane's own partition: any lane may ask for another one).  n = 4 only when
// CENTRE.
template <int TB, bool CENTRE>
__device__ __forceinline__ void part_sums(PartQpelLds<TB>& s, const uint32_t (&v)[9], int qi,
                                          int quads, uint32_t (&c)[9]) {
  using G = QpelGeom<TB>;
  if constexpr (TB == 16) {
    // lane = 4 py + px0 / 4: a row of 16 lanes is 4 pixel rows, rows 0 and 1 the top
#pragma unroll
    for (int n = 0; n < 9; n++) {
      if (n == 4 && !CENTRE) continue;
      const int l = row_sum(qi & 1 ? 0 : v[n]), r = row_sum(qi & 1 ? v[n] : 0);
      const uint32_t q[4] = {
          (uint32_t)(__builtin_amdgcn_readlane(l, 15) + __builtin_amdgcn_readlane(l, 31)),
          (uint32_t)(__builtin_amdgcn_readlane(r, 15) + __builtin_amdgcn_readlane(r, 31)),
          (uint32_t)(__builtin_amdgcn_readlane(l, 47) + __builtin_amdgcn_readlane(l, 63)),
          (uint32_t)(__builtin_amdgcn_readlane(r, 47) + __builtin_amdgcn_readlane(r, 63))};
      c[n] = part_sum(q, quads);
    }
  } else if constexpr (G::NW == 4) {
    // thread = 8 py + px0 / 4: waves 0 and 1 are the top half
    uint32_t l[9], r[9];
#pragma unroll
    for (int n = 0; n < 9; n++) {
      if (n == 4 && !CENTRE) continue;
      l[n] = wave_sum(qi & 1 ? 0 : v[n]);
      r[n] = wave_sum(qi & 1 ? v[n] : 0);
    }
    __syncthreads();  // the previous sums have been read
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int n = 0; n < 9; n++) {
        if (n == 4 && !CENTRE) continue;
        s.qred[((threadIdx.x >> 6) * 9 + n) * 2] = l[n];
        s.qred[((threadIdx.x >> 6) * 9 + n) * 2 + 1] = r[n];
      }
    }
    __syncthreads();
#pragma unroll
    for (int n = 0; n < 9; n++) {
      if (n == 4 && !CENTRE) continue;
      uint32_t q[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const int w = k & 2;  // first wave of the half
        q[k] = s.qred[(w * 9 + n) * 2 + (k & 1)] + s.qred[((w + 1) * 9 + n) * 2 + (k & 1)];
      }
      c[n] = part_sum(q, quads);
    }
  } else {
    static_assert(G::NW == 1, "one wave");
#pragma unroll
    for (int n = 0; n < 9; n++) {
      if (n == 4 && !CENTRE) continue;
      uint32_t q[4];
#pragma unroll
      for (int k = 0; k < 4; k++) q[k] = wave_sum(qi == k ? v[n] : 0);
      c[n] = part_sum(q, quads);
    }
  }
}

// out[n]: the cost of the partition `quads` at the candidates centre + step *
// (dx, dy) in raster order n (n = 4, the centre, only when CENTRE).  The lane's
// group is at (px0, py) of the staged rectangle: cur bytes c, mask m (0: a lane
// outside the rectangle), cc the lane's sum c^2 (SSD).
template <int TB, int COST, bool CENTRE>
__device__ __forceinline__ void part_qpel_costs(PartQpelLds<TB>& s, int px0, int py, uint32_t c,
                                                uint32_t m, uint32_t cc, int qi, int quads,
                                                int cx, int cy, int step, uint32_t (&out)[9]) {
  uint32_t v[9];
#pragma unroll
  for (int n = 0; n < 9; n++) {
    v[n] = 0;
    if (n == 4 && !CENTRE) continue;
    const QpelTaps t = qpel_taps(cx + step * (n % 3 - 1), cy + step * (n / 3 - 1));
    uint32_t pp = 0, pc = 0;
    cost4<TB, COST>(qpel_pred4<TB>(s.hg, px0, py, t) & m, c, pp, pc);
    v[n] = COST == ME_COST_SSD ? pp + cc - 2 * pc : pp;
  }
  part_sums<TB, CENTRE>(s, v, qi, quads, out);
}

// Lane p < 9 of every wave keeps partition p's record (every wave the same
// nine: what a decision reads is the same in all of them), so the nine
// decisions of a candidate are one compare, and what the group loops read of
// them (a vector, a centre, who shares it) is a v_readlane or a ballot.  The
// grids may be refined in place (io.mv[g] == io.in[g]): a workgroup reads its
// macroblock's nine vectors before its first barrier and writes its records
// after its last, and every cell belongs to exactly one macroblock.
template <int TB, int COST>
__global__ __launch_bounds__(QpelGeom<TB>::NT) void me_partition_qpel_kernel(
    const uint8_t* __restrict__ ref, size_t ref_frame_stride, const uint8_t* __restrict__ cur,
    size_t cur_frame_stride, int width, int height, int stride, PartQpelIO io) {
  using G = QpelGeom<TB>;
  static_assert(G::GPL == 1, "one 4-pixel group per lane");
  constexpr int h = TB / 2;
  __shared__ PartQpelLds<TB> s;
  const int nbx = io.nx[0];
  const int bx = (int)blockIdx.x % nbx, by = (int)blockIdx.x / nbx, f = blockIdx.y;
  const int x0 = bx * TB, y0 = by * TB;
  const int bw = min(TB, width - x0), bh = min(TB, height - y0);
  const size_t mb = (size_t)f * nbx * io.ny[0] + (size_t)by * nbx + bx;
  const int px = io.pred ? io.pred[2 * mb] : 0, py = io.pred ? io.pred[2 * mb + 1] : 0;
  ref += (size_t)f * ref_frame_stride;
  cur += (size_t)f * cur_frame_stride;

  // the lane's partition: it exists iff its cell is inside its grid
  const int lane = threadIdx.x & 63, pl = min(lane, P_N - 1);
  const int pg = pq_grid(pl), quads = pq_quads(pl);
  // (its grid's arrays are picked here, into the lane's registers: the nine
  // records leave in one store each, and the loops below keep no pointer table)
  int gnx = 0, gny = 0;
  const int16_t* gin = nullptr;
  int16_t* omv = nullptr;
  uint32_t *ocost = nullptr, *odist = nullptr;
  uint8_t* obits = nullptr;
#pragma unroll
  for (int g = 0; g < 4; g++) {
    if (g == pg) {
      gnx = io.nx[g], gny = io.ny[g], gin = io.in[g];
      omv = io.mv[g], ocost = io.cost[g], odist = io.dist[g], obits = io.bits[g];
    }
  }
  const int cxp = (pg >= 2 ? 2 : 1) * bx + pq_i(pl), cyp = (pg & 1 ? 2 : 1) * by + pq_j(pl);
  const bool exists = lane < P_N && cxp < gnx && cyp < gny;
  const size_t at = (size_t)f * gnx * gny + (size_t)cyp * gnx + cxp;
  const int vx = exists ? gin[2 * at] : 0, vy = exists ? gin[2 * at + 1] : 0;
  const uint32_t exist = (uint32_t)__ballot(exists);

  QpelPix<TB> P;
  qpel_pixels<TB>(P, cur + (size_t)y0 * stride + x0, stride, bw, bh);
  // the lane's quarter, from its nominal position: a lane below a clipped
  // macroblock's last row holds no pixels (P puts it at the origin) but, under
  // SATD, a share of the partial tile above it
  const int qi = ((int)threadIdx.x / G::GW >= h ? 2 : 0) + ((int)threadIdx.x % G::GW * 4 >= h ? 1 : 0);
  const uint32_t cc_all =
      COST == ME_COST_SSD ? __builtin_amdgcn_udot4(P.cur[0], P.cur[0], 0u, false) : 0u;

  uint32_t best = 0, dist = 0;
  int c1 = 4;          // raster index of the stage-1 winner (4: the centre)
  int fx = 0, fy = 0;  // quarter offset of the best candidate from 4 * m

#pragma unroll 1
  for (int g = 0; g < P_N; g++) {
    if (!(exist >> g & 1)) continue;
    // the partitions that hold partition g's vector; g leads them if it is the first
    const int gvx = __builtin_amdgcn_readlane(vx, g), gvy = __builtin_amdgcn_readlane(vy, g);
    const uint32_t members = (uint32_t)__ballot(exists && vx == gvx && vy == gvy);
    if (members & ((1u << g) - 1)) continue;
    const bool member = members >> pl & 1 && lane < P_N;

    // their bounding rectangle, clipped like the macroblock (the partitions
    // that contain the quarters TL, TR, BL, BR: 0x2B, 0x53, 0x8D, 0x115)
    const bool left = members & 0xAFu, top = members & 0x7Bu;       // TL or BL; TL or TR
    const bool right = members & 0x157u, bottom = members & 0x19Du;  // TR or BR; BL or BR
    const int rx = left ? 0 : h, ry = top ? 0 : h;
    const int rw = min(right ? TB : h, bw) - rx, rh = min(bottom ? TB : h, bh) - ry;
    const bool in = P.px0[0] >= rx && P.px0[0] < rx + rw && P.py[0] >= ry && P.py[0] < ry + rh;
    const int lx = in ? P.px0[0] - rx : 0, ly = in ? P.py[0] - ry : 0;
    const uint32_t lm = in ? P.mask[0] : 0, lc = in ? P.cur[0] : 0, lcc = in ? cc_all : 0;
    qpel_stage<TB>(s, ref, width, height, stride, x0 + rx + gvx, y0 + ry + gvy, rw, rh);
    qpel_half_grid<TB>(s, rw, rh);

    // the centre relative to the predictor, in quarter units
    const int ex = 4 * gvx - px, ey = 4 * gvy - py;
    uint32_t c9[9];
    {
      uint32_t rbx[3], rby[3];
#pragma unroll
      for (int i = 0; i < 3; i++) {
        rbx[i] = io.lambda * (uint32_t)rd_bits(ex + 2 * (i - 1));
        rby[i] = io.lambda * (uint32_t)rd_bits(ey + 2 * (i - 1));
      }
      part_qpel_costs<TB, COST, true>(s, lx, ly, lc, lm, lcc, qi, quads, 0, 0, 2, c9);
      uint32_t d = c9[4], b = d + rbx[1] + rby[1];
      int w = 4;
#pragma unroll
      for (int n = 0; n < 9; n++) {
        if (n == 4) continue;
        const uint32_t dn = c9[n], j = dn + rbx[n % 3] + rby[n / 3];
        if (j < b) b = j, d = dn, w = n;
      }
      if (member) {
        best = b, dist = d, c1 = w;
        fx = 2 * (w % 3 - 1), fy = 2 * (w / 3 - 1);
      }
    }

    // stage 2 on the same half grid, once per distinct carried centre
#pragma unroll 1
    for (int l = g; l < P_N; l++) {
      if (!(members >> l & 1)) continue;
      const int lc1 = __builtin_amdgcn_readlane(c1, l);
      const uint32_t same = (uint32_t)__ballot(member && c1 == lc1);
      if (same & ((1u << l) - 1)) continue;
      const int cx = 2 * (lc1 % 3 - 1), cy = 2 * (lc1 / 3 - 1);
      uint32_t rbx[3], rby[3];
#pragma unroll
      for (int i = 0; i < 3; i++) {
        rbx[i] = io.lambda * (uint32_t)rd_bits(ex + cx + i - 1);
        rby[i] = io.lambda * (uint32_t)rd_bits(ey + cy + i - 1);
      }
      part_qpel_costs<TB, COST, false>(s, lx, ly, lc, lm, lcc, qi, quads, cx, cy, 1, c9);
      const bool mine = member && c1 == lc1;
#pragma unroll
      for (int n = 0; n < 9; n++) {
        if (n == 4) continue;
        const uint32_t dn = c9[n], j = dn + rbx[n % 3] + rby[n / 3];
        if (mine && j < best) best = j, dist = dn, fx = cx + n % 3 - 1, fy = cy + n / 3 - 1;
      }
    }
  }

  if (threadIdx.x < P_N) {
    const int qx = 4 * vx + fx, qy = 4 * vy + fy;
    if (exists) {
      omv[2 * at] = (int16_t)qx;
      omv[2 * at + 1] = (int16_t)qy;
      if (ocost) ocost[at] = best;
      if (odist) odist[at] = dist;
      if (obits) obits[at] = (uint8_t)(rd_bits(qx - px) + rd_bits(qy - py));
    }
    // a missing partition's best is 0: it adds nothing
    uint32_t jp[P_N];
#pragma unroll
    for (int p = 0; p < P_N; p++) jp[p] = (uint32_t)__builtin_amdgcn_readlane((int)best, p);
    const uint32_t j0 = jp[P_FULL] + io.lambda, j1 = jp[P_TOP] + jp[P_BOT] + 3 * io.lambda;
    const uint32_t j2 = jp[P_LEFT] + jp[P_RIGHT] + 3 * io.lambda;
    const uint32_t j3 = jp[P_TL] + jp[P_TR] + jp[P_BL] + jp[P_BR] + 5 * io.lambda;
    uint32_t bj = j0;
    int mode = ME_PART_2Nx2N;
    if (j1 < bj) bj = j1, mode = ME_PART_2NxN;
    if (j2 < bj) bj = j2, mode = ME_PART_Nx2N;
    if (j3 < bj) bj = j3, mode = ME_PART_NxN;
    if (threadIdx.x == 0) {
      io.mode[mb] = (uint8_t)mode;
      if (io.mode_cost) io.mode_cost[mb] = bj;
    }
  }
}

int tile_of(int blk) { return blk <= 4 ? 4 : blk <= 8 ? 8 : blk <= 16 ? 16 : blk <= 32 ? 32 : 64; }

// cost: ME_COST_SSD, ME_COST_SAD or ME_COST_SATD (the callers reject the rest).
template <int TB>
void refine_tb(int cost, dim3 grid, hipStream_t stream, const FrameBatch& b, int nbx, int nblk,
               const int16_t* mv_in, int16_t* mv_out, uint32_t* cost_out) {
#define ME_QPEL_REFINE_K(COST)                                                                   \
  hipLaunchKernelGGL((me_qpel_refine_kernel<TB, COST>), grid, dim3(QpelGeom<TB>::NT), 0, stream, \
                     b.ref, b.ref_frame_stride, b.cur, b.cur_frame_stride, b.width, b.height,    \
                     b.stride, b.blk, nbx, nblk, mv_in, mv_out, cost_out)
  if (cost == ME_COST_SSD)
    ME_QPEL_REFINE_K(ME_COST_SSD);
  else if (cost == ME_COST_SATD)
    ME_QPEL_REFINE_K(ME_COST_SATD);
  else
    ME_QPEL_REFINE_K(ME_COST_SAD);
#undef ME_QPEL_REFINE_K
}

template <int TB>
void refine_rd_tb(int cost, dim3 grid, hipStream_t stream, const FrameBatch& b, int nbx, int nblk,
                  uint32_t lambda, const int16_t* pred, const int16_t* mv_in, int16_t* mv_out,
                  uint32_t* cost_out, uint32_t* dist_out) {
#define ME_QPEL_REFINE_RD_K(COST)                                                               \
  hipLaunchKernelGGL((me_qpel_refine_rd_kernel<TB, COST>), grid, dim3(QpelGeom<TB>::NT), 0,     \
                     stream, b.ref, b.ref_frame_stride, b.cur, b.cur_frame_stride, b.width,     \
                     b.height, b.stride, b.blk, nbx, nblk, lambda, pred, mv_in, mv_out,         \
                     cost_out, dist_out)
  if (cost == ME_COST_SSD)
    ME_QPEL_REFINE_RD_K(ME_COST_SSD);
  else if (cost == ME_COST_SATD)
    ME_QPEL_REFINE_RD_K(ME_COST_SATD);
  else
    ME_QPEL_REFINE_RD_K(ME_COST_SAD);
#undef ME_QPEL_REFINE_RD_K
}

}  // namespace

hipError_t launch_qpel_refine_rd(const FrameBatch& b, int cost, uint32_t lambda, const int16_t* pred,
                                 const int16_t* mv_in, int16_t* mv_out, uint32_t* cost_out,
                                 uint32_t* dist_out, hipStream_t stream) {
  const int nbx = (b.width + b.blk - 1) / b.blk, nblk = nbx * ((b.height + b.blk - 1) / b.blk);
  const dim3 grid((unsigned)nblk, (unsigned)b.n_frames);
#define ME_QPEL_REFINE_RD(TB)                                                                   \
  case TB:                                                                                      \
    refine_rd_tb<TB>(cost, grid, stream, b, nbx, nblk, lambda, pred, mv_in, mv_out, cost_out,   \
                     dist_out);                                                                 \
    break
  switch (tile_of(b.blk)) {
    ME_QPEL_REFINE_RD(4);
    ME_QPEL_REFINE_RD(8);
    ME_QPEL_REFINE_RD(16);
    ME_QPEL_REFINE_RD(32);
    ME_QPEL_REFINE_RD(64);
  }
#undef ME_QPEL_REFINE_RD
  return hipGetLastError();
}

hipError_t launch_qpel_refine(const FrameBatch& b, int cost, const int16_t* mv_in, int16_t* mv_out,
                              uint32_t* cost_out, hipStream_t stream) {
  const int nbx = (b.width + b.blk - 1) / b.blk, nblk = nbx * ((b.height + b.blk - 1) / b.blk);
  const dim3 grid((unsigned)nblk, (unsigned)b.n_frames);
#define ME_QPEL_REFINE(TB)                                                                      \
  case TB:                                                                                      \
    refine_tb<TB>(cost, grid, stream, b, nbx, nblk, mv_in, mv_out, cost_out);                   \
    break
  switch (tile_of(b.blk)) {
    ME_QPEL_REFINE(4);
    ME_QPEL_REFINE(8);
    ME_QPEL_REFINE(16);
    ME_QPEL_REFINE(32);
    ME_QPEL_REFINE(64);
  }
#undef ME_QPEL_REFINE
  return hipGetLastError();
}

hipError_t launch_qpel_compensate(const uint8_t* ref, const uint8_t* cur, int width, int height,
                                  int blk, const int16_t* mvq, uint8_t* out5, int write_planes,
                                  unsigned long long* stats, hipStream_t stream) {
  const int nbx = (width + blk - 1) / blk, nblk = nbx * ((height + blk - 1) / blk);
#define ME_QPEL_COMP(TB)                                                                        \
  case TB:                                                                                      \
    hipLaunchKernelGGL(me_qpel_compensate_kernel<TB>, dim3((unsigned)nblk),                     \
                       dim3(QpelGeom<TB>::NT), 0, stream, ref, cur, width, height, blk, nbx,    \
                       mvq, out5, write_planes, stats);                                         \
    break
  switch (tile_of(blk)) {
    ME_QPEL_COMP(4);
    ME_QPEL_COMP(8);
    ME_QPEL_COMP(16);
    ME_QPEL_COMP(32);
    ME_QPEL_COMP(64);
  }
#undef ME_QPEL_COMP
  return hipGetLastError();
}

hipError_t launch_bipred(const FrameBatch& b, const uint8_t* ref1, size_t ref1_frame_stride,
                         int cost, int refine, const int16_t* q0_in, const int16_t* q1_in,
                         int16_t* q0_out, int16_t* q1_out, uint8_t* mode_out, uint32_t* cost_out,
                         uint32_t* cost3_out, hipStream_t stream) {
  const int nbx = (b.width + b.blk - 1) / b.blk, nblk = nbx * ((b.height + b.blk - 1) / b.blk);
  const dim3 grid((unsigned)nblk, (unsigned)b.n_frames);
#define ME_BIPRED_K(TB, COST)                                                                   \
  hipLaunchKernelGGL((me_bipred_kernel<TB, COST>), grid, dim3(QpelGeom<TB>::NT), 0, stream,     \
                     b.ref, b.ref_frame_stride, ref1, ref1_frame_stride, b.cur,                 \
                     b.cur_frame_stride, b.width, b.height, b.stride, b.blk, nbx, nblk, refine, \
                     q0_in, q1_in, q0_out, q1_out, mode_out, cost_out, cost3_out)
#define ME_BIPRED(TB)                  \
  case TB:                             \
    if (cost == ME_COST_SSD)           \
      ME_BIPRED_K(TB, ME_COST_SSD);    \
    else if (cost == ME_COST_SATD)     \
      ME_BIPRED_K(TB, ME_COST_SATD);   \
    else                               \
      ME_BIPRED_K(TB, ME_COST_SAD);    \
    break
  switch (tile_of(b.blk)) {
    ME_BIPRED(4);
    ME_BIPRED(8);
    ME_BIPRED(16);
    ME_BIPRED(32);
    ME_BIPRED(64);
  }
#undef ME_BIPRED
#undef ME_BIPRED_K
  return hipGetLastError();
}

hipError_t launch_partition_qpel(const FrameBatch& b, int cost, uint32_t lambda,
                                 const int16_t* pred, const me_part_fields& in,
                                 const me_part_rd_fields& out, hipStream_t stream) {
  const int h = b.blk / 2;
  const int nbx = (b.width + b.blk - 1) / b.blk, nby = (b.height + b.blk - 1) / b.blk;
  const int nhx = (b.width + h - 1) / h, nhy = (b.height + h - 1) / h;
  const me_part_fields& f = out.f;
  const PartQpelIO io{{in.mv_2nx2n, in.mv_2nxn, in.mv_nx2n, in.mv_nxn},
                      {f.mv_2nx2n, f.mv_2nxn, f.mv_nx2n, f.mv_nxn},
                      {f.cost_2nx2n, f.cost_2nxn, f.cost_nx2n, f.cost_nxn},
                      {out.dist_2nx2n, out.dist_2nxn, out.dist_nx2n, out.dist_nxn},
                      {out.bits_2nx2n, out.bits_2nxn, out.bits_nx2n, out.bits_nxn},
                      f.mode,
                      f.mode_cost,
                      pred,
                      {nbx, nbx, nhx, nhx},
                      {nby, nhy, nby, nhy},
                      lambda};
  const dim3 grid((unsigned)(nbx * nby), (unsigned)b.n_frames);
#define ME_PART_QPEL_K(TB, COST)                                                              \
  hipLaunchKernelGGL((me_partition_qpel_kernel<TB, COST>), grid, dim3(QpelGeom<TB>::NT), 0,   \
                     stream, b.ref, b.ref_frame_stride, b.cur, b.cur_frame_stride, b.width,   \
                     b.height, b.stride, io)
#define ME_PART_QPEL(TB)               \
  case TB:                             \
    if (cost == ME_COST_SSD)           \
      ME_PART_QPEL_K(TB, ME_COST_SSD); \
    else if (cost == ME_COST_SATD)     \
      ME_PART_QPEL_K(TB, ME_COST_SATD);\
    else                               \
      ME_PART_QPEL_K(TB, ME_COST_SAD); \
    break
  switch (b.blk) {  // (the entry points admit 8, 16 and 32 only)
    ME_PART_QPEL(8);
    ME_PART_QPEL(16);
    ME_PART_QPEL(32);
    default:
      return hipErrorInvalidValue;
  }
#undef ME_PART_QPEL
#undef ME_PART_QPEL_K
  return hipGetLastError();
}

hipError_t launch_bipred_compensate(const uint8_t* ref0, const uint8_t* ref1, const uint8_t* cur,
                                    int width, int height, int blk, const int16_t* mv0,
                                    const int16_t* mv1, const uint8_t* mode, uint8_t* out5,
                                    int write_planes, unsigned long long* stats,
                                    hipStream_t stream) {
  const int nbx = (width + blk - 1) / blk, nblk = nbx * ((height + blk - 1) / blk);
#define ME_BIPRED_COMP(TB)                                                                      \
  case TB:                                                                                      \
    hipLaunchKernelGGL(me_bipred_compensate_kernel<TB>, dim3((unsigned)nblk),                   \
                       dim3(QpelGeom<TB>::NT), 0, stream, ref0, ref1, cur, width, height, blk,  \
                       nbx, mv0, mv1, mode, out5, write_planes, stats);                         \
    break
  switch (tile_of(blk)) {
    ME_BIPRED_COMP(4);
    ME_BIPRED_COMP(8);
    ME_BIPRED_COMP(16);
    ME_BIPRED_COMP(32);
    ME_BIPRED_COMP(64);
  }
#undef ME_BIPRED_COMP
  return hipGetLastError();
}

}  // namespace me
