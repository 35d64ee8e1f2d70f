// me_subpel.hip -- quarter-pel refinement of an integer MV field, sub-pel
// motion compensation, and the bi-predictive mode decision over two
// quarter-pel fields with its compensation (include/me.h "quarter-pel" and
// "bi-predictive"; DESIGN.md has the definitions and the LDS layouts).  No
// reference counterpart: the reference stops at integer vectors.
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
