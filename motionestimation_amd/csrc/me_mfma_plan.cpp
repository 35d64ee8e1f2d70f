// me_mfma_plan.cpp -- launch planners of the matrix-core SSD kernels
// (me_mfma.hip, me_band.hip).  Host-only and pure: a plan is a function of an
// MfmaShape, the kernel path code, the device's CU count and a Tuning, so
// the CPU tests (oracle/mfma_plan_dump.cc, oracle/san_main.cc) call the
// planners without a GPU.  They fill the integer fields and byte offsets of
// an MfmaGeom and leave its pointers null (me_mfma.hip binds them).
#include <algorithm>

#include "me_mfma_geom.h"
#include "me_tuning.h"

namespace me {

using std::max;
using std::min;

size_t mfma_merge_tiles(const MfmaShape& p) {
  if (p.blk != 16 || p.width < p.blk) return 0;  // 8x8: no cross-workgroup merge
  const size_t tx = (size_t)((p.width / p.blk + 3) / 4);
  const size_t ty = (size_t)((p.row_end - p.row_begin + 3) / 4);
  return tx * ty;
}

// Block-major (me_mfma_bm16_kernel) or 4x4-block tiles (me_mfma_ssd16_kernel)?
// Block-major measured faster at every S (1080p, S = 2..103: tools/dbg/bm_sweep*.sh);
// the tile kernel remains for row pitches / cur pointers that are not 16-byte aligned.
static bool bm_auto(const MfmaShape& p) { return p.range <= 192; }

// The automatic path's choice for `jobs` frames of p's shape per launch:
// the band-walk kernel (lean: no prepass planes, ~1.0-1.3x the algorithmic
// HBM bytes against ~7x) when its plan runs in one round of workgroups or
// without splitting block rows into segments (each segment re-forms
// 2 ceil(S/16) bands around it).  A single 1080p frame is 8 segments of 9
// rows in one round: 37.5 against 37.8-38.8 us per call on the prepass pair;
// 4K +-64 (2 segments of 68 rows): 265.9 against 254 us, the price of ~18
// against ~122 MB of HBM traffic per search (profiles/r06h_ssd_ab.jsonl, one
// box).  The round-5 figure of 68.8 us was the partial bottom row's second
// launch, now searched inside the walk.
// ME_PATH_MFMA_LEAN (force) takes the band-walk kernel whenever it applies.
// g holds the block-major plan on entry and the band-walk plan on success.
static bool use_bw(const MfmaShape& p, int cus, const Tuning& tu, MfmaGeom* g, int jobs,
                   bool force = false) {
  if (!g->bm) return false;
  MfmaGeom t = *g;
  t.bmv = 0;
  if (!plan_bw(p, cus, tu, &t, jobs) || (!force && t.bw_segs != 1 && !bw_one_round(t, jobs, cus)))
    return false;
  *g = t;
  g->bmv_r = 1;
  g->scratch_bytes = 0;
  return true;
}

// 8x8 blocks: full-height block rows only (a partial bottom row goes to the
// VALU kernels), one workgroup per 4x4-block tile walking its 64-column groups,
// chunks of 16 ME_SSD8_KM rows.
static bool plan_mfma_ssd8(const MfmaShape& p, MfmaGeom* g) {
  const int S = p.range, W = p.width, H = p.height;
  if (S < 1 || W < 8 || H < 8) return false;
  if (!(p.align & ALIGN_4)) return false;
  const int nby = (H + 7) / 8;
  const int r0 = p.row_begin;
  int r1 = p.row_end;
  if (r1 == nby && H % 8) r1--;
  g->row0 = r0;
  g->nrows = r1 - r0;
  if (g->nrows <= 0) return false;
  g->hb = 8;
  g->hb_row = -1;
  g->bmv_r = 1;
  g->nbx = W / 8;
  g->tiles_x = (g->nbx + 3) / 4;
  g->tiles_y = (g->nrows + 3) / 4;
  const int nxmax = min(24 + 2 * S + 1, W - 7);
  g->ngx = (nxmax + 63) / 64;
  g->ngxw = g->ngx;  // one workgroup walks all of a tile's groups
  g->km = ME_SSD8_KM;  // L = 16 km candidate rows per chunk
  const int L = 16 * g->km;
  // 4 copies + keys + S2 table + the words after each copy granule: 31.9 KB (two tiles), 5 workgroups per CU
  g->lds = 4 * (L + 8) * ME_SSD8_WP + 16 * ME_SSD8_NT * 12 + (L + 1) * 256 + (L + 8) * (ME_SSD8_WP / 16) * 4;
  g->ya0 = max(r0 * 8 - S, 0);
  const int ya1 = min(r1 * 8 + S, H);
  g->rp_rows = ya1 - g->ya0;
  g->pitch = (W + 15) & ~15;
  g->rows_alloc = g->rp_rows + 80;
  g->s2h_row0 = 0;
  // S2 plane only: the kernel stages the reference rows itself (no r ^ 0x80 plane)
  const size_t plane = (size_t)g->rows_alloc * g->pitch;
  const size_t s2_plane = plane * 4;
  if (s2_plane >= (1ull << 31)) return false;
  g->rp_bytes = 0;
  g->s2_bytes = (uint32_t)s2_plane;
  g->s2h_off = 0;
  g->scratch_bytes = s2_plane;
  return true;
}

// Full-height block rows [row0, row0 + nrows) and full-width columns of a B = 16
// SSD search; the caller routes partial rows / columns to the VALU kernels.
bool plan_mfma_ssd(const MfmaShape& p, int path, int cus, const Tuning& tu, MfmaGeom* g) {
  *g = MfmaGeom{};
  if (p.cost != COST_SSD || path == 1) return false;  // (path 1: the VALU kernels only)
  if (p.blk == 8) return plan_mfma_ssd8(p, g);
  if (p.blk != 16) return false;
  const int S = p.range, W = p.width, H = p.height;
  if (S < 1 || W < 16 || H < 16) return false;
  if (!(p.align & ALIGN_4)) return false;
  // block-major kernel for S <= 192 (ME_MFMA_BM=0|1: tuning build override)
  const int force_bm = tu.mfma_bm;
  g->bm = S <= 192 && path != 2 && (force_bm == 1 || (force_bm == 2 && bm_auto(p)));
  // window row pitch: a workgroup's 8 blocks span 16 (tc1 - tc0) + 32 <= 16 (S / 8 + 8) + 32
  // bytes (<= 544 up to S = 192)
  g->bm_lp = S <= 64 ? 288 : 544;
  if (g->bm && (p.stride % 16 || !(p.align & ALIGN_CUR16))) g->bm = 0;  // 16-byte cur row loads
  const int nxmax = min(48 + 2 * S + 1, W - 15);
  const int ngx = (nxmax + 63) / 64;
  if (ngx > 4 && !g->bm) return false;  // S > 103: the VALU kernels take it
  const int nby = (H + 15) / 16;
  const int r0 = p.row_begin, r1 = p.row_end;
  g->row0 = r0;
  g->nrows = r1 - r0;
  if (g->nrows <= 0) return false;
  // partial bottom block row (height hb): its lanes read the hb-row S2 plane
  g->hb = H - 16 * (nby - 1);
  g->hb_row = (g->hb < 16 && r1 == nby) ? nby - 1 : -1;
  if (g->hb_row < 0) g->hb = 16;
  g->nbx = W / 16;
  g->tiles_x = (g->nbx + 3) / 4;
  g->tiles_y = (g->nrows + 3) / 4;
  g->ngx = ngx;
  // chunk rows L = P0 + 16 KM: fewest (chunks x (L + P0)) steps on an interior tile
  const int ny = min(48 + 2 * S + 1, H - 15);
  int best = 1 << 30;
  const int force_km = tu.mfma_km;  // ME_MFMA_KM=2|3: tuning build override
  for (int km = 2; km <= 3; km++) {  // km = 1 spills (its lone main-loop pass gets peeled)
    if (force_km && km != force_km) continue;
    const int L = 12 + MFMA_DLY + 16 * km, ch = (ny + L - 1) / L;
    const int cost = ch * (L + 12 + MFMA_DLY);
    if (cost < best) { best = cost; g->km = km; }
  }
  const int L = 12 + MFMA_DLY + 16 * g->km;
  // groups per workgroup: two when the tile needs an even number of groups
  // (whole tiles at 1080p +-32: no merge), else one (4K +-64: 3 workgroups)
  g->ngxw = ngx % 2 == 0 ? 2 : 1;
  if (tu.mfma_ngxw) g->ngxw = tu.mfma_ngxw;  // ME_MFMA_NGXW: tuning build
  if (!g->bm && (ngx + g->ngxw - 1) / g->ngxw > 1 && p.merge_tiles < mfma_merge_tiles(p))
    return false;  // tiles span workgroups: needs the merge buffers
  g->lds = 4 * (L + 15) * (64 * g->ngxw + 32) + 16 * 8 + 16 * 4 + L * 256 * g->ngxw;
  g->bm_wpr = (g->nbx + 7) / 8;
  if (g->bm) g->lds = BM_HDR + 2 * 31 * g->bm_lp;
  // ME_PATH_MFMA_LEAN, S <= 64 (window pitch 288): S2 formed in the workgroup,
  // no prepass planes (ME_MFMA_S2K=0|1 overrides; tuning build)
  const int s2k = tu.mfma_s2k >= 0 ? tu.mfma_s2k : path == 3;
  g->bmv = g->bm && g->bm_lp == BMV_LP && s2k;
  // block rows per workgroup (ME_MFMA_S2R=1|2 overrides; tuning build).  Two
  // rows share each band's S2 (6 bands for two rows at S = 32 instead of
  // 5 + 5; 10 instead of 9 + 9 at S = 64) but synchronise 8 waves per barrier
  // and leave a row idle in the other row's end bands: 16-frame batches, 1080p
  // +-32 35.9 us per frame against 33.8 with one row, 4K +-64 289 against 323
  // (profiles/r04f_ssd_ab.jsonl).  Two rows from S = 48 on.
  g->bmv_r = tu.mfma_s2r > 0 ? tu.mfma_s2r : (S >= 48 ? 2 : 1);
  if (g->bmv) g->lds = g->bmv_r == 2 ? bmv_lds<2>() : bmv_lds<1>();
  g->ya0 = max(r0 * 16 - S, 0);
  const int ya1 = min(r1 * 16 + S, H);
  g->rp_rows = ya1 - g->ya0;
  g->pitch = (W + 15) & ~15;
  // + 80 rows of slack: the last chunk of a tile reads (masked) window rows and
  // S2 entries up to L + 15 rows past the planes' last row.
  // (the block-major kernel reads at most 15 rows past them, and its buffer
  // loads are range-checked: 16 rows of slack)
  g->rows_alloc = g->rp_rows + (g->bm ? 16 : 80);
  // the last tile row's candidate rows start here (its lanes of the partial
  // block row read s2h from there on)
  const int tly_last = 16 * (r0 + 4 * (g->tiles_y - 1));
  g->s2h_row0 = max(tly_last - S, 0) - g->ya0;
  const size_t plane = (size_t)g->rows_alloc * g->pitch;
  const size_t rp_alloc = (plane + 255) & ~(size_t)255;
  const size_t s2_plane = plane * 4;
  const size_t n_s2 = g->hb < 16 ? 2 : 1;
  if (rp_alloc + n_s2 * s2_plane >= (1ull << 31)) return false;
  g->rp_bytes = (uint32_t)plane;
  g->s2_bytes = (uint32_t)(n_s2 * s2_plane);
  g->s2h_off = (uint32_t)s2_plane;
  g->scratch_bytes = rp_alloc + n_s2 * s2_plane;
  // Automatic path, S <= 64: the band-walk kernel (me_band.hip) for the
  // full-height rows, me_mfma_bmv_kernel for a partial bottom row, neither
  // with scratch, when the frame's strips fill the CUs by themselves
  // (use_bw); ME_PATH_MFMA_PREPASS keeps the prepass + block-major pair.
  if (path == 0 || path == 3) use_bw(p, cus, tu, g, 1, path == 3);
  if (g->bmv) g->scratch_bytes = 0;  // no planes: the kernel reads the reference plane
  return true;
}

int wgs_per_job(const MfmaGeom& g) {
  return g.bmv ? (g.nrows + g.bmv_r - 1) / g.bmv_r * g.bm_wpr : g.nrows * g.bm_wpr;
}

// Smallest pitch >= need with pitch = r (mod m): the conflict-free classes of
// the tiles' ds_read_b128 lane groups (window LP = 32 mod 64 bytes, P0 PP = 8
// mod 16 ints; checked for every group of 16 lanes).
static int pitch_at_least(int need, int r, int m) {
  int p = need + ((r - need) % m + m) % m;
  return p;
}

bool plan_bw(const MfmaShape& p, int cu_count, const Tuning& tu, MfmaGeom* g, int jobs) {
  const int S = p.range;
  g->bw = 0;
  if (p.blk != 16 || S < 1 || S > 64 || tu.bw == 0) return false;
  if (p.stride % 16 || !(p.align & ALIGN_CUR16)) return false;  // 16-byte cur row loads
  const int rows = g->nrows - (g->hb_row >= 0 ? 1 : 0);         // full-height rows
  if (rows < 1 || g->nbx < 1) return false;
  // Two ring slots per searcher wave (A fragments of 2 rows: 64 VGPRs): the
  // 2 ceil(S/16) + 1 rows in flight of a column split over 12 / C searchers,
  // the widest strip whose column fits its rows: S <= 16: 6 columns (3 rows
  // on 4 slots); S <= 32: 4 (5 on 6); S <= 48: 3 (7 on 8); S <= 64: 2 (9 on
  // 12).  One workgroup of 12 searchers + 4 producers per CU (four waves per
  // SIMD at <= 128 VGPRs).
  const int nsw = BW_NSW, npw = BW_PW, ns = 2, wgs_cu = 1;
  const int inflight = 2 * ((S + 15) / 16) + 1;
  int C = 0;
  for (int c : {6, 4, 3, 2, 1})
    if (nsw % c == 0 && (nsw / c) * ns >= inflight) {
      C = c;
      break;
    }
  if (C == 0) return false;
  const int npos_max = 16 * ((16 * (C - 1) + 2 * S) / 16 + 2);
  const int lp = npos_max + 16 <= 160 ? 160 : 224;
  if (npos_max + 16 > lp || npos_max / 4 > 52) return false;  // 4 lane rows x 13 output groups
  const int pp = pitch_at_least(npos_max, 8, 16);
  g->bw_wpc = nsw / C;
  g->bw_ns = ns;
  g->bw_nsw = nsw;
  g->bw_pw = npw;
  g->bw_cols = C;
  g->bw_lp = lp;
  g->bw_pp = pp;
  g->bw_strips = (g->nbx + C - 1) / C;
  // Segments: rounds of resident workgroups x (the most bands one segment
  // walks + ~2 bands of prologue), the smallest.  A segment of rows [r0, r1)
  // walks bands lo(r0) .. hi(r1 - 1); even splits, the last segment the
  // rest.  (Uneven splits -- a longer first segment, which walks ceil(S/16)
  // fewer bands, the partial row's segment shorter -- measured 1.5 % slower
  // at 1080p: profiles/r06g_bw_ab.jsonl; longer first and last segments with
  // shorter middle ones, 12 bands worst instead of 13 at 1080p one frame,
  // 1.5 % slower again: 38.6 against 38.0 us per call, r06zl_bw_seg.jsonl.
  // The segments' band counts do not set the time alone.)
  const int cus = cu_count * wgs_cu;
  const int nfull = g->row0 + rows;  // (rows from row0: the job's full-height rows)
  auto lo_b = [&](int br) { return max(16 * br - S, 0) >> 4; };
  auto hi_b = [&](int br) { return min(16 * br + S, p.height - 16) >> 4; };
  const long per = (long)max(jobs, 1) * g->bw_strips;
  long best_t = 1L << 40;
  int best_l = rows, best_segs = 1;
  for (int segs = 1; segs <= max(1, rows / 4); segs++) {
    const int L = (rows + segs - 1) / segs;
    if ((rows + L - 1) / L != segs) continue;  // (an empty last segment)
    const long rounds = (per * segs + cus - 1) / cus;
    int worst = 0;  // bands of the longest segment
    for (int r0 = g->row0; r0 < nfull; r0 += L)
      worst = max(worst, hi_b(min(r0 + L, nfull) - 1) - lo_b(r0) + 1);
    const long t = rounds * (worst + 2);
    if (t < best_t) {
      best_t = t;
      best_l = L;
      best_segs = segs;
    }
  }
  if (tu.bw_seg > 0) {
    best_l = min(rows, tu.bw_seg);
    best_segs = (rows + best_l - 1) / best_l;
  }
  g->bw_seg_rows = best_l;
  g->bw_abl = tu.bw_abl;
  g->bw_segs = best_segs;
  // Launches of whole rounds of strips take the per-XCD tail split instead.
  g->bw_xt = 0;
  g->bw_cx = cu_count / 8;
  if (tu.bw_xt != 0 && tu.bw_seg == 0 && per >= cus && g->bw_cx > 0) {
    g->bw_xt = 1;
    g->bw_seg_rows = rows;
    g->bw_segs = 1;
  }
  g->lds = bw_lds_bytes(lp, pp, ns, nsw);
  if (g->lds > 160 * 1024 / wgs_cu) return false;
  // A partial bottom block row (rows H - hb .. H - 1) joins the walk when its
  // hb-row S2 planes fit in LDS beside the ring: one per band it meets, bands
  // lo .. hb_row (its last candidate row is H - hb = 16 hb_row); otherwise it
  // is a second launch of the lean kernel (launch_bw_jobs).
  g->bw_hb = 0;
  if (g->hb_row >= 0 && tu.bw_hb != 0) {
    const int nhb = g->hb_row - (max(16 * g->hb_row - S, 0) >> 4) + 1;
    const int lds_hb = g->lds + bw_lds_hb_bytes(pp, ns, nhb);
    if (lds_hb <= 160 * 1024 / wgs_cu) {
      g->bw_hb = nhb;
      g->lds = lds_hb;
    }
  }
  g->bw = 1;
  return true;
}

bool bw_one_round(const MfmaGeom& g, int jobs, int cus) {
  return (long)max(jobs, 1) * g.bw_strips * g.bw_segs <= (long)cus;
}

// ------------------------------------------------------------------ batches
// A batch of frames with one geometry shares one prepass launch and one
// block-major launch: a 1080p search is one round of workgroups per CU, so a
// launch per frame pays the grid's fill and drain every frame.
static constexpr size_t MFMA_BATCH_SCRATCH = (size_t)1 << 30;  // prepass planes per launch

bool plan_mfma_batch(const MfmaShape& p, int n, size_t scratch, int path, int cus, const Tuning& tu,
                     MfmaBatch* b) {
  b->jobs = 0;
  b->stride = b->need = 0;
  MfmaGeom& g = b->g;
  if (!plan_mfma_ssd(p, path, cus, tu, &g)) return false;
  // job by job, each on its own single-search plan, also when a job's planes
  // turn out not to be aligned like job 0's (the launcher's check): the
  // scratch always holds one search's prepass planes
  b->need = g.scratch_bytes;
  // (a partial right column: job by job; not the block-major kernel: no batches)
  if (n < 2 || tu.mfma_batch == 0 || g.nbx < p.nbx || !g.bm) return true;
  const int nj = min(n, MAX_JOBS);
  // a launch of several frames may fill the CUs where one frame does not; a
  // band-walk plan keeps the kernel, its segments sized for nj jobs per launch
  if (g.bw)
    plan_bw(p, cus, tu, &g, nj);
  else if (path == 0)
    use_bw(p, cus, tu, &g, nj);
  if (g.bmv || g.bw) {  // no prepass planes
    b->jobs = nj;
    return true;
  }
  // as many jobs' planes per launch as the cap allows, then as the scratch holds
  const size_t stride = (g.scratch_bytes + 255) & ~(size_t)255;
  const size_t cap = min(MFMA_BATCH_SCRATCH / stride, (size_t)nj);
  if (cap < 2) return true;  // (one job's planes alone exceed the cap)
  b->need = max(b->need, cap * stride);
  const size_t m = min(cap, scratch / stride);
  if (m >= 2) {
    b->jobs = (int)m;
    b->stride = stride;
  }
  return true;
}

}  // namespace me
