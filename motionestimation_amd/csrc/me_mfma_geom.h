// me_mfma_geom.h -- the matrix-core SSD path's plan structs, the layout
// constants a kernel and its planner share (each defined here once), and the
// planners' interface (me_mfma_plan.cpp: host-only, pure).  Like me_geom.h,
// nothing here needs HIP: the kernels (me_mfma.hip, me_band.hip) and the CPU
// harnesses (oracle/mfma_plan_dump.cc, oracle/san_main.cc) include it as it
// stands.
#pragma once
#include <initializer_list>

#include "me_geom.h"

#ifdef __HIPCC__
#define ME_HD __host__ __device__
#else
#define ME_HD
#endif

// 8x8 tile kernel (me_mfma_ssd8_kernel): #ifndef defaults, so an A/B build
// that defines one reaches the kernel and its planner alike.
#ifndef ME_SSD8_KM
#define ME_SSD8_KM 3  // 8x8 chunk length L = 16 KM: 48 rows (8K +-128: 64 rows 7.12 ms, 48 6.95-7.0, 32 8.3)
#endif
#ifndef ME_SSD8_NT
#define ME_SSD8_NT 2  // 8x8: horizontally adjacent 4x4-block tiles per workgroup (1 or 2)
#endif
#ifndef ME_SSD8_WP
#define ME_SSD8_WP 80  // 8x8 window copy pitch: 4 x (L + 8 = 56) x 80 + S2 table (L + 1) x 256 = 30 KB at L = 48
#endif

namespace me {

// Equal-geometry SSD searches of one matrix-core launch pair (prepass + main
// kernel): frames of one size and the same block rows.  Job j's planes and
// records are its own, its prepass planes sit at scratch + j * scratch_stride.
// A single search is the one-job table of its own pointers.
struct MfmaJobs {
  int n;
  int wgs;                // main-kernel workgroups per job
  size_t scratch_stride;  // bytes between consecutive jobs' prepass planes
  const uint8_t* ref[MAX_JOBS];
  const uint8_t* cur[MAX_JOBS];
  int16_t* mv[MAX_JOBS];
  uint32_t* cost[MAX_JOBS];
};

// Matrix-core SSD path (me_mfma.hip): B = 16, full-height rows [row0, row0 +
// nrows) x full-width columns [0, nbx); 4x4-block tiles.  The planners fill
// every integer field and leave the five pointers null; the launchers bind
// them (me_mfma.hip): rp at the scratch, the S2 planes at (rp_bytes + 255) &
// ~255 (0 for 8x8, where rp_bytes == 0), s2h another s2h_off bytes on.
struct MfmaGeom {
  int row0, nrows, nbx;
  int tiles_x, tiles_y;
  int ngx;               // 64-position groups per tile
  int ngxw;              // groups per workgroup (16x16 tiles: 1 or 2, 4 waves each; 8x8: all, in turn)
  int km;                // candidate rows per chunk L = 13 + 16 km
  int bm, bm_wpr, bm_lp; // block-major kernel (16x16, S <= 192); workgroups per block row; window pitch
  int bmv;               // block-major kernel forming S2 itself (S <= 64): no prepass, no scratch
  int bmv_r;             // ... its block rows per workgroup (1 or 2)
  int lds;               // dynamic LDS bytes
  int hb, hb_row;        // partial bottom block row: height hb, block row index (-1: none)
  int ya0, rp_rows;      // frame rows [ya0, ya0 + rp_rows) of the prepass planes
  int rows_alloc;        // plane rows written (rp_rows + read slack)
  int pitch;             // row pitch of the planes (entries)
  int s2h_row0;          // first s2h row the kernel reads
  uint32_t rp_bytes, s2_bytes;  // buffer ranges (s2_bytes spans s2 and s2h)
  uint32_t s2h_off;      // byte offset of s2h from s2
  size_t scratch_bytes;
  int8_t* rp;            // ref ^ 0x80
  int* s2;               // 16x16 box sums of (ref - 127)^2
  int* s2h;              // hb x 16 box sums (partial bottom row only)
  unsigned long long* mkeys;  // per tile 16 merge keys (~0 between launches)
  uint32_t* mcnt;        // per tile arrival counters (0 between launches)
  // Band-walk kernel (me_band.hip, 16x16, the default for S <= 64): a
  // workgroup walks a strip of block columns down a segment of block rows,
  // forming each 16-row band's S2 once in LDS for every block row in flight.
  int bw;                // 1: this plan runs on it (full-height rows [row0, row0 + nrows))
  int bw_wpc, bw_ns;     // waves per block column (row classes), ring slots per wave
  int bw_nsw, bw_pw;     // searcher and producer waves per workgroup
  int bw_cols;           // block columns per strip (bw_nsw / bw_wpc)
  int bw_strips;         // strips per job
  int bw_seg_rows;       // block rows per workgroup (segment)
  int bw_segs;           // segments per job
  int bw_xt;             // per-XCD tail split (bw_cx CUs per XCD): workgroup decode in bw_item()
  int bw_cx;
  int bw_lp, bw_pp;      // window row pitch (bytes), P0 plane row pitch (ints)
  int bw_abl;            // tuning build only: ablation bits (ME_BW_ABL), 0 in the product
  int bw_hb;             // S2 planes of a partial bottom row run by the band-walk kernel (0: by bmv)
};

// ---- layout constants of the kernels of me_mfma.hip ----

// Steps between a row's last MFMA and its epilogue (the 16-register accumulator
// ring holds 13 + DLY rows); 2 and 3 measured slower (DESIGN.md, 8x8 blocks).
constexpr int MFMA_DLY = 1;

// me_mfma_bm16_kernel: the LDS bytes ahead of its two band windows
constexpr int BM_CREC = 48;   // cur row record: 16 zero bytes, the row (c ^ 0x7F), 16 zero bytes
constexpr int BM_HDR = 8 * 16 * BM_CREC + 8 * 8 + 8 * 4;  // records, keys, cc

// me_mfma_bmv_kernel<R>
constexpr int BMV_NP = 268;                // S2 / V plane row pitch (ints): 256 positions + 12 V; 67 * 4
constexpr int BMV_PLANE = 16 * BMV_NP * 4; // 17,152 bytes (>= the 6,144 of crec)
constexpr int BMV_LP = 288;
template <int R>
constexpr int bmv_lds() {
  return R * (8 * 8 + 8 * 4) + (R == 2 ? 2 : 1) * BMV_PLANE + 2 * 31 * BMV_LP;
}

// ---- the band-walk kernel's (me_band.hip) ----

constexpr int BW_CREC = 48;          // cur row record: 16 zero bytes, the row (c ^ 0x7F), 16 zero bytes
constexpr int BW_NSW = 12;           // searcher waves per workgroup (three per SIMD)
constexpr int BW_PW = 4;             // producer waves per workgroup (one per SIMD)
constexpr int BW_K = 8;              // band ring: the bands in flight (window + P0 plane each)
constexpr int BW_WIN_ROWS = 31;      // window rows of a band: 16 b .. 16 b + 30

// Producer -> searcher handshake per band slot (LDS): ready[k] = the band
// whose window and P0 plane slot k holds (published after they are written);
// done[k] = searcher waves finished with it (the producer of band b + K
// waits for all of them, then reuses the slot).
struct BwCtl {
  uint32_t trash[4];  // (16-byte aligned) the P0 store of producer lanes without an output
  int ready[BW_K];
  int done[BW_K];
  int hbready[BW_K];  // the partial row's plane of band lo_h + i formed
  int hbcnt[BW_K];    // the partial row's bands searched, per block column
};

// LDS layout (bytes): K windows | K P0 planes | crec (searchers) | staged cur
// rows (searchers) | keys | ctl
ME_HD constexpr int bw_win(int lp) { return BW_WIN_ROWS * lp; }
ME_HD inline int bw_lds_bytes(int lp, int pp, int ns, int nsw) {
  return BW_K * bw_win(lp) + BW_K * 16 * pp * 4 + nsw * 16 * BW_CREC + nsw * 256 + nsw * ns * 8 +
         (int)sizeof(BwCtl);
}
// the partial bottom row's extra LDS: its nhb S2 planes and a key per block
// column of the strip
ME_HD inline int bw_lds_hb_bytes(int pp, int ns, int nhb) {
  (void)ns;
  return nhb ? nhb * 16 * pp * 4 + BW_K * 8 : 0;  // its planes, a key per block column
}

// Per-XCD tail split (bw_xt, see bw_item in me_band.hip): of the nx strip
// items of an XCD of cx CUs, the first *main run whole; the last partial
// round's *kx are cut into *st segments of *L block rows.
ME_HD inline void bw_xcd_split(int nx, int cx, int rows, int* main, int* kx, int* st, int* L) {
  int k = nx % cx, s = 1;
  if (k) {
    s = cx / k < rows / 4 ? cx / k : rows / 4;
    if (s < 1) s = 1;
  }
  const int l = (rows + s - 1) / s;
  *kx = k;
  *L = l;
  *st = (rows + l - 1) / l;
  *main = nx - k;
}
// ... and its grid for `items` strip items (jobs x strips): 8 XCDs x the most
// workgroup slots one of them needs (XCD x owns items / 8 of them, or one more).
inline long bw_xt_grid(long items, int cx, int rows) {
  int wmax = 0;
  for (int nx : {(int)(items / 8), (int)((items + 7) / 8)}) {
    int mainx, kx, st, L;
    bw_xcd_split(nx, cx, rows, &mainx, &kx, &st, &L);
    if (mainx + kx * st > wmax) wmax = mainx + kx * st;
  }
  return 8L * wmax;
}

// ---- the planners (me_mfma_plan.cpp) ----
// Pure functions of the shape, the kernel path code (me_tuning.h:
// kernel_path()), the device's CU count and a Tuning; the wrappers of
// me_mfma.hip read those three once and pass them.

// What a matrix-core plan depends on.
struct MfmaShape {
  int width, height, stride, blk, range, cost;
  int row_begin, row_end;  // block rows
  int nbx;                 // block columns of the search (with a partial right one)
  int align;               // align_class(stride, ref, cur)
  size_t merge_tiles;      // tiles the caller's merge buffers cover (0: none)
};

// Tiles of a B = 16 search over s's block rows (the merge buffers' size).
size_t mfma_merge_tiles(const MfmaShape& s);
// The plan of one search; false: not applicable (the VALU kernels take it).
bool plan_mfma_ssd(const MfmaShape& s, int path, int cus, const Tuning& tu, MfmaGeom* g);
// Band-walk kernel: plan the full-height rows of s into g (g's common fields
// already set by plan_mfma_ssd) for `jobs` jobs per launch.
bool plan_bw(const MfmaShape& s, int cus, const Tuning& tu, MfmaGeom* g, int jobs);
// The band-walk plan g for `jobs` jobs per launch runs in one round of
// workgroups (every segment of every strip resident at once).
bool bw_one_round(const MfmaGeom& g, int jobs, int cus);
// Main-kernel workgroups per job: a block row each, or R rows each on the
// lean path (me_mfma_bmv_kernel<R>).
int wgs_per_job(const MfmaGeom& g);

// How n equal jobs of s's shape run given `scratch` bytes of scratch: in
// launches of `jobs` jobs on geometry g, job j's prepass planes at j * stride
// (0: no planes); jobs == 0: job by job, each on its single-search plan.
// `need` is the scratch that lets the batch run as planned with unlimited
// scratch, and never less than one search's (a batch whose planes are not
// aligned alike falls back to job by job).
struct MfmaBatch {
  MfmaGeom g;
  int jobs;
  size_t stride, need;
};
constexpr size_t MFMA_SCRATCH_UNLIMITED = ~(size_t)0;
bool plan_mfma_batch(const MfmaShape& s, int n, size_t scratch, int path, int cus, const Tuning& tu,
                     MfmaBatch* b);

}  // namespace me
