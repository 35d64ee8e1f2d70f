// me_geom.h -- search geometry shared by the kernels and the host-only
// planners (internal to libme_hip.so).  Plain structs and integer helpers:
// nothing here needs HIP, so me_valu_plan.cpp and the CPU harnesses
// (oracle/plan_dump.cc, oracle/san_main.cc) include it as it stands.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace me {

enum { COST_SSD = 0, COST_SAD = 1, COST_SSIM = 2 };

constexpr int GENERIC_THREADS = 256;
constexpr int GENERIC_LDS_BUDGET = 60 * 1024;
constexpr int QSAD_LDS_BUDGET = 40 * 1024;  // 4 workgroups per CU (160 KB LDS)
constexpr int FLOW_LDS_BUDGET = 160 * 1024;  // the flow kernel: one workgroup per CU

// One search launch: block rows [block_row_begin, block_row_end) of a
// width x height frame.  ref / cur point at frame rows ref_row0 / cur_row0.
// Outputs are indexed (block row - block_row_begin) * nbx + block column.
struct SearchArgs {
  const uint8_t* ref;
  const uint8_t* cur;
  int ref_row0, cur_row0;
  int width, height, stride;
  int blk, range;
  int nbx;
  int block_row_begin, block_row_end;
  int cost_kind;
  int16_t* mv;
  uint32_t* cost;
  uint32_t ref_bytes;  // readable bytes from ref (buffer range check), and from cur
  uint32_t cur_bytes;
  uint32_t* sched;     // SCHED_WORDS u32 (me_kernels.h), zeroed between launches; or null
  uint8_t* scratch;    // device scratch of the MFMA SSD path (mfma_ssd_scratch bytes) or null
  size_t scratch_bytes;
  // MFMA SSD cross-workgroup merge (self-resetting): 16 keys (~0) per tile and
  // one arrival counter (0) per tile, merge_tiles tiles; or null
  unsigned long long* mkeys;
  uint32_t* mcnt;
  size_t merge_tiles;
};

// Bytes the kernels may read from a plane that holds frame rows from row0 on,
// for a search of block rows up to r1 (the DMA descriptors' range): the rows
// the stripe contract guarantees resident (include/me.h).  The ref plane's
// rows end S past the last block row, both at the frame's height.
inline uint32_t resident_bytes(int rows_end, int row0, int stride, int width) {
  const long rows = rows_end - row0;
  return rows > 0 ? (uint32_t)((rows - 1) * (long)stride + width) : 0;
}
inline uint32_t ref_resident_bytes(int r1, int blk, int range, int height, int row0, int stride,
                                   int width) {
  const int end = r1 * blk + range < height ? r1 * blk + range : height;
  return resident_bytes(end, row0, stride, width);
}
inline uint32_t cur_resident_bytes(int r1, int blk, int height, int row0, int stride, int width) {
  const int end = r1 * blk < height ? r1 * blk : height;
  return resident_bytes(end, row0, stride, width);
}

struct QsadGeom {
  int tb;          // blocks per workgroup
  int rows_alloc;  // LDS tile rows (chunks*K + B - 1)
  int row0;        // first block row of the launch
  int nrows;       // block rows in the launch
  int groups;      // 4-wide dx groups per block
  int chunks;      // K-row dy chunks
  int cpp;         // dy chunks per LDS pass
  int pitch;       // bytes per LDS tile row (multiple of 16)
  int tile_bytes;  // rows_alloc * pitch
  uint32_t pitch_magic;  // umulhi(d, pitch_magic) == d / pitch on the staged range
  uint32_t magic_groups; // umulhi(t, magic_groups) == t / groups on an item's tasks
  int threads;     // workgroup size
  int lds;         // dynamic LDS bytes
  int wg_per_row;  // workgroups per block row
  uint32_t magic_wpr;  // umulhi(t, magic_wpr) == t / wg_per_row for every tile index of
                       // the planned rows (host-checked; 0: divide)
  uint32_t magic_tb;   // 0xFFFFFFFF / tb + 1: an item's / nb magic when nb == tb > 1
  int strip_w;     // > 0: tiles run in vertical strips of strip_w tile columns, each
                   // strip top to bottom (wide frames: an XCD's L2 keeps the strip's
                   // window rows while the tile rows that read them pass)
  int nbx_full;    // full-width blocks per row
  int aligned;     // 4-byte aligned global rows and W % 4 == 0: staged by LDS DMA
  int tile16;      // ref tile staged in 16-byte granules (X0, width, rows 16-byte aligned)
  int fold;        // SAD, S % 4 == 0: groups = S/2 cover dx in [-S, S-1]; the dx = +S
                   // column is spread over lanes gi < K, one v_sad_u8 candidate each
  int dyn_tiles;   // dynamic tile pulls when tiles >= dyn_tiles * workgroups (0: never)
  int pull_ahead;  // dynamic: tile ti + pull_ahead is claimed when tile ti starts (1 or 2)
  int flow_slots;  // me_flow_kernel: LDS ring slots (0: the persistent item kernel)
  int prio;        // waves issuing staging raise their issue priority (s_setprio) meanwhile
  int fair;        // me_flow_kernel: lo | hi << 8 | mode << 16 (0: off): a wave whose
                   // wave-task others have overtaken by >= lo / hi pulls raises its
                   // issue priority to 1 / 2 (checked every 4 rows; 8 / 16 by
                   // default) in launches with slot refills (mode 1)
  // me_flow_kernel, candidate pruning by the exact sub-block bound (0: every
  // lane-task runs, the ring is flow_slots slots in lds bytes):
  int prune;         // 1: on; 2: verify (every lane-task runs, a wrongly dead one is reported)
  int prune_bypass;  // 1: after a run of items the bound could not thin, skip it and re-probe
  int prune_stats;   // 1: live / total lane-tasks and bypassed items counted in sched[SCHED_PRUNE..]; 2 (set by the
                     // launch): and the launch's LDS ends with FLOW_HIST_BYTES for the wave-task histogram
  int prune_slots;   // ring slots when pruning without box-sum planes (each slot carries FLOW_PRUNE_BYTES of bound scratch)
  int prune_lds;     // dynamic LDS bytes of that launch
  int prune_split;   // 1: a pruned item's short wave-task is split by dy rows (flow_split_* below); 2: by the earlier rule
  // The pruning launch WITH box-sum planes (FlowJobs::planes): its bound reads
  // the planes from global memory, a slot carries FLOW_SLIM_BYTES of scratch
  // (0 slots: the shape's plane loads could straddle a phase row, no such launch).
  int slim_slots;    // ring slots
  int slim_lds;      // dynamic LDS bytes
};

// ---- row split of a pruned item's partial wave-task (me_flow_kernel) ----
// A wave-task holding n <= 32 list entries runs with P lanes per entry, each
// taking R of the dy rows of the entry's K = 13 row chunk.  The wave's 64 lanes
// allow min(13, 64 / n) parts, so a lane needs ceil(13 / that) rows; the kernel
// has an instance for R = 1, 2, 3, 4 and 7 (and the whole task, 13), so the 5
// rows that n = 17 .. 21 could do with become 7:
//   n       1..4  5..9  10..12  13..16  17..32  33..64
//   R          1     2       3       4       7      13
//   P         13     7       5       4       2       1
// P = ceil(13 / R) depends on R alone (more parts would only repeat rows): lane
// l takes entry l / P and part i = l % P, the rows [row0, row0 + R) with row0 =
// min(i R, 13 - R).  The last part overlaps the one in front where R does not
// divide 13: that saves the row masks of an exact partition, and a candidate
// computed twice gives the same key.  Lanes from n P on repeat entry n - 1 and
// merge nothing.  The fold column's candidate belongs to part 0.
constexpr int FLOW_SPLIT_K = 13;
constexpr int flow_split_rows(int n) {  // (a compare chain: the kernel evaluates it per wave-task)
  return n <= 4 ? 1 : n <= 9 ? 2 : n <= 12 ? 3 : n <= 16 ? 4 : n <= 32 ? 7 : FLOW_SPLIT_K;
}
constexpr int flow_split_parts_of(int R) { return (FLOW_SPLIT_K + R - 1) / R; }
constexpr int flow_split_parts(int n) { return flow_split_parts_of(flow_split_rows(n)); }
constexpr int flow_split_row0(int R, int i) { return i * R < FLOW_SPLIT_K - R ? i * R : FLOW_SPLIT_K - R; }
// Lane `lane` of a task of n entries run with R rows per lane (R a constant of
// the caller's instance: the division compiles to a multiply and a shift).
struct FlowSplitLane {
  int entry;  // list entry of the task, 0 .. n - 1
  int row0;   // first of the lane's R rows of the chunk
  bool live;  // the lane has an entry of its own: it merges its key
  bool fold;  // ... and the fold column's candidate of the entry
};
constexpr FlowSplitLane flow_split_lane(int R, int lane, int n) {
  const int P = flow_split_parts_of(R);
  const int e = (int)((unsigned)lane / (unsigned)P), part = lane - e * P;
  return FlowSplitLane{e < n ? e : n - 1, flow_split_row0(R, part), e < n, e < n && part == 0};
}
// The rule before the 13-way split (1, 2 or 4 lanes per entry): the tuning
// build's ME_PRUNE_SPLIT=2 runs it from the same kernels.
constexpr int flow_split_rows_124(int n) { return n <= 16 ? 4 : n <= 32 ? 7 : FLOW_SPLIT_K; }
constexpr bool flow_split_instance(int R) { return R == 1 || R == 2 || R == 3 || R == 4 || R == 7 || R == FLOW_SPLIT_K; }
constexpr bool flow_split_rule_holds() {  // the chain above is the rule stated in words
  for (int n = 1; n <= 64; n++) {
    const int room = 64 / n < FLOW_SPLIT_K ? 64 / n : FLOW_SPLIT_K;
    int R = (FLOW_SPLIT_K + room - 1) / room;
    while (!flow_split_instance(R)) R++;
    if (flow_split_rows(n) != R) return false;
  }
  return true;
}
constexpr bool flow_split_covers(int R) {  // the parts' union is rows 0..12, none past them
  unsigned m = 0;
  for (int s = 0; s < flow_split_parts_of(R); s++)
    for (int j = 0; j < R; j++) {
      if (flow_split_row0(R, s) + j >= FLOW_SPLIT_K) return false;
      m |= 1u << (flow_split_row0(R, s) + j);
    }
  return m == (1u << FLOW_SPLIT_K) - 1;
}
constexpr bool flow_split_fits() {  // every n has its P * n lanes in the wave, under either rule
  for (int n = 1; n <= 64; n++)
    if (n * flow_split_parts(n) > 64 || n * flow_split_parts_of(flow_split_rows_124(n)) > 64) return false;
  return true;
}
static_assert(flow_split_rule_holds(), "R = ceil(13 / min(13, 64 / n)), rounded up to an instance");
static_assert(flow_split_covers(1) && flow_split_covers(2) && flow_split_covers(3) && flow_split_covers(4) &&
                  flow_split_covers(7) && flow_split_covers(13),
              "parts cover rows 0..12");
static_assert(flow_split_fits(), "64 / P >= the largest n of P");

// Bound scratch of one ring slot of the pruning flow kernel: four x-phase
// planes of 77 rows x 32 box-sum bytes (the live list overlays them once the
// bound is done), minlb[5][4][16] u32 and the cur blocks' 4 x 16 box-sum bytes.
// Plane k, row r, byte i holds q of window position (r, 4 i + k), q = the 4x4
// box sum >> 4.  This is the layout of a launch WITHOUT box-sum planes in the
// context scratch: step 1 of flow_bound fills the slot's planes from the staged
// window.  A launch with them (the prepass me_box_planes_kernel wrote them once
// per reference plane) keeps no planes in the slot: FLOW_SLIM_* below.
constexpr int FLOW_PRUNE_QROWS = 77;
constexpr int FLOW_PRUNE_PLANE = FLOW_PRUNE_QROWS * 32;
constexpr int FLOW_PRUNE_MINLB = 4 * FLOW_PRUNE_PLANE;
constexpr int FLOW_PRUNE_QCUR = FLOW_PRUNE_MINLB + 320 * 4;
constexpr int FLOW_PRUNE_BYTES = FLOW_PRUNE_QCUR + 64;
constexpr int FLOW_CTL_BYTES = 256;  // the pruning launch's control block (FlowCtl)
constexpr int FLOW_HIST_BYTES = 256; // tuning build: 64 counters behind the control block and the item table
// The slim bound scratch of a launch with box-sum planes: the bound's step 2
// loads its plane rows from the job's planes in global memory into registers
// (flow_plane_byte below), so the slot keeps only what outlives the bound or
// is shared between its lanes: the live list (320 u16, verify: 320 flags at
// FLOW_PRUNE_DEAD and U_b[4] at FLOW_PRUNE_UB, the offsets both layouts use),
// minlb and the cur blocks' box sums.
constexpr int FLOW_PRUNE_DEAD = 640;
constexpr int FLOW_PRUNE_UB = 960;
constexpr int FLOW_SLIM_MINLB = 1024;
constexpr int FLOW_SLIM_QCUR = FLOW_SLIM_MINLB + 320 * 4;
constexpr int FLOW_SLIM_BYTES = FLOW_SLIM_QCUR + 64;
static_assert(FLOW_PRUNE_UB + 16 <= FLOW_SLIM_MINLB && FLOW_PRUNE_UB + 16 <= FLOW_PRUNE_MINLB,
              "list, verify flags and U_b lie in front of minlb in both layouts");
static_assert(FLOW_SLIM_BYTES == 2368 && FLOW_SLIM_BYTES % 16 == 0 && FLOW_PRUNE_BYTES % 16 == 0,
              "slots stay 16-byte aligned");
// The chain kernel's pre-bound marker, one word per slot in the free bytes
// between U_b and minlb of the slim scratch: whether minlb and the cur blocks'
// box sums of the slot's NEXT item (item + ring slots of the one published in
// it) are being formed, or stand, while the published item's tasks still run.
constexpr int FLOW_SLIM_MARK = FLOW_PRUNE_UB + 16;
static_assert(FLOW_SLIM_MARK >= 976 && FLOW_SLIM_MARK + 4 <= FLOW_SLIM_MINLB, "the marker lies in the gap 976 .. 1023");
constexpr uint32_t FLOW_MARK_NONE = 0;
constexpr uint32_t flow_mark_busy(int item) { return 2u * (uint32_t)(item + 1); }
constexpr uint32_t flow_mark_done(int item) { return 2u * (uint32_t)(item + 1) + 1u; }

// A search job: block rows [r0, r1) of one frame (or row stripe), its planes
// (ref / cur hold frame rows from ref_row0 / cur_row0, as in SearchArgs) and
// its records (indexed from r0).  Jobs of one launch share the frame geometry.
struct SearchJob {
  const uint8_t* ref;
  int ref_row0;
  const uint8_t* cur;
  int cur_row0;
  int r0, r1;
  int16_t* mv;
  uint32_t* cost;
};

// The single-job arguments of job J (geometry, cost and context buffers from
// base): the one place the resident bytes of a job are derived.
inline SearchArgs job_args(const SearchArgs& base, const SearchJob& J) {
  SearchArgs q = base;
  q.ref = J.ref;
  q.ref_row0 = J.ref_row0;
  q.cur = J.cur;
  q.cur_row0 = J.cur_row0;
  q.block_row_begin = J.r0;
  q.block_row_end = J.r1;
  q.mv = J.mv;
  q.cost = J.cost;
  q.ref_bytes = ref_resident_bytes(J.r1, base.blk, base.range, base.height, J.ref_row0, base.stride,
                                   base.width);
  q.cur_bytes = cur_resident_bytes(J.r1, base.blk, base.height, J.cur_row0, base.stride, base.width);
  return q;
}

// The flow kernel's job table (kernel argument): job j owns launch tiles
// [tile_pre[j], tile_pre[j + 1]).  A batch of frames or stripes (the per-rank
// step of a multi-GPU split) fills the GPU in one launch.
constexpr int MAX_JOBS = 32;
struct FlowJobs {
  int n;
  int tile_pre[MAX_JOBS + 1];
  int r0[MAX_JOBS];
  int ref_row0[MAX_JOBS], cur_row0[MAX_JOBS];
  uint32_t ref_bytes[MAX_JOBS], cur_bytes[MAX_JOBS];
  const uint8_t* ref[MAX_JOBS];
  const uint8_t* cur[MAX_JOBS];
  int16_t* mv[MAX_JOBS];
  uint32_t* cost[MAX_JOBS];
  // The pruning flow launch's box-sum planes (null: the kernel forms the box
  // sums itself): job j's at planes + 64 * plane_off64[j], plane_rows[j] rows
  // (its resident ref rows, from ref_row0) of 4 x plane_pitch bytes.
  uint8_t* planes;
  int plane_pitch;
  uint32_t plane_off64[MAX_JOBS];
  int plane_rows[MAX_JOBS];
};

// ---- launch tile -> job ----
// The rule: tile t belongs to the smallest j with tile_pre[j + 1] > t (a job
// without tiles owns none), clamped to [0, n - 1].  Two forms of it, neither
// with a trip count that grows with j (the kernels read the table from scalar
// memory: every step is a dependent round trip):
//   flow_job_from  the scan from a job j0 <= the tile's job.  A flow workgroup
//                  walks its band's tiles upwards, so the job of its previous
//                  item is such a j0 and the scan steps once per job boundary
//                  between the two tiles.  From j0 = 0 it is the plain scan.
//   flow_job_find  the bisection of the table (at most 5 steps for MAX_JOBS
//                  jobs) where no earlier job is known.
#if defined(__HIPCC__)
#define ME_HOST_DEVICE __host__ __device__
#else
#define ME_HOST_DEVICE
#endif
ME_HOST_DEVICE inline int flow_job_from(const FlowJobs& jb, int tile, int j0) {
  int j = j0;
  while (j + 1 < jb.n && jb.tile_pre[j + 1] <= tile) j++;
  return j;
}
// (the bisection over any copy of tile_pre: the item table's builders read one in LDS)
ME_HOST_DEVICE inline int flow_job_find_in(const int* tile_pre, int n, int tile) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (tile_pre[mid + 1] > tile) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}
// (written out, not through the pointer form: the kernels read jb from their arguments)
ME_HOST_DEVICE inline int flow_job_find(const FlowJobs& jb, int tile) {
  int lo = 0, hi = jb.n - 1;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (jb.tile_pre[mid + 1] > tile) hi = mid;
    else lo = mid + 1;
  }
  return lo;
}

// ---- the flow kernel's items (me_flow_kernel) ----
// Geometry of one work item = (tile of TB blocks, dy pass); j: the flow
// kernel's job (FlowJobs) the tile belongs to.
struct Item {
  int bx0, by, nb, tly, h, a, X0, c0, nch, prow0, prows, j;
};
// A workgroup's items: the XCD band of bid % 8 (a speed heuristic only), member
// m = bid / 8 takes tiles band0 + m, + n_x, ... (every job's tiles, job-major).
struct FlowWalk {
  int tile0, step, nitems;  // item k is launch tile tile0 + k * step
};
ME_HOST_DEVICE inline FlowWalk flow_walk(int ntiles, int nwg, int bid) {
  const int ng = nwg < 8 ? nwg : 8;
  const int x = bid % ng, m = bid / ng;
  const int n_x = nwg / ng + (x < nwg % ng ? 1 : 0);
  const int band0 = (int)((long)ntiles * x / ng), band1 = (int)((long)ntiles * (x + 1) / ng);
  FlowWalk w;
  w.tile0 = band0 + m;
  w.step = n_x;
  w.nitems = band1 - band0 > m ? (band1 - band0 - m + n_x - 1) / n_x : 0;
  return w;
}
// The item table of a pruning launch with box-sum planes: the workgroup decodes
// its items once, in front of its start barrier, into LDS behind its control
// block; the waves then place a pulled task by the prefixes and rebuild the
// item from the packed word, with no job-table load.  Entry k: the index of
// item k's first wave-task (entry nitems: the workgroup's task count) and
// job | tile column << 5 | absolute block row << 16.
struct FlowEntry {
  uint32_t pre, pack;
};
constexpr int FLOW_ENTRY_BYTES = 8;
static_assert(sizeof(FlowEntry) == FLOW_ENTRY_BYTES, "LDS layout of the item table");
static_assert(MAX_JOBS <= 32, "the packed word gives the job 5 bits");
ME_HOST_DEVICE inline uint32_t flow_entry_pack(int j, int col, int by) {
  return (uint32_t)j | (uint32_t)col << 5 | (uint32_t)by << 16;
}
// The item of job j at block row by, first block bx0 (all dy chunks: one
// pass): what job_item_at gives for the tile (row-major tiles, strip_w == 0).
ME_HOST_DEVICE inline Item flow_item_make(const SearchArgs& p, const QsadGeom& g, int B, int K, int j,
                                          int by, int bx0) {
  Item it;
  it.j = j;
  it.bx0 = bx0;
  it.by = by;
  it.nb = g.tb < g.nbx_full - bx0 ? g.tb : g.nbx_full - bx0;
  it.tly = by * B;
  it.h = B < p.height - it.tly ? B : p.height - it.tly;
  it.a = ((bx0 * B - p.range) % 4 + 4) % 4;
  it.X0 = bx0 * B - p.range - it.a;
  it.c0 = 0;
  it.nch = g.cpp < g.chunks ? g.cpp : g.chunks;
  it.prow0 = it.tly - p.range;
  it.prows = it.nch * K + B - 1;
  return it;
}
ME_HOST_DEVICE inline Item flow_entry_item(const SearchArgs& p, const QsadGeom& g, int B, int K, uint32_t pack) {
  return flow_item_make(p, g, B, K, (int)(pack & 31u), (int)(pack >> 16), (int)((pack >> 5) & 2047u) * g.tb);
}
// Launch tile `tile` of job j (rows from r0j, tiles from prej) packed.
ME_HOST_DEVICE inline uint32_t flow_entry_of(const QsadGeom& g, int tile, int j, int prej, int r0j) {
  const int t = tile - prej, row = t / g.wg_per_row;
  return flow_entry_pack(j, t - row * g.wg_per_row, r0j + row);
}
// Wave-tasks of one item: its lane-tasks (valid chunks x blocks x groups) / 64,
// rounded up; *lc0_out: its first valid chunk (the dy clamp at the frame's top).
ME_HOST_DEVICE inline int flow_item_tasks(const SearchArgs& p, const QsadGeom& g, int K, const Item& it,
                                          int* lc0_out) {
  const int S = p.range;
  const int dymin = -S > -it.tly ? -S : -it.tly;
  const int top = p.height - it.h - it.tly, dymax = S < top ? S : top;
  const int a = (dymin + S) / K, b = (dymax + S) / K + 1;
  const int lc0 = a > 0 ? a : 0, lc1 = it.nch < b ? it.nch : b;
  *lc0_out = lc0;
  return ((lc1 - lc0) * it.nb * g.groups + 63) >> 6;
}
// Entries the launch's table needs (the longest walk's items and the end
// entry), or 0: no table (it does not fit `room` bytes, a field does not fit
// its bits, the tiles walk in strips, or more items than cap > 0 allows: the
// tuning build's way to the path without a table).
inline int flow_table_entries(const QsadGeom& g, int ntiles, int nwg, int max_by, int room, int cap) {
  if (nwg < 1 || ntiles < 1) return 0;
  int most = 0;
  for (int bid = 0; bid < nwg; bid++) {
    const int n = flow_walk(ntiles, nwg, bid).nitems;
    if (n > most) most = n;
  }
  if (g.strip_w > 0 || g.wg_per_row > 2048 || max_by >= 65536) return 0;
  if (cap > 0 && most > cap) return 0;
  return (most + 1) * FLOW_ENTRY_BYTES <= room ? most + 1 : 0;
}

// ---- box-sum planes of the pruning flow plan (S = 32, 4-block tiles) ----
// Per job, per resident ref row y (relative to ref_row0), four x-phase rows of
// flow_plane_pitch bytes: row 4 y + k, byte i holds q(y, 4 i + k - 32).  The x
// origin sits S = 32 pixels left of the frame, so the 32 bytes a tile at
// X0 = 64 c - 32 needs start at byte 16 c of every phase row: 16-byte granules
// for the LDS DMA.  Positions no valid candidate uses (x < 0, x > W - 4,
// y > rows - 4) and the pitch padding hold 0.
inline int flow_plane_pitch(int width) { return ((width + 64) / 4 + 15) & ~15; }
// Resident ref rows of job J (ref_resident_bytes' rows).
inline int flow_plane_rows(const SearchJob& J, int blk, int range, int height) {
  const int end = J.r1 * blk + range < height ? J.r1 * blk + range : height;
  return end > J.ref_row0 ? end - J.ref_row0 : 0;
}
inline size_t flow_plane_job_bytes(int width, int rows) {  // a multiple of 64
  return (size_t)rows * 4 * (size_t)flow_plane_pitch(width);
}
// Byte offset in a job's planes of x phase k, byte `byte` of the 32 an item's
// window row yp (0 .. 76) has there: the item's window starts rel = prow0 -
// ref_row0 rows into the job's resident rows, at x = X0 (= 64 c - 32 for tile
// column c).  Unsigned arithmetic: a row above the resident ones wraps past
// 2^31, a row below them lies past the job's bytes, and the buffer range check
// reads either as 0 (the bytes the slot's LDS DMA of the planes brought).  The
// bound's step 2 reads 8 bytes at byte = 4 b + 4 m of phase k (block b, dx
// groups 4m .. 4m + 3), its fold column 4 bytes at byte = 4 b + 16 of phase 0.
// The offset is the sum (mod 2^32) of a part the wave shares and the lane's;
// the kernel forms the two apart and steps the row part by 4 * pitch a row.
ME_HOST_DEVICE inline uint32_t flow_plane_row_byte(int pitch, int rel, int X0, int yp) {
  return (uint32_t)(4 * (rel + yp)) * (uint32_t)pitch + (uint32_t)((X0 + 32) >> 2);
}
ME_HOST_DEVICE inline uint32_t flow_plane_lane_byte(int pitch, int k, int byte) {
  return (uint32_t)k * (uint32_t)pitch + (uint32_t)byte;
}
ME_HOST_DEVICE inline uint32_t flow_plane_byte(int pitch, int rel, int X0, int yp, int k, int byte) {
  return flow_plane_row_byte(pitch, rel, X0, yp) + flow_plane_lane_byte(pitch, k, byte);
}
// Byte offset from a job's cur pointer (its rows start at frame row cur_row0)
// of the r-th (0 .. 3) of the four dwords whose byte sum is the 4x4 box sum
// lane = block << 4 | sub-block row << 2 | sub-block column of the item at
// (tly, bx0) owns: the chain kernel's pre-bound forms the cur blocks' q from
// global memory with them, while the slot's cur area still belongs to the item
// in front.  The bytes are those the slot's cur DMA brings (stage_item_part:
// granule d -> row (d >> 4) & 15 of block d >> 8), B = 16.
ME_HOST_DEVICE inline uint32_t flow_qcur_byte(int cur_row0, int stride, int tly, int bx0, int lane, int r) {
  const int b = lane >> 4, sy = (lane >> 2) & 3, sx = lane & 3;
  return (uint32_t)((tly - cur_row0 + 4 * sy + r) * stride + (bx0 + b) * 16 + 4 * sx);
}
#undef ME_HOST_DEVICE
// No such load straddles the end of a phase row, so none straddles the end of
// the job's bytes (a whole number of phase rows; the loads are 4-byte aligned,
// the pitch a multiple of 16): the last tile column's 32 bytes end inside the pitch.
inline bool flow_plane_loads_fit(int width, int wg_per_row) {
  return wg_per_row >= 1 && 16 * (wg_per_row - 1) + 32 <= flow_plane_pitch(width);
}

// ---- the VALU kernels' planners (me_valu_plan.cpp: host-only, pure) ----

// Alignment class of a search's planes: bit 0 = stride, ref and cur 4-byte
// aligned; bit 1 = stride and ref 16-byte aligned; bit 2 = cur 16-byte aligned.
enum { ALIGN_4 = 1, ALIGN_REF16 = 2, ALIGN_CUR16 = 4, ALIGN_ALL = 7 };
inline int align_class(int stride, const void* ref, const void* cur) {
  const uintptr_t r = (uintptr_t)ref, c = (uintptr_t)cur;
  return (stride % 4 == 0 && r % 4 == 0 && c % 4 == 0 ? ALIGN_4 : 0) |
         (stride % 16 == 0 && r % 16 == 0 ? ALIGN_REF16 : 0) | (c % 16 == 0 ? ALIGN_CUR16 : 0);
}

// What a plan depends on (and, with the CU count and the Tuning, the plan
// cache's key): the frame, the search, the block rows planned for (every job's rows of a
// batched launch) and the alignment class of the planes.
struct PlanShape {
  int width, height, stride, blk, range, cost, rows, align;
  bool operator==(const PlanShape& o) const {
    return width == o.width && height == o.height && stride == o.stride && blk == o.blk &&
           range == o.range && cost == o.cost && rows == o.rows && align == o.align;
  }
};

struct Tuning;  // me_tuning.h

// The item kernel's plan (me_fast_kernel<cost, B, *k_out>) for s on a device
// of `cus` CUs; false: the shape goes to the generic kernel.  g->row0 and
// g->nrows stay 0 (the job table carries the rows).
bool plan_fast(const PlanShape& s, int cus, const Tuning& tu, QsadGeom* g, int* k_out);
// The flow kernel's plan (me_flow_kernel<16, 13>); false: the item kernel's turn.
bool plan_flow(const PlanShape& s, int cus, const Tuning& tu, QsadGeom* g);
// A pruning flow launch over njobs jobs reads its box sums from prepass planes
// (tu.prune_planes, else the automatic rule).
bool flow_planes_on(const Tuning& tu, int njobs);
// Context scratch the SAD search of jobs [0, n) of s's frame needs for its
// flow launches' box-sum planes (s.rows and s.align are not read: the plans
// are made as the dispatcher makes them, over every job's rows and then job by
// job): the largest sum of flow_plane_job_bytes over the jobs of one launch
// (MAX_JOBS consecutive jobs at most).  0: no launch of it uses planes (not
// SAD, no flow plan or one without pruning, planes off).
size_t flow_planes_scratch(const PlanShape& s, int cus, const Tuning& tu, const SearchJob* jobs, int n);

// Plans depend only on the shape: cached_plan keeps them (process-wide, one
// ring of 8 per planner under a mutex: the per-device host threads share them)
// so a steady stream of same-shape searches pays the planner once.  s.align is
// the planes' whole class (align_class; of every job of a batch): each planner
// is keyed by what it reads of it.  K may be null.
enum PlanKind { PLAN_ITEM = 0, PLAN_FLOW = 1 };
bool cached_plan(PlanKind kind, const PlanShape& s, int cus, const Tuning& tu, QsadGeom* g, int* K);

}  // namespace me
