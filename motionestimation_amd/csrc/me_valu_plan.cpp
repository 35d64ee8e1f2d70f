// me_valu_plan.cpp -- launch plans of the VALU search kernels (host-only C++).
//
// plan_fast (the persistent item kernel) and plan_flow (the flow kernel) decide
// for every SAD search, and every SSD search off the matrix cores, which kernel
// instance runs with which tile width, pitch, LDS size and magic divisors.
// Both are pure functions of the shape, the alignment class of the planes, the
// CU count and the tuning overrides: no device query, no statics, so the CPU
// tests pin their plans (tests/test_valu_plan.py) and run them under the
// sanitizers (oracle/san_main.cc).  cached_plan, at the end, is the plan cache
// the dispatcher (me_dispatch.cpp) asks; me_kernels.hip launches the plans.
#include <stdint.h>
#include <string.h>

#include <mutex>
#include <type_traits>

#include "me_geom.h"
#include "me_tuning.h"

namespace me {
namespace {

// LDS tile pitch for rows of `width` bytes: a multiple of 16 with an odd
// 16-byte index (pitch % 32 == 16), so the rows of a tile start in
// alternating halves of the banks.
int tile_pitch(int width) {
  const int pt = (width + 15) & ~15;
  return ((pt >> 4) & 1) ? pt : pt + 16;
}

// Bytes the lanes touch per tile row of tb blocks.  SAD: G groups of 4 dx, the
// block, and aw bytes of alignment word.  SSD: the 2S + 1 columns (+ a <= 3, +
// alignment word).
int sad_row_bytes(int tb, int B, int G, int aw) { return (tb - 1) * B + 4 * G + B + aw; }
int ssd_row_bytes(int tb, int B, int S) { return (tb - 1) * B + 2 * S + 1 + 3 + B + 4; }

// The multiply-high divisor of d, ceil(2^32 / d) for every d but a power of
// two (no pitch is one: odd multiples of 16, at least 48): umulhi(x, magic(d))
// == x / d for every x of the range magic_ok checks.
uint32_t magic(uint32_t d) { return 0xFFFFFFFFu / d + 1u; }
bool magic_ok(uint32_t m, uint32_t d, uint32_t n, uint32_t step = 1) {
  for (uint32_t x = 0; x < n; x += step)
    if ((uint32_t)(((uint64_t)x * m) >> 32) != x / d) return false;
  return true;
}
// An item's / nb for every block count nb of a tile (bg < n)
bool magic_ok_upto(uint32_t tb, uint32_t n) {
  for (uint32_t nb = 2; nb <= tb; nb++)
    if (!magic_ok(magic(nb), nb, n)) return false;
  return true;
}

}  // namespace

// Plan the fast kernels.  SAD lanes own 4 dx (one qsad group), SSD lanes one
// dx; both own K dy.  Search (fold, K, TB, chunks per pass) for the most
// useful work per wave-task (dy padding, the masked 4th column of the last
// SAD group or the fold's extra column, idle lanes of partly filled waves)
// within the LDS budget; then prefer fewer passes and smaller tiles (finer
// work items).  256 threads per workgroup: 4 workgroups of 4 waves per CU at
// the kernels' <= 128 VGPRs.
bool plan_fast(const PlanShape& s, int cus, const Tuning& tu, QsadGeom* g, int* k_out) {
  *g = QsadGeom{};
  const int B = s.blk, S = s.range;
  if (B != 16 && B != 8) return false;
  if (S < 1 || S > 255) return false;
  g->nbx_full = s.width / B;
  if (g->nbx_full < 1) return false;
  const bool sad = s.cost == COST_SAD;
  const int D = 2 * S + 1;
  const int CW = B / 4;
  // Fold needs a = 0 (S % 4 == 0) and the tail words of every block aligned
  // for one ds_read of B bytes (b*B + 2S multiple of B: S % 8 == 0 for B = 16).
  const bool fold_ok = sad && S % 4 == 0 && (B == 8 || S % 8 == 0);
  // SAD rows carry an alignment word for a = (tlx - S) mod 4 <= 3; with S % 4
  // == 0 (tlx a multiple of B) a = 0 and the lanes read exactly 4G + B bytes
  // past the block's first tile column: no word (1080p tb = 3 rows 112 instead
  // of 144 bytes; the 2- and 4-way stripe times moved within box-to-box
  // noise, profiles/r02al_stripe_sweeps.jsonl)
  const int aw = S % 4 == 0 ? 0 : 4;
  // SAD groups: S / 2 with the fold, else worst case a = 3
  const int G_fold = S / 2, G_plain = (2 * S + 3 + 1 + 3) / 4;
  auto row_bytes = [&](int tb, int G) {
    return sad ? sad_row_bytes(tb, B, G, aw) : ssd_row_bytes(tb, B, S);
  };
  static const int Ks[] = {26, 13, 11, 8, 5};
  // K = 26 (8x8 SAD): twice the candidates per lane-task, so the task decode,
  // cur loads, fold column and key merge are paid per 104 candidates, not 52
  // (8K +-128: 18.23 -> 17.40 ms, tb 8 at the compiled pitch 336;
  // profiles/r03ar_plan_8k.jsonl)
  const bool k26_auto = sad && B == 8;
  // K = 5 (a quarter-size wave-task) only for SAD searches too small to give
  // every SIMD two K = 13 wave-tasks (an 8-way 1080p stripe: 1.25 per SIMD, so
  // a quarter of the SIMDs ran a second round); K >= 8 otherwise.
  bool small = false;
  if (sad) {
    const int G13 = fold_ok ? G_fold : G_plain;
    const double lanes = (double)s.rows * (s.width / B) * G13 * ((D + 12) / 13);
    small = lanes / 64.0 < 2.0 * 4 * cus;
  }
  // Tuning build override (tools/plan_sweep.py): ME_PLAN="K,tb,cpp,threads[,fold]",
  // validated in me_api.hip; 0 = free (fold: -1 = free).
  const int force[5] = {tu.plan_k, tu.plan_tb, tu.plan_cpp, tu.plan_threads, tu.plan_fold};
  const int thr = force[3] > 0 ? force[3] : 256;
  const int rows = s.rows;
  double best = -1;
  int bK = 13, bTB = 1, bC = 1, bF = 0, bG = 1;
  for (int fold = 0; fold <= 1; fold++) {
    if (fold && !fold_ok) continue;
    if (force[4] >= 0 && fold != force[4]) continue;
    const int G = sad ? (fold ? G_fold : G_plain) : D;
    // useful share of a lane's candidates (the last group's padding), and the
    // fold's extra cost per task (one B-row v_sad_u8 column + its key)
    const double use_dx = sad ? (fold ? 1.0 : (double)D / (4.0 * G)) : 1.0;
    for (int K : Ks) {
      if (force[0] && K != force[0]) continue;
      // (K = 5 is instantiated for 16x16 SAD only: other small searches keep K >= 8;
      // K = 26 for 8x8 SAD only)
      if (K == 5 && (!sad || B != 16)) continue;
      if (K == 26 && (!sad || B != 8 || (!force[0] && !k26_auto))) continue;
      if (!force[0] && (K == 5) != (small && B == 16)) continue;
      if (fold && G < K) continue;
      const int chunks = (D + K - 1) / K;
      if (K == 5 && !force[0]) {
        // small search: one block per tile, every chunk in one pass, so each
        // block is its own workgroup item (1,020 of them in an 8-way 1080p
        // stripe: about one quarter-size wave-task per wave, all SIMDs busy).
        // No fold (17 groups): the fold's narrower rows measured slower here
        // (9-row stripe 20.2 vs 19.65 us, CIF +-16 12.4 vs 11.05 us,
        // profiles/r02am_small_plan_fold.txt).
        const int pt = tile_pitch(row_bytes(1, G));
        const long lds = 128 + 2 * ((long)B * B + (long)(chunks * K + B - 1) * pt);
        if (lds <= QSAD_LDS_BUDGET && best < 0) {
          best = 1.0; bK = K; bTB = 1; bC = chunks; bF = fold; bG = G;
        }
        continue;
      }
      const double kpad = (double)D / (chunks * K);
      const double tail = fold ? 0.5 * (B * CW + 16) / (K * B * CW * 4 + 340) : 0.0;
      // Waves that hold whole (block, chunk) groups (64 % G == 0 or G % 64
      // == 0) read one cur block and share one row range per wave: measured
      // ~5 % faster than waves straddling blocks (8K B8: G 64 vs 65).
      const double wave_align = (64 % G == 0 || G % 64 == 0) ? 1.03 : 1.0;
      for (int tb = 1; tb <= 16; tb++) {
        if (force[1] && tb != force[1]) continue;
        // One-block tiles restage a whole window per block and leave waves of
        // every item part empty: measured slower than two-block tiles wherever
        // both fit (1080p: 171 vs 121 us static; 4K block rows 0..17, the edge
        // stripe of an 8-way split: 0.228 vs 0.188 ms; profiles/r02h_dyn.jsonl).
        if (tb == 1 && !force[1] && g->nbx_full >= 2) continue;
        const int pt = tile_pitch(row_bytes(tb, G));
        for (int cpp = chunks; cpp >= 1; cpp--) {
          if (force[2] && cpp != force[2]) continue;
          const long lds = 128 + 2 * ((long)tb * B * B + (long)(cpp * K + B - 1) * pt);
          if (lds > QSAD_LDS_BUDGET) continue;
          int passes = 0;
          for (int c0 = 0; c0 < chunks; c0 += cpp) passes++;
          const long items = (long)((g->nbx_full + tb - 1) / tb) * rows * passes;
          // Cost of an item in wave-tasks: its waves (a partly filled wave
          // costs a whole one), for SAD half of the wave slots its last round of
          // `thr` lanes leaves idle (the CU's other workgroups take up the
          // rest: 4K +-64, 68 block rows, tb 5 = 10 waves in rounds of 4:
          // 0.637 ms against tb 8's 0.570, profiles/r02aa_plan_sweep_4k_68rows.jsonl),
          // + ~0.45 for staging, barrier and output (fitted on
          // tools/plan_sweep.py runs).  With few items per workgroup (< 8 of
          // 1024) a partial last round is not amortised at all: whole rounds.
          const bool many = items >= 8L * 1024;
          double cost = 0, useful = 0;
          for (int c0 = 0; c0 < chunks; c0 += cpp) {
            const int t = tb * G * (chunks - c0 < cpp ? chunks - c0 : cpp);
            const int rounds = (t + thr - 1) / thr;
            const int waves = (t + 63) / 64, idle = rounds * (thr / 64) - waves;
            // few items: every extra round lengthens the kernel's tail too
            cost += (many ? waves + (sad ? 0.5 * idle : 0.0) : rounds * (thr / 64) + 0.5 * (rounds - 1)) + 0.45;
            useful += t / 64.0;
          }
          // Workgroups take whole tiles (every pass of a tile runs on the
          // workgroup holding its keys): too few tiles leave workgroup slots
          // idle (and nothing to prefetch): aim for >= 2 tiles per resident
          // workgroup (4 per CU).
          const long tiles = items / passes;
          const double fill = tiles >= 2048 ? 1.0 : (double)tiles / 2048;
          // K = 13 measured best wherever it fits (more candidates per row load
          // and per epilogue than the padding it costs).
          // K = 26 over K = 13 where it fits (8x8 SAD), at the compiled tile
          // pitch 336 if a tb gives it (tb 8: 17.40 ms; tb 12 / 16 at runtime
          // pitches 17.68 / 17.64 ms)
          const double kpref = K == 26 ? (pt == 336 ? 1.05 : 1.03) : K == 13 ? 1.0 : 0.95;
          // the last tile of a block row holds nbx_full % tb blocks
          const double tile_fill =
              (double)g->nbx_full / ((double)((g->nbx_full + tb - 1) / tb) * tb);
          const double score = kpad * kpref * wave_align * tile_fill * use_dx / (1.0 + tail) * useful / cost *
                               (0.7 + 0.3 * fill) - 0.002 * tb;
          if (score > best + 1e-9) {
            best = score; bK = K; bTB = tb; bC = cpp; bF = fold; bG = G;
          }
        }
      }
    }
  }
  if (best < 0) return false;  // nothing fits (only with an ME_PLAN override)
  g->fold = bF;
  g->groups = bG;
  // Dynamic tile pulls from this many tiles per workgroup on (ME_DYN overrides
  // in the tuning build; 0 = static bands only).
  {
    const int dyn_env = tu.dyn;
    // 3: measured (tools/dyn_sweep.sh) -- 4K (3.96 tiles/WG) and 8K gain
    // (8K -11 % with stealing), 1080p (2.7 tiles/WG) loses: its workgroups
    // start items in lockstep and the item-start pulls serialise on the
    // device-scope counters while wave 0 waits.
    g->dyn_tiles = dyn_env >= 0 ? dyn_env : 3;
    // ... and only for tiles of >= 16 wave-tasks: small tiles pay the pull per
    // few tasks (1080p tb = 2: 184 vs 121 us static; profiles/r02h_dyn.jsonl).
    const long tile_lanes = (long)bTB * bG * ((D + bK - 1) / bK);
    if (dyn_env < 0 && tile_lanes < 16L * 64) g->dyn_tiles = 0;
  }
  g->tb = bTB;
  g->cpp = bC;
  g->chunks = (D + bK - 1) / bK;
  g->pitch = tile_pitch(row_bytes(g->tb, g->groups));  // the pitch of the chosen tb
  g->rows_alloc = g->cpp * bK + B - 1;
  g->tile_bytes = g->rows_alloc * g->pitch;
  g->threads = thr;
  g->lds = 2 * (g->tile_bytes + g->tb * B * B) + 128 + 16;
  // r = umulhi(d, magic) == d / pitch for every staged offset d (checked).
  g->pitch_magic = magic((uint32_t)g->pitch);
  if (!magic_ok(g->pitch_magic, (uint32_t)g->pitch, (uint32_t)g->tile_bytes, 4)) return false;
  g->wg_per_row = (g->nbx_full + g->tb - 1) / g->tb;
  // t / wg_per_row by multiply-high for every tile index of these rows
  g->magic_wpr = magic((uint32_t)g->wg_per_row);
  if (!magic_ok(g->magic_wpr, (uint32_t)g->wg_per_row,
                (uint32_t)g->wg_per_row * (uint32_t)(rows > 0 ? rows : 1)))
    g->magic_wpr = 0;
  g->magic_tb = magic((uint32_t)g->tb);
  // The DMA path stages 4-byte granules under the planes' range check, which
  // ends W bytes into the last resident row: with W % 4 != 0 the granule
  // holding that row's last pixels straddles the end and comes back all zero
  // (334 x 51 at a pitch of 336: SADs of candidates on the last row's last two
  // columns too large).  Such frames take the byte-copy staging.
  g->aligned = (s.align & ALIGN_4) != 0 && s.width % 4 == 0;
  // X0 = tb*B*t - S - a is 16-aligned for every tile when a = 0 (S % 4 == 0),
  // S % 16 == 0 and tb * B % 16 == 0; rows of the ref plane 16-aligned; W % 16
  // == 0 keeps the last in-frame granule of the last row inside the range.
  g->tile16 = g->aligned && S % 16 == 0 && (g->tb * B) % 16 == 0 && s.width % 16 == 0 &&
              (s.align & ALIGN_REF16) != 0;
  // umulhi(t, magic_groups) == t / groups for every task index of an item.
  g->magic_groups = magic((uint32_t)g->groups);
  if (!magic_ok(g->magic_groups, (uint32_t)g->groups, (uint32_t)(g->tb * g->groups * g->cpp)))
    return false;
  if (!magic_ok_upto((uint32_t)g->tb, (uint32_t)(g->tb * g->cpp))) return false;  // bg < tb * cpp
  g->prio = tu.prio != 0;
  g->fair = 0;
  g->flow_slots = 0;
  // Wide frames: vertical strips of 16 tiles (8K 8x8: 1,024 pixels plus the
  // window's 2S), so an XCD's contiguous run of the order is a few whole
  // strips and its L2 holds a strip's window rows while they are reread
  // (the row-major order fetched 2.4x the algorithmic bytes at 8K SAD).
  g->strip_w = g->wg_per_row >= 32 && rows >= 32 ? 16 : 0;
  if (tu.strip >= 0) g->strip_w = tu.strip;
  // Dynamic pulls claim a workgroup's next tile when its current one starts if
  // a tile has >= 2 passes (the id is read at the last pass, a barrier later),
  // else two tiles ahead.  Claimed-but-unstarted tiles widen the band of rows
  // an XCD's workgroups touch at once: ahead = 2 at 4K +-64 (128 workgroups
  // per XCD, 3 passes) fetched 1.35x the compulsory bytes, ahead = 1
  // 1.11x, at the same time (profiles/r04l_variants_4k.txt).
  g->pull_ahead = (g->chunks + g->cpp - 1) / g->cpp >= 2 ? 1 : 2;
  if (tu.ahead > 0 && (tu.ahead == 2 || g->pull_ahead == 1)) g->pull_ahead = tu.ahead;
  *k_out = bK;
  return true;
}

// The flow kernel (SAD, 16x16, S = 32, one 1,024-thread workgroup per CU): tiles of tb
// blocks with all their dy chunks, tb * G * chunks a multiple of 64 (every
// wave-task full), a ring of >= 4 slots in LDS, the ref tile in 16-byte
// granules, and >= 2 tiles per CU (fewer leave most of the 16 waves idle: the
// persistent item kernel takes small stripes).
bool plan_flow(const PlanShape& s, int cus, const Tuning& tu, QsadGeom* g) {
  constexpr int FLOW_LDS = FLOW_LDS_BUDGET - 1024;
  *g = QsadGeom{};
  const int B = s.blk, S = s.range;
  if (s.cost != COST_SAD || B != 16) return false;
  // fold (S % 8) and 16-byte tile granules (S % 16).  S <= 32: at 4K +-64 the
  // item kernel's items are already whole waves (8 blocks x 4 chunks x 32
  // groups) and it measured faster (1.086 vs 1.12 ms, profiles/r02p_flow_sweep.txt).
  // The fold spreads the dx = +S column over lanes gi < K: G = S/2 >= K.
  if (S < 16 || S % 16 || S > 32) return false;
  if (tu.flow == 0) return false;
  const int nbx_full = s.width / B;
  const int all16 = ALIGN_REF16 | ALIGN_CUR16;  // stride, ref and cur 16-byte aligned
  if (nbx_full < 1 || s.width % 16 || (s.align & all16) != all16) return false;
  const int D = 2 * S + 1, G = S / 2;
  const int rows = s.rows;  // launch_jobs: every job's rows
  auto pitch_of = [&](int tb) { return tile_pitch(sad_row_bytes(tb, B, G, 4)); };
  auto slots_of = [&](int tb, int K) {
    const int chunks = (D + K - 1) / K;
    const int slot = (chunks * K + B - 1) * pitch_of(tb) + tb * B * B;
    const int ns = (FLOW_LDS - 16 * tb * 8 - (int)sizeof(int) * 40) / slot;
    return ns < 16 ? ns : 16;
  };
  // K = 13, whole tiles per CU, XCD-banded: the widest tile that still gives
  // >= 6 tiles per CU (fine enough for the CUs to finish together), else the
  // narrowest with >= 2 per CU (fewer leave most of the 16 waves idle: the
  // persistent item kernel takes small stripes).
  const int K = 13;
  int best_tb = 0, best_ns = 0;
  if (G >= 13) {
    const int chunks = (D + 12) / 13;
    int fine_tb = 0, fine_ns = 0;
    for (int tb = 1; tb <= 8; tb++) {
      if ((tb * G * chunks) % 64) continue;
      if (tu.plan_tb && tb != tu.plan_tb) continue;  // tuning build
      const int ns = slots_of(tb, 13);
      const long tiles = (long)((nbx_full + tb - 1) / tb) * rows;
      if (ns < 4 || tiles < 2L * cus) continue;
      if (!best_tb) {
        best_tb = tb;
        best_ns = ns;
      }
      if (tiles >= 6L * cus) {
        fine_tb = tb;
        fine_ns = ns;
      }
    }
    if (fine_tb) {
      best_tb = fine_tb;
      best_ns = fine_ns;
    }
    // tb = 4 (the 144-byte pitch compiled into the kernel: row addresses in
    // the ds_read2 offsets) whenever it gives >= 6 tiles per CU: a batch of
    // 8 1080p frames took tb = 8 at the runtime pitch, 84 us per frame
    // against 69-78 for single frames (profiles/r03j_*)
    const long tiles4 = (long)((nbx_full + 3) / 4) * rows;
    if (best_tb != 4 && (4 * G * chunks) % 64 == 0 && pitch_of(4) == 144 && slots_of(4, 13) >= 4 &&
        tiles4 >= 6L * cus && !tu.plan_tb) {
      best_tb = 4;
      best_ns = slots_of(4, 13);
    }
  }
  if (!best_tb) return false;
  const int chunks = (D + K - 1) / K;
  QsadGeom& q = *g;
  q.tb = best_tb;
  q.groups = G;
  q.chunks = chunks;
  q.cpp = chunks;
  q.fold = 1;
  q.nbx_full = nbx_full;
  q.pitch = pitch_of(q.tb);
  q.rows_alloc = chunks * K + B - 1;
  q.tile_bytes = q.rows_alloc * q.pitch;
  q.wg_per_row = (nbx_full + q.tb - 1) / q.tb;
  q.magic_wpr = 0;  // the flow kernel maps a tile once per item: plain division
  q.magic_tb = magic((uint32_t)q.tb);
  q.aligned = 1;
  q.tile16 = 1;
  q.threads = 1024;
  q.dyn_tiles = 0;
  q.pull_ahead = 2;
  // umulhi(d, pitch_magic) == d / pitch for every staged granule offset d,
  // umulhi(t, magic_groups) == t / G for every task index of an item, and
  // an item's / nb for bg < tb * chunks (checked).
  q.pitch_magic = magic((uint32_t)q.pitch);
  if (!magic_ok(q.pitch_magic, (uint32_t)q.pitch, (uint32_t)q.tile_bytes, 16)) return false;
  q.magic_groups = magic((uint32_t)G);
  if (!magic_ok(q.magic_groups, (uint32_t)G, (uint32_t)(q.tb * G * chunks))) return false;
  if (!magic_ok_upto((uint32_t)q.tb, (uint32_t)(q.tb * chunks))) return false;
  const int slot = q.tile_bytes + q.tb * B * B;
  if (tu.flow_slots && tu.flow_slots < best_ns) best_ns = tu.flow_slots;
  q.flow_slots = best_ns;
  q.prio = tu.prio != 0;
  q.fair = tu.fair != 0 ? (tu.fair_lo | tu.fair_hi << 8 | (tu.fair > 1 ? tu.fair : 1) << 16) : 0;
  q.strip_w = 0;
  q.lds = best_ns * slot + best_ns * q.tb * 8 + (int)sizeof(int) * 40;
  if (q.lds > FLOW_LDS_BUDGET) return false;
  // Candidate pruning (the kernel's flow_bound): the shape the bound phase is
  // written for (4 blocks, 16 dx groups, 5 chunks, the compiled 144-byte
  // pitch); every ring slot carries its own bound scratch, so as many bound
  // phases run at once as slots are being refilled and none waits for scratch.
  // A slot grows from 12,544 to 23,744 bytes: 6 slots where 12 fitted.
  if (tu.prune != 0 && q.tb == 4 && G == 16 && chunks == 5 && q.pitch == 144) {
    const int pslot = slot + FLOW_PRUNE_BYTES;
    int ns = (FLOW_LDS - 16 * q.tb * 8 - FLOW_CTL_BYTES) / pslot;
    if (ns > 16) ns = 16;
    if (tu.flow_slots && tu.flow_slots < ns) ns = tu.flow_slots;
    if (ns >= 2) {
      q.prune = tu.prune == 2 ? 2 : 1;
      q.prune_bypass = tu.prune_bypass != 0;
      q.prune_stats = tu.prune_stats;
      q.prune_split = tu.prune_split == 2 ? 2 : tu.prune_split != 0;
      q.prune_slots = ns;
      q.prune_lds = ns * pslot + ns * q.tb * 8 + FLOW_CTL_BYTES;
      // With box-sum planes the bound reads them from global memory and a slot
      // carries FLOW_SLIM_BYTES (14,912 bytes a slot: 10 slots), if none of
      // its plane loads can straddle a phase row's end.
      const int sslot = slot + FLOW_SLIM_BYTES;
      int sns = (FLOW_LDS - 16 * q.tb * 8 - FLOW_CTL_BYTES) / sslot;
      if (sns > 16) sns = 16;  // FlowCtl's arrays
      if (tu.flow_slots && tu.flow_slots < sns) sns = tu.flow_slots;
      if (sns >= 2 && flow_plane_loads_fit(s.width, q.wg_per_row)) {
        q.slim_slots = sns;
        q.slim_lds = sns * sslot + sns * q.tb * 8 + FLOW_CTL_BYTES;
      }
    }
  }
  return true;
}

bool cached_plan(PlanKind kind, const PlanShape& s, int cus, const Tuning& tu, QsadGeom* g, int* K) {
  constexpr int N = 8;
  struct Entry { PlanShape key; int cus; Tuning tu; bool ok; QsadGeom g; int K; };
  static struct { Entry e[N]; int used, next; } rings[2];
  static std::mutex mu;
  static_assert(std::has_unique_object_representations<Tuning>::value, "Tuning compared bytewise");
  // what each planner reads of the class: the item kernel nothing of cur's
  // 16-byte alignment, the flow kernel only whether everything is 16-byte aligned
  const int all16 = ALIGN_REF16 | ALIGN_CUR16;
  PlanShape key = s;
  key.align = kind == PLAN_ITEM ? s.align & (ALIGN_4 | ALIGN_REF16) : (s.align & all16) == all16 ? ALIGN_ALL : 0;
  auto& ring = rings[kind];
  std::lock_guard<std::mutex> lk(mu);
  const Entry* hit = nullptr;
  for (int i = 0; i < ring.used && !hit; i++)
    if (ring.e[i].key == key && ring.e[i].cus == cus && memcmp(&ring.e[i].tu, &tu, sizeof tu) == 0)
      hit = &ring.e[i];
  if (!hit) {
    Entry& e = ring.e[ring.next];
    e.key = key;
    e.cus = cus;
    e.tu = tu;
    e.K = 13;
    e.ok = kind == PLAN_ITEM ? plan_fast(key, cus, tu, &e.g, &e.K) : plan_flow(key, cus, tu, &e.g);
    ring.next = (ring.next + 1) % N;
    if (ring.used < N) ring.used++;
    hit = &e;
  }
  *g = hit->g;
  if (K) *K = hit->K;
  return hit->ok;
}

// Automatic: launches of two or more jobs.  A launch of one job pays a whole
// extra kernel launch for one frame's planes and has few refills to win it
// back on: one 1080p frame measured 68.1-68.9 us with the planes against
// 68.7-69.4 without, overlapping (profiles/planes_single_frame_ab.jsonl; 70.5-
// 71.3 against 69.1-69.6 with the first, slower prepass), so it keeps the
// parent's launch.  Two frames: 107.1-107.6 against 111.0-111.1 us; four:
// 179.0-179.6 against 189.0-189.7; the 16-frame batch 0.643-0.645 ms against
// 0.690-0.693 (profiles/planes_frames{2,4}_ab.jsonl, planes_bench_ab.txt).
bool flow_planes_on(const Tuning& tu, int njobs) {
  if (tu.prune_planes >= 0) return tu.prune_planes != 0;
  return njobs >= 2;
}

size_t flow_planes_scratch(const PlanShape& s, int cus, const Tuning& tu, const SearchJob* jobs, int n) {
  if (s.cost != COST_SAD || n < 1) return 0;
  // jobs [j0, j0 + m) as the dispatcher's flow_jobs plans them
  auto need = [&](int j0, int m) -> size_t {
    if (!flow_planes_on(tu, m < MAX_JOBS ? m : MAX_JOBS)) return 0;
    PlanShape ps = s;
    ps.rows = 0;
    ps.align = align_class(s.stride, jobs[j0].ref, jobs[j0].cur);
    for (int i = j0; i < j0 + m; i++) {
      ps.rows += jobs[i].r1 - jobs[i].r0;
      if ((uintptr_t)jobs[i].ref % 16 || (uintptr_t)jobs[i].cur % 16) return 0;
    }
    QsadGeom g;
    if (!cached_plan(PLAN_FLOW, ps, cus, tu, &g, nullptr) || !g.prune || !g.slim_slots) return 0;
    size_t best = 0, sum = 0;  // the largest window of MAX_JOBS consecutive jobs
    for (int i = j0; i < j0 + m; i++) {
      sum += flow_plane_job_bytes(s.width, flow_plane_rows(jobs[i], s.blk, s.range, s.height));
      if (i - j0 >= MAX_JOBS)
        sum -= flow_plane_job_bytes(s.width, flow_plane_rows(jobs[i - MAX_JOBS], s.blk, s.range, s.height));
      if (sum > best) best = sum;
    }
    return best;
  };
  if (n >= 2) {
    const size_t b = need(0, n);
    if (b) return b;
  }
  size_t best = 0;
  for (int j = 0; j < n; j++) {
    const size_t b = jobs[j].r1 > jobs[j].r0 ? need(j, 1) : 0;
    if (b > best) best = b;
  }
  return best;
}

}  // namespace me
