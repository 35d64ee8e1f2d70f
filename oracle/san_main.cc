// san_main.cc -- CPU sanitizer harness (TEST INFRASTRUCTURE; SURVEY §5 asks
// for the CPU code under TSAN / ASAN).  Built by `make -C oracle asan tsan`
// (tests/test_sanitizers.py runs both), it exercises the host code that runs
// threads or parses untrusted input, without a GPU:
//   - the oracle's pthread pool (orc_full_search: workers pulling block indices
//     from a shared counter), against a single-thread run of the same search;
//   - the stripe planner (me_plan.cpp: me_plan_stripes, me_candidate_count) over
//     many shapes, checking the partition invariants;
//   - the file readers (me_io.cpp) fed truncated, corrupt and hostile files:
//     every one must come back as ME_EIO / ME_EINVAL, never a crash or an
//     out-of-bounds access (the reference's reader never checks its fopen,
//     src/common/utils.c:61-67);
//   - the VALU launch planners (me_valu_plan.cpp: plan_fast, plan_flow) over
//     seeded random shapes, alignment classes, CU counts and tuning overrides,
//     checking what the kernels rely on in every accepted plan;
//   - the matrix-core SSD planners (me_mfma_plan.cpp: the single-search plan,
//     plan_bw, the batch plan) likewise, over every kernel path: the batch's
//     planes fit the scratch that was sized for it, LDS and plane bounds, the
//     kernel instances the launchers dispatch, the band walk's cover;
//   - the search dispatcher (me_dispatch.cpp) over the cases of
//     tests/golden/plans/dispatch.json, from four threads at once (they share
//     the plan cache of me_valu_plan.cpp): every block of every job in
//     exactly one launch, through launch windows of several sizes;
//   - the C ABI's argument rules and record layouts (me_api_rules.cpp): every
//     case of tests/golden/api_args.json through its entry point's rules (the
//     recorded status), then what no GPU recording can hold: every integer of
//     every entry point at INT_MAX and INT_MIN, frame strides of SIZE_MAX, and
//     the layouts of many shapes (regions back to back inside the total).
// Exit status 0 and "san ok" on success; the sanitizers abort otherwise.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <string>
#include <thread>
#include <vector>

#include <limits.h>

#include "api_rules_cases.h"
#include "dispatch_cases.h"
#include "me.h"
#include "me_geom.h"
#include "me_mfma_geom.h"
#include "me_oracle.h"
#include "me_tuning.h"

#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      fprintf(stderr, "san: check failed at %d: %s\n", __LINE__, #x); \
      exit(1);                                                     \
    }                                                              \
  } while (0)

static uint64_t rng = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {  // splitmix64
  uint64_t z = (rng += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static void pool() {
  const int W = 97, H = 61;
  std::vector<uint8_t> ref(W * H), cur(W * H);
  for (int i = 0; i < W * H; i++) {
    ref[i] = (uint8_t)next_u64();
    cur[i] = (uint8_t)(i % 7 == 0 ? ref[i] : next_u64());
  }
  const int kinds[] = {ORC_SSD, ORC_SAD, ORC_MSE_FLOAT};
  for (int kind : kinds)
    for (int blk : {4, 8, 16}) {
      const int n = orc_num_blocks(W, H, blk);
      std::vector<int16_t> mv1(2 * n), mvn(2 * n);
      std::vector<uint32_t> c1(n), cn(n);
      CHECK(orc_full_search(ref.data(), cur.data(), W, H, W, blk, 6, kind, 1, 0, n, mv1.data(),
                            c1.data(), nullptr) == 0);
      // many threads over a small job list: contention on the shared counter
      CHECK(orc_full_search(ref.data(), cur.data(), W, H, W, blk, 6, kind, 13, 0, n, mvn.data(),
                            cn.data(), nullptr) == 0);
      CHECK(mv1 == mvn && c1 == cn);
    }
}

static void planner() {
  for (int t = 0; t < 3000; t++) {
    const int W = 1 + (int)(next_u64() % 4000), H = 1 + (int)(next_u64() % 2500);
    const int blk = 1 + (int)(next_u64() % 64), S = (int)(next_u64() % 300);
    const int n = 1 + (int)(next_u64() % 16);
    std::vector<int> b(n + 1, -1);
    CHECK(me_plan_stripes(W, H, blk, S, n, b.data()) == ME_OK);
    const int nby = (H + blk - 1) / blk;
    CHECK(b[0] == 0 && b[n] == nby);
    for (int i = 0; i < n; i++) CHECK(b[i] <= b[i + 1]);
    (void)me_candidate_count(W, H, blk, S);
  }
  int b[3];
  CHECK(me_plan_stripes(10, 10, 0, 1, 2, b) == ME_EINVAL);
  CHECK(me_plan_stripes(10, 10, 4, 1, 0, b) == ME_EINVAL);
  CHECK(me_plan_stripes(10, 10, 4, 1, 2, nullptr) == ME_EINVAL);
  CHECK(me_candidate_count(352, 288, 8, 12) == 927024ull);
}

static std::string tmp_path(const char* name) {
  const char* d = getenv("TMPDIR");
  return std::string(d && *d ? d : "/tmp") + "/me_san_" + std::to_string(getpid()) + "_" + name;
}

static void write_bytes(const std::string& p, const std::vector<uint8_t>& v) {
  FILE* f = fopen(p.c_str(), "wb");
  CHECK(f);
  if (!v.empty()) CHECK(fwrite(v.data(), 1, v.size(), f) == v.size());
  fclose(f);
}

static void files() {
  const int W = 33, H = 17, B = 8, n_pairs = 3;
  const int nb = me_num_blocks(W, H, B);
  std::vector<int16_t> mv(2 * nb * n_pairs);
  std::vector<uint32_t> co(nb * n_pairs);
  for (auto& x : mv) x = (int16_t)next_u64();
  for (auto& x : co) x = (uint32_t)next_u64();
  const std::string good = tmp_path("good.memv");
  CHECK(me_mv_write(good.c_str(), W, H, B, 5, ME_COST_SAD, nullptr, n_pairs, mv.data(),
                    co.data()) == ME_OK);
  FILE* f = fopen(good.c_str(), "rb");
  CHECK(f);
  std::vector<uint8_t> bytes;
  for (int c; (c = fgetc(f)) != EOF;) bytes.push_back((uint8_t)c);
  fclose(f);
  me_mv_header h;
  std::vector<int> pairs(2 * n_pairs);
  std::vector<int16_t> mv2(mv.size());
  std::vector<uint32_t> co2(co.size());
  CHECK(me_mv_read(good.c_str(), &h, pairs.data(), mv2.data(), co2.data()) == ME_OK);
  CHECK(mv2 == mv && co2 == co);

  const std::string bad = tmp_path("bad.memv");
  // every truncation
  for (size_t len = 0; len < bytes.size(); len++) {
    write_bytes(bad, std::vector<uint8_t>(bytes.begin(), bytes.begin() + len));
    me_mv_header hh;
    CHECK(me_mv_read(bad.c_str(), &hh, pairs.data(), mv2.data(), co2.data()) != ME_OK);
  }
  // corrupt header fields (sizes, counts, flags, magic) and random bytes: the
  // reader may accept a consistent file, but must never write past buffers
  // sized from the good header
  for (int t = 0; t < 400; t++) {
    std::vector<uint8_t> v = bytes;
    const int k = 1 + (int)(next_u64() % 4);
    for (int j = 0; j < k; j++) v[next_u64() % 32] = (uint8_t)next_u64();
    if (t % 5 == 0) v.resize(v.size() + (next_u64() % 64));
    write_bytes(bad, v);
    me_mv_header hh;
    if (me_mv_read_header(bad.c_str(), &hh) != ME_OK) continue;
    const long long nbh = me_num_blocks(hh.width, hh.height, hh.block_size);
    if ((long long)hh.n_pairs * nbh > (long long)nb * n_pairs || hh.n_pairs > (uint32_t)n_pairs)
      continue;  // a caller sizes its buffers from the header it read
    (void)me_mv_read(bad.c_str(), &hh, pairs.data(), mv2.data(), co2.data());
  }
  CHECK(me_mv_read_header(tmp_path("missing.memv").c_str(), &h) == ME_EIO);

  // YUV: a short last frame is not a frame; out-of-range indices are refused
  const std::string yuv = tmp_path("f.yuv");
  std::vector<uint8_t> frames(2 * W * H + W * H / 2);
  for (auto& x : frames) x = (uint8_t)next_u64();
  write_bytes(yuv, frames);
  CHECK(me_yuv_frame_count(yuv.c_str(), W, H, ME_YUV_LUMA) == 2);
  std::vector<uint8_t> dst(W * H);
  CHECK(me_yuv_read_luma(yuv.c_str(), W, H, ME_YUV_LUMA, 1, dst.data(), W) == ME_OK);
  CHECK(memcmp(dst.data(), frames.data() + W * H, W * H) == 0);
  CHECK(me_yuv_read_luma(yuv.c_str(), W, H, ME_YUV_LUMA, 2, dst.data(), W) != ME_OK);
  CHECK(me_yuv_read_luma(yuv.c_str(), W, H, ME_YUV_LUMA, -1, dst.data(), W) != ME_OK);
  CHECK(me_yuv_read_luma(yuv.c_str(), W, H, ME_YUV_I420, 1, dst.data(), W) != ME_OK);
  CHECK(me_yuv_read_luma(yuv.c_str(), 0, H, ME_YUV_LUMA, 0, dst.data(), W) != ME_OK);
  CHECK(me_yuv_frame_count(tmp_path("missing.yuv").c_str(), W, H, ME_YUV_LUMA) == -1);
  unlink(good.c_str());
  unlink(bad.c_str());
  unlink(yuv.c_str());
}

// umulhi(x, m) == x / d for x = 0, step, ... < n
static bool divides(uint32_t m, uint32_t d, uint32_t n, uint32_t step) {
  for (uint32_t x = 0; x < n; x += step)
    if ((uint32_t)(((uint64_t)x * m) >> 32) != x / d) return false;
  return true;
}

// What the item and flow kernels rely on in an accepted plan.
// (min_slots: 4, or less where a tuning override cuts the flow kernel's ring)
static void check_plan(const me::PlanShape& s, const me::QsadGeom& g, int K, bool flow,
                       int min_slots = 4) {
  CHECK(g.row0 == 0 && g.nrows == 0);
  CHECK(g.tb >= 1 && g.groups >= 1 && g.cpp >= 1 && g.chunks >= g.cpp);
  CHECK(g.pitch % 32 == 16);
  CHECK(g.rows_alloc == g.cpp * K + s.blk - 1);
  CHECK(g.tile_bytes == g.rows_alloc * g.pitch);
  CHECK(g.nbx_full == s.width / s.blk);
  CHECK(g.wg_per_row == (g.nbx_full + g.tb - 1) / g.tb);
  // the magic divisors, each over the range its comment in QsadGeom states
  CHECK(divides(g.pitch_magic, (uint32_t)g.pitch, (uint32_t)g.tile_bytes, flow ? 16 : 4));
  CHECK(divides(g.magic_groups, (uint32_t)g.groups, (uint32_t)(g.tb * g.groups * g.cpp), 1));
  if (g.tb > 1)  // (one-block items take no division)
    CHECK(divides(g.magic_tb, (uint32_t)g.tb, (uint32_t)(g.tb * g.cpp), 1));
  if (g.magic_wpr)
    CHECK(divides(g.magic_wpr, (uint32_t)g.wg_per_row, (uint32_t)(g.wg_per_row * s.rows), 1));
  if (flow) {
    CHECK(g.lds <= 160 * 1024);
    CHECK(g.flow_slots >= min_slots && g.flow_slots <= 16);
    CHECK((g.tb * g.groups * g.chunks) % 64 == 0);
    CHECK(g.threads == 1024 && g.fold == 1 && g.tile16 == 1 && g.magic_wpr == 0);
  } else {
    CHECK(g.lds <= me::QSAD_LDS_BUDGET + 16);
    CHECK(g.flow_slots == 0);
    CHECK(!g.tile16 || g.aligned);
    // DMA staging: no 4-byte granule may straddle the end of a frame row (the
    // range check would zero the last resident row's last pixels)
    CHECK(!g.aligned || s.width % 4 == 0);
  }
}

static void valu_planners() {
  const int cu_counts[] = {64, 256, 304};
  const int odd_blks[] = {0, 4, 12, 32};
  int accepted = 0;
  for (int t = 0; t < 2500; t++) {
    me::PlanShape s;
    s.width = 1 + (int)(next_u64() % 8000);
    s.height = 1 + (int)(next_u64() % 4400);
    s.stride = s.width + (next_u64() % 3 ? 0 : (int)(next_u64() % 64));
    s.blk = next_u64() % 8 ? (next_u64() % 2 ? 16 : 8) : odd_blks[next_u64() % 4];
    s.range = (int)(next_u64() % 301);
    if (next_u64() % 2) s.range &= ~15;  // the fold and flow rules want multiples of 4, 8, 16
    if (next_u64() % 4 == 0) s.width &= ~15, s.stride = s.width;
    s.cost = (int)(next_u64() % 2);
    s.rows = 1 + (int)(next_u64() % 9000);
    // planes at every alignment (never dereferenced)
    const uintptr_t mods[] = {0, 0, 0, 4, 8, 1, 2};
    s.align = me::align_class(s.stride, (const void*)(0x10000 + mods[next_u64() % 7]),
                              (const void*)(0x20000 + mods[next_u64() % 7]));
    const int cus = cu_counts[next_u64() % 3];
    // every fourth shape under a tuning override: refused, or as forced
    me::Tuning tu;
    if (t % 4 == 3) {
      const int ks[] = {0, 5, 8, 11, 13, 26};
      tu.plan_k = ks[next_u64() % 6];
      tu.plan_tb = (int)(next_u64() % 17);
      tu.plan_fold = (int)(next_u64() % 3) - 1;
    }
    me::QsadGeom g;
    int K = 0;
    if (me::plan_fast(s, cus, tu, &g, &K)) {
      accepted++;
      CHECK(s.blk == 8 || s.blk == 16);
      CHECK(s.range >= 1 && s.range <= 255 && s.width >= s.blk);
      check_plan(s, g, K, false);
      CHECK(!tu.plan_k || K == tu.plan_k);
      CHECK(!tu.plan_tb || g.tb == tu.plan_tb);
      CHECK(tu.plan_fold < 0 || g.fold == tu.plan_fold);
    }
    if (me::plan_flow(s, cus, tu, &g)) {
      accepted++;
      CHECK(s.cost == me::COST_SAD && s.blk == 16 && s.range == 32 && s.align == me::ALIGN_ALL);
      CHECK((long)g.wg_per_row * s.rows >= 2L * cus);
      check_plan(s, g, 13, true);
      CHECK(!tu.plan_tb || g.tb == tu.plan_tb);
    }
  }
  CHECK(accepted > 1000);
  // the flow kernel's shapes are rare in the draw above: its own pass
  for (int t = 0; t < 400; t++) {
    me::PlanShape s{16 * (1 + (int)(next_u64() % 500)), 1080, 0, 16, 32, me::COST_SAD,
                    1 + (int)(next_u64() % 2000), me::ALIGN_ALL};
    s.stride = s.width + 16 * (int)(next_u64() % 4);
    me::Tuning tu;
    if (t % 4 == 3) tu.plan_tb = 1 + (int)(next_u64() % 8), tu.flow_slots = 2 + (int)(next_u64() % 15);
    me::QsadGeom g;
    if (!me::plan_flow(s, cu_counts[t % 3], tu, &g)) continue;
    // the override may cut the ring below the 4 slots the planner asks for
    if (tu.flow_slots) CHECK(g.flow_slots <= tu.flow_slots);
    check_plan(s, g, 13, true, tu.flow_slots && tu.flow_slots < 4 ? tu.flow_slots : 4);
    CHECK(!tu.plan_tb || g.tb == tu.plan_tb);
  }
}

// What launch_bw and the band-walk kernel rely on in a plan for `jobs` jobs
// per launch (g.nrows counts a partial bottom row, the walk's rows do not).
static void check_bw(const me::MfmaGeom& g, int jobs) {
  const int rows = g.nrows - (g.hb_row >= 0 ? 1 : 0);
  CHECK(g.bw == 1 && rows >= 1);
  CHECK(g.bw_strips * g.bw_cols >= g.nbx && (g.bw_strips - 1) * g.bw_cols < g.nbx);
  CHECK(g.bw_segs >= 1 && g.bw_seg_rows >= 1);
  CHECK((long)g.bw_segs * g.bw_seg_rows >= rows);
  CHECK((long)(g.bw_segs - 1) * g.bw_seg_rows < rows);  // no segment is empty
  CHECK(g.bw_wpc * g.bw_cols == g.bw_nsw);
  const int inst[6][2] = {{6, 160}, {4, 160}, {3, 160}, {3, 224}, {2, 160}, {2, 224}};  // launch_bw's
  bool found = false;
  for (auto& i : inst) found |= g.bw_cols == i[0] && g.bw_lp == i[1];
  CHECK(found && g.bw_ns == 2 && g.bw_nsw == 12 && g.bw_pw == 4);
  CHECK(g.lds <= 160 * 1024);
  CHECK(g.lds == me::bw_lds_bytes(g.bw_lp, g.bw_pp, g.bw_ns, g.bw_nsw) +
                     me::bw_lds_hb_bytes(g.bw_pp, g.bw_ns, g.bw_hb));
  CHECK(g.bw_hb == 0 || g.hb_row >= 0);
  if (!g.bw_xt) return;
  // per-XCD tail split: the launch's grid, decoded as bw_item decodes it,
  // covers every row of every strip item once
  CHECK(g.bw_segs == 1 && g.bw_seg_rows == rows && g.bw_cx >= 1);
  const int U = jobs * g.bw_strips, q = U >> 3, rem = U & 7;
  const long grid = me::bw_xt_grid(U, g.bw_cx, rows);
  CHECK(grid % 8 == 0 && grid < (1L << 31));
  std::vector<int> covered(U, 0);
  for (long b = 0; b < grid; b++) {
    const int x = (int)(b & 7), m = (int)(b >> 3);
    const int nx = q + (x < rem ? 1 : 0), u0 = x * q + (x < rem ? x : rem);
    int mainx, kx, st, L;
    me::bw_xcd_split(nx, g.bw_cx, rows, &mainx, &kx, &st, &L);
    if (m < mainx) {
      covered[u0 + m] += rows;
      continue;
    }
    const int t = m - mainx;
    if (t >= kx * st) continue;
    const int seg = t / kx, r0 = seg * L;
    CHECK(r0 < rows);
    covered[u0 + mainx + t % kx] += (r0 + L < rows ? r0 + L : rows) - r0;
  }
  for (int u = 0; u < U; u++) CHECK(covered[u] == rows);
}

// The matrix-core SSD planners (me_mfma_plan.cpp) over random shapes, paths,
// CU counts, job counts and the tuning overrides that keep a plan valid.
static void mfma_planners() {
  const int cu_counts[] = {64, 256, 304};
  int accepted = 0, walks = 0, batches = 0;
  for (int t = 0; t < 6000; t++) {
    me::MfmaShape s;
    s.width = 1 + (int)(next_u64() % (t % 16 ? 4200 : 17000));
    s.height = 1 + (int)(next_u64() % (t % 16 ? 2400 : 17000));
    if (next_u64() % 4) s.width = (s.width + 15) & ~15;  // (else a partial right column)
    s.stride = s.width + (next_u64() % 3 ? 0 : 4 * (int)(next_u64() % 16));
    if (next_u64() % 2) s.stride = (s.stride + 15) & ~15;
    s.blk = next_u64() % 8 ? (next_u64() % 4 ? 16 : 8) : (int)(next_u64() % 33);
    s.range = next_u64() % 3 ? 1 + (int)(next_u64() % 64) : (int)(next_u64() % 260);
    s.cost = next_u64() % 16 ? me::COST_SSD : me::COST_SAD;
    const int blk = s.blk > 0 ? s.blk : 1, nby = (s.height + blk - 1) / blk;
    s.row_begin = next_u64() % 2 ? 0 : (int)(next_u64() % (nby + 1));
    s.row_end = next_u64() % 2 ? nby : s.row_begin + (int)(next_u64() % (nby - s.row_begin + 1));
    s.nbx = (s.width + blk - 1) / blk;
    const uintptr_t mods[] = {0, 0, 0, 0, 0, 0, 0, 4, 8, 2};
    s.align = me::align_class(s.stride, (const void*)(0x10000 + mods[next_u64() % 10]),
                              (const void*)(0x20000 + mods[next_u64() % 10]));
    s.merge_tiles = next_u64() % 4 ? me::mfma_merge_tiles(s) : (next_u64() % 2 ? 0 : 7);
    const int path = (int)(next_u64() % 5), cus = cu_counts[next_u64() % 3];
    me::Tuning tu;
    if (t % 4 == 3) {
      tu.mfma_s2k = (int)(next_u64() % 3) - 1;
      tu.mfma_s2r = (int)(next_u64() % 3);
      tu.mfma_batch = next_u64() % 4 ? -1 : 0;
      tu.bw = next_u64() % 4 ? -1 : 0;
      tu.bw_hb = next_u64() % 2 ? -1 : 0;
      tu.bw_xt = next_u64() % 2 ? -1 : 0;
      tu.bw_seg = next_u64() % 2 ? 0 : 1 + (int)(next_u64() % 40);
    }
    me::MfmaGeom g;
    if (!me::plan_mfma_ssd(s, path, cus, tu, &g)) {
      me::MfmaBatch b;
      CHECK(!me::plan_mfma_batch(s, 8, me::MFMA_SCRATCH_UNLIMITED, path, cus, tu, &b));
      CHECK(b.jobs == 0 && b.need == 0);
      continue;
    }
    accepted++;
    CHECK(path != 1 && s.cost == me::COST_SSD && (s.blk == 8 || s.blk == 16) && s.range >= 1);
    CHECK(s.align & me::ALIGN_4);
    CHECK(!g.rp && !g.s2 && !g.s2h && !g.mkeys && !g.mcnt);  // the launchers bind them
    CHECK(g.row0 == s.row_begin && g.nrows >= 1 && g.row0 + g.nrows <= s.row_end);
    CHECK(g.nbx == s.width / s.blk && g.nbx >= 1);
    // (b) LDS: what a CU has, and 64 KB unless the launcher raises the limit
    // (the 8x8 kernel, the tile kernel and the band walk call lds_attr)
    CHECK(g.lds > 0 && g.lds <= 160 * 1024);
    if (g.bm && !g.bw) CHECK(g.lds <= 64 * 1024);
    // (c) the planes: the arithmetic the prepass and the kernels index by
    CHECK(g.ya0 >= 0 && g.rp_rows >= 1 && g.ya0 + g.rp_rows <= s.height);
    CHECK(g.rows_alloc >= g.rp_rows + 16 && g.pitch >= s.width && g.pitch % 16 == 0);
    const uint64_t plane = (uint64_t)g.rows_alloc * g.pitch;
    const uint64_t n_s2 = s.blk == 16 && g.hb < 16 ? 2 : 1;
    CHECK(g.rp_bytes == (s.blk == 16 ? plane : 0) && g.s2_bytes == n_s2 * 4 * plane);
    CHECK(g.s2h_off == (s.blk == 16 ? 4 * plane : 0));
    const uint64_t all = (((uint64_t)g.rp_bytes + 255) & ~(uint64_t)255) + g.s2_bytes;
    CHECK(all < (1ull << 31));
    CHECK(g.scratch_bytes == (g.bw || g.bmv ? 0 : all));
    CHECK(g.hb_row < 0 || (g.hb < 16 && g.hb_row == s.row_end - 1 && g.s2h_row0 >= 0));
    // (e) the tile kernel's instances
    if (s.blk == 16 && !g.bm) {
      CHECK((g.ngxw == 1 || g.ngxw == 2) && (g.km == 2 || g.km == 3) && g.ngx >= 1 && g.ngx <= 4);
      CHECK((g.ngx + g.ngxw - 1) / g.ngxw == 1 || s.merge_tiles >= me::mfma_merge_tiles(s));
    }
    if (g.bmv) CHECK(g.bm && g.bm_lp == me::BMV_LP && (g.bmv_r == 1 || g.bmv_r == 2));
    if (g.bm) CHECK(me::wgs_per_job(g) >= 1);  // (the block-major kernels' grid)
    // (d) the band walk, as the single plan and re-planned for more jobs
    if (g.bw) check_bw(g, 1);
    const int jobs = 1 + (int)(next_u64() % 40);
    if (s.blk == 16) {
      me::MfmaGeom w = g;
      if (me::plan_bw(s, cus, tu, &w, jobs)) {
        walks++;
        check_bw(w, jobs);
        CHECK(me::bw_one_round(w, jobs, cus) == ((long)jobs * w.bw_strips * w.bw_segs <= cus));
      }
    }
    // (a) the batch: what the context sizes is what the launcher gets
    me::MfmaBatch need, got;
    CHECK(me::plan_mfma_batch(s, jobs, me::MFMA_SCRATCH_UNLIMITED, path, cus, tu, &need));
    CHECK(need.jobs == 0 || (need.jobs >= 2 && need.jobs <= jobs && need.jobs <= me::MAX_JOBS));
    CHECK(need.need >= (size_t)need.jobs * need.stride && need.need >= g.scratch_bytes);
    CHECK((need.stride == 0) == (need.jobs == 0 || need.g.bw || need.g.bmv));
    if (need.jobs) {
      batches++;
      CHECK(need.g.bm && need.g.nbx == s.nbx && need.stride % 256 == 0);
      CHECK(need.stride == 0 || need.stride >= need.g.scratch_bytes);
      if (need.g.bw) check_bw(need.g, need.jobs);
    }
    CHECK(me::plan_mfma_batch(s, jobs, need.need, path, cus, tu, &got));
    CHECK(got.jobs == need.jobs && got.stride == need.stride);  // sized once, launched as sized
    const size_t avail = next_u64() % 2 ? 0 : (size_t)(next_u64() % (need.need + 1));
    CHECK(me::plan_mfma_batch(s, jobs, avail, path, cus, tu, &got));
    CHECK((size_t)got.jobs * got.stride <= avail && got.jobs <= need.jobs && got.jobs != 1);
  }
  CHECK(accepted > 2000 && walks > 800 && batches > 600);
}

// One pass over the dispatcher's case table: each launch's rectangles painted
// into a grid per job; `cap` launches per dispatch call.
static void dispatch_pass(const std::vector<std::string>& lines, int cap) {
  const me::Tuning tu;
  DispatchCase c;
  int cases = 0;
  for (const std::string& line : lines) {
    if (!parse_dispatch_case(line.c_str(), 256, tu, &c)) continue;
    cases++;
    const int B = c.s.blk, nby = (c.s.height + B - 1) / B, nbx = (c.s.width + B - 1) / B;
    const int nj = (int)c.jobs.size();
    const std::vector<me::Launch> list = dispatch_all(c, 256, tu, cap);
    std::vector<int> grid((size_t)nj * nby * nbx, 0);
    for (const me::Launch& l : list) {
      CHECK(l.kind >= me::LAUNCH_GENERIC && l.kind <= me::LAUNCH_SSIM);
      CHECK(l.job0 >= 0 && l.njobs >= 1 && l.njobs <= me::MAX_JOBS && l.job0 + l.njobs <= nj);
      CHECK(l.njobs == 1 || l.kind == me::LAUNCH_ITEM || l.kind == me::LAUNCH_FLOW || l.kind == me::LAUNCH_MFMA);
      CHECK(0 <= l.bx0 && l.bx0 <= l.bx1 && l.bx1 <= nbx);
      if (l.kind == me::LAUNCH_MFMA) {  // (the kernels cover the plan's rectangle, not the launch's)
        CHECK((size_t)(l.njobs - 1) * l.scratch_stride + l.mg.scratch_bytes <= c.s.scratch_bytes);
        CHECK(l.mg.row0 == l.row_lo && l.mg.row0 + l.mg.nrows == l.row_hi && l.bx0 == 0 && l.mg.nbx == l.bx1);
      }
      for (int j = l.job0; j < l.job0 + l.njobs; j++) {
        const int r0 = me::launch_r0(l, c.jobs[j]), r1 = me::launch_r1(l, c.jobs[j]);
        CHECK(r1 <= r0 || (r0 >= c.jobs[j].r0 && r1 <= c.jobs[j].r1));
        for (int r = r0; r < r1; r++)
          for (int bx = l.bx0; bx < l.bx1; bx++) grid[((size_t)j * nby + r) * nbx + bx]++;
      }
    }
    for (int j = 0; j < nj; j++)
      for (int r = 0; r < nby; r++)
        for (int bx = 0; bx < nbx; bx++)
          CHECK(grid[((size_t)j * nby + r) * nbx + bx] == (r >= c.jobs[j].r0 && r < c.jobs[j].r1 ? 1 : 0));
  }
  CHECK(cases > 100);
}

static void dispatcher() {
  std::vector<std::string> lines;
  FILE* f = fopen(DISPATCH_TABLE, "r");
  CHECK(f != nullptr);
  static char line[1 << 16];
  while (fgets(line, sizeof line, f)) lines.push_back(line);
  fclose(f);
  std::vector<std::thread> th;
  for (int cap : {1, 3, 64, 1024}) th.emplace_back(dispatch_pass, std::cref(lines), cap);
  for (std::thread& t : th) t.join();
}

// Regions back to back, each aligned to its element, and the total the entry
// points asked for before the layouts were functions.
static void check_layout(const me::rules::Layout& L, size_t total) {
  size_t end = 0;
  for (int k = 0; k < L.n; k++) {
    CHECK(L.off[k] == end && L.off[k] % L.elem[k] == 0 && L.bytes[k] % L.elem[k] == 0);
    end += L.bytes[k];
  }
  CHECK(end <= total && L.total == total);
}

static void api_rules() {
  FILE* f = fopen(API_ARGS_TABLE, "r");
  CHECK(f != nullptr);
  static char line[1 << 14];
  char err[512];
  ApiCase c;
  std::vector<std::string> fns;
  int cases = 0;
  while (fgets(line, sizeof line, f)) {
    if (!parse_api_case(line, &c)) continue;
    cases++;
    CHECK(run_api_case(c, c.ndev, err, sizeof err) == c.status && err[0]);
    if (fns.empty() || fns.back() != c.fn) fns.push_back(c.fn);
  }
  fclose(f);
  CHECK(cases > 500 && fns.size() > 25);
  // wild values: refused or accepted, never an overflow or a wild read
  int ApiCase::* const ints[] = {&ApiCase::width, &ApiCase::height, &ApiCase::stride, &ApiCase::blk,
                                 &ApiCase::range, &ApiCase::cost, &ApiCase::n_frames, &ApiCase::refine,
                                 &ApiCase::r0, &ApiCase::r1, &ApiCase::ref_row0, &ApiCase::cur_row0,
                                 &ApiCase::num_blks};
  long long ApiCase::* const sizes[] = {&ApiCase::fs_ref, &ApiCase::fs_cur, &ApiCase::fs_ref1};
  for (const std::string& fn : fns)
    for (int ndev : {1, 2}) {
      ApiCase w;
      w.fn = fn;
      CHECK(run_api_case(w, ndev, err, sizeof err) >= 0);  // (a known entry point)
      for (int v : {INT_MAX, INT_MIN, -INT_MAX}) {
        for (auto m : ints) {
          w = ApiCase{};
          w.fn = fn;
          w.*m = v;
          (void)run_api_case(w, ndev, err, sizeof err);
          w.r0 = w.r1 = v;  // ... and with the rows at the same end
          (void)run_api_case(w, ndev, err, sizeof err);
        }
        w = ApiCase{};
        w.fn = fn;
        w.lambda = (uint32_t)v;
        (void)run_api_case(w, ndev, err, sizeof err);
      }
      for (auto m : sizes)
        for (int n_frames : {1, 2, 4096}) {
          w = ApiCase{};
          w.fn = fn;
          w.n_frames = n_frames;
          w.*m = -1;  // SIZE_MAX
          const int s = run_api_case(w, ndev, err, sizeof err);
          // where a stride that large is read (n_frames > 1), the stack is past 2 GiB
          bool batched = false;
          for (const char* b : {"me_full_search_batch_device", "me_refine_qpel_device", "me_bipred_device",
                                "me_partition_search_device", "me_rd_search_device",
                                "me_refine_qpel_rd_device", "me_partition_rd_search_device"})
            batched |= fn == b;
          if (n_frames > 1 && batched && (m != sizes[2] || fn == "me_bipred_device")) CHECK(s != ME_OK);
        }
    }
  for (int t = 0; t < 2000; t++) {
    const int W = 1 + (int)(next_u64() % 8000), H = 1 + (int)(next_u64() % 4400);
    const int B = 2 * (1 + (int)(next_u64() % 32));
    int n[4];
    CHECK(me_partition_counts(W, H, B, n) == ME_OK);
    const size_t nb = (size_t)me_num_blocks(W, H, B);
    const size_t cells = (size_t)n[0] + n[1] + n[2] + n[3], n0 = (size_t)n[0];
    check_layout(me::rules::layout_mv_cost(nb), 8 * nb);
    check_layout(me::rules::layout_bipred(nb), 28 * nb);
    check_layout(me::rules::layout_rd(nb), (17 * nb + 7) / 8 * 8);
    check_layout(me::rules::layout_partition(n), (8 * cells + 5 * n0 + 7) / 8 * 8);
    check_layout(me::rules::layout_partition_rd(n), (13 * cells + 9 * n0 + 7) / 8 * 8);
  }
}

int main() {
  pool();
  planner();
  files();
  valu_planners();
  mfma_planners();
  dispatcher();
  api_rules();
  printf("san ok\n");
  return 0;
}
