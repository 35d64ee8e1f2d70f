// me_dispatch.cpp -- the search dispatch (host-only C++, pure): which kernel
// family searches which blocks of which job, as a launch list (me_dispatch.h).
// A single search is a list of one job: there is one route.  What it must
// guarantee is coverage: every block of every job's [r0, r1) x [0, nbx) is
// written by exactly one launch (tests/test_dispatch.py paints the lists of
// oracle/dispatch_dump.cc; oracle/san_main.cc runs it under the sanitizers).
//
// The order of the decisions (plans depend on the rows planned for, so a
// batch refused as a whole may be accepted job by job):
//   1. SSIM: job by job.
//   2. SAD on the flow kernel: one plan over every job's rows.
//   3. two or more equal SSD jobs on the matrix cores (plan_mfma_batch).
//   4. two or more jobs on the item kernel, unless the matrix cores take job 0.
//   5. job by job: matrix cores (the generic kernel for the partial right
//      column, the VALU route for the rows the 8x8 kernel leaves), else the
//      flow kernel, else the item kernel, else the generic kernel.
#include "me_dispatch.h"

#include "me_tuning.h"

namespace me {
namespace {

struct Ctx {
  const SearchShape& s;
  const SearchJob* jobs;
  int path, cus;
  const Tuning& tu;
  int nbx, nby;
  int skip, cap, count;
  Launch* out;
  Launch spare;  // where a launch outside [skip, skip + cap) is written
};

Launch& emit(Ctx& c, int kind, int path, int job0, int njobs, int row_lo, int row_hi, int bx0, int bx1) {
  const int i = c.count++ - c.skip;
  Launch& l = i >= 0 && i < c.cap ? c.out[i] : c.spare;
  l.kind = kind;
  l.path = path;
  l.job0 = job0;
  l.njobs = njobs;
  l.row_lo = row_lo;
  l.row_hi = row_hi;
  l.bx0 = bx0;
  l.bx1 = bx1;
  return l;
}

PlanShape plan_shape(const Ctx& c, int rows, const SearchJob& J) {
  const SearchShape& s = c.s;
  return {s.width, s.height, s.stride, s.blk, s.range, s.cost, rows, align_class(s.stride, J.ref, J.cur)};
}

// End of the full-height (and h = B/2) rows of [.., r1) the qsad bodies take;
// a bottom row of another height goes to the generic kernel.
int qsad_rows_end(const Ctx& c, int r1) {
  const int h_last = c.s.height - (c.nby - 1) * c.s.blk;
  return r1 == c.nby && h_last != c.s.blk && h_last != c.s.blk / 2 ? r1 - 1 : r1;
}

void generic(Ctx& c, int path, int job, int r0, int r1, int bx0, int bx1) {
  if (r1 > r0 && bx1 > bx0) emit(c, LAUNCH_GENERIC, path, job, 1, r0, r1, bx0, bx1);
}

// The rows and columns of jobs [j0, j0 + n), each from row lo on, that a qsad
// kernel planned with nbx_full full blocks per row leaves (a bottom row of
// another height, the partial right column): the generic kernel, job by job.
void leftovers(Ctx& c, int j0, int n, int lo, int nbx_full) {
  for (int j = j0; j < j0 + n; j++) {
    const int r0 = c.jobs[j].r0 > lo ? c.jobs[j].r0 : lo, r1 = c.jobs[j].r1;
    if (r1 <= r0) continue;  // (an empty job at the frame's bottom has no bottom row either)
    generic(c, 1, j, qsad_rows_end(c, r1), r1, 0, nbx_full);
    generic(c, 1, j, r0, r1, nbx_full, c.nbx);
  }
}

// SAD jobs [j0, j0 + n) (rows from lo on) on the flow kernel where its plan,
// made over every job's rows, takes them: all in one launch (MAX_JOBS jobs per
// launch).  Past the LDS ring a slot is refilled when its item's last
// wave-task ends; with the fairness check in the kernel (QsadGeom::fair) that
// wave-task no longer lags, and one launch of 8 1080p frames takes 62.5-63 us
// per frame against 71.4 for back-to-back single-frame launches on the same
// box (without the check: 80.9 us, waves spinning on unpublished slots;
// profiles/r03ac_fair_sweep.jsonl).  Tuning build: ME_FLOW_ONE=0 cuts a batch
// into launches of about one ring.  False: the flow kernel does not apply.
bool flow_jobs(Ctx& c, int j0, int n, int lo) {
  if (c.s.cost != COST_SAD) return false;
  const SearchJob* jobs = c.jobs + j0;
  auto begin = [&](int i) { return jobs[i].r0 > lo ? jobs[i].r0 : lo; };
  int rows = 0;  // the planner counts tiles over every job's rows
  for (int i = 0; i < n; i++) {
    rows += jobs[i].r1 - begin(i);
    if ((uintptr_t)jobs[i].ref % 16 || (uintptr_t)jobs[i].cur % 16) return false;
  }
  QsadGeom g;
  if (!cached_plan(PLAN_FLOW, plan_shape(c, rows, jobs[0]), c.cus, c.tu, &g, nullptr)) return false;
  auto tiles_of = [&](int i) { return (long)g.wg_per_row * (qsad_rows_end(c, jobs[i].r1) - begin(i)); };
  long total = 0;
  for (int i = 0; i < n; i++) total += tiles_of(i);
  const long ring = c.tu.flow_one != 0 ? (1L << 40) : (long)g.flow_slots * c.cus;
  const long nl = (total + ring - 1) / ring;  // launches of about total / nl tiles
  const long target = nl > 1 ? (total + nl - 1) / nl : total;
  const int hi = qsad_rows_end(c, c.nby);
  int first = 0;
  long tiles = 0;
  for (int i = 0; i <= n; i++) {
    if (i > first && (i == n || tiles + tiles_of(i) > target || i - first == MAX_JOBS)) {
      emit(c, LAUNCH_FLOW, 1, j0 + first, i - first, lo, hi, 0, g.nbx_full).g = g;
      first = i;
      tiles = 0;
    }
    if (i < n) tiles += tiles_of(i);
  }
  leftovers(c, j0, n, lo, g.nbx_full);
  return true;
}

// VALU jobs [0, n) the item kernel takes (SAD, or SSD off the matrix cores)
// in one launch per MAX_JOBS: per-job launches each paid the persistent
// grid's fill and drain (8 stripes of a 4K frame: 1.165 ms against 1.047 for
// the frame).  False when the jobs' planes differ in alignment class or the
// item kernel does not take the shape.
bool item_jobs(Ctx& c, int n) {
  if (c.s.cost != COST_SAD && c.s.cost != COST_SSD) return false;
  // (the item planner reads nothing of cur's 16-byte alignment)
  const int item_bits = ALIGN_4 | ALIGN_REF16;
  const int ac = align_class(c.s.stride, c.jobs[0].ref, c.jobs[0].cur) & item_bits;
  int rows = 0;  // the planner counts tiles over every job's rows
  for (int i = 0; i < n; i++) {
    rows += c.jobs[i].r1 - c.jobs[i].r0;
    if ((align_class(c.s.stride, c.jobs[i].ref, c.jobs[i].cur) & item_bits) != ac) return false;
  }
  QsadGeom g;
  int K = 0;
  if (!cached_plan(PLAN_ITEM, plan_shape(c, rows, c.jobs[0]), c.cus, c.tu, &g, &K)) return false;
  // Every job shares the launch, however large: with whole frames per XCD band
  // the bands need no halo rows.  8K 8x8 +-128, 16 frames: 17.09 ms and 70.7 MB
  // read per frame in one row-major launch, against 17.26 ms and 89.9 MB one
  // launch per frame (profiles/r04m_variants_8k.txt; round 3 measured the
  // opposite, 124 vs 98 MB, with tiles claimed two ahead).  Row-major: the
  // strip walk, which keeps a single wide frame's window rows in L2, only
  // spreads a batch's working set (same run: strips of 16 tiles 87.9 MB).
  const int per = c.tu.item_batch == 0 ? 1 : MAX_JOBS;  // tuning build: ME_ITEM_BATCH=0
  if (c.tu.strip < 0) g.strip_w = 0;
  for (int i0 = 0; i0 < n; i0 += per) {
    Launch& l = emit(c, LAUNCH_ITEM, 1, i0, n - i0 < per ? n - i0 : per, 0, qsad_rows_end(c, c.nby), 0,
                     g.nbx_full);
    l.g = g;
    l.K = K;
  }
  leftovers(c, 0, n, 0, g.nbx_full);
  return true;
}

MfmaShape mfma_shape(const Ctx& c, const SearchJob& J) {
  const SearchShape& s = c.s;
  return {s.width, s.height, s.stride, s.blk, s.range, s.cost, J.r0, J.r1, c.nbx,
          align_class(s.stride, J.ref, J.cur), s.merge_tiles};
}

// The matrix cores take job J on plan g: an SSD search they plan, with its
// prepass planes inside the scratch given (the band-walk and lean kernels
// need none: scratch_bytes 0).  Steps 4 and 5 both ask this; launch_jobs
// used to ask step 4 only whether there was a scratch at all, which never
// differed: attach_scratch sizes the scratch for the plan before any launch.
bool mfma_takes(const Ctx& c, const SearchJob& J, MfmaGeom* g) {
  return c.s.cost == COST_SSD && plan_mfma_ssd(mfma_shape(c, J), c.path, c.cus, c.tu, g) &&
         g->scratch_bytes <= c.s.scratch_bytes;
}

int mfma_path(const Ctx& c, const MfmaGeom& g) {  // ME_SEARCH_PATH_*
  return g.bw ? 3 : g.bmv ? 4 : c.s.blk == 8 ? 6 : g.bm ? 2 : 5;
}

// Equal-geometry SSD jobs [0, n) as plan_mfma_batch plans them for the
// scratch given.  False: they run job by job.
bool mfma_jobs(Ctx& c, int n) {
  const SearchJob* jobs = c.jobs;
  for (int i = 1; i < n; i++)  // one geometry: the same rows of same-sized frames
    if (jobs[i].r0 != jobs[0].r0 || jobs[i].r1 != jobs[0].r1 || jobs[i].ref_row0 != jobs[0].ref_row0 ||
        jobs[i].cur_row0 != jobs[0].cur_row0)
      return false;
  MfmaBatch b;
  if (!plan_mfma_batch(mfma_shape(c, jobs[0]), n, c.s.scratch_bytes, c.path, c.cus, c.tu, &b) || b.jobs < 2)
    return false;
  // the plan saw job 0's pointers only: every job's planes must meet the same
  // alignment (4-byte DMA sources; the block-major kernel's 16-byte cur row
  // loads), else the batch runs job by job, each planned on its own
  const int need = ALIGN_4 | (b.g.bm ? ALIGN_CUR16 : 0);
  for (int i = 1; i < n; i++)
    if ((align_class(c.s.stride, jobs[i].ref, jobs[i].cur) & need) != need) return false;
  for (int i0 = 0; i0 < n; i0 += b.jobs) {
    Launch& l = emit(c, LAUNCH_MFMA, mfma_path(c, b.g), i0, n - i0 < b.jobs ? n - i0 : b.jobs, jobs[0].r0,
                     jobs[0].r1, 0, b.g.nbx);
    l.mg = b.g;
    l.scratch_stride = b.stride;
  }
  return true;
}

// Rows [r0, r1) of job j on the VALU kernels.
void valu_job(Ctx& c, int j, int r0, int r1) {
  if (flow_jobs(c, j, 1, r0)) return;
  QsadGeom g;
  int K = 0;
  if (!cached_plan(PLAN_ITEM, plan_shape(c, r1 - r0, c.jobs[j]), c.cus, c.tu, &g, &K))
    return generic(c, 1, j, r0, r1, 0, c.nbx);
  Launch& l = emit(c, LAUNCH_ITEM, 1, j, 1, r0, qsad_rows_end(c, r1), 0, g.nbx_full);
  l.g = g;
  l.K = K;
  leftovers(c, j, 1, r0, g.nbx_full);
}

void one_job(Ctx& c, int j) {
  const SearchJob& J = c.jobs[j];
  if (J.r1 <= J.r0) return;
  if (c.s.cost == COST_SSIM) {
    emit(c, LAUNCH_SSIM, 0, j, 1, J.r0, J.r1, 0, c.nbx);
    return;
  }
  MfmaGeom mg;
  if (!mfma_takes(c, J, &mg)) return valu_job(c, j, J.r0, J.r1);
  // Matrix cores: every full-width block (the partial bottom row included);
  // the partial right column stays on the generic kernel.
  const int rest = mg.row0 + mg.nrows;  // < r1: a partial bottom row the MFMA kernel left (B = 8)
  const int path = mfma_path(c, mg);
  Launch& l = emit(c, LAUNCH_MFMA, path, j, 1, J.r0, rest, 0, mg.nbx);
  l.mg = mg;
  l.scratch_stride = 0;
  generic(c, path, j, J.r0, rest, mg.nbx, c.nbx);
  if (rest < J.r1) valu_job(c, j, rest, J.r1);
}

}  // namespace

int dispatch_batch(const SearchShape& s, const SearchJob* jobs, int n, int path, int cus,
                   const Tuning& tu, int skip, Launch* out, int cap) {
  Ctx c{s, jobs, path, cus, tu, (s.width + s.blk - 1) / s.blk, (s.height + s.blk - 1) / s.blk,
        skip, cap, 0, out, {}};
  if (n < 2) return -1;
  if (flow_jobs(c, 0, n, 0)) return c.count;
  // SSD jobs of one geometry share the matrix cores' launches (prepass planes
  // per job in the context scratch); others go one by one
  if (mfma_jobs(c, n)) return c.count;
  MfmaGeom mg;
  if (!mfma_takes(c, jobs[0], &mg) && item_jobs(c, n)) return c.count;
  return -1;
}

int dispatch_job(const SearchShape& s, const SearchJob* jobs, int j, int path, int cus,
                 const Tuning& tu, Launch* out) {
  Ctx c{s, jobs, path, cus, tu, (s.width + s.blk - 1) / s.blk, (s.height + s.blk - 1) / s.blk,
        0, DISPATCH_JOB_MAX, 0, out, {}};
  one_job(c, j);
  return c.count;
}

}  // namespace me
