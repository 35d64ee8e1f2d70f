// me_dispatch.h -- which kernel family searches which blocks of which job
// (me_dispatch.cpp: host-only, pure).  Like the planners it needs no HIP: the
// executor (launch_jobs, me_kernels.hip) walks the list it returns, and the
// CPU harnesses (oracle/dispatch_dump.cc, oracle/san_main.cc) read it.
#pragma once
#include "me_geom.h"
#include "me_mfma_geom.h"

namespace me {

// What the jobs of one call share: the frame, the search, and what the
// context lends it (tiles its merge buffers cover, bytes of its scratch; 0
// without the buffers).
struct SearchShape {
  int width, height, stride, blk, range, cost;
  size_t merge_tiles, scratch_bytes;
};

enum LaunchKind { LAUNCH_GENERIC, LAUNCH_ITEM, LAUNCH_FLOW, LAUNCH_MFMA, LAUNCH_SSIM };

// One step of the executor: `kind` over jobs [job0, job0 + njobs), of job J
// the block rows [max(J.r0, row_lo), min(J.r1, row_hi)) x columns [bx0, bx1).
// GENERIC and SSIM serve one job.  An MFMA launch is every kernel of its plan
// (prepass + main kernel; the band walk and its bottom-row launch): they
// share the rectangle.  ITEM and FLOW launches are issued even when their
// rectangles are empty (the executor then enqueues nothing): `path` is noted
// either way.
struct Launch {
  int kind;
  int path;  // ME_SEARCH_PATH_* code the executor notes (note_path); 0: the kernel's launcher does
  int job0, njobs;
  int row_lo, row_hi, bx0, bx1;
  QsadGeom g;  // ITEM, FLOW
  int K;       // ITEM: the me_fast_kernel instance's rows per chunk
  MfmaGeom mg;  // MFMA (pointers null: the executor binds them)
  size_t scratch_stride;  // MFMA: bytes between the jobs' prepass planes
};
inline int launch_r0(const Launch& l, const SearchJob& J) { return J.r0 > l.row_lo ? J.r0 : l.row_lo; }
inline int launch_r1(const Launch& l, const SearchJob& J) { return J.r1 < l.row_hi ? J.r1 : l.row_hi; }

// The launches that search every block of jobs [0, n) exactly once, in
// stream order, for the kernel path code `path` (me_tuning.h) on a device of
// `cus` CUs.  Of a job the dispatcher reads the rows, ref_row0 / cur_row0 and
// the pointer values (alignment); it dereferences nothing.  Two steps, so
// that a list of any length is planned once:
//
// dispatch_batch: the launches that take jobs [0, n) together (n >= 2), or
// -1: they run job by job.  Returns the number of launches and writes those
// numbered [skip, skip + cap) to out: a caller whose array is too small calls
// again with the next skip (same arguments, same list; the plans are cached).
int dispatch_batch(const SearchShape& s, const SearchJob* jobs, int n, int path, int cus,
                   const Tuning& tu, int skip, Launch* out, int cap);
// dispatch_job: the launches of job j by itself (a single search; a job of a
// refused batch), at most DISPATCH_JOB_MAX, into out.  Returns their number.
constexpr int DISPATCH_JOB_MAX = 5;  // MFMA, its right column, the rest row's qsad launch and leftovers
int dispatch_job(const SearchShape& s, const SearchJob* jobs, int j, int path, int cus,
                 const Tuning& tu, Launch* out);

}  // namespace me
