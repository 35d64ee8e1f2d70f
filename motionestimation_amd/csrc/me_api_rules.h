// me_api_rules.h -- the C ABI's argument rules and the record-buffer layouts of
// its host entry points (include/me.h).  Host-only and pure: no HIP dependency,
// no context (oracle/api_rules_dump.cc and oracle/san_main.cc build it alone).
// A rule returns ME_OK, or the entry point's status with its me_last_error text
// in err[n].  Pointers are only compared with null; n_devs: the context's
// device count.  me_api.hip and me_api_stages.hip say in which order the rules
// apply.  Not installed.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "me.h"

namespace me {
namespace rules {

// SATD costs sub-pel candidates only: the composite entry points search at SAD.
inline me_cost search_cost(me_cost cost) { return cost == ME_COST_SATD ? ME_COST_SAD : cost; }
// The status s with the printf-style message in err[n]: how every rule refuses,
// and how an entry point refuses what takes a single `if` (a null output).
me_status fail(char* err, size_t n, me_status s, const char* fmt, ...);
// "<what> on <n_devs> devices (one device only)": ME_EUNSUPPORTED.
me_status one_device(int n_devs, const char* what, char* err, size_t n);

// Planes, geometry and cost of an integer search (me::check_args).
me_status args(const void* ref, const void* cur, int width, int height, int stride, int blk,
               int range, int cost, const void* mv, char* err, size_t n);
// A stripe's block rows [r0, r1) of nby and its planes' first rows against the
// stripe contract; the message is prefixed with "job <job>: " for job >= 0.
me_status stripe(int nby, int blk, int range, int r0, int r1, int ref_row0, int cur_row0, int job,
                 char* err, size_t n);

// A batch of n_frames frames: n_frames in [1, 4096]; then, plane by plane,
// frames do not overlap (frame_stride >= frame_bytes when n_frames > 1) and the
// plane stack stays below 2 GiB, so no frame address is formed from a wild
// stride.  No planes: the n_frames rule alone.
struct FramePlane {
  size_t frame_stride;
  unsigned long long frame_bytes;
};
me_status frame_batch(int n_frames, const FramePlane* planes, int n_planes, char* err, size_t n);

// The refinement's and the bi-prediction's own rules on top of args().
me_status qpel(int cost, const void* mv_q, char* err, size_t n);
me_status bipred(int cost, const void* ref1, const void* q1, const void* out0, const void* out1,
                 const void* mode, char* err, size_t n);
// Partition search; counts: the four grids' cell counts.  partition_rd: the
// same rules with the rate-constrained search's lambda limit.
me_status partition(int n_devs, const void* ref, const void* cur, int width, int height, int stride,
                    int blk, int range, int cost, uint32_t lambda, const me_part_fields* out,
                    int counts[4], char* err, size_t n);
me_status partition_rd(int n_devs, const void* ref, const void* cur, int width, int height,
                       int stride, int blk, int range, int cost, uint32_t lambda,
                       const me_part_rd_fields* out, int counts[4], char* err, size_t n);
// Partition-wise quarter-pel refinement of in's four integer grids into out
// (B, plane size, cost, lambda, one device; no search range).
me_status partition_qpel(int n_devs, const void* ref, const void* cur, int width, int height,
                         int stride, int blk, int cost, uint32_t lambda, const me_part_fields* in,
                         const me_part_rd_fields* out, int counts[4], char* err, size_t n);
me_status partition_leaf(int n_devs, int width, int height, int blk, int n_frames,
                         const me_part_fields* in, const void* leaf, char* err, size_t n);
// Rate-constrained search; rd_ctx: what its refinement shares with it.
me_status rd_ctx(int n_devs, uint32_t lambda, const char* what, char* err, size_t n);
me_status rd(int n_devs, const void* ref, const void* cur, int width, int height, int stride,
             int blk, int range, int cost, uint32_t lambda, const void* mv, const void* block_cost,
             char* err, size_t n);

// Per-element rules of the host entry points.  vectors: every component of
// n_fields fields of n_blocks vectors within +-max (max_name: its constant).
me_status vectors(const int16_t* const* fields, int n_fields, size_t n_blocks, int max,
                  const char* max_name, char* err, size_t n);
me_status pred_modes(const uint8_t* mode, size_t n_blocks, char* err, size_t n);
// pixels: every int of both planes in [0, 255], narrowed into ref8 / cur8 on the way.
me_status pixels(const int* ref, const int* cur, size_t count, uint8_t* ref8, uint8_t* cur8, char* err,
                 size_t n);

// d.rec of a host entry point: region k at [off[k], off[k] + bytes[k]), its
// elements elem[k] bytes wide; total: the bytes the entry point asks grow for.
struct Layout {
  int n;
  size_t off[19], bytes[19], elem[19], total;
};
enum { REC_MV, REC_COST };                                       // layout_mv_cost
enum { BI_Q0, BI_Q1, BI_COST, BI_COST3, BI_MODE };               // layout_bipred
enum { RD_PRED, RD_MV, RD_COST, RD_DIST, RD_BITS };              // layout_rd
enum { PART_MV = 0, PART_COST = 4, PART_MODE_COST = 8, PART_MODE = 9 };  // + grid 0..3
enum { PRD_PRED = 0, PRD_MV = 1, PRD_COST = 5, PRD_DIST = 9, PRD_MODE_COST = 13, PRD_BITS = 14,
       PRD_MODE = 18 };
Layout layout_mv_cost(size_t n_blocks);
Layout layout_bipred(size_t n_blocks);
Layout layout_rd(size_t n_blocks);
Layout layout_partition(const int counts[4]);
Layout layout_partition_rd(const int counts[4]);

}  // namespace rules
}  // namespace me
