// me_kernels.h -- device-side launch interface (internal to libme_hip.so).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <type_traits>

#include "me.h"
#include "me_dispatch.h"
#include "me_geom.h"
#include "me_mfma_geom.h"

namespace me {

// sched holds SCHED_WORDS u32: [0, 16) the item kernel's 8 two-ended band
// counters (u64: owner claims in the low half, thieves in the high half),
// [SCHED_ARRIVE] its arrivals (the last workgroup out re-zeroes [0, 17)),
// [SCHED_ERR]: a kernel whose bounded wait expired sets it (the host reads and
// clears it: device_status, me_device_check).
constexpr int SCHED_WORDS = 96;
constexpr int SCHED_ARRIVE = 16;
constexpr int SCHED_ERR = 31;
// Tuning build only (QsadGeom::prune_stats): the pruning flow kernel's counts
// since the words were last zeroed: live lane-tasks, all lane-tasks, items
// whose bound was bypassed, items.
constexpr int SCHED_PRUNE = 24;
// ... and its executed wave-tasks run whole, with 2 and with 4 or more lanes per
// list entry (the row split, me_geom.h flow_split_parts): three words.
constexpr int SCHED_SPLIT = 28;
// ... and those of its h = B items by the list entries n = 1 .. 64 the task
// held (word n - 1; a bypassed item's tasks hold 64): what the row split's rule
// is chosen from.
constexpr int SCHED_SPLIT_HIST = 32;
static_assert(SCHED_SPLIT_HIST + 64 <= SCHED_WORDS, "the histogram lies inside sched");
// ... and the chain kernel's pre-bound (flow_fill): items pre-bound, items whose
// post-bound met the marker BUSY, items that fell back (bounded items of a slot's
// second or later turn that found no pre-bound and ran the whole bound): three words.
constexpr int SCHED_PRE = 20;

// The packed key of a candidate: the unsigned minimum of keys is the smallest
// cost and, among equal costs, the first displacement in raster order.
__device__ __forceinline__ uint64_t make_key(uint32_t cost, int dx, int dy) {
  return ((uint64_t)cost << 32) | ((uint32_t)(dy + 32768) << 16) | (uint32_t)(dx + 32768);
}

// Compile-time loop: every index is a constant, so register arrays indexed by
// it never fall back to scratch (plain #pragma unroll gives up on big bodies).
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// Write block `out`'s MV from a merged 64-bit key (cost << 32 | (dy + 32768)
// << 16 | (dx + 32768)): one 4-byte store of the (mvx, mvy) int16 pair when the
// records are 4-byte aligned, else two 2-byte stores.  (8K 8x8 WRITE_SIZE reads
// 2x the record bytes either way: a tile's 8 blocks store 32 contiguous bytes
// per array, below the 64-byte write granule the counter appears to tally.)
__device__ __forceinline__ void store_mv(int16_t* mv, int out, unsigned long long kk) {
  if (((uintptr_t)mv & 3) == 0) {
    reinterpret_cast<uint32_t*>(mv)[out] = (uint32_t)kk ^ 0x80008000u;
  } else {
    mv[2 * out] = (int16_t)((int)(kk & 0xFFFF) - 32768);
    mv[2 * out + 1] = (int16_t)((int)((kk >> 16) & 0xFFFF) - 32768);
  }
}

// Search every job (geometry, cost and context buffers from base): asks the
// dispatcher (me_dispatch.cpp) which kernel family takes which blocks and
// walks its launch list.  A single search is a list of one job.
hipError_t launch_jobs(const SearchArgs& base, const SearchJob* jobs, int n, hipStream_t stream);
// Scratch bytes the flow launches of launch_jobs(base, jobs, n) want for their
// box-sum planes (flow_planes_scratch, me_valu_plan.cpp, for this device and
// tuning; 0: none).  A search lent less runs without planes.
int last_flow_table();  // entries of the last planes launch's LDS item table (0: it ran without; -1: no such launch yet)
size_t flow_planes_need(const SearchArgs& base, const SearchJob* jobs, int n);

// Matrix-core SSD path (me_mfma.hip, me_band.hip).  MfmaGeom, MfmaJobs and the
// planners are in me_mfma_geom.h / me_mfma_plan.cpp (host-only, pure); the
// sizing wrappers below read kernel_path(), tuning() and cu_count() once and
// call them for the context (attach_scratch).
size_t mfma_merge_tiles(const SearchArgs& p);  // tiles the merge buffers must cover
size_t mfma_ssd_scratch(const SearchArgs& p);  // 0: path not applicable
// Scratch for n equal-geometry jobs of p's shape in batched launches (at most
// MAX_JOBS per launch, capped near 1 GiB), never less than mfma_ssd_scratch(p):
// plan_mfma_batch's need.
size_t mfma_batch_scratch(const SearchArgs& p, int n);
// Every kernel of the plan g (a dispatcher's MFMA launch) over the n
// equal-geometry jobs at `jobs`, job j's prepass planes at base.scratch + j *
// scratch_stride: binds g's pointers from base and fills the job table.
hipError_t launch_mfma(const SearchArgs& base, const SearchJob* jobs, int n, MfmaGeom g,
                       size_t scratch_stride, hipStream_t stream);
// Band-walk kernel (me_band.hip): launch every job of jb on the plan g.
hipError_t launch_bw(const SearchArgs& p, const MfmaGeom& g, const MfmaJobs& jb, hipStream_t stream);
// Tiles of cross-workgroup merge buffers (mkeys: 16 u64 keys each, ~0; mcnt:
// one u32 counter each, 0) the search of p needs (the MFMA SSD kernels).
size_t merge_tiles_needed(const SearchArgs& p);
bool mfma_disabled();

// Records the kernel family of a search being launched (ME_SEARCH_PATH_*):
// process-wide (me_last_search_path) and, inside a PathScope, for the
// context device the search runs on (me_ctx_last_search_path).
void note_path(int path);
int last_path();
// Raise fn's dynamic-LDS limit to lds (> 64 KB) on the current device, once
// per (kernel, device, larger size): process-wide cache, thread-safe.
hipError_t lds_attr(const void* fn, int lds);
hipError_t launch_generic(const SearchArgs& p, int bx0, int nbx_range, int row0, int nrows,
                          hipStream_t stream);
// CUs of the current device (every device of a context is the same part; 256,
// the MI355X's, when the query fails): queried once, thread-safe.
int cu_count();

// SSIM-cost search (me_ssim.hip): every block of rows [block_row_begin, block_row_end).
hipError_t launch_ssim(const SearchArgs& p, hipStream_t stream);
// Scratch bytes of the SSIM search's patch-statistics plane (0: not applicable).
size_t ssim_scratch(const SearchArgs& p);

// Consumers of the MV field (me_post.hip).
hipError_t launch_compensate(const uint8_t* ref, const uint8_t* cur, int width, int height,
                             int blk, const int16_t* mv, uint8_t* out5, int write_planes,
                             unsigned long long* stats, hipStream_t stream);

// The frames the batched launchers below work on: n_frames whole frames of
// one shape, frame f's planes at ref + f * ref_frame_stride and cur + f *
// cur_frame_stride (one frame: the strides are not read).  The searches'
// `fast`: full-size blocks on the packed-u16 kernel (their *_kernel_variant said
// FAST and planes and frame strides are 4-byte aligned), the clipped ones on
// the generic kernel; otherwise every block on the generic kernel.
struct FrameBatch {
  const uint8_t* ref;
  size_t ref_frame_stride;
  const uint8_t* cur;
  size_t cur_frame_stride;
  int width, height, stride, blk, n_frames;
};

// Partition search (me_partition.hip; geometry in me_tile_geom.h).
// out: device pointers (host struct).
hipError_t launch_partition_search(const FrameBatch& b, int range, uint32_t lambda, bool fast,
                                   const me_part_fields& out, hipStream_t stream);
hipError_t launch_partition_leaf(int width, int height, int blk, int n_frames,
                                 const me_part_fields& in, int16_t* leaf, hipStream_t stream);

// Quarter-pel refinement and sub-pel compensation (me_subpel.hip).
// launch_qpel_refine: n_frames whole frames (planes at + f * frame stride,
// records at + 2 * f * nblk / + f * nblk); mv_out may be mv_in, cost_out may
// be null; any int16 vector reads inside the planes.  No context scratch.
hipError_t launch_qpel_refine(const FrameBatch& b, int cost, const int16_t* mv_in, int16_t* mv_out,
                              uint32_t* cost_out, hipStream_t stream);
// launch_qpel_refine on cost + lambda * bits(q - pred) (include/me.h
// "rate-constrained motion search"): pred laid out like mv_in, null = all zero;
// cost_out (J) and dist_out (the cost at the result) may be null.
hipError_t launch_qpel_refine_rd(const FrameBatch& b, int cost, uint32_t lambda, const int16_t* pred,
                                 const int16_t* mv_in, int16_t* mv_out, uint32_t* cost_out,
                                 uint32_t* dist_out, hipStream_t stream);
// Rate-constrained integer search (me_rd.hip; geometry in me_tile_geom.h and
// me_rd.h).  Records
// and predictors (null: all zero) at + f * nblk (x 2 for vectors); dist and
// bits may be null.
hipError_t launch_rd_search(const FrameBatch& b, int range, uint32_t lambda, bool fast,
                            const int16_t* pred, int16_t* mv, uint32_t* cost, uint32_t* dist,
                            uint8_t* bits, hipStream_t stream);
// Rate-constrained partition search (me_partition.hip): launch_partition_search
// on J_p = SAD_p + lambda * bits(4 d - pred), pred [n_frames][nby][nbx][2]
// quarter-pel or null (all zero).
hipError_t launch_partition_rd_search(const FrameBatch& b, int range, uint32_t lambda, bool fast,
                                      const int16_t* pred, const me_part_rd_fields& out,
                                      hipStream_t stream);
// Partition-wise quarter-pel refinement (me_subpel.hip): the four integer grids
// of `in` (the rest of it is not read) refined partition by partition on
// cost + lambda * bits(q - pred) and the mode decided on the refined J.  Frames,
// records and pred laid out as for launch_partition_rd_search; out's grids may
// be in's; blk in {8, 16, 32}.  No context scratch.
hipError_t launch_partition_qpel(const FrameBatch& b, int cost, uint32_t lambda,
                                 const int16_t* pred, const me_part_fields& in,
                                 const me_part_rd_fields& out, hipStream_t stream);
// launch_compensate with quarter-pel vectors and edge-replicated samples.
hipError_t launch_qpel_compensate(const uint8_t* ref, const uint8_t* cur, int width, int height,
                                  int blk, const int16_t* mvq, uint8_t* out5, int write_planes,
                                  unsigned long long* stats, hipStream_t stream);

// Bi-prediction (me_subpel.hip): per block the costs of ref0 at q0, ref1 at q1
// and their rounded average, the joint quarter-step refinement of the pair
// (refine != 0) and the mode.  Frames and records laid out as for
// launch_qpel_refine; mode_out one byte per block, cost3_out [3] per block;
// the outputs may be the inputs, cost_out / cost3_out may be null.  No context
// scratch; any int16 vector reads inside the planes.  b.ref is ref0.
hipError_t launch_bipred(const FrameBatch& b, const uint8_t* ref1, size_t ref1_frame_stride,
                         int cost, int refine, const int16_t* q0_in, const int16_t* q1_in,
                         int16_t* q0_out, int16_t* q1_out, uint8_t* mode_out, uint32_t* cost_out,
                         uint32_t* cost3_out, hipStream_t stream);
// launch_qpel_compensate with two references and a mode byte (0, 1, 2) per block.
hipError_t launch_bipred_compensate(const uint8_t* ref0, const uint8_t* ref1, const uint8_t* cur,
                                    int width, int height, int blk, const int16_t* mv0,
                                    const int16_t* mv1, const uint8_t* mode, uint8_t* out5,
                                    int write_planes, unsigned long long* stats,
                                    hipStream_t stream);

}  // namespace me
