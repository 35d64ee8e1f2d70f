/*
 * me.h -- C ABI of the MI355X full-search block-matching engine (libme_hip.so).
 *
 * Drop-in boundary for the reference's hot path (souravBhat/MotionEstimation,
 * paths relative to the reference tree):
 *
 *   reference seam                                   replaced by
 *   -----------------------------------------------  ---------------------------------
 *   dispatch region src/cpu/main.c:144-158           me_full_search()
 *     (thpool_init(100) + one findBestBlkMse job       frame level, host planes,
 *      per block + thpool_wait)                        synchronous
 *   findBestBlkMse  src/cpu/main.c:67-82             me_full_search() / me_find_best_blocks()
 *     + findBestMatchMse :39-64 + computeMse :18-36    (per-block calls make no sense on a GPU)
 *   GPU host region src/gpu/main_mse.cu:202-229      me_full_search_device() (HBM-resident,
 *     (H2D, f_findBestMatchBlock<<<>>>, D2H)           stream-ordered)
 *   block list filled for motionCompensatedFrame     me_find_best_blocks() writes the
 *     src/common/utils.c:102-108                       reference's block records
 *
 * Semantics (identical to src/cpu on the same inputs):
 *   - blocks tile the frame in raster order, ceil(W/B) x ceil(H/B), partial
 *     blocks on the right/bottom edges   (src/common/prediction_frame.c:9-23)
 *   - candidates: every top-left whose whole block fits the window
 *     [tl - S, br + S] clamped to the frame   (src/cpu/main.c:53-54, 73-76)
 *   - the first minimum in raster order (y outer, x inner, strict <) wins
 *     (src/cpu/main.c:53-60)
 *   - MV = candidate top-left - block top-left   (src/cpu/main.c:58-59)
 *   - ME_COST_SSD reproduces the reference's float-MSE choice bit for bit:
 *     block_cost = integer SSD of the chosen vector and the reference's score
 *     is (float)block_cost / (float)(w*h) for w*h <= 256; larger blocks are
 *     searched with the reference's float accumulation replayed exactly.
 *   - ME_COST_SAD: same loops and tie rule with |cur - ref| (the reference
 *     has no SAD; parity is against the repo's CPU restatement).
 *     The 1080p-class kernel skips candidates an exact lower bound proves
 *     strictly worse than one already evaluated; vectors and costs remain
 *     the exhaustive search's, bit for bit.
 *   - ME_COST_SSIM: the reference's SSIM search (src/common/ssim.c:3-108,
 *     src/cpu/main_ssim.c:15-29), float arithmetic replayed in its order.
 *
 * Conventions: host buffers are caller-owned; host entry points are
 * synchronous on return.  A context is used by one host thread at a time.
 * Errors are returned, never exit()ed (the reference exits: main.c:134-139).
 */
#ifndef ME_H
#define ME_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ME_API_VERSION 1

typedef enum {
  ME_OK = 0,
  ME_EINVAL = 1,      /* bad argument (sizes, null pointers, block/range limits) */
  ME_ENOMEM = 2,      /* host or device allocation failed */
  ME_EDEVICE = 3,     /* HIP runtime / kernel launch error */
  ME_ECOMM = 4,       /* RCCL error in the multi-device gather */
  ME_EUNSUPPORTED = 5, /* valid request this build cannot serve */
  ME_EIO = 6           /* file missing, short or malformed (me_yuv_* / me_mv_*) */
} me_status;

typedef enum {
  ME_COST_SSD = 0, /* reference parity: float MSE argmin; cost = SSD */
  ME_COST_SAD = 1, /* sum of absolute differences */
  ME_COST_SSIM = 2, /* reference parity with src/common/ssim.c: float SSIM argmax
                       (first strict maximum above 0); cost = the score's float
                       bits; MV (0, 0) and cost 0 where no score is above 0 */
  ME_COST_SATD = 3  /* sum of absolute 4x4 Hadamard-transformed differences
                       ("SATD cost" below): the quarter-pel refinements and the
                       bi-prediction only; every integer search returns
                       ME_EUNSUPPORTED for it */
} me_cost;

/* ---- SATD cost (ME_COST_SATD) ----
 * Exact integers; no reference counterpart, parity is against the numpy
 * restatement tests/satd_ref.py.  For a block clipped to bw x bh with
 * prediction P and current block C:
 *   - residual: d(i, j) = C(i, j) - P(i, j) inside the block, 0 outside.
 *   - tiles: a 4x4 grid anchored at the block's own top-left, ceil(bw / 4) x
 *     ceil(bh / 4) tiles, partial tiles zero padded; every block_size in
 *     [1, 64] (a 1x1 block is one tile with one non-zero residual).
 *   - transform: T = H D H^T per tile, H the order-4 +-1 Hadamard matrix (sum
 *     |T| does not depend on the row order of H).
 *   - satd = (sum over tiles of sum |T_uv|) >> 1.  The shift is exact: the 16
 *     coefficients of a tile all have the parity of the tile's residual sum.
 *   - bounds: |T_uv| <= 16 * 255 = 4080; a tile's satd <= 8160; a 64x64
 *     block's <= 2,088,960, so satd + 66 * 2^24 < 2^32 and ME_RD_MAX_LAMBDA
 *     holds for the rate-constrained refinement as it is.
 *   - identities: SAD <= 2 satd <= 16 SAD, and per tile sum T^2 = 16 sum d^2.
 * Where it is accepted only cost(.) changes: stages, candidate order, carried
 * centre, strict <, tie rules, edge replication and mode order are those of
 * the entry point.  The composite entry points (me_full_search_qpel,
 * me_full_search_rd_qpel, me_full_search_bipred) run their integer searches at
 * ME_COST_SAD and everything after them at SATD. */

/* Limits of this build. */
#define ME_MAX_BLOCK 64    /* block_size in [1, 64]  (SSD of 64x64 < 2^32) */
#define ME_MAX_RANGE 1024  /* search_range in [0, 1024] */
/* stride * height < 2^31 bytes per plane (ME_EUNSUPPORTED otherwise). */

typedef struct me_ctx me_ctx;

/* Create a context on n_devices HIP devices (device_ids may be NULL with
 * n_devices <= 1: the current device).  With n_devices > 1 every search is
 * split into macroblock row stripes, one per device, and the per-stripe MV
 * fields are gathered to device_ids[0] with one RCCL ncclGather.  A device id
 * may repeat: repeated ids run their stripes one after another on that device
 * and are gathered by device copies (exercises the stripe path on one GPU). */
me_status me_create(me_ctx** ctx, const int* device_ids, int n_devices);
void me_destroy(me_ctx* ctx);

const char* me_status_str(me_status s);
/* Detail of the last error on this context ("" if none). */
const char* me_last_error(const me_ctx* ctx);
/* Library version string, e.g. "me_hip 1 gfx950". */
const char* me_version(void);

/* Kernel path (process-wide; A/B tests and diagnostics).  Results are
 * identical on every path.
 *   ME_PATH_AUTO: SSD with 16x16 and 8x8 blocks on the matrix cores (i8 MFMA),
 *     everything else on the VALU kernels.  16x16 SSD with S <= 64 runs the
 *     band-walk kernel (each 16-row band's S2 term formed once in LDS for
 *     every block row in flight, no context scratch, ~1.1x the algorithmic
 *     HBM bytes: DESIGN.md) when a launch's strips of block columns fill the
 *     GPU's CUs by themselves (e.g. 16 1080p frames per batched call);
 *     otherwise (single frames, small batches, larger ranges) the prepass +
 *     block-major pair.
 *   ME_PATH_VALU: VALU kernels only, SSIM included (every SSIM block on the
 *     float-chain kernels; the other paths run 16x16 SSIM with S <= 64 on the
 *     matrix cores).
 *   ME_PATH_MFMA_TILES: 16x16 SSD on the 4x4-block-tile MFMA kernel (the
 *     fallback for rows that are not 16-byte aligned).
 *   ME_PATH_MFMA_LEAN: 16x16 SSD with S <= 64 on the band-walk kernel for
 *     every launch (single frames split into segments of block rows; no
 *     context scratch); a partial bottom block row, or rows the band-walk
 *     kernel cannot take, on the per-workgroup S2 kernel (me_mfma_bmv_kernel).
 *   ME_PATH_MFMA_PREPASS: 16x16 SSD on the S2 prepass + block-major kernel
 *     (5 bytes of context scratch per reference pixel per frame of a batch).
 * The environment variable ME_PATH=auto|valu|tiles|lean|prepass sets the
 * initial value (anything else is ignored with a message on stderr). */
typedef enum {
  ME_PATH_PROCESS = -1,  /* me_ctx_set_kernel_path only: follow the process-wide path */
  ME_PATH_AUTO = 0,
  ME_PATH_VALU = 1,
  ME_PATH_MFMA_TILES = 2,
  ME_PATH_MFMA_LEAN = 3,
  ME_PATH_MFMA_PREPASS = 4
} me_path;
void me_set_kernel_path(me_path path);

/* Per-context kernel path (one host thread per context, as every entry point):
 * the searches of ctx -- planning, scratch and launch, on every device of the
 * context and on the pair pipeline's worker threads -- use `path` (an
 * me_path value) instead of the process-wide one; ME_PATH_PROCESS (the
 * default of a new context) follows me_set_kernel_path / ME_PATH again.
 * ME_EINVAL for an unknown value.  Graphs captured earlier keep the kernels
 * they recorded. */
me_status me_ctx_set_kernel_path(me_ctx* ctx, int path);

/* The kernel family that ran the most recent search launched in this process
 * (any context, any thread -- me_ctx_last_search_path is the per-context one;
 * diagnostics and tests, e.g. that the AUTO path of
 * a 16x16 SSD search is the band-walk kernel).  The matrix-core SSD kernels
 * report the kernel of the frame's full-height block rows; an SSIM search
 * reports whether the matrix-core kernel took its full-width blocks. */
typedef enum {
  ME_SEARCH_PATH_NONE = 0,           /* no search launched yet */
  ME_SEARCH_PATH_VALU = 1,           /* SAD and SSD VALU kernels (flow, item, generic) */
  ME_SEARCH_PATH_MFMA_PREPASS = 2,   /* S2 prepass + block-major MFMA kernel */
  ME_SEARCH_PATH_MFMA_BANDWALK = 3,  /* band-walk MFMA kernel (me_band.hip) */
  ME_SEARCH_PATH_MFMA_LEAN = 4,      /* per-workgroup S2 MFMA kernel (bmv) */
  ME_SEARCH_PATH_MFMA_TILES = 5,     /* 4x4-block-tile MFMA kernel */
  ME_SEARCH_PATH_MFMA_8X8 = 6,       /* 8x8-block MFMA kernel */
  ME_SEARCH_PATH_SSIM = 7,           /* SSIM float-chain kernels */
  ME_SEARCH_PATH_SSIM_MFMA = 8       /* SSIM: the launch's full-width 16x16 blocks on the
                                        matrix-core kernel (S <= 64) */
} me_search_path;
int me_last_search_path(void);
/* The kernel family (me_search_path) of the most recent search launched by
 * ctx on its device devs[device_index] (the index into me_create's device
 * list); ME_SEARCH_PATH_NONE before its first search, -1 for a bad argument.
 * Per context: a search on another context or thread does not change it. */
int me_ctx_last_search_path(const me_ctx* ctx, int device_index);

/* Tiling helpers (src/common/prediction_frame.c:9-11). */
int me_num_blocks(int width, int height, int block_size);
/* Exact number of candidates the search evaluates (reference clamping). */
uint64_t me_candidate_count(int width, int height, int block_size, int search_range);

/* Frame-level search on host Y planes (8-bit, row pitch `stride` >= width).
 * mv_xy: [nblocks][2] int16 (mvx, mvy), block_cost: [nblocks] (may be NULL). */
me_status me_full_search(me_ctx* ctx, const uint8_t* ref, const uint8_t* cur,
                         int width, int height, int stride, int block_size,
                         int search_range, me_cost cost, int16_t* mv_xy,
                         uint32_t* block_cost);

/* Same search on HBM-resident planes of ctx's first device, enqueued on
 * `stream` (a hipStream_t; NULL = the legacy default stream), asynchronous.
 * d_mv_xy / d_block_cost are device arrays of nblocks entries.
 * Searches of one context are ordered by the library: one enqueued on another
 * stream than the previous search waits for it on the GPU (an event recorded
 * on the previous stream at the switch; the host never blocks), so a stream
 * passed here must stay valid until the context's next search is enqueued.
 * After the stream has finished, me_device_check() reports a search whose
 * in-kernel invariant broke (the synchronous entry points check on their own). */
me_status me_full_search_device(me_ctx* ctx, const uint8_t* d_ref,
                                const uint8_t* d_cur, int width, int height,
                                int stride, int block_size, int search_range,
                                me_cost cost, int16_t* d_mv_xy,
                                uint32_t* d_block_cost, void* stream);

/* One row stripe: block rows [block_row_begin, block_row_end).  d_ref holds
 * frame rows starting at ref_row0 and must cover
 *   [max(0, block_row_begin*B - S), min(H, block_row_end*B + S)),
 * d_cur holds frame rows starting at cur_row0 and must cover
 *   [block_row_begin*B, min(H, block_row_end*B)).
 * Outputs hold the stripe's blocks only, raster order.  This is the unit a
 * multi-process (one rank per GPU) caller shards with. */
me_status me_full_search_stripe_device(me_ctx* ctx, const uint8_t* d_ref,
                                       int ref_row0, const uint8_t* d_cur,
                                       int cur_row0, int width, int height,
                                       int stride, int block_size,
                                       int search_range, me_cost cost,
                                       int block_row_begin, int block_row_end,
                                       int16_t* d_mv_xy, uint32_t* d_block_cost,
                                       void* stream);

/* Several stripes (of one frame or of several frames of the same geometry)
 * searched together: each job is what one me_full_search_stripe_device call
 * would take -- its planes with their first resident rows, its block rows and
 * its output records -- and the results are those of one call per job.  The
 * jobs of a call share launches where the kernels allow it, so a batch fills
 * the GPU where one small stripe cannot: the per-rank step of a multi-GPU
 * split over several frames (a rank may hold different row ranges of
 * different frames, balancing its total rows).  Asynchronous on `stream`. */
typedef struct me_stripe_job {
  const uint8_t* d_ref;
  int ref_row0;
  const uint8_t* d_cur;
  int cur_row0;
  int block_row_begin, block_row_end;
  int16_t* d_mv_xy;        /* (block_row_end - block_row_begin) * ceil(W/B) records */
  uint32_t* d_block_cost;  /* may be NULL */
} me_stripe_job;
me_status me_search_stripes_device(me_ctx* ctx, int width, int height, int stride,
                                   int block_size, int search_range, me_cost cost,
                                   const me_stripe_job* jobs, int n_jobs, void* stream);

/* A batch of n_frames same-shaped stripes (or whole frames: block rows
 * [0, nby)): frame f's rows at d_ref + f * ref_frame_stride and
 * d_cur + f * cur_frame_stride bytes (frames must not overlap), its records at
 * d_mv_xy + 2 * f * nblk and d_block_cost + f * nblk, nblk = (block_row_end -
 * block_row_begin) * ceil(W/B).  The equal-stripes case of
 * me_search_stripes_device.  Each plane stack of the batch stays below 2 GiB
 * ((n_frames - 1) * stride + one frame's bytes; ME_EUNSUPPORTED otherwise). */
me_status me_full_search_batch_device(me_ctx* ctx, const uint8_t* d_ref,
                                      size_t ref_frame_stride, int ref_row0,
                                      const uint8_t* d_cur, size_t cur_frame_stride,
                                      int cur_row0, int width, int height, int stride,
                                      int block_size, int search_range, me_cost cost,
                                      int block_row_begin, int block_row_end, int n_frames,
                                      int16_t* d_mv_xy, uint32_t* d_block_cost,
                                      void* stream);

/* Balanced stripe plan: bounds[0..n_shards] block-row boundaries, each stripe
 * carrying about the same search cost.  The cost of a block row is its block
 * count times (3 * (2S+1) + ny) / 4, ny = its exact candidate-row count: the
 * kernels compute a clipped top / bottom block row at nearly the price of an
 * interior one (whole dy chunks, one staged window per tile), so edge rows are
 * discounted by a quarter of their candidate deficit, not all of it. */
me_status me_plan_stripes(int width, int height, int block_size,
                          int search_range, int n_shards, int* bounds);

/* ---- multi-process stripes (one process per GPU) ----
 * The one exchange step of a sharded search, issued from C so a rank's step
 * costs two native calls instead of a Python collective.  Rank 0 calls
 * me_comm_unique_id and sends the ME_COMM_ID_BYTES bytes to the other ranks
 * out of band (e.g. a torch.distributed broadcast); every rank then calls
 * me_comm_init with them (collective: all ranks at once) to build an RCCL
 * communicator on ctx's first device.  No reference counterpart: the
 * reference is single-process. */
#define ME_COMM_ID_BYTES 128
me_status me_comm_unique_id(void* id);
me_status me_comm_init(me_ctx* ctx, const void* id, int n_ranks, int rank);
/* Gather `bytes` from every rank's device buffer d_send into rank 0's d_recv
 * (n_ranks * bytes, rank order; d_recv is ignored on other ranks), enqueued on
 * `stream` (a hipStream_t) after the work already on it; asynchronous. */
me_status me_gather_device(me_ctx* ctx, const void* d_send, size_t bytes, void* d_recv,
                           void* stream);
/* Failure detection for the exchange (the reference checks CUDA
 * errors once, at exit: src/gpu/main_mse.cu:275-276).  Waits at most
 * timeout_ms for the work enqueued so far on `stream` (the rank's searches and
 * gathers) while polling RCCL's asynchronous error (ncclCommGetAsyncError).
 * ME_OK: the stream drained and RCCL reports no error.  ME_ECOMM: RCCL
 * reported an error, or the wait timed out (a peer rank stalled or died); the
 * communicator is then aborted (ncclCommAbort), so this rank's RCCL kernels
 * return and the stream can be synchronised instead of hanging, and every
 * later me_gather_device / me_comm_check on the context fails with ME_ECOMM
 * until me_comm_init builds a new communicator (all ranks, a fresh id).
 * me_last_error names the cause.  The multi-device me_full_search waits the
 * same way (ME_COMM_TIMEOUT_MS) and rebuilds its group after a failure. */
#define ME_COMM_TIMEOUT_MS 60000
me_status me_comm_check(me_ctx* ctx, void* stream, int timeout_ms);

/* ME_EDEVICE if a search kernel of this context reported a broken in-kernel
 * invariant (a bounded wait that expired: the kernel ends instead of hanging
 * the GPU, and that search's MV field is invalid) since the last check; the
 * report is cleared.  Call after the searches' streams have finished.
 * me_full_search, me_find_best_blocks and me_search_pairs check on their own;
 * the word is per device, so such a synchronous call also fails with
 * ME_EDEVICE when an earlier, still unchecked asynchronous search on the
 * device broke its invariant, and the report stays pending for that
 * search's own me_device_check as well. */
me_status me_device_check(me_ctx* ctx);

/* ---- captured steps (hipGraph) ----
 * A per-frame step of device entry points (e.g. a stripe search and its
 * me_gather_device) recorded once and replayed with one launch: the sharded
 * step of a small stripe is bound by host enqueue time, not by the GPU.
 * Counterpart of the reference's per-frame host region (src/gpu/main_mse.cu:202-229).
 *   me_capture_begin(ctx, s); me_full_search_stripe_device(ctx, ..., s);
 *   me_gather_device(ctx, ..., s); me_capture_end(ctx, s, &g);
 *   per frame: me_graph_launch(g, s);
 * `stream` is a created hipStream_t (not NULL).  Run each search once
 * uncaptured first: it sizes the context's scratch, and a captured search that
 * would have to grow it fails with ME_EINVAL.  The captured calls only record;
 * nothing runs until me_graph_launch, which orders the graph after the
 * context's previous search like any search.  A graph whose context scratch
 * was regrown since capture (a larger search ran) is refused (ME_EINVAL).
 * Destroy graphs before their context. */
typedef struct me_graph me_graph;
me_status me_capture_begin(me_ctx* ctx, void* stream);
me_status me_capture_end(me_ctx* ctx, void* stream, me_graph** graph);
me_status me_graph_launch(me_graph* graph, void* stream);
void me_graph_destroy(me_graph* graph);

/* Reference block record, field for field src/common/block.h:6-19 (44 B). */
typedef struct me_ref_block {
  int idx_x, idx_y;
  int top_left_x, top_left_y;
  int bottom_right_x, bottom_right_y;
  int width, height;
  int is_best_match_found;
  int motion_vectorX, motion_vectorY;
} me_ref_block;

/* Adapter for the reference driver: takes its int-widened planes
 * (src/common/utils.c:49-53), searches with ME_COST_SSD and fills
 * motion_vectorX/Y and is_best_match_found = 1 of every block exactly as the
 * thread-pool loop at src/cpu/main.c:144-158 does.  blks must hold the
 * me_num_blocks() records createPredictionFrame produced. */
me_status me_find_best_blocks(me_ctx* ctx, const int* ref_frame,
                              const int* cur_frame, int width, int height,
                              int block_size, int search_range,
                              me_ref_block* blks, int num_blks);

/* ---- consumers of the MV field (src/common/utils.c:94-164) on the GPU ---- */

/* mc[p] = ref[p + mv(block of p)], host planes, synchronous. */
me_status me_motion_compensate(me_ctx* ctx, const uint8_t* ref, int width,
                               int height, int block_size, const int16_t* mv_xy,
                               uint8_t* mc);

/* The reference's 5-plane output [ref, cur, mc, |ref-cur|, |mc-cur|]
 * (src/cpu/main.c:161-168) into out[5*W*H], plus the PSNR of mc vs cur with
 * the reference's MAX = largest pixel rule (src/common/utils.c:137-164). */
me_status me_compensate_planes(me_ctx* ctx, const uint8_t* ref,
                               const uint8_t* cur, int width, int height,
                               int block_size, const int16_t* mv_xy,
                               uint8_t* out5, double* psnr);

/* ---- quarter-pel refinement and sub-pel compensation ----
 * No reference counterpart (the reference stops at integer vectors); parity is
 * against the numpy restatement tests/qpel_ref.py.  Exact integer arithmetic,
 * the H.264 luma interpolation (DESIGN.md "Quarter-pel refinement" has it in
 * full):
 *   - a quarter-pel vector (qx, qy) is int16, four units per pixel; the
 *     integer vector m is 4 * m.
 *   - reference samples are EDGE REPLICATED, R(x, y) = ref[clamp(y)][clamp(x)]:
 *     no sample is outside the frame.  This is the one deliberate difference
 *     from the integer me_motion_compensate, which writes 0 for out-of-frame
 *     pixels and stays as it is.
 *   - half samples: the 6-tap (1, -5, 20, 20, -5, 1) filter, clip255((b1 + 16)
 *     >> 5) horizontally and vertically; the centre half sample filters the
 *     unrounded horizontal intermediates vertically, clip255((j1 + 512) >> 10).
 *   - quarter samples: (a + b + 1) >> 1 of the two nearest half-grid samples
 *     along the odd axis; with both axes odd, of the horizontal and the
 *     vertical half sample among the four corners (never the pixel or the
 *     centre half sample).
 *   - refinement of a block (partial edge blocks keep their true size): start
 *     at 4 * m; stage 1 tries the eight neighbours at step 2 (half-pel), stage
 *     2 the eight at step 1 around stage 1's winner; candidates in raster
 *     order (dy outer), a candidate wins only with a strictly smaller cost, so
 *     ties go to the centre, then to the first candidate.  No window: the
 *     result is within 3 quarter units of 4 * m per axis.
 *   - ME_COST_SAD, ME_COST_SSD and ME_COST_SATD; ME_COST_SSIM returns
 *     ME_EUNSUPPORTED.
 * Whole frames on one device only: a stripe would need reference rows beyond
 * its documented cover (3 more above and below), and a multi-device context's
 * stripes likewise, so neither is offered. */
#define ME_QPEL_MAX_MV 8000 /* |component| of an integer input vector: 4 * m +- 3 fits int16 */

/* Refine n_frames >= 1 whole frames of one geometry on HBM-resident planes of
 * ctx's first device: frame f's planes at d_ref + f * ref_frame_stride and
 * d_cur + f * cur_frame_stride bytes, its integer records at d_mv_xy + 2 * f *
 * nblk, its results at d_mv_q + 2 * f * nblk and d_block_cost + f * nblk (nblk
 * = me_num_blocks; the layout of me_full_search_batch_device).  d_block_cost
 * may be NULL; d_mv_q == d_mv_xy (in place) is allowed.  Asynchronous on
 * `stream`, ordered after the context's previous search like any search; uses
 * no context scratch, so it can be captured (me_capture_begin) without a
 * warm-up call.  Precondition: |m| <= ME_QPEL_MAX_MV per component (not
 * checked: the field is on the device); any int16 value still reads only
 * inside the planes, its result is then unspecified. */
me_status me_refine_qpel_device(me_ctx* ctx, const uint8_t* d_ref, size_t ref_frame_stride,
                                const uint8_t* d_cur, size_t cur_frame_stride, int width,
                                int height, int stride, int block_size, me_cost cost,
                                int n_frames, const int16_t* d_mv_xy, int16_t* d_mv_q,
                                uint32_t* d_block_cost, void* stream);

/* The same on host planes, synchronous.  mv_xy: the integer field (ME_EINVAL
 * for a component beyond ME_QPEL_MAX_MV); mv_q: [nblocks][2] int16 quarter-pel
 * vectors; block_cost: [nblocks] cost at mv_q (may be NULL). */
me_status me_refine_qpel(me_ctx* ctx, const uint8_t* ref, const uint8_t* cur, int width,
                         int height, int stride, int block_size, me_cost cost,
                         const int16_t* mv_xy, int16_t* mv_q, uint32_t* block_cost);

/* me_full_search and the refinement back to back on the device: the integer
 * field never visits the host.  With ME_COST_SATD the integer search runs at
 * ME_COST_SAD and the refinement at SATD.  One context device
 * (ME_EUNSUPPORTED with several). */
me_status me_full_search_qpel(me_ctx* ctx, const uint8_t* ref, const uint8_t* cur, int width,
                              int height, int stride, int block_size, int search_range,
                              me_cost cost, int16_t* mv_q, uint32_t* block_cost);

/* me_motion_compensate / me_compensate_planes with quarter-pel vectors: mc[p]
 * is the prediction sample of p's block at that block's mv_q (edge replicated:
 * see above); planes and PSNR are formed from mc exactly as the integer
 * versions do. */
me_status me_motion_compensate_qpel(me_ctx* ctx, const uint8_t* ref, int width, int height,
                                    int block_size, const int16_t* mv_q, uint8_t* mc);
me_status me_compensate_planes_qpel(me_ctx* ctx, const uint8_t* ref, const uint8_t* cur,
                                    int width, int height, int block_size,
                                    const int16_t* mv_q, uint8_t* out5, double* psnr);

/* ---- bi-predictive mode decision, joint refinement and compensation ----
 * A current frame with two references (a past ref0 and a future ref1) and a
 * quarter-pel field against each.  No reference counterpart; parity is against
 * the numpy restatement tests/bipred_ref.py.  Exact integers throughout
 * (DESIGN.md "Bi-prediction" has it in full).  P0(q) / P1(q) are the
 * quarter-pel prediction blocks defined above, from ref0 / ref1:
 *   - bi-prediction sample: PB(q0, q1) = (P0(q0) + P1(q1) + 1) >> 1 per pixel
 *     (H.264 default weighting).
 *   - costs of a block (partial edge blocks keep their true size), SAD, SSD
 *     or SATD against the current block: c0 = cost(P0(q0)), c1 = cost(P1(q1)),
 *     cb = cost(PB(b0, b1)), (b0, b1) starting at (q0, q1).
 *   - joint refinement (refine != 0): two passes at quarter step, each over
 *     the eight neighbours + (dx, dy), dx, dy in {-1, 0, 1}, in raster order
 *     (dy outer); the centre's cost is carried over and a candidate wins only
 *     if strictly smaller.  Pass 1 holds b0 and moves b1; pass 2 holds pass
 *     1's b1 and moves b0.  With refine == 0, (b0, b1) = (q0, q1).
 *   - mode: L0, L1, BI are tried in that order and a later one replaces the
 *     best only if strictly smaller (ties go to L0, then L1); one byte per
 *     block; block_cost is the winner's cost; cost3[nblk][3] = (c0, c1, cb).
 *   - output vectors: (b0, b1) for mode BI, otherwise (q0, q1) unchanged.
 *   - compensation: mc of a block is P0(v0), P1(v1) or PB(v0, v1) by its mode;
 *     the 5 planes are [ref0, cur, mc, |ref0 - cur|, |mc - cur|], PSNR by the
 *     rule of me_compensate_planes.
 *   - ME_COST_SSIM, stripes and contexts with several devices are not
 *     supported (ME_EUNSUPPORTED), for the quarter-pel refinement's reasons. */
typedef enum me_pred_mode { ME_PRED_L0 = 0, ME_PRED_L1 = 1, ME_PRED_BI = 2 } me_pred_mode;
#define ME_BIPRED_MAX_Q 32766 /* |component| of an input quarter-pel vector: q +- 1 fits int16 */

/* n_frames >= 1 whole frames of one geometry on HBM-resident planes of ctx's
 * first device, laid out as for me_refine_qpel_device: frame f's planes at
 * d_ref0 + f * ref0_frame_stride, d_ref1 + f * ref1_frame_stride and d_cur +
 * f * cur_frame_stride bytes, its records at + 2 * f * nblk (vectors), + f *
 * nblk (d_mode, d_block_cost) and + 3 * f * nblk (d_cost3).  d_block_cost and
 * d_cost3 may be NULL; d_mv_out0 == d_mv_q0 and d_mv_out1 == d_mv_q1 (in
 * place) are allowed.  Asynchronous on `stream`, ordered after the context's
 * previous search; uses no context scratch, so it can be captured without a
 * warm-up call.  Precondition: |q| <= ME_BIPRED_MAX_Q per component (not
 * checked: the fields are on the device); any int16 value still reads only
 * inside the planes, its result is then unspecified. */
me_status me_bipred_device(me_ctx* ctx, const uint8_t* d_ref0, size_t ref0_frame_stride,
                           const uint8_t* d_ref1, size_t ref1_frame_stride, const uint8_t* d_cur,
                           size_t cur_frame_stride, int width, int height, int stride,
                           int block_size, me_cost cost, int refine, int n_frames,
                           const int16_t* d_mv_q0, const int16_t* d_mv_q1, int16_t* d_mv_out0,
                           int16_t* d_mv_out1, uint8_t* d_mode, uint32_t* d_block_cost,
                           uint32_t* d_cost3, void* stream);

/* The same on host planes of row pitch `stride`, synchronous.  ME_EINVAL for
 * an input component beyond ME_BIPRED_MAX_Q.  block_cost and cost3 may be NULL. */
me_status me_bipred(me_ctx* ctx, const uint8_t* ref0, const uint8_t* ref1, const uint8_t* cur,
                    int width, int height, int stride, int block_size, me_cost cost, int refine,
                    const int16_t* mv_q0, const int16_t* mv_q1, int16_t* mv_out0,
                    int16_t* mv_out1, uint8_t* mode, uint32_t* block_cost, uint32_t* cost3);

/* Both integer searches (ref0 and ref1 against cur), both quarter-pel
 * refinements, then the bi-prediction with refine = 1, back to back on the
 * device: no field visits the host.  With ME_COST_SATD both integer searches
 * run at ME_COST_SAD, both refinements and the bi-prediction at SATD.  One
 * context device (ME_EUNSUPPORTED with several).  block_cost may be NULL. */
me_status me_full_search_bipred(me_ctx* ctx, const uint8_t* ref0, const uint8_t* ref1,
                                const uint8_t* cur, int width, int height, int stride,
                                int block_size, int search_range, me_cost cost, int16_t* mv_out0,
                                int16_t* mv_out1, uint8_t* mode, uint32_t* block_cost);

/* me_motion_compensate_qpel / me_compensate_planes_qpel with two references
 * and a mode per block (ME_EINVAL for a mode byte above ME_PRED_BI). */
me_status me_motion_compensate_bipred(me_ctx* ctx, const uint8_t* ref0, const uint8_t* ref1,
                                      int width, int height, int block_size, const int16_t* mv0,
                                      const int16_t* mv1, const uint8_t* mode, uint8_t* mc);
me_status me_compensate_planes_bipred(me_ctx* ctx, const uint8_t* ref0, const uint8_t* ref1,
                                      const uint8_t* cur, int width, int height, int block_size,
                                      const int16_t* mv0, const int16_t* mv1, const uint8_t* mode,
                                      uint8_t* out5, double* psnr);

/* ---- variable-block-size partition search with mode decision ----
 * One pass over the candidates of every B x B macroblock yields the best
 * integer vector of the macroblock, of its two B x h halves, its two h x B
 * halves and its four h x h quarters (h = B / 2), and the cheapest of the four
 * shapes.  No reference counterpart; parity is against the numpy restatement
 * tests/partition_ref.py.  Exact integers (DESIGN.md "Partition search"):
 *   - grids: nbx = ceil(W/B), nby = ceil(H/B), nhx = ceil(W/h), nhy = ceil(H/h).
 *     Macroblock (bx, by) has its top-left at (x0, y0) = (bx B, by B) and is
 *     clipped to the frame: bw x bh.
 *   - partitions of a macroblock: the nominal rectangles clipped to the frame;
 *     empty ones do not exist.  2Nx2N: the macroblock; 2NxN: two B x h (top,
 *     bottom); Nx2N: two h x B (left, right); NxN: four h x h.
 *   - each shape's field is stored in the raster order of its own grid over
 *     the frame (the non-empty partitions are exactly the grids' cells):
 *     2Nx2N nbx x nby; 2NxN nbx x nhy, cell (bx, 2 by + j) is half j of
 *     macroblock (bx, by); Nx2N nhx x nby; NxN nhx x nhy.
 *   - candidates of a macroblock: exactly me_full_search's at block size B,
 *     top-left (cx, cy) with cx in [max(0, x0 - S), min(W, x0 + bw + S) - bw],
 *     cy likewise.  Every partition of the macroblock is costed at the same
 *     displacements d = (cx - x0, cy - y0), its pixels against the reference
 *     pixels at + d (always inside the frame).  The displacement set is the
 *     macroblock's own, not the one a B/2 search would give the sub-block (the
 *     two differ where the frame clamps).
 *   - winner per partition: the first minimum in raster order of the
 *     displacements (dy outer, dx inner, strict <); its cost is its SAD.  So
 *     the 2Nx2N field and costs are me_full_search's at (B, S, SAD) bit for
 *     bit, and the four NxN records of a full-size macroblock whose window is
 *     not clamped on any side are me_full_search's at (B/2, S).
 *   - mode: J(2Nx2N) = c + lambda, J(2NxN) = sum of halves + 2 lambda,
 *     J(Nx2N) = sum of halves + 2 lambda, J(NxN) = sum of quarters + 4 lambda,
 *     the sums over the non-empty partitions, the lambda multipliers always the
 *     nominal 1, 2, 2, 4.  Modes are tried in the order 0, 1, 2, 3 and a later
 *     one replaces the best only if strictly smaller.  mode: one byte per
 *     macroblock; mode_cost: its J.  lambda <= ME_PART_MAX_LAMBDA, so J cannot
 *     overflow (B = 32: 261,120 + 4 * 2^24 < 2^32).
 *   - leaf field: on the NxN grid; cell (hx, hy) belongs to macroblock
 *     (hx / 2, hy / 2) of mode m and takes the vector of the partition that
 *     contains it: m = 0 mv_2nx2n[by][bx], m = 1 mv_2nxn[hy][bx], m = 2
 *     mv_nx2n[by][hx], m = 3 mv_nxn[hy][hx].  It is an ordinary integer field
 *     of block size h: me_motion_compensate, me_compensate_planes,
 *     me_refine_qpel* and me_mv_write take it unchanged at block_size = B / 2,
 *     and sum |mc - cur| over the frame = sum over the macroblocks of
 *     J - lambda * (nominal vector count of the mode).
 *   - limits: B in {8, 16, 32} and S <= ME_PART_MAX_RANGE (ME_EUNSUPPORTED
 *     otherwise); ME_COST_SAD only (SSD and SSIM: ME_EUNSUPPORTED; follow-ups,
 *     SSD belongs on the matrix cores); whole frames on the context's first
 *     device only (a context with several devices: ME_EUNSUPPORTED; there is no
 *     stripe entry point); stride * height < 2^31. */
typedef enum me_part_mode {
  ME_PART_2Nx2N = 0,
  ME_PART_2NxN = 1,
  ME_PART_Nx2N = 2,
  ME_PART_NxN = 3
} me_part_mode;
#define ME_PART_MAX_RANGE 128
#define ME_PART_MAX_LAMBDA (1u << 24)

/* The records of a partition search, one array per grid (host arrays for the
 * host entry points, device arrays for the device ones).  The mv_* arrays and
 * mode are required; the cost_* arrays and mode_cost may be NULL. */
typedef struct me_part_fields {
  int16_t* mv_2nx2n;   /* [nby][nbx][2] */
  int16_t* mv_2nxn;    /* [nhy][nbx][2] */
  int16_t* mv_nx2n;    /* [nby][nhx][2] */
  int16_t* mv_nxn;     /* [nhy][nhx][2] */
  uint32_t* cost_2nx2n;
  uint32_t* cost_2nxn;
  uint32_t* cost_nx2n;
  uint32_t* cost_nxn;
  uint8_t* mode;       /* [nby][nbx] me_part_mode */
  uint32_t* mode_cost; /* [nby][nbx] J of the chosen mode */
} me_part_fields;

/* counts[0..4) = cells of the 2Nx2N, 2NxN, Nx2N and NxN grids.  Host only. */
me_status me_partition_counts(int width, int height, int block_size, int counts[4]);

enum { ME_PART_KERNEL_GENERIC = 0, ME_PART_KERNEL_FAST = 1 };
/* The kernel that takes the frame's full-size macroblocks: ME_PART_KERNEL_FAST
 * (the packed-u16 quadrant kernel: B = 16, S <= 64, width and row pitch
 * multiples of 4, at least one full-size macroblock; it also needs planes and
 * frame strides that are multiples of 4 bytes, which the launch checks on top)
 * or ME_PART_KERNEL_GENERIC; -1 for arguments the search rejects.  Chosen by
 * B, S and the row alignment only, never by the frame size.  Clipped
 * macroblocks of any frame run on the generic kernel.  Host only; the launch
 * consults this same function. */
int me_partition_kernel_variant(int width, int height, int stride, int block_size,
                                int search_range);

/* Search n_frames >= 1 whole frames of one geometry on HBM-resident planes of
 * ctx's first device, laid out as for me_refine_qpel_device: frame f's planes
 * at d_ref + f * ref_frame_stride and d_cur + f * cur_frame_stride bytes, its
 * records at each pointer of d_out + f * that grid's count (x 2 for vectors).
 * d_out is a HOST struct of device pointers, read before the call returns.
 * Asynchronous on `stream`, ordered after the context's previous search like
 * any search; uses no context scratch, so it can be captured
 * (me_capture_begin) without a warm-up call. */
me_status me_partition_search_device(me_ctx* ctx, const uint8_t* d_ref, size_t ref_frame_stride,
                                     const uint8_t* d_cur, size_t cur_frame_stride, int width,
                                     int height, int stride, int block_size, int search_range,
                                     me_cost cost, uint32_t lambda, int n_frames,
                                     const me_part_fields* d_out, void* stream);

/* The same on host planes of row pitch `stride` into host arrays, synchronous. */
me_status me_partition_search(me_ctx* ctx, const uint8_t* ref, const uint8_t* cur, int width,
                              int height, int stride, int block_size, int search_range,
                              me_cost cost, uint32_t lambda, const me_part_fields* out);

/* The leaf field of n_frames searched frames on the device: d_in's four mv_*
 * arrays and mode (the costs are not read), d_leaf_mv [n_frames][nhy][nhx][2].
 * Asynchronous on `stream`, ordered like a search.  A mode byte above 3 is
 * read as ME_PART_NxN (not checked: the field is on the device). */
me_status me_partition_leaf_field_device(me_ctx* ctx, int width, int height, int block_size,
                                         int n_frames, const me_part_fields* d_in,
                                         int16_t* d_leaf_mv, void* stream);

/* The leaf field of one frame on the host: no context and no GPU.  ME_EINVAL
 * for a mode byte above 3. */
me_status me_partition_leaf_field(int width, int height, int block_size,
                                  const me_part_fields* in, int16_t* leaf_mv);

/* ---- rate-constrained motion search: J = SAD + lambda * bits(mv - predictor) ----
 * The integer full search and the quarter-pel refinement with the cost of
 * coding the vector in the objective.  No reference counterpart; parity is
 * against the numpy restatement tests/rd_ref.py.  Exact integers (DESIGN.md
 * "Rate-constrained search"):
 *   - bits(v) = 2 * floor(log2(2 |v| + 1)) + 1, the length of the signed
 *     exp-Golomb code se(v): 0 -> 1; +-1 -> 3; +-2, +-3 -> 5; +-4 .. +-7 -> 7.
 *   - a predictor p = (px, py) per block is int16 in QUARTER-pel units, the
 *     units of me_refine_qpel's output: a previous frame's refined field is a
 *     predictor as it stands.  A NULL predictor array means all zero.  Any
 *     int16 value is legal: |4 d - p| <= 4 * 1024 + 32,767, so bits <= 33 per
 *     component and R <= 66.
 *   - integer search: for block b and displacement d = (dx, dy),
 *     R(d) = bits(4 dx - px) + bits(4 dy - py), J(d) = SAD(d) + lambda * R(d).
 *     The candidates are me_full_search's at (B, S), clamping included; the
 *     winner is the first minimum of J in raster order (dy outer, dx inner,
 *     strict <).  Per block: the vector (int16, integer units), block_cost = J,
 *     block_dist = SAD, block_bits = R (one byte).  lambda <= ME_RD_MAX_LAMBDA,
 *     so J < 2^32 (64 * 64 * 255 + 66 * 2^24).  With lambda = 0 the vectors and
 *     costs are me_full_search's at SAD bit for bit, whatever the predictor.
 *   - refinement: me_refine_qpel's procedure (stages, candidate order, centre
 *     carried, strict <) on Jq(q) = cost(P(q)) + lambda * (bits(qx - px) +
 *     bits(qy - py)), cost SAD, SSD or SATD.  Outputs mv_q, block_cost = Jq,
 *     block_dist = cost(P(mv_q)).  With lambda = 0 it is me_refine_qpel bit for
 *     bit.  Jq < 2^32 for SSD too (64 * 64 * 255^2 + 66 * 2^24).
 *   - limits: the search costs ME_COST_SAD only (SSD and SSIM:
 *     ME_EUNSUPPORTED; follow-ups), B in [1, ME_MAX_BLOCK], S <=
 *     ME_RD_MAX_RANGE (ME_EUNSUPPORTED above); the refinement has
 *     me_refine_qpel's limits.  Both: whole frames on the context's first
 *     device only (a context with several devices or repeated ids:
 *     ME_EUNSUPPORTED; no stripe entry point); lambda above ME_RD_MAX_LAMBDA or
 *     a negative range: ME_EINVAL. */
#define ME_RD_MAX_RANGE 128
#define ME_RD_MAX_LAMBDA (1u << 24)
/* Largest lambda of the fast kernel: its 32-bit lane key J << 6 | index needs
 * J <= 65,280 + 66 lambda < 2^26. */
#define ME_RD_FAST_MAX_LAMBDA 1015811u

/* bits(v) as defined above, for any int.  Host only. */
int me_mv_bits(int v);

enum { ME_RD_KERNEL_GENERIC = 0, ME_RD_KERNEL_FAST = 1 };
/* The kernel that takes the frame's full-size blocks: ME_RD_KERNEL_FAST (B =
 * 16, S <= 64, width and row pitch multiples of 4, at least one full-size
 * block, lambda <= ME_RD_FAST_MAX_LAMBDA; it also needs planes and frame
 * strides that are multiples of 4 bytes, which the launch checks on top) or
 * ME_RD_KERNEL_GENERIC; -1 for arguments the search rejects.  Chosen by B, S,
 * the row alignment and lambda only, never by the frame size.  Clipped blocks
 * of any frame run on the generic kernel.  Host only; the launch consults this
 * same function. */
int me_rd_kernel_variant(int width, int height, int stride, int block_size, int search_range,
                         uint32_t lambda);

/* Search n_frames >= 1 whole frames of one geometry on HBM-resident planes of
 * ctx's first device, laid out as for me_refine_qpel_device: frame f's planes
 * at d_ref + f * ref_frame_stride and d_cur + f * cur_frame_stride bytes, its
 * predictors at d_pred_q + 2 * f * nblk, its results at d_mv_xy + 2 * f * nblk
 * and d_block_cost / d_block_dist / d_block_bits + f * nblk.  d_pred_q (all
 * zero), d_block_dist and d_block_bits may be NULL.  Asynchronous on `stream`,
 * ordered after the context's previous search like any search; uses no context
 * scratch, so it can be captured (me_capture_begin) without a warm-up call. */
me_status me_rd_search_device(me_ctx* ctx, const uint8_t* d_ref, size_t ref_frame_stride,
                              const uint8_t* d_cur, size_t cur_frame_stride, int width,
                              int height, int stride, int block_size, int search_range,
                              me_cost cost, uint32_t lambda, int n_frames,
                              const int16_t* d_pred_q, int16_t* d_mv_xy, uint32_t* d_block_cost,
                              uint32_t* d_block_dist, uint8_t* d_block_bits, void* stream);

/* The same on host planes of row pitch `stride` into host arrays, synchronous. */
me_status me_rd_search(me_ctx* ctx, const uint8_t* ref, const uint8_t* cur, int width,
                       int height, int stride, int block_size, int search_range, me_cost cost,
                       uint32_t lambda, const int16_t* pred_q, int16_t* mv_xy,
                       uint32_t* block_cost, uint32_t* block_dist, uint8_t* block_bits);

/* me_refine_qpel_device / me_refine_qpel with the rate term: d_pred_q laid out
 * like d_mv_xy (NULL: all zero), d_block_cost = Jq and d_block_dist = the
 * distortion at d_mv_q (each may be NULL). */
me_status me_refine_qpel_rd_device(me_ctx* ctx, const uint8_t* d_ref, size_t ref_frame_stride,
                                   const uint8_t* d_cur, size_t cur_frame_stride, int width,
                                   int height, int stride, int block_size, me_cost cost,
                                   uint32_t lambda, int n_frames, const int16_t* d_pred_q,
                                   const int16_t* d_mv_xy, int16_t* d_mv_q,
                                   uint32_t* d_block_cost, uint32_t* d_block_dist, void* stream);
me_status me_refine_qpel_rd(me_ctx* ctx, const uint8_t* ref, const uint8_t* cur, int width,
                            int height, int stride, int block_size, me_cost cost, uint32_t lambda,
                            const int16_t* pred_q, const int16_t* mv_xy, int16_t* mv_q,
                            uint32_t* block_cost, uint32_t* block_dist);

/* me_rd_search then me_refine_qpel_rd back to back on the device with the same
 * predictor and lambda, as me_full_search_qpel does: the integer field never
 * visits the host.  ME_COST_SAD (the search's limit), or ME_COST_SATD: the
 * search then runs at SAD and the refinement at SATD, the encoder's usual
 * split.  One context device.  pred_q and block_cost may be NULL. */
me_status me_full_search_rd_qpel(me_ctx* ctx, const uint8_t* ref, const uint8_t* cur, int width,
                                 int height, int stride, int block_size, int search_range,
                                 me_cost cost, uint32_t lambda, const int16_t* pred_q,
                                 int16_t* mv_q, uint32_t* block_cost);

/* ---- rate-constrained partition search: J per partition, mode by rate ----
 * The partition search with the cost of coding each vector in the objective
 * and the mode priced by its code length.  No reference counterpart; parity is
 * against the numpy restatement tests/partition_rd_ref.py.  Grids, partitions,
 * candidate displacements, storage order and the leaf field are those of
 * "partition search" above, unchanged; bits(v) and the quarter-pel predictor
 * units are those of "rate-constrained motion search".  On top of them (exact
 * integers; DESIGN.md "Rate-constrained partition search"):
 *   - predictor: one int16 (px, py) per macroblock in quarter-pel units,
 *     pred_q[nby][nbx][2], the layout of me_rd_search's predictor at block size
 *     B, so one array feeds both calls.  NULL means all zero; any int16 value
 *     is legal.  All nine partitions of a macroblock use the macroblock's
 *     predictor: it is what an encoder knows before it has chosen the shape.
 *   - rate and cost: the rate of displacement d = (dx, dy) of macroblock b is
 *     R_b(d) = bits(4 dx - px) + bits(4 dy - py) <= 66; the cost of partition p
 *     of b at d is J_p(d) = SAD_p(d) + lambda * R_b(d).
 *   - winner per partition: the first minimum of J_p in raster order of the
 *     displacements (dy outer, dx inner, strict <).  Per cell of each grid: the
 *     vector, cost = J_p, dist = SAD_p and bits = R (one byte).
 *   - mode: J(m) = sum of J_p over the non-empty partitions of shape m +
 *     lambda * mbits(m), mbits = (1, 3, 3, 5), the ue(m) code lengths.  Modes
 *     are tried in the order 0, 1, 2, 3 and a later one replaces the best only
 *     if strictly smaller.  mode: one byte; mode_cost: J(mode) as u32.
 *   - limits: lambda <= ME_PART_RD_MAX_LAMBDA, which keeps J below 2^32 at
 *     B = 32 (261,120 + (4 * 66 + 5) * 2^23 < 2^32); a larger lambda returns
 *     ME_EINVAL.  Every other limit is me_partition_search's: B in {8, 16, 32}
 *     and S <= ME_PART_MAX_RANGE, SAD only, whole frames on the context's
 *     first device only (several devices or repeated ids: ME_EUNSUPPORTED),
 *     stride * height < 2^31.
 *   - identities: (E1) with lambda = 0 the four vector fields, their costs,
 *     mode and mode_cost are me_partition_search's at lambda = 0 bit for bit,
 *     whatever the predictor, and dist == cost.  (E2) The 2Nx2N records
 *     (vector, J, dist, bits) are me_rd_search's at (B, S, lambda, the same
 *     predictor) bit for bit, for every B.  (E3) The NxN records of a full-size
 *     macroblock whose window is clamped on no side are me_rd_search's at
 *     (B/2, S, lambda) with each macroblock's predictor repeated over its four
 *     quarters.  (E4) For lambda1 < lambda2 and every cell, bits1 >= bits2 and
 *     dist1 <= dist2.  (E5) With the leaf field compensated by
 *     me_compensate_planes at B/2, sum |mc - cur| = sum over the macroblocks of
 *     the dist_p of the chosen mode's partitions = sum of (mode_cost - lambda *
 *     (mbits(mode) + sum of bits_p)). */
#define ME_PART_RD_MAX_LAMBDA (1u << 23)

/* The records of a rate-constrained partition search: f as in me_part_fields
 * (cost_* = J_p; mv_* and mode required, the rest optional), plus the
 * distortion and the rate of every cell, laid out like the cost_* arrays. */
typedef struct me_part_rd_fields {
  me_part_fields f;
  uint32_t* dist_2nx2n; /* each may be NULL */
  uint32_t* dist_2nxn;
  uint32_t* dist_nx2n;
  uint32_t* dist_nxn;
  uint8_t* bits_2nx2n;  /* each may be NULL */
  uint8_t* bits_2nxn;
  uint8_t* bits_nx2n;
  uint8_t* bits_nxn;
} me_part_rd_fields;

/* The kernel that takes the frame's full-size macroblocks: ME_PART_KERNEL_FAST
 * where me_partition_kernel_variant says so and lambda <= ME_RD_FAST_MAX_LAMBDA
 * (the fast kernel's 32-bit lane key J << 6 | index needs 65,280 + 66 lambda <
 * 2^26, as in me_rd_kernel_variant), else ME_PART_KERNEL_GENERIC; -1 for
 * arguments the search rejects.  Host only; the launch consults this same
 * function (and checks the planes' and frame strides' 4-byte alignment on
 * top). */
int me_partition_rd_kernel_variant(int width, int height, int stride, int block_size,
                                   int search_range, uint32_t lambda);

/* Search n_frames >= 1 whole frames of one geometry on HBM-resident planes of
 * ctx's first device, laid out as for me_partition_search_device; frame f's
 * predictors at d_pred_q + 2 * f * nbx * nby (NULL: all zero).  d_out is a HOST
 * struct of device pointers, read before the call returns.  Asynchronous on
 * `stream`, ordered after the context's previous search like any search; uses
 * no context scratch, so it can be captured (me_capture_begin) without a
 * warm-up call.  me_partition_leaf_field* take &d_out->f as they are. */
me_status me_partition_rd_search_device(me_ctx* ctx, const uint8_t* d_ref,
                                        size_t ref_frame_stride, const uint8_t* d_cur,
                                        size_t cur_frame_stride, int width, int height,
                                        int stride, int block_size, int search_range,
                                        me_cost cost, uint32_t lambda, int n_frames,
                                        const int16_t* d_pred_q, const me_part_rd_fields* d_out,
                                        void* stream);

/* The same on host planes of row pitch `stride` and host arrays, synchronous. */
me_status me_partition_rd_search(me_ctx* ctx, const uint8_t* ref, const uint8_t* cur, int width,
                                 int height, int stride, int block_size, int search_range,
                                 me_cost cost, uint32_t lambda, const int16_t* pred_q,
                                 const me_part_rd_fields* out);

/* ---- partition-wise quarter-pel refinement with sub-pel mode decision ----
 * Takes the four integer grids of a partition search to quarter-pel, each of
 * the nine partitions of a macroblock refined as one rectangle under J = cost +
 * lambda * bits, and decides the mode again on the refined J.  No reference
 * counterpart; parity is against the numpy restatement
 * tests/partition_qpel_ref.py.  Grids, partitions, storage order, clipping and
 * the leaf field are those of "partition search"; samples, stages, candidate
 * order, the carried centre and strict < are those of "quarter-pel
 * refinement"; bits(v), the predictor units and the one-predictor-per-macroblock
 * rule are those of "rate-constrained partition search".  On top of them (exact
 * integers; DESIGN.md "Partition-wise quarter-pel refinement"):
 *   - input: the four integer vector grids mv_2nx2n, mv_2nxn, mv_nx2n, mv_nxn
 *     of a me_part_fields; nothing else of the struct is read.  Any integer
 *     fields are legal, not only a search's output; precondition |component|
 *     <= ME_QPEL_MAX_MV (checked by the host call; the device call reads inside
 *     the planes for any int16 but 4 m +- 3 must fit int16).
 *   - refinement of a cell: each non-empty partition p of macroblock b is a
 *     rectangle (x, y, w, h) clipped to the frame with integer vector m_p.  It
 *     is refined by me_refine_qpel_rd's procedure on that rectangle: start at
 *     4 m_p, stage 1 the eight neighbours at step 2, stage 2 the eight
 *     neighbours of stage 1's winner at step 1, each in raster order, the
 *     centre carried, a candidate replacing the best only if strictly smaller,
 *     on Jq_p(q) = cost_p(P(q)) + lambda * (bits(qx - px_b) + bits(qy - py_b)).
 *     cost is SAD, SSD or SATD over the rectangle's pixels only; SATD tiles are
 *     anchored at the partition's top-left (partition offsets are multiples of
 *     h >= 4, so these are the macroblock-anchored tiles too).
 *   - output per cell of each grid: the quarter-pel vector, cost = Jq_p, dist =
 *     cost_p at the result, bits = the result's rate as one byte (|q - p| <=
 *     4 * 8000 + 3 + 32,768: 33 bits per component, R <= 66).
 *   - mode: J(m) = sum of Jq_p over the non-empty partitions of shape m +
 *     lambda * mbits(m), mbits = (1, 3, 3, 5).  Modes are tried in the order
 *     0, 1, 2, 3 and a later one replaces the best only if strictly smaller.
 *     mode: one byte per macroblock; mode_cost: J(mode) as u32.
 *   - limits: lambda <= ME_PART_RD_MAX_LAMBDA, which keeps J below 2^32 for SSD
 *     at B = 32 (66,585,600 + 269 * 2^23 = 2,323,121,152); a larger lambda
 *     returns ME_EINVAL.  B in {8, 16, 32} (others ME_EUNSUPPORTED);
 *     ME_COST_SSIM returns ME_EUNSUPPORTED; whole frames on the context's first
 *     device only (several devices or repeated ids: ME_EUNSUPPORTED); stride *
 *     height < 2^31.
 *   - identities: (Q1) the 2Nx2N records (vector, J, dist) are
 *     me_refine_qpel_rd's at block size B on mv_2nx2n with the same predictor,
 *     bit for bit, for every cost.  (Q2) The NxN records of every cell, clipped
 *     ones included, are me_refine_qpel_rd's at block size h on mv_nxn with
 *     each macroblock's predictor repeated over its four quarters.  (Q3) With
 *     lambda = 0, cost == dist and the 2Nx2N and NxN vectors are
 *     me_refine_qpel's.  (Q4) mode and mode_cost follow from the cost arrays
 *     alone by the mode rule.  (Q5) With the leaf field of the output
 *     compensated by me_compensate_planes_qpel at B/2, at ME_COST_SAD
 *     sum |mc - cur| = sum over the macroblocks of the dist of the chosen
 *     mode's partitions: a prediction sample depends only on the pixel and the
 *     vector, so a partition's vector repeated over its cells reproduces the
 *     partition's prediction.  (Q6) Every cell's J is at most the J of its own
 *     centre 4 m_p. */

/* Refine n_frames >= 1 whole frames on HBM-resident planes of ctx's first
 * device; layout and batching are me_partition_rd_search_device's (frame f's
 * planes at + f * frame stride, its records at each pointer + f * that grid's
 * count, its predictors at d_pred_q + 2 * f * nbx * nby, NULL: all zero).
 * d_in and d_out are HOST structs of device pointers, read before the call
 * returns.  d_out->f.mv_* and d_out->f.mode are required, everything else of
 * d_out may be NULL.  In place (d_out->f.mv_x == d_in->mv_x) is allowed: a
 * workgroup reads its macroblock's records before it writes them and every cell
 * belongs to exactly one macroblock.  Asynchronous on `stream`, ordered like a
 * search; uses no context scratch, so it can be captured (me_capture_begin)
 * without a warm-up call.  me_partition_leaf_field* copy int16 vectors whatever
 * their unit: they take &d_out->f unchanged and give the quarter-pel leaf field
 * (block size B/2) that me_compensate_planes_qpel takes. */
me_status me_partition_refine_qpel_device(me_ctx* ctx, const uint8_t* d_ref,
                                          size_t ref_frame_stride, const uint8_t* d_cur,
                                          size_t cur_frame_stride, int width, int height,
                                          int stride, int block_size, me_cost cost,
                                          uint32_t lambda, int n_frames, const int16_t* d_pred_q,
                                          const me_part_fields* d_in,
                                          const me_part_rd_fields* d_out, void* stream);

/* The same on host planes of row pitch `stride` and host arrays, synchronous.
 * A component beyond ME_QPEL_MAX_MV in any of the four input grids: ME_EINVAL. */
me_status me_partition_refine_qpel(me_ctx* ctx, const uint8_t* ref, const uint8_t* cur, int width,
                                   int height, int stride, int block_size, me_cost cost,
                                   uint32_t lambda, const int16_t* pred_q,
                                   const me_part_fields* in, const me_part_rd_fields* out);

/* me_partition_rd_search at SAD, the refinement above at `cost` and, if
 * leaf_mv_q is not NULL, the leaf field ([nhy][nhx][2], quarter-pel units),
 * back to back on the device with the same predictor and lambda: no field
 * visits the host in between.  ME_COST_SAD, or ME_COST_SATD (the search then
 * runs at SAD and the refinement at SATD); any other cost gets the status
 * me_full_search_rd_qpel gives it.  One context device.  pred_q may be NULL. */
me_status me_partition_search_qpel(me_ctx* ctx, const uint8_t* ref, const uint8_t* cur, int width,
                                   int height, int stride, int block_size, int search_range,
                                   me_cost cost, uint32_t lambda, const int16_t* pred_q,
                                   const me_part_rd_fields* out, int16_t* leaf_mv_q);

/* ---- frame-pair streaming ---- */

/* Pinned (page-locked) host memory.  Frames that live in it are DMAed
 * straight to the device by me_search_pairs; other frames are staged. */
void* me_host_alloc(size_t bytes);
void me_host_free(void* p);

/* Search a list of frame pairs.  frames[0..n_frames) are host Y planes
 * (width x height, row pitch stride); pairs[2*n], pairs[2*n+1] are the
 * (ref, cur) frame indices of pair n, e.g. {0,1, 1,2, 2,3} for a sequence or
 * {0,1, 0,3} for one reference against two currents.  Replaces the
 * reference's one-pair-per-process driver (src/cpu/main.c:109-179): each
 * frame is uploaded once per device, the upload of pair n+1's frames overlaps
 * the search of pair n, and with several context devices the pairs are split
 * into contiguous runs, one per device (no collective: pairs are
 * independent).  Results are those of me_full_search on each pair:
 * mv_xy [n_pairs][nblocks][2], block_cost [n_pairs][nblocks] (may be NULL).
 * Synchronous. */
me_status me_search_pairs(me_ctx* ctx, const uint8_t* const* frames, int n_frames,
                          int width, int height, int stride, int block_size,
                          int search_range, me_cost cost, const int* pairs,
                          int n_pairs, int16_t* mv_xy, uint32_t* block_cost);

/* ---- files: u8 YUV planes and the MV-field format ---- */

/* Raw YUV files as the reference reads and writes them (src/common/utils.c:29-92)
 * but kept in u8 (no int32 widening).  ME_YUV_LUMA: W*H bytes per frame (the
 * reference's frames/ForemanYF*.yuv); ME_YUV_I420: W*H*3/2 bytes per frame,
 * luma first. */
typedef enum { ME_YUV_LUMA = 0, ME_YUV_I420 = 1 } me_yuv_layout;

/* Whole frames in the file, or -1 if it cannot be opened. */
int64_t me_yuv_frame_count(const char* path, int width, int height, me_yuv_layout layout);
/* Luma plane of frame `frame_index` into dst (row pitch dst_stride >= width). */
me_status me_yuv_read_luma(const char* path, int width, int height, me_yuv_layout layout,
                           int frame_index, uint8_t* dst, int dst_stride);
/* Write (append != 0: append) `bytes` bytes, e.g. the 5-plane output of
 * me_compensate_planes (utils.c:75-92 yuvWriteFrame). */
me_status me_yuv_write(const char* path, const uint8_t* data, size_t bytes, int append);

/* MV-field file, little-endian:
 *   header (32 B): "MEMV", u16 version = 1, u16 flags (bit 0: costs present,
 *                  bit 1: vectors are in quarter-pel units, me_mv_write_qpel),
 *                  i32 width, height, block_size, search_range, cost, u32 n_pairs
 *   per pair:      i32 ref_index, i32 cur_index,
 *                  nblocks x (i16 mvx, i16 mvy)   raster order
 *                  nblocks x u32 cost             if flags & 1
 * nblocks = me_num_blocks(width, height, block_size). */
typedef struct me_mv_header {
  char magic[4];
  uint16_t version, flags;
  int32_t width, height, block_size, search_range, cost;
  uint32_t n_pairs;
} me_mv_header;

/* pairs: [n_pairs][2] frame indices (NULL: pair n = (n, n+1));
 * block_cost may be NULL (flags bit 0 cleared). */
me_status me_mv_write(const char* path, int width, int height, int block_size,
                      int search_range, me_cost cost, const int* pairs, int n_pairs,
                      const int16_t* mv_xy, const uint32_t* block_cost);
/* The same file with quarter-pel vectors (me_refine_qpel, me_full_search_qpel):
 * flags bit 1 set, everything else as me_mv_write.  The readers accept flags
 * 0-3 and hand them back unchanged in the header; the records are read the
 * same way. */
me_status me_mv_write_qpel(const char* path, int width, int height, int block_size,
                           int search_range, me_cost cost, const int* pairs, int n_pairs,
                           const int16_t* mv_q, const uint32_t* block_cost);
me_status me_mv_read_header(const char* path, me_mv_header* hdr);
/* Read everything; buffers sized from the header (pairs [n_pairs][2],
 * mv_xy [n_pairs][nblocks][2], block_cost [n_pairs][nblocks]); any may be
 * NULL to skip it.  A file without costs leaves block_cost untouched. */
me_status me_mv_read(const char* path, me_mv_header* hdr, int* pairs, int16_t* mv_xy,
                     uint32_t* block_cost);

#ifdef __cplusplus
}
#endif
#endif /* ME_H */
