// me_api_stages.hip -- C ABI of libme_hip.so (include/me.h), the stages that
// work on a searched field: compensation, quarter-pel refinement,
// bi-prediction, partition search, the rate-constrained searches and the
// partition-wise quarter-pel refinement.
//
// Every entry point is its argument rules (me_api_rules.cpp, in the order
// written here), then for a host call upload_planes and a record layout, then
// enqueue() of one launcher on a FrameBatch, then download().  The context, the
// integer searches and the helpers they share are me_api.hip's.
#include <hip/hip_runtime.h>
#include <math.h>

#include "me_internal.h"

namespace me {
namespace R = rules;
namespace {

// Where a rule writes its message; return a status that is not ME_OK.
#define ERR(c) (c)->err, sizeof (c)->err
#define TRY(x)                          \
  do {                                  \
    const me_status s_ = (x);           \
    if (s_ != ME_OK) return s_;         \
  } while (0)

// The arguments hold: clear the message and enqueue one launch of `family` on
// s after the device's previous search (not while capturing: me_graph_launch
// orders the graph).  launch: (hipStream_t) -> hipError_t.
template <typename F>
me_status enqueue(me_ctx* c, Dev& d, hipStream_t s, const char* family, F&& launch) {
  c->err[0] = 0;
  if (!capturing(s)) TRY(order_on(c, d, s));
  const hipError_t e = launch(s);
  if (e != hipSuccess) return fail(c, ME_EDEVICE, "%s launch: %s", family, hipGetErrorString(e));
  return ME_OK;
}

// The one frame upload_planes left packed: ref (d.ref or a third plane) and d.cur.
FrameBatch packed(const Dev& d, const uint8_t* ref, int width, int height, int blk) {
  return FrameBatch{ref, 0, d.cur, 0, width, height, width, blk, 1};
}

// The fast kernel a *_kernel_variant function names also needs planes and
// frame strides that are multiples of 4 bytes for its LDS DMA.
bool dma_fast(bool variant_is_fast, const FrameBatch& b) {
  return variant_is_fast &&
         ((uintptr_t)b.ref | (uintptr_t)b.cur |
          (b.n_frames > 1 ? b.ref_frame_stride | b.cur_frame_stride : 0)) % 4 == 0;
}

// Records to the caller on d.stream; a null host array is an output not asked for.
me_status download(me_ctx* c, Dev& d, void* host, const void* dev, size_t bytes) {
  if (host) HIPCHK(c, hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, d.stream));
  return ME_OK;
}
me_status upload(me_ctx* c, Dev& d, void* dev, const void* host, size_t bytes) {
  HIPCHK(c, hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, d.stream));
  return ME_OK;
}
// Every region of L with a host array, in L's order (sync: then wait for them).
me_status download_all(me_ctx* c, Dev& d, const R::Layout& L, void* const* host, bool sync) {
  for (int k = 0; k < L.n; k++) TRY(download(c, d, host[k], d.rec + L.off[k], L.bytes[k]));
  if (sync) HIPCHK(c, hipStreamSynchronize(d.stream));
  return ME_OK;
}

// The frame-batch rule for a ref and a cur plane of stride * height bytes.
me_status check_frames(me_ctx* c, int n_frames, int stride, int height, size_t rfs, size_t cfs) {
  const unsigned long long fb = (unsigned long long)stride * height;
  const R::FramePlane p[2] = {{rfs, fb}, {cfs, fb}};
  return R::frame_batch(n_frames, p, 2, ERR(c));
}

// ---- compensation (me_post.hip, me_subpel.hip) ----

me_status grow_compensation(me_ctx* c, Dev& d, size_t out_bytes) {
  size_t scap = d.stats ? 16 : 0;
  const me_status s = grow(c, (void**)&d.stats, &scap, 16);
  return s != ME_OK ? s : grow(c, (void**)&d.out5, &d.out_cap, out_bytes);
}

// Run the compensation kernel `launch` enqueues into d.out5 / d.stats, hand the
// planes out and close the PSNR.
template <typename F>
me_status finish_compensation(me_ctx* c, Dev& d, int width, int height, uint8_t* out,
                              size_t out_bytes, double* psnr, F&& launch) {
  HIPCHK(c, hipMemsetAsync(d.stats, 0, 16, d.stream));
  HIPCHK(c, launch());
  unsigned long long st[2] = {0, 0};
  HIPCHK(c, hipMemcpyAsync(out, d.out5, out_bytes, hipMemcpyDeviceToHost, d.stream));
  HIPCHK(c, hipMemcpyAsync(st, d.stats, 16, hipMemcpyDeviceToHost, d.stream));
  HIPCHK(c, hipStreamSynchronize(d.stream));
  if (psnr) {  // utils.c:147-154, double arithmetic on the exact integer sum
    double mse = (double)st[0];
    mse /= (double)width * height;
    *psnr = mse == 0 ? 99.0 : 20 * log10((double)st[1]) - 10 * log10(mse);
  }
  return ME_OK;
}

me_status compensate(me_ctx* c, const uint8_t* ref, const uint8_t* cur, int width, int height,
                     int blk, const int16_t* mv_xy, uint8_t* out, int planes, double* psnr,
                     bool qpel = false) {
  TRY(check_args(c, ref, cur ? cur : ref, width, height, width, blk, 0, ME_COST_SSD, mv_xy));
  if (!out) return fail(c, ME_EINVAL, "null output");
  Dev& d = c->devs[0];
  HIPCHK(c, hipSetDevice(d.id));
  TRY(own_stream(c, d));
  const size_t plane = (size_t)width * height;
  const size_t nb = (size_t)me_num_blocks(width, height, blk);
  const R::Layout L = R::layout_mv_cost(nb);
  TRY(grow(c, (void**)&d.ref, &d.frame_cap, 2 * plane));
  d.cur = d.ref + plane;
  TRY(grow(c, (void**)&d.rec, &d.rec_cap, L.total));
  const size_t out_bytes = planes ? 5 * plane : plane;
  TRY(grow_compensation(c, d, out_bytes));
  // (the planes are packed: plain copies, not upload_planes' 2-D ones)
  int16_t* dmv = rec_at<int16_t>(d, L, R::REC_MV);
  TRY(upload(c, d, d.ref, ref, plane));
  TRY(upload(c, d, d.cur, cur ? cur : ref, plane));
  TRY(upload(c, d, dmv, mv_xy, L.bytes[R::REC_MV]));
  return finish_compensation(c, d, width, height, out, out_bytes, psnr, [&] {
    return (qpel ? launch_qpel_compensate : launch_compensate)(
        d.ref, d.cur, width, height, blk, dmv, d.out5, planes, d.stats, d.stream);
  });
}

me_status compensate_bipred(me_ctx* c, const uint8_t* ref0, const uint8_t* ref1, const uint8_t* cur,
                            int width, int height, int blk, const int16_t* mv0, const int16_t* mv1,
                            const uint8_t* mode, uint8_t* out, int planes, double* psnr) {
  if (!cur) cur = ref0;
  TRY(check_args(c, ref0, cur, width, height, width, blk, 0, ME_COST_SSD, mv0));
  if (!ref1 || !mv1 || !mode || !out)
    return fail(c, ME_EINVAL, "null bi-prediction plane, field, mode or output pointer");
  const size_t nb = (size_t)me_num_blocks(width, height, blk);
  TRY(R::pred_modes(mode, nb, ERR(c)));
  Dev& d = c->devs[0];
  const R::Layout L = R::layout_bipred(nb);
  TRY(upload_planes(c, d, {ref0, cur, ref1}, width, height, width, L.total));
  const size_t plane = (size_t)width * height;
  const size_t out_bytes = planes ? 5 * plane : plane;
  TRY(grow_compensation(c, d, out_bytes));
  int16_t *q0 = rec_at<int16_t>(d, L, R::BI_Q0), *q1 = rec_at<int16_t>(d, L, R::BI_Q1);
  uint8_t* dmode = rec_at<uint8_t>(d, L, R::BI_MODE);
  TRY(upload(c, d, q0, mv0, L.bytes[R::BI_Q0]));
  TRY(upload(c, d, q1, mv1, L.bytes[R::BI_Q1]));
  TRY(upload(c, d, dmode, mode, L.bytes[R::BI_MODE]));
  return finish_compensation(c, d, width, height, out, out_bytes, psnr, [&] {
    return launch_bipred_compensate(d.ref, d.ref + 2 * plane, d.cur, width, height, blk, q0, q1,
                                        dmode, d.out5, planes, d.stats, d.stream);
  });
}

// ---- the rule sequences several entry points share ----

// check_args at the search's cost, then the refinement's own rules.
me_status check_refine(me_ctx* c, const void* ref, const void* cur, int width, int height,
                       int stride, int blk, int range, me_cost cost, const void* mv,
                       const void* mv_q) {
  const me_status s =
      check_args(c, ref, cur, width, height, stride, blk, range, R::search_cost(cost), mv);
  return s != ME_OK ? s : R::qpel(cost, mv_q, ERR(c));
}

// ... and the bi-prediction's.
me_status check_bipred(me_ctx* c, const void* ref0, const void* ref1, const void* cur, int width,
                       int height, int stride, int blk, int range, me_cost cost, const void* q0,
                       const void* q1, const void* out0, const void* out1, const void* mode) {
  const me_status s =
      check_args(c, ref0, cur, width, height, stride, blk, range, R::search_cost(cost), q0);
  return s != ME_OK ? s : R::bipred(cost, ref1, q1, out0, out1, mode, ERR(c));
}

// The integer search of the packed frame `ref` / d.cur into mv / cost at the
// search's cost (SATD: SAD), then its refinement in place: the searched
// vectors stay inside the window (|m| <= ME_MAX_RANGE).
me_status search_and_refine(me_ctx* c, Dev& d, const uint8_t* ref, int width, int height, int blk,
                            int range, me_cost cost, int16_t* mv, uint32_t* bcost) {
  const SearchJob J{ref, 0, d.cur, 0, 0, (height + blk - 1) / blk, mv, bcost};
  SearchArgs p = make_args(J, width, height, width, blk, range, R::search_cost(cost));
  TRY(attach_scratch(c, d, p));
  TRY(launch_ordered(c, d, p, &J, 1, d.stream));
  const FrameBatch b = packed(d, ref, width, height, blk);
  return enqueue(c, d, d.stream, "quarter-pel refinement",
                 [&](hipStream_t st) { return launch_qpel_refine(b, cost, mv, mv, bcost, st); });
}

// d.rec under layout_partition_rd as a struct of device pointers.
me_part_rd_fields part_rd_records(Dev& d, const R::Layout& L) {
  auto v = [&](int k) { return rec_at<int16_t>(d, L, R::PRD_MV + k); };
  auto w = [&](int k) { return rec_at<uint32_t>(d, L, k); };
  auto u = [&](int k) { return rec_at<uint8_t>(d, L, k); };
  const int C = R::PRD_COST, Di = R::PRD_DIST, Bi = R::PRD_BITS;
  return me_part_rd_fields{{v(0), v(1), v(2), v(3), w(C), w(C + 1), w(C + 2), w(C + 3),
                            u(R::PRD_MODE), w(R::PRD_MODE_COST)},
                           w(Di), w(Di + 1), w(Di + 2), w(Di + 3),
                           u(Bi), u(Bi + 1), u(Bi + 2), u(Bi + 3)};
}
// The host arrays of out in layout_partition_rd's order (the predictors stay).
void part_rd_host(const me_part_rd_fields* out, void* (&to)[19]) {
  const me_part_fields& f = out->f;
  void* const t[19] = {nullptr,         f.mv_2nx2n,      f.mv_2nxn,       f.mv_nx2n,
                       f.mv_nxn,        f.cost_2nx2n,    f.cost_2nxn,     f.cost_nx2n,
                       f.cost_nxn,      out->dist_2nx2n, out->dist_2nxn,  out->dist_nx2n,
                       out->dist_nxn,   f.mode_cost,     out->bits_2nx2n, out->bits_2nxn,
                       out->bits_nx2n,  out->bits_nxn,   f.mode};
  for (int k = 0; k < 19; k++) to[k] = t[k];
}

}  // namespace
}  // namespace me

using namespace me;

extern "C" {

me_status me_motion_compensate(me_ctx* c, const uint8_t* ref, int width, int height, int blk,
                               const int16_t* mv_xy, uint8_t* mc) {
  return compensate(c, ref, nullptr, width, height, blk, mv_xy, mc, 0, nullptr);
}

me_status me_compensate_planes(me_ctx* c, const uint8_t* ref, const uint8_t* cur, int width,
                               int height, int blk, const int16_t* mv_xy, uint8_t* out5,
                               double* psnr) {
  if (!cur) return fail(c, ME_EINVAL, "null cur");
  return compensate(c, ref, cur, width, height, blk, mv_xy, out5, 1, psnr);
}

// ---- quarter-pel refinement and sub-pel compensation (me_subpel.hip) ----

me_status me_refine_qpel_device(me_ctx* c, const uint8_t* d_ref, size_t ref_frame_stride,
                                const uint8_t* d_cur, size_t cur_frame_stride, int width,
                                int height, int stride, int blk, me_cost cost, int n_frames,
                                const int16_t* d_mv_xy, int16_t* d_mv_q, uint32_t* d_block_cost,
                                void* stream) {
  if (!c) return ME_EINVAL;
  TRY(R::frame_batch(n_frames, nullptr, 0, ERR(c)));
  TRY(check_refine(c, d_ref, d_cur, width, height, stride, blk, 0, cost, d_mv_xy, d_mv_q));
  TRY(check_frames(c, n_frames, stride, height, ref_frame_stride, cur_frame_stride));
  const FrameBatch b{d_ref, ref_frame_stride, d_cur, cur_frame_stride, width, height, stride, blk,
                     n_frames};
  return enqueue(c, c->devs[0], (hipStream_t)stream, "quarter-pel refinement", [&](hipStream_t st) {
    return launch_qpel_refine(b, cost, d_mv_xy, d_mv_q, d_block_cost, st);
  });
}

me_status me_refine_qpel(me_ctx* c, const uint8_t* ref, const uint8_t* cur, int width, int height,
                         int stride, int blk, me_cost cost, const int16_t* mv_xy, int16_t* mv_q,
                         uint32_t* block_cost) {
  TRY(check_refine(c, ref, cur, width, height, stride, blk, 0, cost, mv_xy, mv_q));
  const size_t nb = (size_t)me_num_blocks(width, height, blk);
  TRY(R::vectors(&mv_xy, 1, nb, ME_QPEL_MAX_MV, "ME_QPEL_MAX_MV", ERR(c)));
  const R::Layout L = R::layout_mv_cost(nb);
  Dev& d = c->devs[0];
  TRY(upload_planes(c, d, {ref, cur}, width, height, stride, L.total));
  int16_t* dmv = rec_at<int16_t>(d, L, R::REC_MV);
  uint32_t* dcost = rec_at<uint32_t>(d, L, R::REC_COST);
  TRY(upload(c, d, dmv, mv_xy, L.bytes[R::REC_MV]));
  const FrameBatch b = packed(d, d.ref, width, height, blk);
  TRY(enqueue(c, d, d.stream, "quarter-pel refinement", [&](hipStream_t st) {
    return launch_qpel_refine(b, cost, dmv, dmv, dcost, st);
  }));
  void* const out[2] = {mv_q, block_cost};
  return download_all(c, d, L, out, true);
}

me_status me_full_search_qpel(me_ctx* c, const uint8_t* ref, const uint8_t* cur, int width,
                              int height, int stride, int blk, int range, me_cost cost,
                              int16_t* mv_q, uint32_t* block_cost) {
  TRY(check_refine(c, ref, cur, width, height, stride, blk, range, cost, mv_q, mv_q));
  TRY(R::one_device((int)c->devs.size(), "quarter-pel search", ERR(c)));
  const R::Layout L = R::layout_mv_cost((size_t)me_num_blocks(width, height, blk));
  Dev& d = c->devs[0];
  TRY(upload_planes(c, d, {ref, cur}, width, height, stride, L.total));
  TRY(search_and_refine(c, d, d.ref, width, height, blk, range, cost,
                        rec_at<int16_t>(d, L, R::REC_MV),
                        rec_at<uint32_t>(d, L, R::REC_COST)));
  void* const out[2] = {mv_q, block_cost};
  TRY(download_all(c, d, L, out, false));
  return device_status(c, d, d.stream);
}

me_status me_motion_compensate_qpel(me_ctx* c, const uint8_t* ref, int width, int height, int blk,
                                    const int16_t* mv_q, uint8_t* mc) {
  return compensate(c, ref, nullptr, width, height, blk, mv_q, mc, 0, nullptr, true);
}

me_status me_compensate_planes_qpel(me_ctx* c, const uint8_t* ref, const uint8_t* cur, int width,
                                    int height, int blk, const int16_t* mv_q, uint8_t* out5,
                                    double* psnr) {
  if (!cur) return fail(c, ME_EINVAL, "null cur");
  return compensate(c, ref, cur, width, height, blk, mv_q, out5, 1, psnr, true);
}

// ---- bi-prediction (me_subpel.hip) ----

me_status me_bipred_device(me_ctx* c, const uint8_t* d_ref0, size_t ref0_frame_stride,
                           const uint8_t* d_ref1, size_t ref1_frame_stride, const uint8_t* d_cur,
                           size_t cur_frame_stride, int width, int height, int stride, int blk,
                           me_cost cost, int refine, int n_frames, const int16_t* d_mv_q0,
                           const int16_t* d_mv_q1, int16_t* d_mv_out0, int16_t* d_mv_out1,
                           uint8_t* d_mode, uint32_t* d_block_cost, uint32_t* d_cost3,
                           void* stream) {
  if (!c) return ME_EINVAL;
  TRY(R::frame_batch(n_frames, nullptr, 0, ERR(c)));
  TRY(check_bipred(c, d_ref0, d_ref1, d_cur, width, height, stride, blk, 0, cost, d_mv_q0,
                   d_mv_q1, d_mv_out0, d_mv_out1, d_mode));
  // plane by plane: the first plane that breaks either rule is the one reported
  const unsigned long long fb = (unsigned long long)stride * height;
  for (size_t v : {ref0_frame_stride, ref1_frame_stride, cur_frame_stride}) {
    const R::FramePlane p{v, fb};
    TRY(R::frame_batch(n_frames, &p, 1, ERR(c)));
  }
  const FrameBatch b{d_ref0, ref0_frame_stride, d_cur, cur_frame_stride, width, height, stride, blk,
                     n_frames};
  return enqueue(c, c->devs[0], (hipStream_t)stream, "bi-prediction", [&](hipStream_t st) {
    return launch_bipred(b, d_ref1, ref1_frame_stride, cost, refine, d_mv_q0, d_mv_q1,
                             d_mv_out0, d_mv_out1, d_mode, d_block_cost, d_cost3, st);
  });
}

me_status me_bipred(me_ctx* c, const uint8_t* ref0, const uint8_t* ref1, const uint8_t* cur,
                    int width, int height, int stride, int blk, me_cost cost, int refine,
                    const int16_t* mv_q0, const int16_t* mv_q1, int16_t* mv_out0,
                    int16_t* mv_out1, uint8_t* mode, uint32_t* block_cost, uint32_t* cost3) {
  TRY(check_bipred(c, ref0, ref1, cur, width, height, stride, blk, 0, cost, mv_q0, mv_q1,
                   mv_out0, mv_out1, mode));
  const size_t nb = (size_t)me_num_blocks(width, height, blk);
  const int16_t* const q[2] = {mv_q0, mv_q1};
  TRY(R::vectors(q, 2, nb, ME_BIPRED_MAX_Q, "ME_BIPRED_MAX_Q", ERR(c)));
  const R::Layout L = R::layout_bipred(nb);
  Dev& d = c->devs[0];
  TRY(upload_planes(c, d, {ref0, cur, ref1}, width, height, stride, L.total));
  int16_t *q0 = rec_at<int16_t>(d, L, R::BI_Q0), *q1 = rec_at<int16_t>(d, L, R::BI_Q1);
  TRY(upload(c, d, q0, mv_q0, L.bytes[R::BI_Q0]));
  TRY(upload(c, d, q1, mv_q1, L.bytes[R::BI_Q1]));
  const FrameBatch b = packed(d, d.ref, width, height, blk);
  TRY(enqueue(c, d, d.stream, "bi-prediction", [&](hipStream_t st) {
    return launch_bipred(b, d.ref + 2 * (size_t)width * height, 0, cost, refine, q0, q1, q0,
                                  q1, rec_at<uint8_t>(d, L, R::BI_MODE),
                                  rec_at<uint32_t>(d, L, R::BI_COST),
                                  rec_at<uint32_t>(d, L, R::BI_COST3), st);
  }));
  void* const out[5] = {mv_out0, mv_out1, block_cost, cost3, mode};
  return download_all(c, d, L, out, true);
}

me_status me_full_search_bipred(me_ctx* c, const uint8_t* ref0, const uint8_t* ref1,
                                const uint8_t* cur, int width, int height, int stride, int blk,
                                int range, me_cost cost, int16_t* mv_out0, int16_t* mv_out1,
                                uint8_t* mode, uint32_t* block_cost) {
  TRY(check_bipred(c, ref0, ref1, cur, width, height, stride, blk, range, cost, mv_out0,
                   mv_out1, mv_out0, mv_out1, mode));
  TRY(R::one_device((int)c->devs.size(), "bi-predictive search", ERR(c)));
  const R::Layout L = R::layout_bipred((size_t)me_num_blocks(width, height, blk));
  Dev& d = c->devs[0];
  TRY(upload_planes(c, d, {ref0, cur, ref1}, width, height, stride, L.total));
  const uint8_t* d_ref1 = d.ref + 2 * (size_t)width * height;
  int16_t *q0 = rec_at<int16_t>(d, L, R::BI_Q0), *q1 = rec_at<int16_t>(d, L, R::BI_Q1);
  uint32_t* dcost = rec_at<uint32_t>(d, L, R::BI_COST);
  // search and refine against ref0, then ref1 (dcost is overwritten by each
  // stage; the bi-prediction's is the one that is read back)
  TRY(search_and_refine(c, d, d.ref, width, height, blk, range, cost, q0, dcost));
  TRY(search_and_refine(c, d, d_ref1, width, height, blk, range, cost, q1, dcost));
  const FrameBatch b = packed(d, d.ref, width, height, blk);
  TRY(enqueue(c, d, d.stream, "bi-prediction", [&](hipStream_t st) {
    return launch_bipred(b, d_ref1, 0, cost, 1, q0, q1, q0, q1,
                                  rec_at<uint8_t>(d, L, R::BI_MODE), dcost, nullptr, st);
  }));
  void* const out[5] = {mv_out0, mv_out1, block_cost, nullptr, mode};
  TRY(download_all(c, d, L, out, false));
  return device_status(c, d, d.stream);
}

me_status me_motion_compensate_bipred(me_ctx* c, const uint8_t* ref0, const uint8_t* ref1,
                                      int width, int height, int blk, const int16_t* mv0,
                                      const int16_t* mv1, const uint8_t* mode, uint8_t* mc) {
  return compensate_bipred(c, ref0, ref1, nullptr, width, height, blk, mv0, mv1, mode, mc, 0,
                           nullptr);
}

me_status me_compensate_planes_bipred(me_ctx* c, const uint8_t* ref0, const uint8_t* ref1,
                                      const uint8_t* cur, int width, int height, int blk,
                                      const int16_t* mv0, const int16_t* mv1, const uint8_t* mode,
                                      uint8_t* out5, double* psnr) {
  if (!cur) return fail(c, ME_EINVAL, "null cur");
  return compensate_bipred(c, ref0, ref1, cur, width, height, blk, mv0, mv1, mode, out5, 1, psnr);
}

// ---- partition search (me_partition.hip, me_partition_plan.cpp) ----

me_status me_partition_search_device(me_ctx* c, const uint8_t* d_ref, size_t ref_frame_stride,
                                     const uint8_t* d_cur, size_t cur_frame_stride, int width,
                                     int height, int stride, int blk, int range, me_cost cost,
                                     uint32_t lambda, int n_frames, const me_part_fields* d_out,
                                     void* stream) {
  if (!c) return ME_EINVAL;
  TRY(R::frame_batch(n_frames, nullptr, 0, ERR(c)));
  int n[4];
  TRY(R::partition((int)c->devs.size(), d_ref, d_cur, width, height, stride, blk, range, cost,
                   lambda, d_out, n, ERR(c)));
  TRY(check_frames(c, n_frames, stride, height, ref_frame_stride, cur_frame_stride));
  const FrameBatch b{d_ref, ref_frame_stride, d_cur, cur_frame_stride, width, height, stride, blk,
                     n_frames};
  const bool fast = dma_fast(
      me_partition_kernel_variant(width, height, stride, blk, range) == ME_PART_KERNEL_FAST, b);
  return enqueue(c, c->devs[0], (hipStream_t)stream, "partition search", [&](hipStream_t st) {
    return launch_partition_search(b, range, lambda, fast, *d_out, st);
  });
}

me_status me_partition_search(me_ctx* c, const uint8_t* ref, const uint8_t* cur, int width,
                              int height, int stride, int blk, int range, me_cost cost,
                              uint32_t lambda, const me_part_fields* out) {
  if (!c) return ME_EINVAL;
  int n[4];
  TRY(R::partition((int)c->devs.size(), ref, cur, width, height, stride, blk, range, cost,
                   lambda, out, n, ERR(c)));
  const R::Layout L = R::layout_partition(n);
  Dev& d = c->devs[0];
  TRY(upload_planes(c, d, {ref, cur}, width, height, stride, L.total));
  auto v = [&](int k) { return rec_at<int16_t>(d, L, R::PART_MV + k); };
  auto w = [&](int k) { return rec_at<uint32_t>(d, L, R::PART_COST + k); };
  const me_part_fields D{v(0), v(1), v(2), v(3), w(0), w(1), w(2), w(3), rec_at<uint8_t>(d, L, R::PART_MODE),
                         w(4)};  // (the mode costs follow the four cost grids)
  const FrameBatch b = packed(d, d.ref, width, height, blk);
  const bool fast = dma_fast(
      me_partition_kernel_variant(width, height, width, blk, range) == ME_PART_KERNEL_FAST, b);
  TRY(enqueue(c, d, d.stream, "partition search", [&](hipStream_t st) {
    return launch_partition_search(b, range, lambda, fast, D, st);
  }));
  void* const to[10] = {out->mv_2nx2n,   out->mv_2nxn,  out->mv_nx2n,   out->mv_nxn, out->cost_2nx2n,
                        out->cost_2nxn,  out->cost_nx2n, out->cost_nxn, out->mode_cost, out->mode};
  return download_all(c, d, L, to, true);
}

me_status me_partition_leaf_field_device(me_ctx* c, int width, int height, int blk, int n_frames,
                                         const me_part_fields* d_in, int16_t* d_leaf_mv,
                                         void* stream) {
  if (!c) return ME_EINVAL;
  TRY(R::partition_leaf((int)c->devs.size(), width, height, blk, n_frames, d_in,
                        d_leaf_mv, ERR(c)));
  return enqueue(c, c->devs[0], (hipStream_t)stream, "partition leaf field", [&](hipStream_t st) {
    return launch_partition_leaf(width, height, blk, n_frames, *d_in, d_leaf_mv, st);
  });
}

// ---- rate-constrained search (me_rd.hip, me_rd_plan.cpp, me_subpel.hip) ----

me_status me_rd_search_device(me_ctx* c, const uint8_t* d_ref, size_t ref_frame_stride,
                              const uint8_t* d_cur, size_t cur_frame_stride, int width,
                              int height, int stride, int blk, int range, me_cost cost,
                              uint32_t lambda, int n_frames, const int16_t* d_pred_q,
                              int16_t* d_mv_xy, uint32_t* d_block_cost, uint32_t* d_block_dist,
                              uint8_t* d_block_bits, void* stream) {
  if (!c) return ME_EINVAL;
  TRY(R::rd((int)c->devs.size(), d_ref, d_cur, width, height, stride, blk, range, cost,
            lambda, d_mv_xy, d_block_cost, ERR(c)));
  TRY(check_frames(c, n_frames, stride, height, ref_frame_stride, cur_frame_stride));
  const FrameBatch b{d_ref, ref_frame_stride, d_cur, cur_frame_stride, width, height, stride, blk,
                     n_frames};
  const bool fast = dma_fast(
      me_rd_kernel_variant(width, height, stride, blk, range, lambda) == ME_RD_KERNEL_FAST, b);
  return enqueue(c, c->devs[0], (hipStream_t)stream, "rate-constrained search", [&](hipStream_t st) {
    return launch_rd_search(b, range, lambda, fast, d_pred_q, d_mv_xy, d_block_cost,
                                d_block_dist, d_block_bits, st);
  });
}

me_status me_rd_search(me_ctx* c, const uint8_t* ref, const uint8_t* cur, int width, int height,
                       int stride, int blk, int range, me_cost cost, uint32_t lambda,
                       const int16_t* pred_q, int16_t* mv_xy, uint32_t* block_cost,
                       uint32_t* block_dist, uint8_t* block_bits) {
  if (!c) return ME_EINVAL;
  TRY(R::rd((int)c->devs.size(), ref, cur, width, height, stride, blk, range, cost,
            lambda, mv_xy, block_cost, ERR(c)));
  const R::Layout L = R::layout_rd((size_t)me_num_blocks(width, height, blk));
  Dev& d = c->devs[0];
  TRY(upload_planes(c, d, {ref, cur}, width, height, stride, L.total));
  int16_t* d_pred = pred_q ? rec_at<int16_t>(d, L, R::RD_PRED) : nullptr;  // (null: zeros)
  if (d_pred) TRY(upload(c, d, d_pred, pred_q, L.bytes[R::RD_PRED]));
  const FrameBatch b = packed(d, d.ref, width, height, blk);
  const bool fast = dma_fast(
      me_rd_kernel_variant(width, height, width, blk, range, lambda) == ME_RD_KERNEL_FAST, b);
  TRY(enqueue(c, d, d.stream, "rate-constrained search", [&](hipStream_t st) {
    return launch_rd_search(b, range, lambda, fast, d_pred, rec_at<int16_t>(d, L, R::RD_MV),
                                     rec_at<uint32_t>(d, L, R::RD_COST),
                                     rec_at<uint32_t>(d, L, R::RD_DIST),
                                     rec_at<uint8_t>(d, L, R::RD_BITS), st);
  }));
  void* const out[5] = {nullptr, mv_xy, block_cost, block_dist, block_bits};
  return download_all(c, d, L, out, true);
}

me_status me_refine_qpel_rd_device(me_ctx* c, const uint8_t* d_ref, size_t ref_frame_stride,
                                   const uint8_t* d_cur, size_t cur_frame_stride, int width,
                                   int height, int stride, int blk, me_cost cost, uint32_t lambda,
                                   int n_frames, const int16_t* d_pred_q, const int16_t* d_mv_xy,
                                   int16_t* d_mv_q, uint32_t* d_block_cost,
                                   uint32_t* d_block_dist, void* stream) {
  if (!c) return ME_EINVAL;
  TRY(check_refine(c, d_ref, d_cur, width, height, stride, blk, 0, cost, d_mv_xy, d_mv_q));
  TRY(R::rd_ctx((int)c->devs.size(), lambda, "rate-constrained refinement", ERR(c)));
  TRY(check_frames(c, n_frames, stride, height, ref_frame_stride, cur_frame_stride));
  const FrameBatch b{d_ref, ref_frame_stride, d_cur, cur_frame_stride, width, height, stride, blk,
                     n_frames};
  return enqueue(c, c->devs[0], (hipStream_t)stream, "rate-constrained refinement", [&](hipStream_t st) {
    return launch_qpel_refine_rd(b, cost, lambda, d_pred_q, d_mv_xy, d_mv_q, d_block_cost,
                                     d_block_dist, st);
  });
}

me_status me_refine_qpel_rd(me_ctx* c, const uint8_t* ref, const uint8_t* cur, int width,
                            int height, int stride, int blk, me_cost cost, uint32_t lambda,
                            const int16_t* pred_q, const int16_t* mv_xy, int16_t* mv_q,
                            uint32_t* block_cost, uint32_t* block_dist) {
  TRY(check_refine(c, ref, cur, width, height, stride, blk, 0, cost, mv_xy, mv_q));
  TRY(R::rd_ctx((int)c->devs.size(), lambda, "rate-constrained refinement", ERR(c)));
  const size_t nb = (size_t)me_num_blocks(width, height, blk);
  TRY(R::vectors(&mv_xy, 1, nb, ME_QPEL_MAX_MV, "ME_QPEL_MAX_MV", ERR(c)));
  const R::Layout L = R::layout_rd(nb);
  Dev& d = c->devs[0];
  TRY(upload_planes(c, d, {ref, cur}, width, height, stride, L.total));
  int16_t* dmv = rec_at<int16_t>(d, L, R::RD_MV);
  int16_t* d_pred = pred_q ? rec_at<int16_t>(d, L, R::RD_PRED) : nullptr;  // (null: zeros)
  if (d_pred) TRY(upload(c, d, d_pred, pred_q, L.bytes[R::RD_PRED]));
  TRY(upload(c, d, dmv, mv_xy, L.bytes[R::RD_MV]));
  const FrameBatch b = packed(d, d.ref, width, height, blk);
  TRY(enqueue(c, d, d.stream, "rate-constrained refinement", [&](hipStream_t st) {
    return launch_qpel_refine_rd(b, cost, lambda, d_pred, dmv, dmv,
                                          rec_at<uint32_t>(d, L, R::RD_COST),
                                          rec_at<uint32_t>(d, L, R::RD_DIST), st);
  }));
  void* const out[5] = {nullptr, mv_q, block_cost, block_dist, nullptr};
  return download_all(c, d, L, out, true);
}

me_status me_full_search_rd_qpel(me_ctx* c, const uint8_t* ref, const uint8_t* cur, int width,
                                 int height, int stride, int blk, int range, me_cost cost,
                                 uint32_t lambda, const int16_t* pred_q, int16_t* mv_q,
                                 uint32_t* block_cost) {
  if (!c) return ME_EINVAL;
  // (block_cost is optional here: the search's own cost array is d.rec's)
  // (SATD: the search runs at SAD, the refinement at SATD)
  TRY(R::rd((int)c->devs.size(), ref, cur, width, height, stride, blk, range,
            R::search_cost(cost), lambda, mv_q, mv_q, ERR(c)));
  const R::Layout L = R::layout_rd((size_t)me_num_blocks(width, height, blk));
  Dev& d = c->devs[0];
  TRY(upload_planes(c, d, {ref, cur}, width, height, stride, L.total));
  int16_t* dmv = rec_at<int16_t>(d, L, R::RD_MV);
  uint32_t* dcost = rec_at<uint32_t>(d, L, R::RD_COST);
  int16_t* d_pred = pred_q ? rec_at<int16_t>(d, L, R::RD_PRED) : nullptr;  // (null: zeros)
  if (d_pred) TRY(upload(c, d, d_pred, pred_q, L.bytes[R::RD_PRED]));
  const FrameBatch b = packed(d, d.ref, width, height, blk);
  const bool fast = dma_fast(
      me_rd_kernel_variant(width, height, width, blk, range, lambda) == ME_RD_KERNEL_FAST, b);
  TRY(enqueue(c, d, d.stream, "rate-constrained search", [&](hipStream_t st) {
    return launch_rd_search(b, range, lambda, fast, d_pred, dmv, dcost, nullptr, nullptr,
                                     st);
  }));
  // the searched vectors stay inside the window (|m| <= ME_RD_MAX_RANGE): refine in place
  TRY(enqueue(c, d, d.stream, "rate-constrained refinement", [&](hipStream_t st) {
    return launch_qpel_refine_rd(b, cost, lambda, d_pred, dmv, dmv, dcost, nullptr,
                                          st);
  }));
  void* const out[5] = {nullptr, mv_q, block_cost, nullptr, nullptr};
  return download_all(c, d, L, out, true);
}

// ---- rate-constrained partition search (me_partition.hip) ----

me_status me_partition_rd_search_device(me_ctx* c, const uint8_t* d_ref, size_t ref_frame_stride,
                                        const uint8_t* d_cur, size_t cur_frame_stride, int width,
                                        int height, int stride, int blk, int range, me_cost cost,
                                        uint32_t lambda, int n_frames, const int16_t* d_pred_q,
                                        const me_part_rd_fields* d_out, void* stream) {
  if (!c) return ME_EINVAL;
  TRY(R::frame_batch(n_frames, nullptr, 0, ERR(c)));
  int n[4];
  TRY(R::partition_rd((int)c->devs.size(), d_ref, d_cur, width, height, stride, blk, range,
                      cost, lambda, d_out, n, ERR(c)));
  TRY(check_frames(c, n_frames, stride, height, ref_frame_stride, cur_frame_stride));
  const FrameBatch b{d_ref, ref_frame_stride, d_cur, cur_frame_stride, width, height, stride, blk,
                     n_frames};
  const bool fast = dma_fast(me_partition_rd_kernel_variant(width, height, stride, blk, range,
                                                            lambda) == ME_PART_KERNEL_FAST, b);
  return enqueue(c, c->devs[0], (hipStream_t)stream, "rate-constrained partition search", [&](hipStream_t st) {
    return launch_partition_rd_search(b, range, lambda, fast, d_pred_q, *d_out, st);
  });
}

me_status me_partition_rd_search(me_ctx* c, const uint8_t* ref, const uint8_t* cur, int width,
                                 int height, int stride, int blk, int range, me_cost cost,
                                 uint32_t lambda, const int16_t* pred_q,
                                 const me_part_rd_fields* out) {
  if (!c) return ME_EINVAL;
  int n[4];
  TRY(R::partition_rd((int)c->devs.size(), ref, cur, width, height, stride, blk, range,
                      cost, lambda, out, n, ERR(c)));
  const R::Layout L = R::layout_partition_rd(n);
  Dev& d = c->devs[0];
  TRY(upload_planes(c, d, {ref, cur}, width, height, stride, L.total));
  int16_t* d_pred = pred_q ? rec_at<int16_t>(d, L, R::PRD_PRED) : nullptr;  // (null: zeros)
  if (d_pred) TRY(upload(c, d, d_pred, pred_q, L.bytes[R::PRD_PRED]));
  auto v = [&](int k) { return rec_at<int16_t>(d, L, R::PRD_MV + k); };
  auto w = [&](int k) { return rec_at<uint32_t>(d, L, k); };
  auto u = [&](int k) { return rec_at<uint8_t>(d, L, k); };
  const int C = R::PRD_COST, Di = R::PRD_DIST, Bi = R::PRD_BITS;
  const me_part_rd_fields D{{v(0), v(1), v(2), v(3), w(C), w(C + 1), w(C + 2), w(C + 3), u(R::PRD_MODE),
                             w(R::PRD_MODE_COST)},
                            w(Di), w(Di + 1), w(Di + 2), w(Di + 3), u(Bi), u(Bi + 1), u(Bi + 2), u(Bi + 3)};
  const FrameBatch b = packed(d, d.ref, width, height, blk);
  const bool fast = dma_fast(me_partition_rd_kernel_variant(width, height, width, blk, range,
                                                            lambda) == ME_PART_KERNEL_FAST, b);
  TRY(enqueue(c, d, d.stream, "rate-constrained partition search", [&](hipStream_t st) {
    return launch_partition_rd_search(b, range, lambda, fast, d_pred, D, st);
  }));
  const me_part_fields& f = out->f;
  void* const to[19] = {nullptr,         f.mv_2nx2n,      f.mv_2nxn,       f.mv_nx2n,
                        f.mv_nxn,        f.cost_2nx2n,    f.cost_2nxn,     f.cost_nx2n,
                        f.cost_nxn,      out->dist_2nx2n, out->dist_2nxn,  out->dist_nx2n,
                        out->dist_nxn,   f.mode_cost,     out->bits_2nx2n, out->bits_2nxn,
                        out->bits_nx2n,  out->bits_nxn,   f.mode};
  return download_all(c, d, L, to, true);
}

// ---- partition-wise quarter-pel refinement (me_subpel.hip) ----

me_status me_partition_refine_qpel_device(me_ctx* c, const uint8_t* d_ref, size_t ref_frame_stride,
                                          const uint8_t* d_cur, size_t cur_frame_stride, int width,
                                          int height, int stride, int blk, me_cost cost,
                                          uint32_t lambda, int n_frames, const int16_t* d_pred_q,
                                          const me_part_fields* d_in,
                                          const me_part_rd_fields* d_out, void* stream) {
  if (!c) return ME_EINVAL;
  TRY(R::frame_batch(n_frames, nullptr, 0, ERR(c)));
  int n[4];
  TRY(R::partition_qpel((int)c->devs.size(), d_ref, d_cur, width, height, stride, blk, cost,
                        lambda, d_in, d_out, n, ERR(c)));
  TRY(check_frames(c, n_frames, stride, height, ref_frame_stride, cur_frame_stride));
  const FrameBatch b{d_ref, ref_frame_stride, d_cur, cur_frame_stride, width, height, stride, blk,
                     n_frames};
  return enqueue(c, c->devs[0], (hipStream_t)stream, "partition-wise refinement", [&](hipStream_t st) {
    return launch_partition_qpel(b, cost, lambda, d_pred_q, *d_in, *d_out, st);
  });
}

me_status me_partition_refine_qpel(me_ctx* c, const uint8_t* ref, const uint8_t* cur, int width,
                                   int height, int stride, int blk, me_cost cost, uint32_t lambda,
                                   const int16_t* pred_q, const me_part_fields* in,
                                   const me_part_rd_fields* out) {
  if (!c) return ME_EINVAL;
  int n[4];
  TRY(R::partition_qpel((int)c->devs.size(), ref, cur, width, height, stride, blk, cost, lambda,
                        in, out, n, ERR(c)));
  const int16_t* const grids[4] = {in->mv_2nx2n, in->mv_2nxn, in->mv_nx2n, in->mv_nxn};
  for (int g = 0; g < 4; g++)
    TRY(R::vectors(&grids[g], 1, (size_t)n[g], ME_QPEL_MAX_MV, "ME_QPEL_MAX_MV", ERR(c)));
  const R::Layout L = R::layout_partition_rd(n);
  Dev& d = c->devs[0];
  TRY(upload_planes(c, d, {ref, cur}, width, height, stride, L.total));
  int16_t* d_pred = pred_q ? rec_at<int16_t>(d, L, R::PRD_PRED) : nullptr;  // (null: zeros)
  if (d_pred) TRY(upload(c, d, d_pred, pred_q, L.bytes[R::PRD_PRED]));
  const me_part_rd_fields D = part_rd_records(d, L);
  // the integer grids go where the refined ones come out: refined in place
  int16_t* const dmv[4] = {D.f.mv_2nx2n, D.f.mv_2nxn, D.f.mv_nx2n, D.f.mv_nxn};
  for (int g = 0; g < 4; g++) TRY(upload(c, d, dmv[g], grids[g], L.bytes[R::PRD_MV + g]));
  const FrameBatch b = packed(d, d.ref, width, height, blk);
  TRY(enqueue(c, d, d.stream, "partition-wise refinement", [&](hipStream_t st) {
    return launch_partition_qpel(b, cost, lambda, d_pred, D.f, D, st);
  }));
  void* to[19];
  part_rd_host(out, to);
  return download_all(c, d, L, to, true);
}

me_status me_partition_search_qpel(me_ctx* c, const uint8_t* ref, const uint8_t* cur, int width,
                                   int height, int stride, int blk, int range, me_cost cost,
                                   uint32_t lambda, const int16_t* pred_q,
                                   const me_part_rd_fields* out, int16_t* leaf_mv_q) {
  if (!c) return ME_EINVAL;
  int n[4];
  // (SATD: the search runs at SAD, the refinement at SATD)
  TRY(R::partition_rd((int)c->devs.size(), ref, cur, width, height, stride, blk, range,
                      R::search_cost(cost), lambda, out, n, ERR(c)));
  const R::Layout L = R::layout_partition_rd(n);
  const size_t leaf_bytes = 4 * (size_t)n[3];  // after the records (L.total is 8-aligned)
  Dev& d = c->devs[0];
  TRY(upload_planes(c, d, {ref, cur}, width, height, stride, L.total + leaf_bytes));
  int16_t* d_pred = pred_q ? rec_at<int16_t>(d, L, R::PRD_PRED) : nullptr;  // (null: zeros)
  if (d_pred) TRY(upload(c, d, d_pred, pred_q, L.bytes[R::PRD_PRED]));
  const me_part_rd_fields D = part_rd_records(d, L);
  int16_t* d_leaf = reinterpret_cast<int16_t*>(d.rec + L.total);
  const FrameBatch b = packed(d, d.ref, width, height, blk);
  const bool fast = dma_fast(me_partition_rd_kernel_variant(width, height, width, blk, range,
                                                            lambda) == ME_PART_KERNEL_FAST, b);
  TRY(enqueue(c, d, d.stream, "rate-constrained partition search", [&](hipStream_t st) {
    return launch_partition_rd_search(b, range, lambda, fast, d_pred, D, st);
  }));
  // the searched vectors stay inside the window (|m| <= ME_PART_MAX_RANGE): refine in place
  TRY(enqueue(c, d, d.stream, "partition-wise refinement", [&](hipStream_t st) {
    return launch_partition_qpel(b, cost, lambda, d_pred, D.f, D, st);
  }));
  if (leaf_mv_q) {
    TRY(enqueue(c, d, d.stream, "partition leaf field", [&](hipStream_t st) {
      return launch_partition_leaf(width, height, blk, 1, D.f, d_leaf, st);
    }));
    TRY(download(c, d, leaf_mv_q, d_leaf, leaf_bytes));
  }
  void* to[19];
  part_rd_host(out, to);
  return download_all(c, d, L, to, true);
}

}  // extern "C"

#undef TRY
#undef ERR
