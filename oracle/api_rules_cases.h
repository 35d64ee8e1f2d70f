// api_rules_cases.h -- the cases of tests/golden/api_args.json read back line
// by line, and each entry point's rule sequence over csrc/me_api_rules.cpp alone
// (TEST INFRASTRUCTURE; oracle/api_rules_dump.cc, oracle/san_main.cc).  The
// sequences restate the order in which me_api.hip and me_api_stages.hip apply
// the rules; tests/test_gpu_api_rules.py holds the library itself to the same
// table.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "me.h"
#include "me_api_rules.h"
#include "me_geom.h"

struct ApiCase {
  std::string name, fn, null, message;
  int width = 48, height = 32, stride = 48, blk = 16, range = 4, cost = 1, n_frames = 1, refine = 1;
  int r0 = 0, r1 = 2, ref_row0 = 0, cur_row0 = 0, num_blks = 6, n_jobs = 2, ndev = 1;
  long long lambda = 4, fs_ref = 48 * 32, fs_cur = 48 * 32, fs_ref1 = 48 * 32;
  int elem = -1, elem_val = 0, elem_arr = 0, mode_idx = -1, mode_val = 0, pix_idx = -1, pix_val = 0;
  int status = 0, loose = 0;
  bool is_null(const char* p) const { return (" " + null + " ").find(std::string(" ") + p + " ") != std::string::npos; }
};

inline bool api_key(const char* line, const char* key, const char** at) {
  const std::string k = std::string("\"") + key + "\":";
  const char* p = strstr(line, k.c_str());
  if (p) *at = p + k.size();
  return p != nullptr;
}
inline void api_int(const char* line, const char* key, long long* v) {
  const char* p;
  if (api_key(line, key, &p)) sscanf(p, "%lld", v);
}
inline void api_int(const char* line, const char* key, int* v) {
  long long w = *v;
  api_int(line, key, &w);
  *v = (int)w;
}
inline void api_str(const char* line, const char* key, std::string* v) {
  const char* p;
  if (!api_key(line, key, &p) || *p != '"') return;
  const char* e = strchr(p + 1, '"');  // (no message holds a quote)
  if (e) v->assign(p + 1, e);
}

inline bool parse_api_case(const char* line, ApiCase* c) {
  *c = ApiCase{};
  if (strncmp(line, "{\"name\":", 8)) return false;
  api_str(line, "name", &c->name), api_str(line, "fn", &c->fn), api_str(line, "null", &c->null);
  api_str(line, "message", &c->message);
#define API_INT(f) api_int(line, #f, &c->f)
  API_INT(width), API_INT(height), API_INT(stride), API_INT(blk), API_INT(range), API_INT(cost);
  API_INT(n_frames), API_INT(refine), API_INT(r0), API_INT(r1), API_INT(ref_row0), API_INT(cur_row0);
  API_INT(num_blks), API_INT(n_jobs), API_INT(ndev), API_INT(lambda), API_INT(fs_ref), API_INT(fs_cur);
  API_INT(fs_ref1), API_INT(elem), API_INT(elem_val), API_INT(elem_arr), API_INT(mode_idx);
  API_INT(mode_val), API_INT(pix_idx), API_INT(pix_val), API_INT(status), API_INT(loose);
#undef API_INT
  if (c->fn.empty()) c->fn = c->name.substr(0, c->name.find(':'));  // (the table leaves it out)
  return !c->fn.empty();
}

// The status and message entry point c.fn gives c's arguments on a context of
// ndev devices.  Returns -1 for an entry point it does not know.
inline int run_api_case(const ApiCase& c, int ndev, char* err, size_t n) {
  namespace R = me::rules;
  static const char buf = 0;  // what every non-null pointer points at
  auto P = [&](const char* name) { return c.is_null(name) ? nullptr : (const void*)&buf; };
  const std::string& f = c.fn;
  const int W = c.width, H = c.height, St = c.stride, B = c.blk, S = c.range;
  const uint32_t lambda = (uint32_t)c.lambda;
  const size_t fs_ref = (size_t)c.fs_ref, fs_cur = (size_t)c.fs_cur, fs_ref1 = (size_t)c.fs_ref1;
  const me_cost search_cost = R::search_cost((me_cost)c.cost);
  me_status s = ME_OK;
  err[0] = 0;
#define RULE(x) \
  if ((s = (x)) != ME_OK) return s
  auto frames = [&](int np, const size_t* fs, const unsigned long long* bytes) {
    R::FramePlane p[2];
    for (int k = 0; k < np; k++) p[k] = R::FramePlane{fs[k], bytes[k]};
    return R::frame_batch(c.n_frames, p, np, err, n);
  };
  const unsigned long long fb = (unsigned long long)St * H, fb2[2] = {fb, fb};
  const size_t fs2[2] = {fs_ref, fs_cur};
  const size_t nb = W > 0 && H > 0 && B > 0 ? (size_t)me_num_blocks(W, H, B) : 0;
  // the arrays whose elements a rule reads (sized only once the geometry passed)
  auto field = [&](int arr) {
    std::vector<int16_t> v(2 * nb, 0);
    if (c.elem >= 0 && c.elem_arr == arr) v[c.elem] = (int16_t)c.elem_val;
    return v;
  };
  me_part_fields pf{};
  me_part_rd_fields prf{};
  {
    int16_t* const mv = (int16_t*)&buf;
    pf.mv_2nx2n = c.is_null("f.mv_2nx2n") ? nullptr : mv;
    pf.mv_2nxn = c.is_null("f.mv_2nxn") ? nullptr : mv;
    pf.mv_nx2n = c.is_null("f.mv_nx2n") ? nullptr : mv;
    pf.mv_nxn = c.is_null("f.mv_nxn") ? nullptr : mv;
    pf.mode = c.is_null("f.mode") ? nullptr : (uint8_t*)&buf;
    prf.f = pf;
  }
  const me_part_fields* fields = c.is_null("fields") ? nullptr : &pf;
  const me_part_rd_fields* rd_fields = c.is_null("fields") ? nullptr : &prf;
  int counts[4];
  const int nby = B > 0 ? (int)(((long long)H + B - 1) / B) : 0;

  if (f == "me_full_search")
    return R::args(P("ref"), P("cur"), W, H, St, B, S, c.cost, P("mv"), err, n);
  if (f == "me_full_search_device" || f == "me_full_search_stripe_device") {
    const bool whole = f == "me_full_search_device";
    RULE(R::args(P("ref"), P("cur"), W, H, St, B, S, c.cost, P("mv"), err, n));
    return R::stripe(nby, B, S, whole ? 0 : c.r0, whole ? nby : c.r1, whole ? 0 : c.ref_row0,
                     whole ? 0 : c.cur_row0, -1, err, n);
  }
  if (f == "me_search_stripes_device") {
    if (!P("jobs") || c.n_jobs < 0) return R::fail(err, n, ME_EINVAL, "job list");
    for (int j = 0; j < c.n_jobs; j++) {  // the case's violation is the last job's
      const bool last = j == c.n_jobs - 1;
      RULE(R::args(last ? P("job.ref") : &buf, last ? P("job.cur") : &buf, W, H, St, B, S, c.cost,
                   last ? P("job.mv") : &buf, err, n));
      RULE(R::stripe(nby, B, S, last ? c.r0 : 0, last ? c.r1 : 2, last ? c.ref_row0 : 0,
                     last ? c.cur_row0 : 0, j, err, n));
    }
    return ME_OK;
  }
  if (f == "me_full_search_batch_device") {
    RULE(R::frame_batch(c.n_frames, nullptr, 0, err, n));
    RULE(R::args(P("ref"), P("cur"), W, H, St, B, S, c.cost, P("mv"), err, n));
    RULE(R::stripe(nby, B, S, c.r0, c.r1, 0, 0, -1, err, n));
    // (first rows far outside int's middle overflow me_geom.h's row count: kept apart)
    auto mid = [](int v) { return v < -(1 << 30) ? -(1 << 30) : v > (1 << 30) ? 1 << 30 : v; };
    const unsigned long long bytes[2] = {me::ref_resident_bytes(c.r1, B, S, H, mid(c.ref_row0), St, W),
                                         me::cur_resident_bytes(c.r1, B, H, mid(c.cur_row0), St, W)};
    RULE(frames(2, fs2, bytes));
    // (then frame by frame as a job list: equal jobs, so job 0 reports)
    return R::stripe(nby, B, S, c.r0, c.r1, c.ref_row0, c.cur_row0, 0, err, n);
  }
  if (f == "me_find_best_blocks") {
    RULE(R::args(P("ref"), P("cur"), W, H, W, B, S, ME_COST_SSD, P("blks"), err, n));
    if (c.num_blks != (int)nb) return R::fail(err, n, ME_EINVAL, "num_blks %d != %d", c.num_blks, (int)nb);
    std::vector<int> ref((size_t)W * H, 0), cur((size_t)W * H, 0);
    if (c.pix_idx >= 0) cur[c.pix_idx] = c.pix_val;
    std::vector<uint8_t> r8(ref.size()), c8(ref.size());
    return R::pixels(ref.data(), cur.data(), ref.size(), r8.data(), c8.data(), err, n);
  }
  if (f == "me_motion_compensate" || f == "me_motion_compensate_qpel" ||
      f == "me_compensate_planes" || f == "me_compensate_planes_qpel") {
    const bool planes = f.find("planes") != std::string::npos;
    if (planes && !P("cur")) return R::fail(err, n, ME_EINVAL, "null cur");
    RULE(R::args(P("ref"), planes ? P("cur") : P("ref"), W, H, W, B, 0, ME_COST_SSD, P("mv"), err, n));
    return P("out") ? ME_OK : R::fail(err, n, ME_EINVAL, "null output");
  }
  if (f == "me_motion_compensate_bipred" || f == "me_compensate_planes_bipred") {
    const bool planes = f.find("planes") != std::string::npos;
    if (planes && !P("cur")) return R::fail(err, n, ME_EINVAL, "null cur");
    RULE(R::args(P("ref"), planes ? P("cur") : P("ref"), W, H, W, B, 0, ME_COST_SSD, P("mv"), err, n));
    if (!P("ref1") || !P("q1") || !P("mode") || !P("out"))
      return R::fail(err, n, ME_EINVAL, "null bi-prediction plane, field, mode or output pointer");
    std::vector<uint8_t> mode(nb, 0);
    if (c.mode_idx >= 0) mode[c.mode_idx] = (uint8_t)c.mode_val;
    return R::pred_modes(mode.data(), nb, err, n);
  }
  const bool rd_refine = f == "me_refine_qpel_rd_device" || f == "me_refine_qpel_rd";
  if (f == "me_refine_qpel_device" || f == "me_refine_qpel" || f == "me_full_search_qpel" || rd_refine) {
    const bool full = f == "me_full_search_qpel", device = f.find("_device") != std::string::npos;
    if (f == "me_refine_qpel_device") RULE(R::frame_batch(c.n_frames, nullptr, 0, err, n));
    RULE(R::args(P("ref"), P("cur"), W, H, St, B, full ? S : 0, search_cost, full ? P("mv_q") : P("mv"),
                 err, n));
    RULE(R::qpel(c.cost, P("mv_q"), err, n));
    if (full) return R::one_device(ndev, "quarter-pel search", err, n);
    if (rd_refine) RULE(R::rd_ctx(ndev, lambda, "rate-constrained refinement", err, n));
    if (device) return frames(2, fs2, fb2);
    const std::vector<int16_t> mv = field(0);
    const int16_t* const fields1[1] = {mv.data()};
    return R::vectors(fields1, 1, nb, ME_QPEL_MAX_MV, "ME_QPEL_MAX_MV", err, n);
  }
  if (f == "me_bipred_device" || f == "me_bipred" || f == "me_full_search_bipred") {
    const bool full = f == "me_full_search_bipred";
    if (f == "me_bipred_device") RULE(R::frame_batch(c.n_frames, nullptr, 0, err, n));
    RULE(R::args(P("ref"), P("cur"), W, H, St, B, full ? S : 0, search_cost, full ? P("out0") : P("mv"),
                 err, n));
    RULE(R::bipred(c.cost, P("ref1"), full ? P("out1") : P("q1"), P("out0"), P("out1"), P("mode"),
                   err, n));
    if (full) return R::one_device(ndev, "bi-predictive search", err, n);
    if (f == "me_bipred_device") {
      for (size_t v : {fs_ref, fs_ref1, fs_cur}) RULE(frames(1, &v, &fb));
      return ME_OK;
    }
    const std::vector<int16_t> q0 = field(0), q1 = field(1);
    const int16_t* const q[2] = {q0.data(), q1.data()};
    return R::vectors(q, 2, nb, ME_BIPRED_MAX_Q, "ME_BIPRED_MAX_Q", err, n);
  }
  if (f == "me_partition_search_device" || f == "me_partition_search") {
    const bool device = f == "me_partition_search_device";
    if (device) RULE(R::frame_batch(c.n_frames, nullptr, 0, err, n));
    RULE(R::partition(ndev, P("ref"), P("cur"), W, H, St, B, S, c.cost, lambda, fields, counts, err, n));
    return device ? frames(2, fs2, fb2) : ME_OK;
  }
  if (f == "me_partition_rd_search_device" || f == "me_partition_rd_search") {
    const bool device = f == "me_partition_rd_search_device";
    if (device) RULE(R::frame_batch(c.n_frames, nullptr, 0, err, n));
    RULE(R::partition_rd(ndev, P("ref"), P("cur"), W, H, St, B, S, c.cost, lambda, rd_fields, counts,
                         err, n));
    return device ? frames(2, fs2, fb2) : ME_OK;
  }
  if (f == "me_partition_leaf_field_device")
    return R::partition_leaf(ndev, W, H, B, c.n_frames, fields, P("leaf"), err, n);
  if (f == "me_rd_search_device" || f == "me_rd_search") {
    RULE(R::rd(ndev, P("ref"), P("cur"), W, H, St, B, S, c.cost, lambda, P("mv"), P("cost_out"), err, n));
    return f == "me_rd_search_device" ? frames(2, fs2, fb2) : ME_OK;
  }
  if (f == "me_full_search_rd_qpel")
    return R::rd(ndev, P("ref"), P("cur"), W, H, St, B, S, search_cost, lambda, P("mv_q"), P("mv_q"),
                 err, n);
#undef RULE
  return -1;
}
