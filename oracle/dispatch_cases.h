// dispatch_cases.h -- the case lines of tests/golden/plans/dispatch.json (TEST
// INFRASTRUCTURE; read by oracle/dispatch_dump.cc and oracle/san_main.cc).
// A record starts with
//   {"name":"..","width":..,"height":..,"stride":..,"blk":..,"range":..,"cost":..,
//    "path":..,"scratch":..,"jobs":[[r0,r1,ref_row0,cur_row0,ref_mod,cur_mod],..]
// path: the kernel path code (me_tuning.h).  scratch: bytes of context scratch,
// or -1 for what attach_scratch sizes (the largest job's single-search need
// and, for equal jobs, the batch's).  ref_mod / cur_mod: the job's plane
// addresses modulo 256 (fabricated pointers: the dispatcher reads alignment
// only).
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "me_dispatch.h"
#include "me_tuning.h"

struct DispatchCase {
  char name[64];
  me::SearchShape s;  // merge_tiles and scratch_bytes as the context lends them
  int path;
  long long scratch;  // as written in the record
  std::vector<me::SearchJob> jobs;
  std::vector<int> mods;  // ref_mod, cur_mod per job
};

// False: the line is no case record.
inline bool parse_dispatch_case(const char* line, int cus, const me::Tuning& tu, DispatchCase* c) {
  me::SearchShape& s = c->s;
  s = me::SearchShape{};
  int off = 0;
  if (sscanf(line,
             " {\"name\":\"%63[^\"]\",\"width\":%d,\"height\":%d,\"stride\":%d,\"blk\":%d,\"range\":%d,"
             "\"cost\":%d,\"path\":%d,\"scratch\":%lld,\"jobs\":[%n",
             c->name, &s.width, &s.height, &s.stride, &s.blk, &s.range, &s.cost, &c->path, &c->scratch,
             &off) != 9 || !off)
    return false;
  c->jobs.clear();
  c->mods.clear();
  for (const char* p = line + off; *p == '[' || *p == ',';) {
    if (*p == ',') p++;
    int r0, r1, rr, cr, rm, cm, used = 0;
    if (sscanf(p, "[%d,%d,%d,%d,%d,%d]%n", &r0, &r1, &rr, &cr, &rm, &cm, &used) != 6 || !used) return false;
    p += used;
    const uintptr_t j = c->jobs.size();
    c->jobs.push_back({(const uint8_t*)(0x10000000u + (j << 24) + (uintptr_t)rm), rr,
                       (const uint8_t*)(0x50000000u + (j << 24) + (uintptr_t)cm), cr, r0, r1, nullptr,
                       nullptr});
    c->mods.push_back(rm);
    c->mods.push_back(cm);
  }
  const int nj = (int)c->jobs.size(), nbx = (s.width + s.blk - 1) / s.blk;
  if (nj < 1) return false;
  // the context's buffers, as attach_scratch sizes them for this call
  bool same = true;
  size_t need = 0;
  for (int j = 0; j < nj; j++) {
    const me::SearchJob& J = c->jobs[j];
    me::MfmaShape ms{s.width, s.height, s.stride, s.blk, s.range, s.cost, J.r0, J.r1, nbx,
                     me::align_class(s.stride, J.ref, J.cur), ~(size_t)0};
    if (J.r1 > J.r0 && s.cost == me::COST_SSD && me::mfma_merge_tiles(ms) > s.merge_tiles)
      s.merge_tiles = me::mfma_merge_tiles(ms);
    me::MfmaGeom g;
    if (me::plan_mfma_ssd(ms, c->path, cus, tu, &g) && g.scratch_bytes > need) need = g.scratch_bytes;
    same = same && J.r0 == c->jobs[0].r0 && J.r1 == c->jobs[0].r1 && J.ref_row0 == c->jobs[0].ref_row0 &&
           J.cur_row0 == c->jobs[0].cur_row0;
  }
  if (same && nj > 1) {
    const me::SearchJob& J = c->jobs[0];
    const me::MfmaShape ms{s.width, s.height, s.stride, s.blk, s.range, s.cost, J.r0, J.r1, nbx,
                           me::align_class(s.stride, J.ref, J.cur), s.merge_tiles};
    me::MfmaBatch b;
    me::plan_mfma_batch(ms, nj, me::MFMA_SCRATCH_UNLIMITED, c->path, cus, tu, &b);
    if (b.need > need) need = b.need;
  }
  s.scratch_bytes = c->scratch >= 0 ? (size_t)c->scratch : need;
  return true;
}

// The whole list of a case as launch_jobs walks it: the batch's launches
// through a window of `cap` per call, else job by job.
inline std::vector<me::Launch> dispatch_all(const DispatchCase& c, int cus, const me::Tuning& tu, int cap) {
  const int n = (int)c.jobs.size();
  std::vector<me::Launch> win((size_t)(cap > me::DISPATCH_JOB_MAX ? cap : me::DISPATCH_JOB_MAX)), list;
  for (int skip = 0;; skip += cap) {
    const int total = me::dispatch_batch(c.s, c.jobs.data(), n, c.path, cus, tu, skip, win.data(), cap);
    if (total < 0) break;
    for (int i = 0; i < cap && skip + i < total; i++) list.push_back(win[(size_t)i]);
    if (skip + cap >= total) return list;
  }
  for (int j = 0; j < n; j++) {
    const int k = me::dispatch_job(c.s, c.jobs.data(), j, c.path, cus, tu, win.data());
    list.insert(list.end(), win.begin(), win.begin() + k);
  }
  return list;
}
