// mfma_plan_dump.cc -- print the matrix-core SSD planners' plans for a table of
// shapes (TEST INFRASTRUCTURE; built by `make -C oracle mfma_plan_dump` from
// me_mfma_plan.cpp alone, no GPU and no libme_hip).
//
//   mfma_plan_dump tests/golden/plans/mfma_plans.json
//
// The fixture holds one record per line; each starts with the rule it is
// there for and the shape
//   {"note":"..","width":..,"height":..,"stride":..,"blk":..,"range":..,
//    "cost":..,"r0":..,"r1":..,"nbx":..,"align":..,"merge":..,"path":..
// (block rows [r0, r1); merge: tiles the merge buffers cover; path: the
// kernel path code) followed by what the commit before the planners moved out
// of me_mfma.hip / me_band.hip planned.  For every such line this prints the
// record the planners give now (256 CUs, default Tuning), in the same form:
// the single-search plan (every integer field of MfmaGeom), its scratch, the
// merge tiles, for 16x16 with S <= 64 plan_bw applied to that plan for 1, 2,
// 8, 16 and 32 jobs, and the batch scratch of 2, 8, 16, 32 and 33 jobs.
// tests/test_mfma_plan.py requires the two to be equal field by field.
#include <stdio.h>

#include "me_mfma_geom.h"
#include "me_tuning.h"

static const int CUS = 256;

static void print_bw(const me::MfmaGeom& g) {
  printf("\"lds\":%d,\"bw\":%d,\"bw_wpc\":%d,\"bw_ns\":%d,\"bw_nsw\":%d,\"bw_pw\":%d,\"bw_cols\":%d,"
         "\"bw_strips\":%d,\"bw_seg_rows\":%d,\"bw_segs\":%d,\"bw_xt\":%d,\"bw_cx\":%d,\"bw_lp\":%d,"
         "\"bw_pp\":%d,\"bw_abl\":%d,\"bw_hb\":%d",
         g.lds, g.bw, g.bw_wpc, g.bw_ns, g.bw_nsw, g.bw_pw, g.bw_cols, g.bw_strips, g.bw_seg_rows,
         g.bw_segs, g.bw_xt, g.bw_cx, g.bw_lp, g.bw_pp, g.bw_abl, g.bw_hb);
}

static void print_geom(const me::MfmaGeom& g) {
  printf("\"row0\":%d,\"nrows\":%d,\"nbx\":%d,\"tiles_x\":%d,\"tiles_y\":%d,\"ngx\":%d,\"ngxw\":%d,"
         "\"km\":%d,\"bm\":%d,\"bm_wpr\":%d,\"bm_lp\":%d,\"bmv\":%d,\"bmv_r\":%d,\"hb\":%d,"
         "\"hb_row\":%d,\"ya0\":%d,\"rp_rows\":%d,\"rows_alloc\":%d,\"pitch\":%d,\"s2h_row0\":%d,"
         "\"rp_bytes\":%u,\"s2_bytes\":%u,\"s2h_off\":%u,\"scratch_bytes\":%zu,",
         g.row0, g.nrows, g.nbx, g.tiles_x, g.tiles_y, g.ngx, g.ngxw, g.km, g.bm, g.bm_wpr, g.bm_lp,
         g.bmv, g.bmv_r, g.hb, g.hb_row, g.ya0, g.rp_rows, g.rows_alloc, g.pitch, g.s2h_row0,
         g.rp_bytes, g.s2_bytes, g.s2h_off, g.scratch_bytes);
  print_bw(g);
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: mfma_plan_dump FIXTURE.json\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "r");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  const me::Tuning tu;
  static char line[16384];
  char note[256];
  int n = 0;
  while (fgets(line, sizeof line, f)) {
    me::MfmaShape s;
    int path;
    if (sscanf(line,
               " {\"note\":\"%255[^\"]\",\"width\":%d,\"height\":%d,\"stride\":%d,\"blk\":%d,"
               "\"range\":%d,\"cost\":%d,\"r0\":%d,\"r1\":%d,\"nbx\":%d,\"align\":%d,\"merge\":%zu,"
               "\"path\":%d",
               note, &s.width, &s.height, &s.stride, &s.blk, &s.range, &s.cost, &s.row_begin,
               &s.row_end, &s.nbx, &s.align, &s.merge_tiles, &path) != 13)
      continue;
    me::MfmaGeom g;
    const bool ok = me::plan_mfma_ssd(s, path, CUS, tu, &g);
    printf("{\"note\":\"%s\",\"width\":%d,\"height\":%d,\"stride\":%d,\"blk\":%d,\"range\":%d,"
           "\"cost\":%d,\"r0\":%d,\"r1\":%d,\"nbx\":%d,\"align\":%d,\"merge\":%zu,\"path\":%d,"
           "\"ok\":%s,\"scratch\":%zu,\"merge_tiles\":%zu",
           note, s.width, s.height, s.stride, s.blk, s.range, s.cost, s.row_begin, s.row_end, s.nbx,
           s.align, s.merge_tiles, path, ok ? "true" : "false", ok ? g.scratch_bytes : (size_t)0,
           me::mfma_merge_tiles(s));
    if (ok) {
      printf(",\"g\":{");
      print_geom(g);
      printf("}");
    }
    if (ok && s.blk == 16 && s.range <= 64) {
      printf(",\"plan_bw\":[");
      const int jobs[] = {1, 2, 8, 16, 32};
      for (int i = 0; i < 5; i++) {
        me::MfmaGeom t = g;
        const bool bw = me::plan_bw(s, CUS, tu, &t, jobs[i]);
        printf("%s{\"jobs\":%d,\"ok\":%s", i ? "," : "", jobs[i], bw ? "true" : "false");
        if (bw) {
          printf(",\"one_round\":%s,", me::bw_one_round(t, jobs[i], CUS) ? "true" : "false");
          print_bw(t);
        }
        printf("}");
      }
      printf("]");
    }
    printf(",\"batch_scratch\":[");
    const int ns[] = {2, 8, 16, 32, 33};
    for (int i = 0; i < 5; i++) {
      me::MfmaBatch b;
      me::plan_mfma_batch(s, ns[i], me::MFMA_SCRATCH_UNLIMITED, path, CUS, tu, &b);
      printf("%s%zu", i ? "," : "", b.need);
    }
    printf("]}\n");
    n++;
  }
  fclose(f);
  return n > 0 ? 0 : 1;
}
