// plan_dump.cc -- print the VALU planners' plans for a table of shapes (TEST
// INFRASTRUCTURE; built by `make -C oracle plan_dump` from me_valu_plan.cpp
// alone, no GPU and no libme_hip).
//
//   plan_dump tests/golden/plans/valu_plans.json
//
// The fixture holds one record per line; each starts with the shape
//   {"planner":"fast"|"flow","width":..,"height":..,"stride":..,"blk":..,
//    "range":..,"cost":..,"rows":..,"align":..
// followed by the plan recorded from the commit before the planners moved out
// of me_kernels.hip.  For every such line this prints the record the planners
// give now (256 CUs, default Tuning), in the same form;
// tests/test_valu_plan.py requires the two to be equal field by field.
#include <stdio.h>
#include <string.h>

#include "me_geom.h"
#include "me_tuning.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: plan_dump FIXTURE.json\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "r");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  const me::Tuning tu;
  char line[2048], planner[8];
  int n = 0;
  while (fgets(line, sizeof line, f)) {
    me::PlanShape s;
    if (sscanf(line,
               " {\"planner\":\"%7[a-z]\",\"width\":%d,\"height\":%d,\"stride\":%d,\"blk\":%d,"
               "\"range\":%d,\"cost\":%d,\"rows\":%d,\"align\":%d",
               planner, &s.width, &s.height, &s.stride, &s.blk, &s.range, &s.cost, &s.rows,
               &s.align) != 9)
      continue;
    const bool flow = strcmp(planner, "flow") == 0;
    me::QsadGeom g;
    int K = 13;
    const bool ok = flow ? me::plan_flow(s, 256, tu, &g) : me::plan_fast(s, 256, tu, &g, &K);
    printf("{\"planner\":\"%s\",\"width\":%d,\"height\":%d,\"stride\":%d,\"blk\":%d,\"range\":%d,"
           "\"cost\":%d,\"rows\":%d,\"align\":%d,\"ok\":%s",
           planner, s.width, s.height, s.stride, s.blk, s.range, s.cost, s.rows, s.align,
           ok ? "true" : "false");
    if (ok)
      printf(",\"K\":%d,\"tb\":%d,\"rows_alloc\":%d,\"groups\":%d,\"chunks\":%d,\"cpp\":%d,"
             "\"pitch\":%d,\"tile_bytes\":%d,\"pitch_magic\":%u,\"magic_groups\":%u,\"threads\":%d,"
             "\"lds\":%d,\"wg_per_row\":%d,\"magic_wpr\":%u,\"magic_tb\":%u,\"strip_w\":%d,"
             "\"nbx_full\":%d,\"aligned\":%d,\"tile16\":%d,\"fold\":%d,\"dyn_tiles\":%d,"
             "\"pull_ahead\":%d,\"flow_slots\":%d,\"prio\":%d,\"fair\":%d",
             K, g.tb, g.rows_alloc, g.groups, g.chunks, g.cpp, g.pitch, g.tile_bytes, g.pitch_magic,
             g.magic_groups, g.threads, g.lds, g.wg_per_row, g.magic_wpr, g.magic_tb, g.strip_w,
             g.nbx_full, g.aligned, g.tile16, g.fold, g.dyn_tiles, g.pull_ahead, g.flow_slots,
             g.prio, g.fair);
    printf("}\n");
    n++;
  }
  fclose(f);
  return n > 0 ? 0 : 1;
}
