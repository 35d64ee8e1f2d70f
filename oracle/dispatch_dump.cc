// dispatch_dump.cc -- print the search dispatcher's launch lists for a table of
// cases (TEST INFRASTRUCTURE; built by `make -C oracle dispatch_dump` from
// me_dispatch.cpp and the two planner files alone, no GPU and no libme_hip).
//
//   dispatch_dump tests/golden/plans/dispatch.json
//
// The fixture holds one record per line; each starts with the case
// (dispatch_cases.h).  For every such line this prints the case again and the list the
// dispatcher gives now (256 CUs, default Tuning): per launch the kind, the
// path code noted, the job range, the block rectangle [r0, r1, bx0, bx1] of
// each of its jobs, and the plan fields that select kernel and grid.
// tests/test_dispatch.py paints the rectangles and compares the records.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "dispatch_cases.h"

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: dispatch_dump FIXTURE.json\n");
    return 2;
  }
  FILE* f = fopen(argv[1], "r");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  const me::Tuning tu;
  const int CUS = 256;
  static char line[1 << 16];
  int n = 0;
  DispatchCase c;
  while (fgets(line, sizeof line, f)) {
    if (!parse_dispatch_case(line, CUS, tu, &c)) continue;
    const me::SearchShape& s = c.s;
    const std::vector<me::SearchJob>& jobs = c.jobs;
    const int nj = (int)jobs.size();
    // a small window on purpose: long lists come through several calls
    const std::vector<me::Launch> list = dispatch_all(c, CUS, tu, 7);

    printf("{\"name\":\"%s\",\"width\":%d,\"height\":%d,\"stride\":%d,\"blk\":%d,\"range\":%d,\"cost\":%d,"
           "\"path\":%d,\"scratch\":%lld,\"jobs\":[",
           c.name, s.width, s.height, s.stride, s.blk, s.range, s.cost, c.path, c.scratch);
    for (int j = 0; j < nj; j++)
      printf("%s[%d,%d,%d,%d,%d,%d]", j ? "," : "", jobs[j].r0, jobs[j].r1, jobs[j].ref_row0,
             jobs[j].cur_row0, c.mods[2 * j], c.mods[2 * j + 1]);
    printf("],\"launches\":[");
    static const char* kinds[] = {"GENERIC", "ITEM", "FLOW", "MFMA", "SSIM"};
    for (size_t i = 0; i < list.size(); i++) {
      const me::Launch& l = list[i];
      printf("%s{\"kind\":\"%s\",\"path\":%d,\"job0\":%d,\"njobs\":%d,\"rects\":[", i ? "," : "",
             kinds[l.kind], l.path, l.job0, l.njobs);
      for (int j = 0; j < l.njobs; j++)
        printf("%s[%d,%d,%d,%d]", j ? "," : "", me::launch_r0(l, jobs[l.job0 + j]),
               me::launch_r1(l, jobs[l.job0 + j]), l.bx0, l.bx1);
      printf("]");
      if (l.kind == me::LAUNCH_ITEM || l.kind == me::LAUNCH_FLOW)
        printf(",\"K\":%d,\"tb\":%d,\"pitch\":%d,\"threads\":%d,\"lds\":%d,\"wg_per_row\":%d,\"strip_w\":%d,"
               "\"nbx_full\":%d,\"flow_slots\":%d,\"prune\":%d",
               l.kind == me::LAUNCH_ITEM ? l.K : 13, l.g.tb, l.g.pitch, l.g.threads, l.g.lds,
               l.g.wg_per_row, l.g.strip_w, l.g.nbx_full, l.g.flow_slots, l.g.prune);
      if (l.kind == me::LAUNCH_MFMA)
        printf(",\"bw\":%d,\"bmv\":%d,\"bm\":%d,\"row0\":%d,\"nrows\":%d,\"nbx\":%d,\"lds\":%d,"
               "\"plan_scratch\":%zu,\"scratch_stride\":%zu",
               l.mg.bw, l.mg.bmv, l.mg.bm, l.mg.row0, l.mg.nrows, l.mg.nbx, l.mg.lds,
               l.mg.scratch_bytes, l.scratch_stride);
      printf("}");
    }
    printf("]}\n");
    n++;
  }
  fclose(f);
  return n > 0 ? 0 : 1;
}
