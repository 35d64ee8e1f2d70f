// flow_planes_dump.cc -- the box-sum planes' scratch sizing on the CPU (built by
// tools.mk from me_valu_plan.cpp alone: no GPU, no libme_hip).
//
//   flow_planes_dump W H BLK RANGE COST(0 ssd | 1 sad) PLANES(-1 | 0 | 1) R0:R1:REF_ROW0 ...
//
// One job per R0:R1:REF_ROW0 (block rows [R0, R1) of a W x H frame, 16-byte
// aligned planes of stride W whose ref holds the frame's rows from REF_ROW0).
// Prints one JSON line: what flow_planes_scratch asks of the context scratch
// for 256 CUs (Tuning::prune_planes = PLANES, else default), whether the flow
// plan over every job's rows exists and prunes, the row pitch, and every
// job's rows and bytes (tests/test_sad_planes_scratch.py).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "me_geom.h"
#include "me_tuning.h"

int main(int argc, char** argv) {
  if (argc < 8) {
    fprintf(stderr, "usage: flow_planes_dump W H BLK RANGE COST PLANES R0:R1:REF_ROW0 ...\n");
    return 2;
  }
  const int W = atoi(argv[1]), H = atoi(argv[2]), B = atoi(argv[3]), S = atoi(argv[4]), cost = atoi(argv[5]);
  me::Tuning tu;
  tu.prune_planes = atoi(argv[6]);
  std::vector<me::SearchJob> jobs;
  int rows = 0;
  for (int i = 7; i < argc; i++) {
    int r0, r1, ref0;
    if (sscanf(argv[i], "%d:%d:%d", &r0, &r1, &ref0) != 3) return 2;
    // (never dereferenced: the planners read the pointers' alignment only)
    jobs.push_back(me::SearchJob{(const uint8_t*)0x10000, ref0, (const uint8_t*)0x20000, r0 * B, r0, r1,
                                 nullptr, nullptr});
    rows += r1 - r0;
  }
  const me::PlanShape s{W, H, W, B, S, cost, rows, me::ALIGN_ALL};
  me::QsadGeom g;
  const bool ok = me::plan_flow(s, 256, tu, &g);
  const size_t need = me::flow_planes_scratch(s, 256, tu, jobs.data(), (int)jobs.size());
  printf("{\"need\":%zu,\"flow\":%s,\"prune\":%d,\"tb\":%d,\"pitch\":%d,\"jobs\":[", need, ok ? "true" : "false",
         ok ? g.prune : 0, ok ? g.tb : 0, me::flow_plane_pitch(W));
  for (size_t i = 0; i < jobs.size(); i++) {
    const int r = me::flow_plane_rows(jobs[i], B, S, H);
    printf("%s{\"rows\":%d,\"bytes\":%zu}", i ? "," : "", r, me::flow_plane_job_bytes(W, r));
  }
  printf("]}\n");
  return 0;
}
