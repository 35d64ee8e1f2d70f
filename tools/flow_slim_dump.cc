// flow_slim_dump.cc -- the pruning flow launch's two scratch layouts and the
// bound's plane loads on the CPU (built by tools.mk from me_valu_plan.cpp and
// me_geom.h alone: no GPU, no libme_hip).  tests/test_flow_slim_plan.py.
//
//   flow_slim_dump plan W H STRIDE ROWS SLOTS
//     plan_flow for ROWS block rows of a W x H frame on 256 CUs, Tuning::
//     flow_slots = SLOTS (0: free).  One JSON line: the slot counts and LDS
//     bytes of the layout without planes (prune_*) and with them (slim_*).
//
//   flow_slim_dump fit W0 W1
//     Every width W0 <= W <= W1: whether the flow plan over 4,096 block rows
//     prunes, and then whether any lane's load (8 bytes at 16 c + 4 b + 4 m of a
//     phase row, 4 at 16 c + 4 b + 16) of any tile column c ends past the pitch.
//     One JSON line: the widths planned, those with planes, the offenders.
//
//   flow_slim_dump addr W H R0 R1 REF_ROW0 OUT
//     One job (block rows [R0, R1), ref rows from REF_ROW0): for every full-
//     height tile (block row by, tile column c) the kernel's byte offsets,
//     written to OUT as uint32: [by][c][yp 0..76][lane 0..63] of step 2 (lane =
//     block b, phase k, group m: flow_plane_byte(.., yp, k, 4 b + 4 m)), then
//     [by][c][n 0..19][lane] of the fold column (lane = block b, row y:
//     flow_plane_byte(.., y + 4 n, 0, 4 b + 16)).  One JSON line: the pitch,
//     the job's plane rows and bytes, the tile columns and the block rows dumped.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "me_geom.h"
#include "me_tuning.h"

static int plan(int argc, char** argv) {
  if (argc != 7) return 2;
  const int W = atoi(argv[2]), H = atoi(argv[3]), stride = atoi(argv[4]), rows = atoi(argv[5]);
  me::Tuning tu;
  tu.flow_slots = atoi(argv[6]);
  const me::PlanShape s{W, H, stride, 16, 32, me::COST_SAD, rows, me::ALIGN_ALL};
  me::QsadGeom g;
  const bool ok = me::plan_flow(s, 256, tu, &g);
  printf("{\"flow\":%s,\"prune\":%d,\"tb\":%d,\"pitch\":%d,\"tile_bytes\":%d,\"wg_per_row\":%d,"
         "\"prune_slots\":%d,\"prune_lds\":%d,\"slim_slots\":%d,\"slim_lds\":%d,"
         "\"prune_bytes\":%d,\"slim_bytes\":%d,\"ctl_bytes\":%d,\"lds_budget\":%d,\"plane_pitch\":%d}\n",
         ok ? "true" : "false", g.prune, g.tb, g.pitch, g.tile_bytes, g.wg_per_row, g.prune_slots, g.prune_lds,
         g.slim_slots, g.slim_lds, me::FLOW_PRUNE_BYTES, me::FLOW_SLIM_BYTES, me::FLOW_CTL_BYTES,
         me::FLOW_LDS_BUDGET, me::flow_plane_pitch(W));
  return 0;
}

static int fit(int argc, char** argv) {
  if (argc != 4) return 2;
  const int W0 = atoi(argv[2]), W1 = atoi(argv[3]);
  me::Tuning tu;
  int planned = 0, slim = 0;
  std::vector<int> bad;
  for (int W = W0; W <= W1; W++) {
    const me::PlanShape s{W, 1088, W, 16, 32, me::COST_SAD, 4096, me::ALIGN_ALL};
    me::QsadGeom g;
    if (!me::plan_flow(s, 256, tu, &g) || !g.prune) continue;
    planned++;
    if (g.slim_slots) slim++;
    const int pitch = me::flow_plane_pitch(W);
    bool ok = true;
    // every lane of every tile column, through the kernel's formula (rel = yp = 0: byte in the phase row)
    for (int c = 0; c < g.wg_per_row; c++)
      for (int lane = 0; lane < 64; lane++) {
        const int b = lane >> 4, k = (lane >> 2) & 3, m = lane & 3;
        const uint32_t o2 = me::flow_plane_byte(pitch, 0, 64 * c - 32, 0, k, 4 * b + 4 * m) - (uint32_t)(k * pitch);
        const uint32_t of = me::flow_plane_byte(pitch, 0, 64 * c - 32, 0, 0, 4 * b + 16);
        ok = ok && o2 % 4 == 0 && of % 4 == 0 && o2 + 8 <= (uint32_t)pitch && of + 4 <= (uint32_t)pitch;
      }
    // (the planner's own check must say the same, and gates the slim layout by it)
    if (!ok || !me::flow_plane_loads_fit(W, g.wg_per_row) || !g.slim_slots) bad.push_back(W);
  }
  printf("{\"planned\":%d,\"slim\":%d,\"bad\":[", planned, slim);
  for (size_t i = 0; i < bad.size(); i++) printf("%s%d", i ? "," : "", bad[i]);
  printf("]}\n");
  return 0;
}

static int addr(int argc, char** argv) {
  if (argc != 8) return 2;
  const int W = atoi(argv[2]), H = atoi(argv[3]), r0 = atoi(argv[4]), r1 = atoi(argv[5]), ref0 = atoi(argv[6]);
  const int B = 16, S = 32;
  const me::SearchJob J{nullptr, ref0, nullptr, r0 * B, r0, r1, nullptr, nullptr};
  const int pitch = me::flow_plane_pitch(W), rows = me::flow_plane_rows(J, B, S, H);
  const int ncols = (W / B + 3) / 4;
  std::vector<uint32_t> out;
  std::vector<int> bys;
  for (int by = r0; by < r1; by++)
    if (H - by * B >= B) bys.push_back(by);  // (an h = 8 bottom row is not bounded: no plane loads)
  for (int by : bys)
    for (int c = 0; c < ncols; c++)
      for (int yp = 0; yp < me::FLOW_PRUNE_QROWS; yp++)
        for (int lane = 0; lane < 64; lane++) {
          const int b = lane >> 4, k = (lane >> 2) & 3, m = lane & 3;
          out.push_back(me::flow_plane_byte(pitch, by * B - S - ref0, 64 * c - 32, yp, k, 4 * b + 4 * m));
        }
  for (int by : bys)
    for (int c = 0; c < ncols; c++)
      for (int n = 0; n < 20; n++)
        for (int lane = 0; lane < 64; lane++)
          out.push_back(me::flow_plane_byte(pitch, by * B - S - ref0, 64 * c - 32, (lane & 15) + 4 * n, 0,
                                            4 * (lane >> 4) + 16));
  FILE* f = fopen(argv[7], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size() || fclose(f)) return 1;
  printf("{\"pitch\":%d,\"rows\":%d,\"bytes\":%zu,\"ncols\":%d,\"bys\":[", pitch, rows,
         me::flow_plane_job_bytes(W, rows), ncols);
  for (size_t i = 0; i < bys.size(); i++) printf("%s%d", i ? "," : "", bys[i]);
  printf("]}\n");
  return 0;
}

int main(int argc, char** argv) {
  int r = 2;
  if (argc >= 2 && !strcmp(argv[1], "plan")) r = plan(argc, argv);
  if (argc >= 2 && !strcmp(argv[1], "fit")) r = fit(argc, argv);
  if (argc >= 2 && !strcmp(argv[1], "addr")) r = addr(argc, argv);
  if (r == 2) fprintf(stderr, "usage: flow_slim_dump plan W H STRIDE ROWS SLOTS | fit W0 W1 | addr W H R0 R1 REF_ROW0 OUT\n");
  return r;
}
