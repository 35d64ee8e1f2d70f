// flow_prebound_dump.cc -- the chain kernel's pre-bound on the CPU (built by
// tools.mk from me_geom.h alone: no GPU, no libme_hip).
//
//   flow_prebound_dump W H STRIDE R0 R1 CUR_ROW0 OUT
//
// One job: block rows [R0, R1) of a W x H frame of 16x16 blocks in 4-block
// tiles, whose cur plane holds the frame's rows from CUR_ROW0 in rows of
// STRIDE bytes.  Writes to OUT, for every full-height block row, tile column,
// lane and r = 0 .. 3, the u32 byte offset flow_qcur_byte gives (the function
// the kernel calls), 0xFFFFFFFF for the lanes of blocks past the tile's last
// (the kernel masks them), and prints one JSON line: the rows and columns
// dumped, every tile column's block count, and the slim scratch layout with
// the pre-bound's marker (tests/test_flow_prebound_geom.py).
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "me_geom.h"

int main(int argc, char** argv) {
  if (argc != 8) {
    fprintf(stderr, "usage: flow_prebound_dump W H STRIDE R0 R1 CUR_ROW0 OUT\n");
    return 2;
  }
  const int W = atoi(argv[1]), H = atoi(argv[2]), stride = atoi(argv[3]), r0 = atoi(argv[4]), r1 = atoi(argv[5]),
            cur_row0 = atoi(argv[6]);
  constexpr int B = 16, TB = 4;
  const int nbx = W / B, ncols = (nbx + TB - 1) / TB;
  std::vector<uint32_t> out;
  std::vector<int> bys;
  for (int by = r0; by < r1; by++) {
    if (H - by * B < B) continue;  // the h = B/2 row is not bounded
    bys.push_back(by);
    for (int c = 0; c < ncols; c++) {
      const int bx0 = c * TB, nb = nbx - bx0 < TB ? nbx - bx0 : TB;
      for (int lane = 0; lane < 64; lane++)
        for (int r = 0; r < 4; r++)
          out.push_back((lane >> 4) < nb ? me::flow_qcur_byte(cur_row0, stride, by * B, bx0, lane, r) : 0xFFFFFFFFu);
    }
  }
  FILE* f = fopen(argv[7], "wb");
  if (!f || fwrite(out.data(), 4, out.size(), f) != out.size() || fclose(f) != 0) return 1;
  printf("{\"ncols\":%d,\"nbx\":%d,\"bys\":[", ncols, nbx);
  for (size_t i = 0; i < bys.size(); i++) printf("%s%d", i ? "," : "", bys[i]);
  printf("],\"mark\":%d,\"mark_bytes\":4,\"list_bytes\":%d,\"dead\":%d,\"dead_bytes\":320,\"ub\":%d,\"ub_bytes\":16,"
         "\"minlb\":%d,\"minlb_bytes\":%d,\"qcur\":%d,\"qcur_bytes\":64,\"slim_bytes\":%d,"
         "\"none\":%u,\"busy7\":%u,\"done7\":%u}\n",
         me::FLOW_SLIM_MARK, 320 * 2, me::FLOW_PRUNE_DEAD, me::FLOW_PRUNE_UB, me::FLOW_SLIM_MINLB, 320 * 4,
         me::FLOW_SLIM_QCUR, me::FLOW_SLIM_BYTES, me::FLOW_MARK_NONE, me::flow_mark_busy(7), me::flow_mark_done(7));
  return 0;
}
