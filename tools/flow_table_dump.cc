// flow_table_dump.cc -- the flow kernel's LDS item table of me_geom.h on the CPU
// (built by tools.mk from the header alone: no GPU, no libme_hip).  The kernel
// compiles the same functions: flow_walk, flow_job_find_in, flow_entry_of,
// flow_entry_item, flow_item_tasks (tests/test_flow_item_table.py).
//
//   flow_table_dump W H NWG BID ROOM CAP R0:T0,R0:T1,... [STRIP_W]
//       A launch of the pruning flow plan's shape (16x16 blocks, +-32, 4-block
//       tiles, 13-row chunks) over a W x H frame geometry: job j starts at
//       block row R0 and owns Tj launch tiles (0: a job without tiles), row-major
//       from that row.  NWG workgroups; BID one of them, or -1 for all.  ROOM:
//       the LDS bytes left for the table, CAP: the tuning build's item limit
//       (0: none).  One JSON line per workgroup: the launch's table entries
//       (flow_table_entries; 0: no table), the workgroup's tiles, per item the
//       table's prefix (nitems + 1 of them), packed word, first valid chunk and
//       the rebuilt Item [j, bx0, by, nb, tly, h, a, X0, c0, nch, prow0, prows].
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "me_geom.h"

int main(int argc, char** argv) {
  if (argc != 8 && argc != 9) {
    fprintf(stderr, "usage: flow_table_dump W H NWG BID ROOM CAP R0:T0,R0:T1,... [STRIP_W]\n");
    return 2;
  }
  constexpr int B = 16, K = 13, S = 32;
  const int W = atoi(argv[1]), H = atoi(argv[2]), nwg = atoi(argv[3]), one = atoi(argv[4]);
  const int room = atoi(argv[5]), cap = atoi(argv[6]);
  if (W < B || W % B || H < 1 || nwg < 1) return 2;
  me::SearchArgs p{};
  p.width = W;
  p.height = H;
  p.blk = B;
  p.range = S;
  me::QsadGeom g{};
  g.tb = 4;
  g.groups = S / 2;
  g.chunks = g.cpp = (2 * S + 1 + K - 1) / K;
  g.nbx_full = W / B;
  g.wg_per_row = (g.nbx_full + g.tb - 1) / g.tb;
  g.strip_w = argc == 9 ? atoi(argv[8]) : 0;  // (only the table's refusal of a strip walk reads it)
  me::FlowJobs jb;
  jb.n = 0;
  jb.tile_pre[0] = 0;
  int max_by = 0;
  for (const char* s = argv[7]; *s;) {
    char* end;
    const long r0 = strtol(s, &end, 10);
    if (end == s || *end != ':' || r0 < 0 || jb.n >= me::MAX_JOBS) return 2;
    s = end + 1;
    const long t = strtol(s, &end, 10);
    if (end == s || t < 0 || (*end && *end != ',')) return 2;
    jb.r0[jb.n] = (int)r0;
    jb.tile_pre[jb.n + 1] = jb.tile_pre[jb.n] + (int)t;
    if (t > 0) {
      const int last = (int)r0 + ((int)t - 1) / g.wg_per_row;
      if (last > max_by) max_by = last;
    }
    jb.n++;
    s = *end == ',' ? end + 1 : end;
  }
  if (jb.n < 1) return 2;
  const int ntiles = jb.tile_pre[jb.n];
  const int entries = me::flow_table_entries(g, ntiles, nwg, max_by, room, cap);
  for (int bid = one < 0 ? 0 : one; bid < (one < 0 ? nwg : one + 1); bid++) {
    const me::FlowWalk w = me::flow_walk(ntiles, nwg, bid);
    // the table as the workgroup fills it: counts, then exclusive prefixes
    std::vector<me::FlowEntry> tab(w.nitems + 1);
    std::vector<int> lc0(w.nitems);
    for (int k = 0; k < w.nitems; k++) {
      const int tile = w.tile0 + k * w.step;
      const int j = me::flow_job_find_in(jb.tile_pre, jb.n, tile);
      tab[k].pack = me::flow_entry_of(g, tile, j, jb.tile_pre[j], jb.r0[j]);
      tab[k].pre = (uint32_t)me::flow_item_tasks(p, g, K, me::flow_entry_item(p, g, B, K, tab[k].pack), &lc0[k]);
    }
    uint32_t base = 0;
    for (int k = 0; k <= w.nitems; k++) {
      const uint32_t c = k < w.nitems ? tab[k].pre : 0u;
      tab[k].pre = base;
      base += c;
    }
    printf("{\"bid\":%d,\"entries\":%d,\"tiles\":[", bid, entries);
    for (int k = 0; k < w.nitems; k++) printf("%s%d", k ? "," : "", w.tile0 + k * w.step);
    printf("],\"pre\":[");
    for (int k = 0; k <= w.nitems; k++) printf("%s%u", k ? "," : "", tab[k].pre);
    printf("],\"pack\":[");
    for (int k = 0; k < w.nitems; k++) printf("%s%u", k ? "," : "", tab[k].pack);
    printf("],\"lc0\":[");
    for (int k = 0; k < w.nitems; k++) printf("%s%d", k ? "," : "", lc0[k]);
    printf("],\"items\":[");
    for (int k = 0; k < w.nitems; k++) {
      const me::Item it = me::flow_entry_item(p, g, B, K, tab[k].pack);
      printf("%s[%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d]", k ? "," : "", it.j, it.bx0, it.by, it.nb, it.tly, it.h, it.a,
             it.X0, it.c0, it.nch, it.prow0, it.prows);
    }
    printf("]}\n");
  }
  return 0;
}
