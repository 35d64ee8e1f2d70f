// flow_job_dump.cc -- the launch tile -> job rule of me_geom.h on the CPU (built
// by tools.mk from the header alone: no GPU, no libme_hip).  The flow kernel
// compiles the same two functions (tests/test_flow_job_lookup.py).
//
//   flow_job_dump table C0,C1,...
//       A job table of those tile counts (0: a job without tiles).  One JSON
//       line: per launch tile its job by flow_job_find and by flow_job_from
//       from job 0.
//   flow_job_dump walk NWG NB C0,C1,...
//       me_flow_kernel's walk of that table with NWG workgroups and a ring of
//       NB slots.  One JSON line per workgroup: its tiles, the job of every
//       item as a wave finds it (the first by flow_job_find, each later one by
//       flow_job_from from the item before it), and the job of every refill
//       target (item k + NB, by flow_job_from from item k's job; -1: none).
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "me_geom.h"

static bool table(const char* arg, me::FlowJobs* jb) {
  jb->n = 0;
  jb->tile_pre[0] = 0;
  for (const char* s = arg; *s;) {
    char* end;
    const long c = strtol(s, &end, 10);
    if (end == s || c < 0 || jb->n >= me::MAX_JOBS) return false;
    jb->tile_pre[jb->n + 1] = jb->tile_pre[jb->n] + (int)c;
    jb->n++;
    s = *end == ',' ? end + 1 : end;
    if (*end && *end != ',') return false;
  }
  return jb->n > 0;
}

static void print_list(const char* name, const std::vector<int>& v, const char* tail) {
  printf("\"%s\":[", name);
  for (size_t i = 0; i < v.size(); i++) printf("%s%d", i ? "," : "", v[i]);
  printf("]%s", tail);
}

int main(int argc, char** argv) {
  me::FlowJobs jb;
  if (argc == 3 && !strcmp(argv[1], "table") && table(argv[2], &jb)) {
    std::vector<int> find, scan;
    for (int t = 0; t < jb.tile_pre[jb.n]; t++) {
      find.push_back(me::flow_job_find(jb, t));
      scan.push_back(me::flow_job_from(jb, t, 0));
    }
    printf("{");
    print_list("find", find, ",");
    print_list("scan", scan, "}\n");
    return 0;
  }
  if (argc == 5 && !strcmp(argv[1], "walk") && table(argv[4], &jb)) {
    const int nwg = atoi(argv[2]), NB = atoi(argv[3]);
    if (nwg < 1 || NB < 1) return 2;
    // me_flow_kernel's tiles of workgroup bid: band x = bid % 8 of the launch,
    // member m = bid / 8 takes band0 + m, + n_x, ...
    const int ntiles = jb.tile_pre[jb.n];
    const int ng = nwg < 8 ? nwg : 8;
    for (int bid = 0; bid < nwg; bid++) {
      const int x = bid % ng, m = bid / ng;
      const int n_x = nwg / ng + (x < nwg % ng ? 1 : 0);
      const int band0 = (int)((long)ntiles * x / ng), band1 = (int)((long)ntiles * (x + 1) / ng);
      const int nitems = band1 - band0 > m ? (band1 - band0 - m + n_x - 1) / n_x : 0;
      std::vector<int> tiles, adv, refill;
      for (int k = 0; k < nitems; k++) {
        tiles.push_back(band0 + m + k * n_x);
        adv.push_back(k == 0 ? me::flow_job_find(jb, tiles[k]) : me::flow_job_from(jb, tiles[k], adv[k - 1]));
      }
      for (int k = 0; k < nitems; k++)
        refill.push_back(k + NB < nitems ? me::flow_job_from(jb, tiles[k + NB], adv[k]) : -1);
      printf("{\"bid\":%d,", bid);
      print_list("tiles", tiles, ",");
      print_list("adv", adv, ",");
      print_list("refill", refill, "}\n");
    }
    return 0;
  }
  fprintf(stderr, "usage: flow_job_dump table C0,C1,... | walk NWG NB C0,C1,...\n");
  return 2;
}
