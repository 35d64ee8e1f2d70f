// api_rules_dump.cc -- the C ABI's argument rules and record layouts without a
// GPU (TEST INFRASTRUCTURE; tests/test_api_rules.py).  Links
// csrc/me_api_rules.cpp and the host-only files its rules call, nothing else.
//
//   api_rules_dump TABLE [NDEV]   one JSON line per case of TABLE (the format of
//                                 tests/golden/api_args.json): the status and
//                                 message its entry point's rules give on a
//                                 context of NDEV devices (default: the case's)
//   api_rules_dump --layouts W H B   every record layout for a WxH frame, block B
#include <stdio.h>
#include <stdlib.h>

#include "api_rules_cases.h"

static void print_layout(const char* name, const me::rules::Layout& L, const char* end) {
  printf("\"%s\":{\"total\":%zu,\"regions\":[", name, L.total);
  for (int k = 0; k < L.n; k++)
    printf("%s[%zu,%zu,%zu]", k ? "," : "", L.off[k], L.bytes[k], L.elem[k]);
  printf("]}%s", end);
}

int main(int argc, char** argv) {
  if (argc == 5 && !strcmp(argv[1], "--layouts")) {
    const int W = atoi(argv[2]), H = atoi(argv[3]), B = atoi(argv[4]);
    int counts[4];
    if (me_partition_counts(W, H, B, counts) != ME_OK) return 2;
    const size_t nb = (size_t)me_num_blocks(W, H, B);
    printf("{\"n_blocks\":%zu,\"counts\":[%d,%d,%d,%d],", nb, counts[0], counts[1], counts[2], counts[3]);
    print_layout("mv_cost", me::rules::layout_mv_cost(nb), ",");
    print_layout("bipred", me::rules::layout_bipred(nb), ",");
    print_layout("rd", me::rules::layout_rd(nb), ",");
    print_layout("partition", me::rules::layout_partition(counts), ",");
    print_layout("partition_rd", me::rules::layout_partition_rd(counts), "}\n");
    return 0;
  }
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "r");
  if (!f) return 2;
  static char line[1 << 14];
  ApiCase c;
  while (fgets(line, sizeof line, f)) {
    if (!parse_api_case(line, &c)) continue;
    char err[512];
    const int s = run_api_case(c, argc > 2 ? atoi(argv[2]) : c.ndev, err, sizeof err);
    printf("{\"name\":\"%s\",\"status\":%d,\"message\":\"%s\"}\n", c.name.c_str(), s, err);
  }
  fclose(f);
  return 0;
}
