// flow_split_dump.cc -- the row split's rule of me_geom.h on the CPU (built by
// tools.mk into bin/flow_split_dump; tests/test_flow_split_rule.py reads it).
// One JSON line per n = 1 .. 64 list entries of a wave-task:
//   {"n":, "rows":, "parts":, "rows_124":, "parts_124":,
//    "lanes": [[entry, first row, live, fold] x 64], "lanes_124": the same}
// what flow_split_lane, the function flow_split_task places its lanes with,
// gives for the 64 lanes under the rule and under the earlier one.
#include <stdio.h>

#include "me_geom.h"

static void lanes(const char* name, int R, int n) {
  printf(",\"%s\":[", name);
  for (int l = 0; l < 64; l++) {
    const me::FlowSplitLane s = me::flow_split_lane(R, l, n);
    printf("%s[%d,%d,%d,%d]", l ? "," : "", s.entry, s.row0, s.live ? 1 : 0, s.fold ? 1 : 0);
  }
  printf("]");
}

int main() {
  for (int n = 1; n <= 64; n++) {
    const int R = me::flow_split_rows(n), R0 = me::flow_split_rows_124(n);
    printf("{\"n\":%d,\"rows\":%d,\"parts\":%d,\"rows_124\":%d,\"parts_124\":%d", n, R, me::flow_split_parts(n), R0,
           me::flow_split_parts_of(R0));
    lanes("lanes", R, n);
    lanes("lanes_124", R0, n);
    printf("}\n");
  }
  return 0;
}
