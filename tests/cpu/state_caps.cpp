// Host build of the state tables' sizing rule (banjax_amd/csrc/bjx_common.h:
// table_cap_for, arena_cap_for, clamp_cap) for tests/test_state_caps_cpu.py: a
// program with its own main.  Each argument is a decimal n and prints
// "n table_cap_for(n) arena_cap_for(n)"; an argument "w:f:c" prints
// "clamp clamp_cap(w, f, c)".
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../banjax_amd/csrc/bjx_common.h"

int main(int argc, char **argv) {
  for (int k = 1; k < argc; ++k) {
    if (strchr(argv[k], ':')) {
      char *p = argv[k];
      const uint64_t w = strtoull(p, &p, 10), f = strtoull(p + 1, &p, 10), c = strtoull(p + 1, &p, 10);
      printf("clamp %" PRIu64 "\n", bjx::clamp_cap(w, f, c));
    } else {
      const uint64_t n = strtoull(argv[k], nullptr, 10);
      printf("%" PRIu64 " %" PRIu64 " %" PRIu64 "\n", n, bjx::table_cap_for(n), bjx::arena_cap_for(n));
    }
  }
  return 0;
}
