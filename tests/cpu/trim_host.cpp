// Host build of the trim's host parts (banjax_amd/csrc/state_trim.h) for
// tests/test_state_trim_cpu.py: a stand-alone program that reads commands from
// the file given as argv[1] and prints one answer per command (also the
// sanitizer run).  Values are decimal int64.
//   check NULL | check <flags>            -> "check ok" | "check <message>"
//   geom                                  -> "geom <shift>:<bins> ..." (the digits must tile 64 bits)
//   sel <k> <v>...                        -> "sel none" (k == 0 or no more than k values) |
//       "sel <the (k + 1)-th largest> <cut> <saturated>": the select driven as the
//       engine drives it, the digit histograms computed here over the array
//   plus <v>                              -> "plus <v + 1, saturating> <saturated>"
//   pick <floor> <c_states> <sat> <c_ips> <sat>   -> "pick <C> <bound> <budget_met>"
//   node <n>, then n lines "p <cutoff> <bound> <met> <select_ms>"  -> "node <C> <bound> <met> <select_ms>"
//   sum <n>, then n lines "s <9 counts> <select_ms> <device_ms>"   -> "sum <9 counts> <select_ms> <device_ms>"
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../banjax_amd/csrc/state_trim.h"

static_assert(sizeof(bjx_trim_budget) == 32, "bjx_trim_budget is 32 bytes");
static_assert(sizeof(bjx_trim_stats) == 104, "bjx_trim_stats is 104 bytes");

// the select over v[0, n), exactly the engine's loop: per pass a histogram of
// the keys under the prefix, then bjx_trim::step
static bool select_kth(const int64_t *v, size_t n, uint64_t k, int64_t *out) {
  using namespace bjx_trim;
  Select s;
  for (uint32_t p = 0; p < kDigits; ++p) {
    std::vector<uint64_t> hist(digit_bins(p), 0);  // exact size: a digit past its bins is a write past an allocation
    for (size_t i = 0; i < n; ++i) {
      const uint64_t key = key_of(v[i]);
      if (under(key, s.prefix, p)) ++hist[digit(key, p)];
    }
    if (p == 0) {
      uint64_t total = 0;
      for (uint64_t c : hist) total += c;
      if (total != n) exit(3);
      if (unbounded(k, total)) return false;
      s.rank = k + 1;
    }
    if (!step(&s, hist.data())) exit(3);
  }
  if (!s.done() || s.rank < 1) exit(3);
  *out = value_of(s.prefix);
  return true;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  std::ifstream in(argv[1]);
  if (!in) return 2;
  std::string line;
  while (std::getline(in, line)) {
    std::istringstream ls(line);
    std::string cmd;
    if (!(ls >> cmd)) continue;
    if (cmd == "check") {
      std::string a;
      ls >> a;
      bjx_trim_budget b{};
      if (a != "NULL") b.flags = (uint32_t)strtoul(a.c_str(), nullptr, 10);
      const char *why = bjx_trim::check_budget(a == "NULL" ? nullptr : &b);
      printf("check %s\n", why ? why : "ok");
    } else if (cmd == "geom") {
      uint64_t covered = 0;
      printf("geom");
      for (uint32_t p = 0; p < bjx_trim::kDigits; ++p) {
        const uint64_t m = (uint64_t)(bjx_trim::digit_bins(p) - 1) << bjx_trim::digit_shift(p);
        if (covered & m) return 3;
        covered |= m;
        if (bjx_trim::digit_bins(p) > bjx_trim::kBins) return 3;
        printf(" %u:%u", bjx_trim::digit_shift(p), bjx_trim::digit_bins(p));
      }
      if (covered != ~0ull) return 3;
      printf("\n");
    } else if (cmd == "sel") {
      uint64_t k = 0;
      ls >> k;
      std::vector<int64_t> v;
      for (std::string t; ls >> t;) v.push_back((int64_t)strtoll(t.c_str(), nullptr, 10));
      v.shrink_to_fit();
      int64_t got = 0;
      if (!select_kth(v.data(), v.size(), k, &got)) {
        printf("sel none\n");
      } else {
        const bjx_trim::Cut c = bjx_trim::cut_after(got);
        printf("sel %" PRId64 " %" PRId64 " %d\n", got, c.c, (int)c.saturated);
      }
    } else if (cmd == "plus") {
      std::string t;
      ls >> t;
      const bjx_trim::Cut c = bjx_trim::cut_after((int64_t)strtoll(t.c_str(), nullptr, 10));
      printf("plus %" PRId64 " %d\n", c.c, (int)c.saturated);
    } else if (cmd == "pick") {
      std::string f, a, b;
      int sa = 0, sb = 0;
      ls >> f >> a >> sa >> b >> sb;
      bjx_trim::Cut cs, ci;
      cs.c = (int64_t)strtoll(a.c_str(), nullptr, 10); cs.saturated = sa != 0;
      ci.c = (int64_t)strtoll(b.c_str(), nullptr, 10); ci.saturated = sb != 0;
      const bjx_trim::Picked P = bjx_trim::pick((int64_t)strtoll(f.c_str(), nullptr, 10), cs, ci);
      printf("pick %" PRId64 " %u %u\n", P.cutoff, P.bound, P.budget_met);
    } else if (cmd == "node") {
      size_t n = 0;
      ls >> n;
      std::vector<bjx_trim::Picked> p(n);
      for (size_t k = 0; k < n; ++k) {
        if (!std::getline(in, line)) return 2;
        std::istringstream ss(line);
        std::string c;
        ss >> cmd >> c >> p[k].bound >> p[k].budget_met >> p[k].select_ms;
        if (cmd != "p") return 2;
        p[k].cutoff = (int64_t)strtoll(c.c_str(), nullptr, 10);
      }
      p.shrink_to_fit();
      const bjx_trim::Picked N = bjx_trim::node_pick(p.data(), n);
      printf("node %" PRId64 " %u %u %g\n", N.cutoff, N.bound, N.budget_met, N.select_ms);
    } else if (cmd == "sum") {
      size_t n = 0;
      ls >> n;
      bjx_trim_stats t{};
      for (size_t k = 0; k < n; ++k) {
        if (!std::getline(in, line)) return 2;
        std::istringstream ss(line);
        bjx_trim_stats s{};
        ss >> cmd >> s.states_before >> s.states_dropped >> s.states_dropped_live >> s.ips_before >> s.ips_dropped >>
            s.arena_bytes_before >> s.arena_bytes_after >> s.device_bytes_before >> s.device_bytes_after >> s.select_ms >>
            s.device_ms;
        if (cmd != "s") return 2;
        bjx_trim::add(&t, s);
      }
      printf("sum %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64
             " %g %g\n",
             t.states_before, t.states_dropped, t.states_dropped_live, t.ips_before, t.ips_dropped, t.arena_bytes_before,
             t.arena_bytes_after, t.device_bytes_before, t.device_bytes_after, t.select_ms, t.device_ms);
    } else {
      return 2;
    }
  }
  return 0;
}
