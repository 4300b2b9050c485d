// Host build of the state removal's host parts (banjax_amd/csrc/state_remove.h)
// for tests/test_state_remove_cpu.py: a stand-alone program that reads commands
// from the file given as argv[1] and prints one answer per command (also the
// sanitizer run).  Strings travel as hex, "-" for the empty string, "N" for a
// NULL pointer (length 0), "N<len>" for a NULL pointer with a length.
//   check <filter ip> <filter name> <no_list 0|1> <entry>...   -> "check ok" | "check <message>"
//       no_list 1 with entries: n_ips = their count, ips = NULL
//   big <len> <count>                                          -> as check: `count` entries of `len` bytes each
//       that share one small buffer (only the lengths may be read)
//   pack <filter ip> <entry>...                                -> "pack n_list=<n> has_ip=<0|1> restrict=<0|1>
//       nothing=<0|1> sel=<first>+<count> off=<o0,o1,..> bytes=<hex>"
//   sum <n>, then n lines "s <10 fields of bjx_remove_stats>"  -> "sum <10 fields>"
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <memory>
#include <sstream>
#include <string>

#include "../../banjax_amd/csrc/state_remove.h"

static_assert(sizeof(bjx_remove_stats) == 80, "bjx_remove_stats is 80 bytes");

// one string argument: exact-size storage, so a read past it is a read past an allocation
struct Arg {
  std::unique_ptr<char[]> mem;
  bjx_str s{nullptr, 0};
};
static Arg arg(const std::string &h) {
  Arg a;
  if (h[0] == 'N') {
    a.s.len = h.size() > 1 ? (size_t)strtoull(h.c_str() + 1, nullptr, 10) : 0;
    return a;
  }
  const size_t n = h == "-" ? 0 : h.size() / 2;
  a.mem.reset(new char[n ? n : 1]);
  for (size_t k = 0; k < n; ++k) a.mem[k] = (char)strtoul(h.substr(2 * k, 2).c_str(), nullptr, 16);
  a.s.ptr = a.mem.get();
  a.s.len = n;
  return a;
}
static std::string hex(const uint8_t *p, size_t n) {
  if (!n) return "-";
  static const char *d = "0123456789abcdef";
  std::string out;
  for (size_t k = 0; k < n; ++k) { out.push_back(d[p[k] >> 4]); out.push_back(d[p[k] & 15]); }
  return out;
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
      std::string fip, fname;
      int no_list = 0;
      ls >> fip >> fname >> no_list;
      if (fip == "NOFILTER") {
        const char *why = bjx_remove::check_args(nullptr, nullptr, 0);
        printf("check %s\n", why ? why : "ok");
        continue;
      }
      Arg a = arg(fip), b = arg(fname);
      std::vector<Arg> keep;
      for (std::string h; ls >> h;) keep.push_back(arg(h));
      std::vector<bjx_str> v;
      for (auto &x : keep) v.push_back(x.s);
      v.shrink_to_fit();
      bjx_state_filter f{};
      f.ip = a.s;
      f.name = b.s;
      const char *why = bjx_remove::check_args(&f, no_list || v.empty() ? nullptr : v.data(), no_list ? keep.size() : v.size());
      printf("check %s\n", why ? why : "ok");
    } else if (cmd == "big") {
      uint64_t len = 0, count = 0;
      ls >> len >> count;
      char small[4] = {1, 2, 3, 4};
      std::vector<bjx_str> v((size_t)count, bjx_str{small, (size_t)len});
      bjx_state_filter f{};
      const char *why = bjx_remove::check_args(&f, v.data(), v.size());
      printf("check %s\n", why ? why : "ok");
    } else if (cmd == "pack") {
      std::string fip;
      ls >> fip;
      Arg a = arg(fip);
      std::vector<Arg> keep;
      for (std::string h; ls >> h;) keep.push_back(arg(h));
      std::vector<bjx_str> v;
      for (auto &x : keep) v.push_back(x.s);
      v.shrink_to_fit();
      bjx_state_filter f{};
      f.ip = a.s;
      if (bjx_remove::check_args(&f, v.empty() ? nullptr : v.data(), v.size())) return 3;
      bjx_remove::List L;
      bjx_remove::pack(f, v.empty() ? nullptr : v.data(), v.size(), &L);
      if (L.off.size() != (size_t)L.n_entries() + 1 || L.off.back() != L.bytes.size()) return 3;
      if (L.restrict && !L.nothing && (uint64_t)L.sel_first + L.sel_count > L.n_entries()) return 3;
      printf("pack n_list=%u has_ip=%d restrict=%d nothing=%d sel=%u+%u off=", L.n_list, (int)L.has_ip, (int)L.restrict,
             (int)L.nothing, L.sel_first, L.sel_count);
      for (size_t k = 0; k < L.off.size(); ++k) printf("%s%u", k ? "," : "", L.off[k]);
      printf(" bytes=%s\n", hex(L.bytes.data(), L.bytes.size()).c_str());
    } else if (cmd == "sum") {
      size_t n = 0;
      ls >> n;
      bjx_remove_stats t{};
      for (size_t k = 0; k < n; ++k) {
        if (!std::getline(in, line)) return 2;
        std::istringstream ss(line);
        bjx_remove_stats s{};
        ss >> cmd >> s.states_before >> s.states_dropped >> s.ips_before >> s.ips_dropped >> s.ips_found >>
            s.arena_bytes_before >> s.arena_bytes_after >> s.device_bytes_before >> s.device_bytes_after >> s.device_ms;
        if (cmd != "s") return 2;
        bjx_remove::add(&t, s);
      }
      printf("sum %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64
             " %g\n",
             t.states_before, t.states_dropped, t.ips_before, t.ips_dropped, t.ips_found, t.arena_bytes_before,
             t.arena_bytes_after, t.device_bytes_before, t.device_bytes_after, t.device_ms);
    } else {
      return 2;
    }
  }
  return 0;
}
