// Host build of the host parts of the selection by network
// (banjax_amd/csrc/state_nets.h) for tests/test_state_nets_cpu.py: a stand-alone
// program that reads commands from the file given as argv[1] and prints one
// answer per command (also the sanitizer run).  Strings travel as hex, "-" for
// the empty string, "N" for a NULL pointer (length 0), "N<len>" for a NULL
// pointer with a length.
//   check <filter ip> <filter name> <list 0|1> <entry>...  -> "check ok" | "check <message>"
//       list 0: nets = NULL, n_nets = the number of entries given
//       filter ip "NOFILTER": f = NULL
//   many <count>                                           -> as check: n_nets = count over one shared
//       entry (only used past BJX_NETS_MAX, where no entry may be read)
//   build <entry>...      -> "build bad=<index> (<the message that names it>)" | "build dir=<4|6>/<bits>:<first>+<count>,.. k4=<hex8>,..
//       k6=<hex16><hex16>,.. entry=<canonical index>,.."  ("-" for an empty list)
//   holds <ip> <entry>... -> "holds <0|1> canon=<i>,.."  (every canonical network that holds the IP text)
//   sum <n_nets> <shards>, then per shard "s <count>..." or "s N" (no array) -> "sum <count>..."
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <memory>
#include <sstream>
#include <string>

#include "../../banjax_amd/csrc/state_nets.h"

static_assert(sizeof(bjx_nets::Dir) == 16, "a directory row is 16 bytes");
static_assert(BJX_NETS_MAX == 65536, "BJX_NETS_MAX");

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
struct Args {
  std::vector<Arg> keep;
  std::vector<bjx_str> v;
  explicit Args(std::istringstream &ls) {
    for (std::string h; ls >> h;) keep.push_back(arg(h));
    for (auto &x : keep) v.push_back(x.s);
    v.shrink_to_fit();
  }
};

// the table's own invariants: every length's keys sorted, distinct and masked; the rows tile the arrays
static bool sane(const bjx_nets::Table &T, size_t n_entries) {
  if (T.dir.size() != (size_t)T.n_dir4 + T.n_dir6 || T.n_dir4 > 33 || T.n_dir6 > 129 || T.entry.size() != n_entries) return false;
  uint32_t at4 = 0, at6 = 0;
  for (size_t d = 0; d < T.dir.size(); ++d) {
    const bjx_nets::Dir &D = T.dir[d];
    const bool v4 = d < T.n_dir4;
    if (!D.count || D.bits > (v4 ? 32u : 128u) || D.first != (v4 ? at4 : at6)) return false;
    if (d && d != T.n_dir4 && T.dir[d - 1].bits >= D.bits) return false;
    for (uint32_t k = D.first; k < D.first + D.count; ++k) {
      if (v4) {
        if (T.k4[k] & ~bjx_nets::mask32(D.bits)) return false;
        if (k > D.first && T.k4[k - 1] >= T.k4[k]) return false;
      } else {
        const uint64_t h = T.k6[2 * k], l = T.k6[2 * k + 1];
        if ((h & ~bjx_nets::mask64(D.bits)) || (l & ~(D.bits > 64 ? bjx_nets::mask64(D.bits - 64) : 0ull))) return false;
        if (k > D.first && (T.k6[2 * k - 2] > h || (T.k6[2 * k - 2] == h && T.k6[2 * k - 1] >= l))) return false;
      }
    }
    (v4 ? at4 : at6) += D.count;
  }
  if (at4 != T.k4.size() || 2 * (size_t)at6 != T.k6.size()) return false;
  for (uint32_t c : T.entry)
    if (c >= T.n_canon()) return false;
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
      std::string fip, fname;
      int list = 0;
      ls >> fip;
      if (fip == "NOFILTER") {
        Arg one = arg("312e322e332e34");
        const char *why = bjx_nets::check_args(nullptr, &one.s, 1);
        printf("check %s\n", why ? why : "ok");
        continue;
      }
      ls >> fname >> list;
      Arg a = arg(fip), b = arg(fname);
      Args A(ls);
      bjx_state_filter f{};
      f.ip = a.s;
      f.name = b.s;
      bjx_str none{nullptr, 0};
      const char *why = bjx_nets::check_args(&f, list ? (A.v.empty() ? &none : A.v.data()) : nullptr, A.v.size());
      printf("check %s\n", why ? why : "ok");
    } else if (cmd == "many") {
      uint64_t count = 0;
      ls >> count;
      Arg one = arg("312e322e332e34");
      bjx_state_filter f{};
      const char *why = bjx_nets::check_args(&f, &one.s, (size_t)count);
      printf("check %s\n", why ? why : "ok");
    } else if (cmd == "build") {
      Args A(ls);
      bjx_state_filter f{};
      if (bjx_nets::check_args(&f, A.v.data(), A.v.size())) return 3;
      bjx_nets::Table T;
      const int64_t bad = bjx_nets::build(A.v.data(), A.v.size(), &T);
      if (bad >= 0) {
        printf("build bad=%" PRId64 " (%s)\n", bad, bjx_nets::bad_entry(bad).c_str());
        continue;
      }
      if (!sane(T, A.v.size())) return 3;
      // the image is the three arrays, back to back
      std::vector<uint8_t> img;
      uint64_t o_dir = 0, o_k4 = 0;
      const uint64_t total = T.image(&img, &o_dir, &o_k4);
      if (total != img.size() || o_dir != T.k6.size() * 8 || o_k4 != o_dir + T.dir.size() * 16 || total != o_k4 + T.k4.size() * 4 ||
          (T.k4.size() && memcmp(img.data() + o_k4, T.k4.data(), T.k4.size() * 4)) ||
          (T.k6.size() && memcmp(img.data(), T.k6.data(), T.k6.size() * 8)))
        return 3;
      printf("build dir=");
      for (size_t d = 0; d < T.dir.size(); ++d)
        printf("%s%d/%u:%u+%u", d ? "," : "", d < T.n_dir4 ? 4 : 6, T.dir[d].bits, T.dir[d].first, T.dir[d].count);
      printf(" k4=%s", T.k4.empty() ? "-" : "");
      for (size_t k = 0; k < T.k4.size(); ++k) printf("%s%08x", k ? "," : "", T.k4[k]);
      printf(" k6=%s", T.k6.empty() ? "-" : "");
      for (size_t k = 0; k < T.k6.size(); k += 2) printf("%s%016" PRIx64 "%016" PRIx64, k ? "," : "", T.k6[k], T.k6[k + 1]);
      printf(" entry=");
      for (size_t k = 0; k < T.entry.size(); ++k) printf("%s%u", k ? "," : "", T.entry[k]);
      printf("\n");
    } else if (cmd == "holds") {
      std::string ip;
      ls >> ip;
      Arg a = arg(ip);
      Args A(ls);
      bjx_nets::Table T;
      if (bjx_nets::build(A.v.data(), A.v.size(), &T) >= 0) return 3;
      std::vector<uint32_t> canon;
      const bool all = T.holds(reinterpret_cast<const uint8_t *>(a.s.ptr), (uint32_t)a.s.len, &canon);
      const bool any = T.holds(reinterpret_cast<const uint8_t *>(a.s.ptr), (uint32_t)a.s.len);
      if (all != any || all != !canon.empty()) return 3;
      printf("holds %d canon=%s", (int)any, canon.empty() ? "-" : "");
      for (size_t k = 0; k < canon.size(); ++k) printf("%s%u", k ? "," : "", canon[k]);
      printf("\n");
    } else if (cmd == "sum") {
      size_t n_nets = 0, shards = 0;
      ls >> n_nets >> shards;
      std::vector<uint64_t> t;
      for (size_t k = 0; k < shards; ++k) {
        if (!std::getline(in, line)) return 2;
        std::istringstream ss(line);
        std::string w;
        ss >> w;
        if (w != "s") return 2;
        std::unique_ptr<uint64_t[]> s(new uint64_t[n_nets ? n_nets : 1]);
        size_t got = 0;
        bool null = false;
        while (ss >> w) {
          if (w == "N") { null = true; break; }
          if (got == n_nets) return 2;
          s[got++] = strtoull(w.c_str(), nullptr, 10);
        }
        if (!null && got != n_nets) return 2;
        bjx_nets::add(&t, null ? nullptr : s.get(), n_nets);
      }
      printf("sum");
      for (uint64_t v : t) printf(" %" PRIu64, v);
      printf("\n");
    } else {
      return 2;
    }
  }
  return 0;
}
