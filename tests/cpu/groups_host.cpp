// Host build of the groups query's host parts (banjax_amd/csrc/state_groups.h)
// for tests/test_state_groups_cpu.py: a stand-alone program that reads
// commands from the file given as argv[1] and prints one answer per command
// (also the sanitizer run).  Numbers are decimal; an address is IP text.
//   spec <v4_bits> <v6_bits> <order> <limit>    -> "spec ok" | "spec <message>"
//   filter <order> <limit> <ip: - none, N null with a length, else text> <name: the same>
//                                              -> "filter ok" | "filter <message>"
//   pack <ip text> <v4_bits> <v6_bits>         -> "pack <4|6> <hi hex> <lo hex>" | "pack none" (no address)
//   bits <v4_bits> <v6_bits>                   -> "bits <lo_begin> <lo_end> <hi_begin> <hi_end>"
//   row <fam6> <hi hex> <lo hex> <n_ips> <n_states> <hits> <newest> <v4_bits> <v6_bits>
//                                              -> "row <32 hex digits of addr> <family> <bits> <n_ips> <n_states> <hits_sum> <newest_start_ns>"
//   before <order> <rec a> <rec b>             -> "before <0|1>" (a rec: fam6 hi lo n_ips n_states hits newest)
//   merge <cap> <v4_bits> <v6_bits> <order> <limit> <min_ips> <n lists>, then per list "l <n recs>"
//       and n lines "g <rec>" in key order      -> "merge capacity" | "merge <n_groups> <n_groups_min> <n_rows>"
//       followed by n_rows lines "r <row as above>"
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../banjax_amd/csrc/state_groups.h"

static_assert(sizeof(bjx_group_spec) == 24, "bjx_group_spec is 24 bytes");
static_assert(sizeof(bjx_group_row) == 56, "bjx_group_row is 56 bytes");
static_assert(sizeof(bjx_state_groups) == 72, "bjx_state_groups is 72 bytes");

using bjx_groups::Rec;

static Rec read_rec(std::istream &in) {
  Rec r{};
  int64_t hits, newest;
  in >> r.fam6 >> std::hex >> r.hi >> r.lo >> std::dec >> r.n_ips >> r.n_states >> hits >> newest;
  r.hits = (uint64_t)hits;
  r.newest = bjx_groups::start_key(newest);
  return r;
}

static void print_row(const char *tag, const bjx_group_row &o) {
  printf("%s ", tag);
  for (int k = 0; k < 16; ++k) printf("%02x", o.addr[k]);
  printf(" %u %u %" PRIu64 " %" PRIu64 " %" PRId64 " %" PRId64 "\n", o.family, o.bits, o.n_ips, o.n_states, o.hits_sum,
         o.newest_start_ns);
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  std::ifstream file(argv[1]);
  std::string line;
  while (std::getline(file, line)) {
    std::istringstream in(line);
    std::string cmd;
    in >> cmd;
    if (cmd == "spec") {
      bjx_group_spec g{};
      in >> g.v4_bits >> g.v6_bits >> g.order >> g.limit;
      const char *why = bjx_groups::check_spec(&g);
      printf("spec %s\n", why ? why : "ok");
      if (bjx_groups::check_spec(nullptr) == nullptr) return 3;
    } else if (cmd == "filter") {
      bjx_state_filter f{};
      std::string ip, name;
      in >> f.order >> f.limit >> ip >> name;
      if (ip == "N") f.ip.len = 3;
      else if (ip != "-") { f.ip.ptr = ip.data(); f.ip.len = ip.size(); }
      if (name == "N") f.name.len = 3;
      else if (name != "-") { f.name.ptr = name.data(); f.name.len = name.size(); }
      const char *why = bjx_groups::check_filter(&f);
      printf("filter %s\n", why ? why : "ok");
      if (bjx_groups::check_filter(nullptr) == nullptr) return 3;
    } else if (cmd == "pack") {
      std::string ip;
      uint32_t b4, b6;
      in >> ip >> b4 >> b6;
      // the bytes in an allocation of their exact size: a read past them is a read past an allocation
      std::vector<uint8_t> text(ip.begin(), ip.end());
      uint8_t a[16];
      bool is4;
      if (!bjx::go_parse_addr(text.data(), (uint32_t)text.size(), a, &is4)) { printf("pack none\n"); continue; }
      uint32_t fam6;
      uint64_t hi, lo;
      bjx_groups::pack(a, b4, b6, &fam6, &hi, &lo);
      printf("pack %d %" PRIx64 " %" PRIx64 "\n", fam6 ? 6 : 4, hi, lo);
    } else if (cmd == "bits") {
      uint32_t b4, b6;
      in >> b4 >> b6;
      const bjx_groups::SortBits b = bjx_groups::sort_bits(b4, b6);
      printf("bits %d %d %d %d\n", b.lo_begin, b.lo_end, b.hi_begin, b.hi_end);
    } else if (cmd == "row") {
      const Rec r = read_rec(in);
      bjx_group_spec g{};
      in >> g.v4_bits >> g.v6_bits;
      print_row("row", bjx_groups::row_of(r, g));
    } else if (cmd == "before") {
      uint32_t order;
      in >> order;
      const Rec a = read_rec(in), b = read_rec(in);
      printf("before %d\n", bjx_groups::row_before(a, b, order) ? 1 : 0);
    } else if (cmd == "merge") {
      uint64_t cap;
      size_t n_lists;
      bjx_group_spec g{};
      in >> cap >> g.v4_bits >> g.v6_bits >> g.order >> g.limit >> g.min_ips >> n_lists;
      std::vector<std::vector<Rec>> lists(n_lists);
      bjx_groups::Counts total;
      for (auto &l : lists) {
        std::getline(file, line);
        std::istringstream head(line);
        std::string tag;
        size_t n;
        head >> tag >> n;
        if (tag != "l") return 3;
        for (size_t k = 0; k < n; ++k) {
          std::getline(file, line);
          std::istringstream rec(line);
          rec >> tag;
          if (tag != "g") return 3;
          l.push_back(read_rec(rec));
          if (l.size() > 1 && !bjx_groups::key_less(l[l.size() - 2], l.back())) return 4;  // the script's lists are in key order
        }
        bjx_groups::Counts c;
        c.n_matched = 7 * n; c.n_ips_matched = 3 * n; c.n_ips_unparsed = n; c.n_states_unparsed = 2 * n;
        c.device_ms = (double)n;
        bjx_groups::add(&total, c);
      }
      std::vector<Rec> merged;
      if (!bjx_groups::merge(lists, cap, &merged)) { printf("merge capacity\n"); continue; }
      for (size_t k = 1; k < merged.size(); ++k)
        if (!bjx_groups::key_less(merged[k - 1], merged[k])) return 5;
      bjx_state_groups out;
      std::vector<bjx_group_row> rows;
      bjx_groups::finish(merged, g, total, &out, &rows);
      size_t n_all = 0, n_max = 0;
      for (auto &l : lists) { n_all += l.size(); n_max = l.size() > n_max ? l.size() : n_max; }
      if (out.n_matched != 7 * n_all || out.n_ips_matched != 3 * n_all || out.n_ips_unparsed != n_all ||
          out.n_states_unparsed != 2 * n_all || out.device_ms != (double)n_max || out.n_rows != rows.size() ||
          (out.rows != nullptr) != !rows.empty())
        return 6;
      printf("merge %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", out.n_groups, out.n_groups_min, out.n_rows);
      for (const bjx_group_row &o : rows) print_row("r", o);
    } else if (!cmd.empty()) {
      return 2;
    }
  }
  return 0;
}
