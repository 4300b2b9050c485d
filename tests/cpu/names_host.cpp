// Host build of the names query's host parts (banjax_amd/csrc/state_names.h)
// for tests/test_state_names_cpu.py: a stand-alone program that reads
// commands from the file given as argv[1] and prints one answer per command
// (also the sanitizer run).  Numbers are decimal; a name is hex digits, "-"
// the empty name.
//   spec <order> <limit>                        -> "spec ok" | "spec <message>"
//   filter <order> <limit> <ip: - none, N null with a length, else text> <name: the same>
//                                               -> "filter ok" | "filter <message>"
//   bucket <hits>                               -> "bucket <b>"
//   before <order> <item a> <item b>            -> "before <0|1>"
//       (an item: name n_states hits_sum max_hits newest oldest)
//   acc <n>, then n lines "s <hits> <start>"    -> "acc <row>" of add_state over them
//   merge <cap> <order> <limit> <min_states> <n lists>, then per list "l <n items>"
//       and n lines "i <item> <16 hist counts>"  -> "merge capacity" | "merge <n_names> <n_names_min> <n_rows>"
//       followed by n_rows lines "r <row>"
//   a row: <name> <n_states> <hits_sum> <max_hits> <newest> <oldest> <16 hist counts>
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../banjax_amd/csrc/state_names.h"

static_assert(sizeof(bjx_names_spec) == 16, "bjx_names_spec is 16 bytes");
static_assert(sizeof(bjx_name_row) == 184, "bjx_name_row is 184 bytes");
static_assert(sizeof(bjx_state_names) == 72, "bjx_state_names is 72 bytes");

using bjx_names::Item;
using bjx_names::Rec;

static std::string unhex(const std::string &h) {
  std::string out;
  if (h == "-") return out;
  for (size_t k = 0; k + 1 < h.size(); k += 2) out.push_back((char)strtoul(h.substr(k, 2).c_str(), nullptr, 16));
  return out;
}

static Item read_item(std::istream &in, bool with_hist) {
  Item it{};
  std::string name;
  int64_t hits, max_hits, newest, oldest;
  in >> name >> it.r.n_states >> hits >> max_hits >> newest >> oldest;
  it.name = unhex(name);
  it.r.hits = (uint64_t)hits;
  it.r.max_hits = bjx_names::key_of(max_hits);
  it.r.newest = bjx_names::key_of(newest);
  it.r.oldest_inv = ~bjx_names::key_of(oldest);
  if (with_hist)
    for (int b = 0; b < BJX_NAMES_HIST; ++b) in >> it.r.hist[b];
  return it;
}

static void print_row(const char *tag, const bjx_name_row &o, const uint8_t *bytes) {
  printf("%s ", tag);
  if (!o.name_len) printf("-");
  for (uint32_t k = 0; k < o.name_len; ++k) printf("%02x", bytes[o.name_off + k]);
  printf(" %" PRIu64 " %" PRId64 " %" PRId64 " %" PRId64 " %" PRId64, o.n_states, o.hits_sum, o.max_hits, o.newest_start_ns,
         o.oldest_start_ns);
  for (int b = 0; b < BJX_NAMES_HIST; ++b) printf(" %" PRIu64, o.hist[b]);
  printf("\n");
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
      bjx_names_spec s{};
      in >> s.order >> s.limit;
      const char *why = bjx_names::check_spec(&s);
      printf("spec %s\n", why ? why : "ok");
      if (bjx_names::check_spec(nullptr) == nullptr) return 3;
    } else if (cmd == "filter") {
      bjx_state_filter f{};
      std::string ip, name;
      in >> f.order >> f.limit >> ip >> name;
      if (ip == "N") f.ip.len = 3;
      else if (ip != "-") { f.ip.ptr = ip.data(); f.ip.len = ip.size(); }
      if (name == "N") f.name.len = 3;
      else if (name != "-") { f.name.ptr = name.data(); f.name.len = name.size(); }
      const char *why = bjx_names::check_filter(&f);
      printf("filter %s\n", why ? why : "ok");
      if (bjx_names::check_filter(nullptr) == nullptr) return 3;
    } else if (cmd == "bucket") {
      int64_t hits;
      in >> hits;
      printf("bucket %u\n", bjx_names::bucket(hits));
    } else if (cmd == "before") {
      uint32_t order;
      in >> order;
      const Item a = read_item(in, false), b = read_item(in, false);
      printf("before %d\n", bjx_names::row_before(a, b, order) ? 1 : 0);
    } else if (cmd == "acc") {
      size_t n;
      in >> n;
      Rec r{};
      for (size_t k = 0; k < n; ++k) {
        std::getline(file, line);
        std::istringstream rec(line);
        std::string tag;
        int64_t hits, start;
        rec >> tag >> hits >> start;
        if (tag != "s") return 3;
        bjx_names::add_state(&r, hits, start);
      }
      const uint8_t none = 0;
      print_row("acc", bjx_names::row_of(r, 0, 0), &none);
    } else if (cmd == "merge") {
      uint64_t cap;
      size_t n_lists;
      bjx_names_spec s{};
      in >> cap >> s.order >> s.limit >> s.min_states >> n_lists;
      std::vector<std::vector<Item>> lists(n_lists);
      bjx_names::Counts total;
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
          if (tag != "i") return 3;
          l.push_back(read_item(rec, true));
        }
        bjx_names::Counts c;
        c.n_matched = 7 * n; c.n_ips_matched = 3 * n;
        c.device_ms = (double)n;
        bjx_names::add(&total, c);
      }
      std::vector<Item> merged;
      if (!bjx_names::merge(lists, cap, &merged)) { printf("merge capacity\n"); continue; }
      for (size_t k = 1; k < merged.size(); ++k)
        if (!bjx_names::name_less(merged[k - 1].name, merged[k].name)) return 5;
      bjx_state_names out;
      std::vector<bjx_name_row> rows;
      std::vector<uint8_t> bytes;
      bjx_names::finish(merged, s, total, &out, &rows, &bytes);
      size_t n_all = 0, n_max = 0;
      for (auto &l : lists) { n_all += l.size(); n_max = l.size() > n_max ? l.size() : n_max; }
      if (out.n_matched != 7 * n_all || out.n_ips_matched != 3 * n_all || out.device_ms != (double)n_max ||
          out.n_rows != rows.size() || (out.rows != nullptr) != !rows.empty() || out.n_bytes != bytes.size())
        return 6;
      printf("merge %" PRIu64 " %" PRIu64 " %" PRIu64 "\n", out.n_names, out.n_names_min, out.n_rows);
      const uint8_t none = 0;
      for (const bjx_name_row &o : rows) print_row("r", o, bytes.empty() ? &none : bytes.data());
    } else if (!cmd.empty()) {
      return 2;
    }
  }
  return 0;
}
