// Host build of the state query's host parts (banjax_amd/csrc/state_query.h)
// for tests/test_state_query_cpu.py: a stand-alone program that reads commands
// from the file given as argv[1] and prints one answer per command (also the
// sanitizer run).  Strings travel as hex, "-" for the empty string.
//   filter <order> <limit>                    -> "filter ok" | "filter <message>"
//   key <int64>...                            -> "key <u64>..."  (key_desc)
//   ranks <name>...                           -> "ranks <rank of each name>"
//   merge <order> <limit> <n_shards>, then per shard
//     shard <n_matched> <n_ips_matched> <n_rows> <device_ms>
//     row <ip> <name> <hits> <start_ns>       (n_rows of them)
//                                             -> "merged <n_matched> <n_ips_matched> <n_rows> <device_ms>"
//                                                and "row <ip> <name> <hits> <start_ns>" per row
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>

#include <fstream>
#include <sstream>

#include "../../banjax_amd/csrc/state_query.h"

static std::string unhex(const std::string &h) {
  std::string out;
  if (h == "-") return out;
  for (size_t k = 0; k + 1 < h.size(); k += 2) out.push_back((char)strtoul(h.substr(k, 2).c_str(), nullptr, 16));
  return out;
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
    if (cmd == "filter") {
      bjx_state_filter f{};
      ls >> f.order >> f.limit;
      const char *why = bjx_query::check_filter(&f);
      printf("filter %s\n", why ? why : "ok");
    } else if (cmd == "key") {
      printf("key");
      for (int64_t v; ls >> v;) printf(" %" PRIu64, bjx_query::key_desc(v));
      printf("\n");
    } else if (cmd == "ranks") {
      std::vector<std::string> names;
      for (std::string h; ls >> h;) names.push_back(unhex(h));
      std::vector<uint32_t> rank, by_rank;
      bjx_query::name_ranks(names, &rank, &by_rank);
      printf("ranks");
      for (size_t k = 0; k < names.size(); ++k) {
        if (by_rank[rank[k]] != k) return 3;
        printf(" %u", rank[k]);
      }
      printf("\n");
    } else if (cmd == "merge") {
      uint32_t order = 0, limit = 0, n_shards = 0;
      ls >> order >> limit >> n_shards;
      // exact-size storage per shard: a read past a shard's rows or bytes is a read past an allocation
      std::vector<std::vector<bjx_state_row>> rows(n_shards);
      std::vector<std::vector<uint8_t>> bytes(n_shards);
      std::vector<bjx_state_rows> ans(n_shards);
      for (uint32_t s = 0; s < n_shards; ++s) {
        if (!std::getline(in, line)) return 2;
        std::istringstream hs(line);
        bjx_state_rows a{};
        hs >> cmd >> a.n_matched >> a.n_ips_matched >> a.n_rows >> a.device_ms;
        if (cmd != "shard") return 2;
        std::vector<bjx_state_row> rr;
        std::vector<uint8_t> bb;
        for (uint64_t r = 0; r < a.n_rows; ++r) {
          if (!std::getline(in, line)) return 2;
          std::istringstream rs(line);
          std::string ip, name;
          bjx_state_row w{};
          rs >> cmd >> ip >> name >> w.hits >> w.start_ns;
          if (cmd != "row") return 2;
          ip = unhex(ip);
          name = unhex(name);
          // name first, then IP: the merge may not assume the engine's layout of the bytes
          w.name_off = bb.size(); w.name_len = (uint32_t)name.size();
          bb.insert(bb.end(), name.begin(), name.end());
          w.ip_off = bb.size(); w.ip_len = (uint32_t)ip.size();
          bb.insert(bb.end(), ip.begin(), ip.end());
          rr.push_back(w);
        }
        rows[s].assign(rr.begin(), rr.end());
        rows[s].shrink_to_fit();
        bytes[s].assign(bb.begin(), bb.end());
        bytes[s].shrink_to_fit();
        a.rows = rows[s].empty() ? nullptr : rows[s].data();
        a.bytes = bytes[s].empty() ? nullptr : bytes[s].data();
        a.n_bytes = bytes[s].size();
        ans[s] = a;
      }
      bjx_state_rows out{};
      std::vector<bjx_state_row> mr;
      std::vector<uint8_t> mb;
      bjx_query::merge(ans, order, limit, &out, &mr, &mb);
      printf("merged %" PRIu64 " %" PRIu64 " %" PRIu64 " %g\n", out.n_matched, out.n_ips_matched, out.n_rows, out.device_ms);
      for (uint64_t r = 0; r < out.n_rows; ++r) {
        const bjx_state_row &w = out.rows[r];
        if (w.ip_off + w.ip_len > out.n_bytes || w.name_off + w.name_len > out.n_bytes) return 3;
        printf("row %s %s %" PRId64 " %" PRId64 "\n", hex(w.ip_len ? out.bytes + w.ip_off : nullptr, w.ip_len).c_str(),
               hex(w.name_len ? out.bytes + w.name_off : nullptr, w.name_len).c_str(), w.hits, w.start_ns);
      }
    } else {
      return 2;
    }
  }
  return 0;
}
