// State query (bjx_state_query / bjx_node_state_query, include/banjax_gpu.h;
// DESIGN.md §2 "Query").  Host-only: the filter checks, the sort key, the
// name-rank table and the node's merge of its shards' answers.  engine.hip and
// node.cpp include it; tests/cpu/query_host.cpp builds it without a GPU.
//
// Order of the rows (total, a function of the logical state alone): primary
// key descending (hits or interval_start_ns), then IP in first-seen order
// ascending, then rule name bytewise ascending.  As one 128-bit key, smaller
// first: {key_desc(primary), ip id << 24 | rank(name)}.
#ifndef BJX_STATE_QUERY_H
#define BJX_STATE_QUERY_H

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <numeric>
#include <string>
#include <vector>

#include "../../include/banjax_gpu.h"

namespace bjx_query {

// NULL when the filter can be answered, else what is wrong with it
inline const char *check_filter(const bjx_state_filter *f) {
  if (!f) return "no filter";
  if (f->limit > BJX_QUERY_MAX_ROWS) return "limit: more than BJX_QUERY_MAX_ROWS rows";
  if (f->order != BJX_QUERY_BY_HITS && f->order != BJX_QUERY_BY_START) return "order: not a bjx_query_order";
  return nullptr;
}

// no state can pass (not an error: zero rows, zero counts)
inline bool empty_window(const bjx_state_filter &f) { return f.min_start_ns > f.max_start_ns; }

// int64 -> u64 whose ascending order is the value's descending order (the
// sign bit flipped makes the order unsigned, the complement turns it round)
#ifdef __HIPCC__
__host__ __device__
#endif
inline uint64_t key_desc(int64_t v) { return ~((uint64_t)v ^ 0x8000000000000000ull); }

// rank[id] = position of names[id] among all the names sorted bytewise
// (std::string compares as unsigned bytes, shorter first on a common prefix);
// by_rank[r] = the id at position r
inline void name_ranks(const std::vector<std::string> &names, std::vector<uint32_t> *rank, std::vector<uint32_t> *by_rank) {
  by_rank->resize(names.size());
  std::iota(by_rank->begin(), by_rank->end(), 0u);
  std::sort(by_rank->begin(), by_rank->end(), [&](uint32_t a, uint32_t b) { return names[a] < names[b]; });
  rank->assign(names.size(), 0);
  for (uint32_t r = 0; r < by_rank->size(); ++r) (*rank)[(*by_rank)[r]] = r;
}

// The node's merge.  Every shard answered the same filter and limit, its rows
// in the order above; an IP lives on one shard and the global first-seen order
// is shard-major, so among equal primaries shard k's rows come before shard
// k + 1's and each shard's stay as they are: a stable sort of the
// concatenation by the primary key alone.  The global first `limit` states are
// among the shards' first `limit` each.  Counts are summed, device_ms is the
// slowest shard's.  rows / bytes receive the merged answer (offsets rebased).
inline void merge(const std::vector<bjx_state_rows> &shards, uint32_t order, uint32_t limit, bjx_state_rows *out,
                  std::vector<bjx_state_row> *rows, std::vector<uint8_t> *bytes) {
  struct Ref { uint32_t shard; uint32_t row; int64_t primary; };
  std::vector<Ref> all;
  bjx_state_rows t{};
  for (uint32_t s = 0; s < shards.size(); ++s) {
    const bjx_state_rows &a = shards[s];
    t.n_matched += a.n_matched;
    t.n_ips_matched += a.n_ips_matched;
    if (a.device_ms > t.device_ms) t.device_ms = a.device_ms;
    for (uint64_t r = 0; r < a.n_rows; ++r)
      all.push_back({s, (uint32_t)r, order == BJX_QUERY_BY_START ? a.rows[r].start_ns : a.rows[r].hits});
  }
  std::stable_sort(all.begin(), all.end(), [](const Ref &a, const Ref &b) { return a.primary > b.primary; });
  if (all.size() > limit) all.resize(limit);
  rows->clear();
  bytes->clear();
  for (const Ref &x : all) {
    const bjx_state_rows &a = shards[x.shard];
    bjx_state_row r = a.rows[x.row];
    const uint64_t io = r.ip_off, no = r.name_off;
    if (io > a.n_bytes || r.ip_len > a.n_bytes - io || no > a.n_bytes || r.name_len > a.n_bytes - no) continue;  // (never)
    r.ip_off = bytes->size();
    bytes->insert(bytes->end(), a.bytes + io, a.bytes + io + r.ip_len);
    r.name_off = bytes->size();
    bytes->insert(bytes->end(), a.bytes + no, a.bytes + no + r.name_len);
    rows->push_back(r);
  }
  t.n_rows = rows->size();
  t.rows = rows->empty() ? nullptr : rows->data();
  t.bytes = bytes->empty() ? nullptr : bytes->data();
  t.n_bytes = bytes->size();
  *out = t;
}

}  // namespace bjx_query

#endif  // BJX_STATE_QUERY_H
