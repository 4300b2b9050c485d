// Per-rule-name totals over the state (bjx_state_query_names /
// bjx_node_state_query_names, include/banjax_gpu.h; DESIGN.md §2 "Names").
// Host-only logic: the spec and filter checks, the histogram bucket of a hit
// count, the record the device writes per name, the order of the rows, and
// the node's merge of its shards' lists by name bytes with its cap.
// engine.hip and node.cpp include it (the scan kernel runs bucket() per
// state); tests/cpu/names_host.cpp builds it without a GPU.
#ifndef BJX_STATE_NAMES_H
#define BJX_STATE_NAMES_H

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/banjax_gpu.h"
#include "bjx_common.h"
#include "state_query.h"

namespace bjx_names {

// the most names a node merges on the host (a record and the name's bytes each while it does)
constexpr uint64_t kNamesNodeMax = 1ull << 20;

// NULL when the call can be answered, else what is wrong with its arguments
inline const char *check_spec(const bjx_names_spec *s) {
  if (!s) return "no spec";
  if (s->order > BJX_NAMES_BY_NAME) return "spec: order is not a bjx_names_order";
  if (s->limit > BJX_NAMES_MAX_ROWS) return "spec: limit above BJX_NAMES_MAX_ROWS";
  return nullptr;
}
// what bjx_state_query refuses in *f (order and limit change nothing else
// here), and a length without bytes as the groups call refuses it
inline const char *check_filter(const bjx_state_filter *f) {
  if (const char *why = bjx_query::check_filter(f)) return why;
  if (f->ip.len && !f->ip.ptr) return "filter: ip with a length and no bytes";
  if (f->name.len && !f->name.ptr) return "filter: name with a length and no bytes";
  if ((uint64_t)f->ip.len >= (1ull << 32)) return "filter: ip of 2^32 bytes or more";
  return nullptr;
}

// ---- the histogram: bucket 0 holds hits <= 0, bucket b the hits of bit
// length b (2^(b-1) <= hits < 2^b), bucket 15 everything from 2^14 on
BJX_HD uint32_t bucket(int64_t hits) {
  if (hits <= 0) return 0;
  const uint32_t len = 64u - (uint32_t)__builtin_clzll((unsigned long long)hits);
  return len < BJX_NAMES_HIST - 1 ? len : BJX_NAMES_HIST - 1;
}

// a signed value as an unsigned key of the same order, and back
BJX_HD uint64_t key_of(int64_t v) { return (uint64_t)v ^ 0x8000000000000000ull; }
BJX_HD int64_t value_of(uint64_t key) { return (int64_t)(key ^ 0x8000000000000000ull); }

// ---- one name, as the device accumulates it, compacts it and the node
// merges it (176 B).  Every field starts at zero and only grows under
// add / max, so a memset prepares it: the extrema are kept as keys (key_of),
// the oldest start as the complement of its key, so that it is a maximum too
struct Rec {
  uint64_t hits;        // the sum as two's complement: it wraps as Go's int does
  uint64_t max_hits;    // key_of(the largest hits)
  uint64_t newest;      // key_of(the largest start)
  uint64_t oldest_inv;  // ~key_of(the smallest start)
  uint64_t hist[BJX_NAMES_HIST];
  uint64_t n_states;    // the histogram's sum (written by the compaction)
  uint32_t id, _pad;    // the engine's name id (written by the compaction)
};
static_assert(sizeof(Rec) == 176, "bjx_names::Rec is 176 bytes");

// one state into a record (the model of what the scan does with atomics)
inline void add_state(Rec *t, int64_t hits, int64_t start) {
  t->hits += (uint64_t)hits;
  t->max_hits = std::max(t->max_hits, key_of(hits));
  t->newest = std::max(t->newest, key_of(start));
  t->oldest_inv = std::max(t->oldest_inv, ~key_of(start));
  t->hist[bucket(hits)] += 1;
  t->n_states += 1;
}
// two parts of one name (an (ip, name) state lives on one engine: the counts add up)
inline void combine(Rec *t, const Rec &s) {
  t->hits += s.hits;
  t->max_hits = std::max(t->max_hits, s.max_hits);
  t->newest = std::max(t->newest, s.newest);
  t->oldest_inv = std::max(t->oldest_inv, s.oldest_inv);
  for (int b = 0; b < BJX_NAMES_HIST; ++b) t->hist[b] += s.hist[b];
  t->n_states += s.n_states;
}

// a record with its name's bytes: what the engine hands to the node and what the rows are made of
struct Item {
  std::string name;
  Rec r;
};

// ---- the order of the rows: the primary key descending, then the name
// bytewise ascending, a prefix before the longer name (std::string's order
// compares as unsigned bytes)
inline bool primary_before(const Rec &a, const Rec &b, uint32_t order) {
  switch (order) {
    case BJX_NAMES_BY_STATES: return a.n_states > b.n_states;
    case BJX_NAMES_BY_HITS: return (int64_t)a.hits > (int64_t)b.hits;
    case BJX_NAMES_BY_MAX_HITS: return a.max_hits > b.max_hits;
    case BJX_NAMES_BY_NEWEST: return a.newest > b.newest;
    default: return false;  // BJX_NAMES_BY_NAME: the name alone
  }
}
inline bool name_less(const std::string &a, const std::string &b) {
  const size_t n = std::min(a.size(), b.size());
  const int c = n ? memcmp(a.data(), b.data(), n) : 0;
  return c != 0 ? c < 0 : a.size() < b.size();
}
inline bool row_before(const Item &a, const Item &b, uint32_t order) {
  if (primary_before(a.r, b.r, order)) return true;
  if (primary_before(b.r, a.r, order)) return false;
  return name_less(a.name, b.name);
}

// what a names query counts besides its names
struct Counts {
  uint64_t n_matched = 0, n_ips_matched = 0;
  double device_ms = 0;
};
inline void add(Counts *t, const Counts &s) {
  t->n_matched += s.n_matched; t->n_ips_matched += s.n_ips_matched;
  if (s.device_ms > t->device_ms) t->device_ms = s.device_ms;
}

// ---- the node's merge.  Every list is complete, in any order, and holds a
// name once; a name may appear in several lists.  false, and *out
// unspecified, when the lists together hold more than cap names.
inline bool merge(const std::vector<std::vector<Item>> &lists, uint64_t cap, std::vector<Item> *out) {
  uint64_t total = 0;
  for (const auto &l : lists) total += l.size();
  if (total > cap) return false;
  std::vector<Item> all;
  all.reserve(total);
  for (const auto &l : lists) all.insert(all.end(), l.begin(), l.end());
  std::stable_sort(all.begin(), all.end(), [](const Item &a, const Item &b) { return name_less(a.name, b.name); });
  out->clear();
  for (Item &it : all) {
    if (!out->empty() && out->back().name == it.name) combine(&out->back().r, it.r);
    else out->push_back(std::move(it));
  }
  return true;
}

inline bjx_name_row row_of(const Rec &r, uint64_t name_off, uint32_t name_len) {
  bjx_name_row o;
  memset(&o, 0, sizeof o);
  o.name_off = name_off; o.name_len = name_len;
  o.n_states = r.n_states;
  o.hits_sum = (int64_t)r.hits;
  o.max_hits = value_of(r.max_hits);
  o.newest_start_ns = value_of(r.newest);
  o.oldest_start_ns = value_of(~r.oldest_inv);
  for (int b = 0; b < BJX_NAMES_HIST; ++b) o.hist[b] = r.hist[b];
  return o;
}

// From a complete list (a name once, any order) to the answer: min_states,
// the order, the limit.  rows and bytes receive the rows and their names;
// out's counts come from c.
inline void finish(std::vector<Item> list, const bjx_names_spec &s, const Counts &c, bjx_state_names *out,
                   std::vector<bjx_name_row> *rows, std::vector<uint8_t> *bytes) {
  memset(out, 0, sizeof *out);
  out->n_matched = c.n_matched; out->n_ips_matched = c.n_ips_matched;
  out->n_names = list.size();
  out->device_ms = c.device_ms;
  const uint64_t min_states = s.min_states;
  list.erase(std::remove_if(list.begin(), list.end(), [min_states](const Item &a) { return a.r.n_states < min_states; }), list.end());
  out->n_names_min = list.size();
  const uint32_t order = s.order;
  std::sort(list.begin(), list.end(), [order](const Item &a, const Item &b) { return row_before(a, b, order); });
  if (list.size() > s.limit) list.resize(s.limit);
  rows->clear();
  bytes->clear();
  for (const Item &it : list) {
    rows->push_back(row_of(it.r, bytes->size(), (uint32_t)it.name.size()));
    bytes->insert(bytes->end(), it.name.begin(), it.name.end());
  }
  out->n_rows = rows->size();
  out->rows = rows->empty() ? nullptr : rows->data();
  out->bytes = bytes->empty() ? nullptr : bytes->data();
  out->n_bytes = bytes->size();
}

}  // namespace bjx_names

// One engine's complete name list as the node asks for it (engine.hip; not
// part of the C ABI): every name with a selected state, in no particular
// order, min_states, order and limit not applied.  BJX_ERR_CAPACITY, before
// anything is copied, when the engine alone holds more than `room` names.
// Takes the engine lock.
int bjx_names_list(bjx_engine *e, const bjx_state_filter *f, const bjx_names_spec *s, uint64_t room,
                   std::vector<bjx_names::Item> *list, bjx_names::Counts *counts);

#endif  // BJX_STATE_NAMES_H
