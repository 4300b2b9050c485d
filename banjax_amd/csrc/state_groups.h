// Top networks by prefix (bjx_state_query_groups / bjx_node_state_query_groups,
// include/banjax_gpu.h; DESIGN.md §2 "Groups").  Host-only logic: the spec and
// filter checks, how a parsed address becomes a group key (family, masked
// address) and which bits of that key a sort has to look at, the group record
// the device writes, the order of the rows, and the node's merge of its
// shards' group lists with its cap.  engine.hip and node.cpp include it (the
// key kernel runs pack() per held IP); tests/cpu/groups_host.cpp builds it
// without a GPU.
//
// Group of an IP: the membership rule of the nets calls (state_nets.h).  The
// 16-byte form go_parse_addr gives is v4-mapped -> family 4, the address
// masked to v4_bits; every other address -> family 6, masked to v6_bits.  As a
// key, smaller first: (family 4 before 6, the masked address bytewise) -- one
// family bit above 128 address bits, an IPv4 address in the low 32 of them.
#ifndef BJX_STATE_GROUPS_H
#define BJX_STATE_GROUPS_H

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../../include/banjax_gpu.h"
#include "bjx_common.h"
#include "state_query.h"

namespace bjx_groups {

// the most groups a node merges on the host (56 bytes each while it does)
constexpr uint64_t kGroupsNodeMax = 1ull << 24;

// NULL when the call can be answered, else what is wrong with its arguments
inline const char *check_spec(const bjx_group_spec *g) {
  if (!g) return "no spec";
  if (g->v4_bits > 32) return "spec: v4_bits above 32";
  if (g->v6_bits > 128) return "spec: v6_bits above 128";
  if (g->order != BJX_GROUPS_BY_IPS && g->order != BJX_GROUPS_BY_STATES && g->order != BJX_GROUPS_BY_HITS)
    return "spec: order is not a bjx_group_order";
  if (g->limit > BJX_GROUPS_MAX_ROWS) return "spec: limit above BJX_GROUPS_MAX_ROWS";
  return nullptr;
}
// what bjx_state_query refuses in *f (order and limit change nothing else
// here), and a length without bytes as the nets calls refuse it
inline const char *check_filter(const bjx_state_filter *f) {
  if (const char *why = bjx_query::check_filter(f)) return why;
  if (f->ip.len && !f->ip.ptr) return "filter: ip with a length and no bytes";
  if (f->name.len && !f->name.ptr) return "filter: name with a length and no bytes";
  if ((uint64_t)f->ip.len >= (1ull << 32)) return "filter: ip of 2^32 bytes or more";
  return nullptr;
}

// ---- the key
BJX_HD uint32_t mask32(uint32_t bits) { return bits ? ~0u << (32 - bits) : 0u; }
BJX_HD uint64_t mask64(uint32_t bits) { return bits >= 64 ? ~0ull : (bits ? ~0ull << (64 - bits) : 0ull); }
BJX_HD uint64_t be64(const uint8_t *a) {
  uint64_t v = 0;
  for (int k = 0; k < 8; ++k) v = (v << 8) | a[k];
  return v;
}
// a: go_parse_addr's 16 bytes.  *fam6 0: IPv4, the masked address in the low
// 32 bits of *lo and *hi 0; 1: IPv6, (hi, lo) the masked address
BJX_HD void pack(const uint8_t a[16], uint32_t v4_bits, uint32_t v6_bits, uint32_t *fam6, uint64_t *hi, uint64_t *lo) {
  if (bjx::is_v4_mapped(a)) {
    const uint32_t ip = ((uint32_t)a[12] << 24) | ((uint32_t)a[13] << 16) | ((uint32_t)a[14] << 8) | a[15];
    *fam6 = 0; *hi = 0; *lo = ip & mask32(v4_bits);
    return;
  }
  *fam6 = 1;
  *hi = be64(a) & mask64(v6_bits);
  *lo = v6_bits > 64 ? be64(a + 8) & mask64(v6_bits - 64) : 0ull;
}

// The bits of the two key words in which keys can differ: [begin, end) of the
// low word and of the high word (begin == end: none, that sort is skipped).
// The low word holds IPv4's 32 bits and IPv6's last 64.
struct SortBits {
  int lo_begin = 0, lo_end = 0, hi_begin = 0, hi_end = 0;
};
inline SortBits sort_bits(uint32_t v4_bits, uint32_t v6_bits) {
  SortBits b;
  if (v6_bits > 64) { b.lo_begin = (int)(128 - v6_bits); b.lo_end = 64; }
  if (v4_bits) {
    if (b.lo_end == 0) { b.lo_begin = (int)(32 - v4_bits); b.lo_end = 32; }
    else b.lo_begin = std::min(b.lo_begin, (int)(32 - v4_bits));
  }
  if (v6_bits) { b.hi_begin = (int)(64 - std::min<uint32_t>(v6_bits, 64)); b.hi_end = 64; }
  return b;
}

// ---- one group, as the device writes it and the node merges it (56 B).
// n_ips is 64 bits wide: an engine holds fewer than 2^31 IPs, a node's /0
// group is the sum over its engines
struct Rec {
  uint64_t hi, lo;     // the masked address (pack)
  uint64_t n_states;
  uint64_t hits;       // the sum as two's complement: it wraps as Go's int does
  uint64_t newest;     // the largest start with its sign bit flipped (unsigned order = signed order)
  uint64_t n_ips;
  uint32_t fam6, _pad;
};
static_assert(sizeof(Rec) == 56, "bjx_groups::Rec is 56 bytes");
BJX_HD uint64_t start_key(int64_t v) { return (uint64_t)v ^ 0x8000000000000000ull; }
BJX_HD int64_t start_of(uint64_t key) { return (int64_t)(key ^ 0x8000000000000000ull); }

// key order: the order of an engine's list, and the rows' tie order
inline bool key_less(const Rec &a, const Rec &b) {
  if (a.fam6 != b.fam6) return a.fam6 < b.fam6;
  if (a.hi != b.hi) return a.hi < b.hi;
  return a.lo < b.lo;
}
inline bool key_same(const Rec &a, const Rec &b) { return a.fam6 == b.fam6 && a.hi == b.hi && a.lo == b.lo; }
// two parts of one group (an IP lives on one engine: the counts add up)
inline void combine(Rec *t, const Rec &s) {
  t->n_ips += s.n_ips;
  t->n_states += s.n_states;
  t->hits += s.hits;
  if (s.newest > t->newest) t->newest = s.newest;
}

inline bjx_group_row row_of(const Rec &r, const bjx_group_spec &g) {
  bjx_group_row o;
  memset(&o, 0, sizeof o);
  if (r.fam6) {
    for (int k = 0; k < 8; ++k) {
      o.addr[k] = (uint8_t)(r.hi >> (56 - 8 * k));
      o.addr[8 + k] = (uint8_t)(r.lo >> (56 - 8 * k));
    }
    o.family = 6; o.bits = g.v6_bits;
  } else {
    for (int k = 0; k < 4; ++k) o.addr[k] = (uint8_t)(r.lo >> (24 - 8 * k));
    o.family = 4; o.bits = g.v4_bits;
  }
  o.n_ips = r.n_ips; o.n_states = r.n_states;
  o.hits_sum = (int64_t)r.hits;
  o.newest_start_ns = start_of(r.newest);
  return o;
}

// ---- the order of the rows: the primary key descending, then key order
// a before b by the primary key alone
inline bool primary_before(const Rec &a, const Rec &b, uint32_t order) {
  if (order == BJX_GROUPS_BY_IPS) return a.n_ips > b.n_ips;
  if (order == BJX_GROUPS_BY_STATES) return a.n_states > b.n_states;
  return (int64_t)a.hits > (int64_t)b.hits;
}
inline bool row_before(const Rec &a, const Rec &b, uint32_t order) {
  if (primary_before(a, b, order)) return true;
  if (primary_before(b, a, order)) return false;
  return key_less(a, b);
}

// what a groups query counts besides its groups
struct Counts {
  uint64_t n_matched = 0, n_ips_matched = 0, n_ips_unparsed = 0, n_states_unparsed = 0;
  double device_ms = 0;
};
inline void add(Counts *t, const Counts &s) {
  t->n_matched += s.n_matched; t->n_ips_matched += s.n_ips_matched;
  t->n_ips_unparsed += s.n_ips_unparsed; t->n_states_unparsed += s.n_states_unparsed;
  if (s.device_ms > t->device_ms) t->device_ms = s.device_ms;
}

// ---- the node's merge.  Every list is complete and in key order; a group
// may appear in several (the owner of an IP is a hash of its bytes).  false,
// and *out unspecified, when the lists together hold more than cap groups.
inline bool merge(const std::vector<std::vector<Rec>> &lists, uint64_t cap, std::vector<Rec> *out) {
  uint64_t total = 0;
  for (const auto &l : lists) total += l.size();
  if (total > cap) return false;
  std::vector<Rec> all;
  all.reserve(total);
  for (const auto &l : lists) all.insert(all.end(), l.begin(), l.end());
  if (lists.size() > 1) std::stable_sort(all.begin(), all.end(), key_less);
  out->clear();
  for (const Rec &r : all) {
    if (!out->empty() && key_same(out->back(), r)) combine(&out->back(), r);
    else out->push_back(r);
  }
  return true;
}

// From a complete list in key order to the answer: min_ips, the order, the
// limit.  rows receives the rows; out's counts come from c.
inline void finish(const std::vector<Rec> &list, const bjx_group_spec &g, const Counts &c, bjx_state_groups *out,
                   std::vector<bjx_group_row> *rows) {
  std::vector<Rec> pass;
  for (const Rec &r : list)
    if (r.n_ips >= g.min_ips) pass.push_back(r);
  memset(out, 0, sizeof *out);
  out->n_matched = c.n_matched; out->n_ips_matched = c.n_ips_matched;
  out->n_ips_unparsed = c.n_ips_unparsed; out->n_states_unparsed = c.n_states_unparsed;
  out->n_groups = list.size();
  out->n_groups_min = pass.size();
  out->device_ms = c.device_ms;
  // (key order is the tie order, so a stable sort by the primary key alone)
  const uint32_t order = g.order;
  std::stable_sort(pass.begin(), pass.end(), [order](const Rec &a, const Rec &b) { return primary_before(a, b, order); });
  if (pass.size() > g.limit) pass.resize(g.limit);
  rows->clear();
  for (const Rec &r : pass) rows->push_back(row_of(r, g));
  out->n_rows = rows->size();
  out->rows = rows->empty() ? nullptr : rows->data();
}

}  // namespace bjx_groups

// One engine's complete group list as the node asks for it (engine.hip; not
// part of the C ABI): every group of the selection in key order, min_ips,
// order and limit not applied.  BJX_ERR_CAPACITY, before anything is copied,
// when the engine alone holds more than `room` groups.  Takes the engine lock.
int bjx_groups_list(bjx_engine *e, const bjx_state_filter *f, const bjx_group_spec *g, uint64_t room,
                    std::vector<bjx_groups::Rec> *list, bjx_groups::Counts *counts);

#endif  // BJX_STATE_GROUPS_H
