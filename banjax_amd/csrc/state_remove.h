// State removal (bjx_state_remove / bjx_node_state_remove, include/banjax_gpu.h;
// DESIGN.md §2 "Remove").  Host-only: the argument checks, the packed IP list
// the engine uploads, the meaning of the filter's ip together with a list, and
// the node's sum of its shards' stats.  engine.hip and node.cpp include it;
// tests/cpu/remove_host.cpp builds it without a GPU.
#ifndef BJX_STATE_REMOVE_H
#define BJX_STATE_REMOVE_H

#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/banjax_gpu.h"

namespace bjx_remove {

constexpr uint64_t kMaxListBytes = 1ull << 32;    // the list's bytes in total stay below this (u32 offsets)
constexpr uint64_t kMaxListEntries = 0xFFFFFFFEull;  // entries + the filter's ip + the end offset fit u32 indices

// NULL when the call can be answered, else what is wrong with its arguments.
// Only the lengths are read: no entry's bytes are touched before this passes.
inline const char *check_args(const bjx_state_filter *f, const bjx_str *ips, size_t n_ips) {
  if (!f) return "no filter";
  if (f->ip.len && !f->ip.ptr) return "filter: ip with a length and no bytes";
  if (f->name.len && !f->name.ptr) return "filter: name with a length and no bytes";
  if (n_ips && !ips) return "ips: a count and no list";
  if ((uint64_t)n_ips > kMaxListEntries) return "ips: 2^32 entries or more";
  uint64_t total = f->ip.ptr ? (uint64_t)f->ip.len : 0;
  if (total >= kMaxListBytes) return "filter: ip of 2^32 bytes or more";
  for (size_t k = 0; k < n_ips; ++k) {
    if (ips[k].len && !ips[k].ptr) return "ips: an entry with a length and no bytes";
    if ((uint64_t)ips[k].len >= kMaxListBytes - total) return "ips: 2^32 bytes or more in total";
    total += ips[k].len;
  }
  return nullptr;
}

// The list as the device reads it: entry k is bytes[off[k], off[k + 1]).
// Entries [0, n_list) are the caller's list as given (duplicates and empty
// entries included); with a filter ip one more entry follows, that IP, at
// index n_list (has_ip).
//
// What restricts the selection (the list and the filter's ip mean both):
//   no list, no ip   nothing does (restrict == false)
//   ip alone         entry n_list
//   list alone       entries [0, n_list)
//   both             entry n_list when the list holds those bytes, else no IP
//                    can be selected (nothing == true)
struct List {
  std::vector<uint32_t> off;
  std::vector<uint8_t> bytes;
  uint32_t n_list = 0;
  bool has_ip = false, restrict = false, nothing = false;
  uint32_t sel_first = 0, sel_count = 0;  // the entries an IP must be among (restrict && !nothing)
  uint32_t n_entries() const { return n_list + (has_ip ? 1u : 0u); }
};

// check_args passed
inline void pack(const bjx_state_filter &f, const bjx_str *ips, size_t n_ips, List *L) {
  *L = List{};
  L->n_list = (uint32_t)n_ips;
  L->has_ip = f.ip.ptr != nullptr;
  uint64_t total = L->has_ip ? f.ip.len : 0;
  for (size_t k = 0; k < n_ips; ++k) total += ips[k].len;
  L->off.reserve(n_ips + 2);
  L->bytes.reserve(total);
  bool listed = false;
  for (size_t k = 0; k < n_ips; ++k) {
    L->off.push_back((uint32_t)L->bytes.size());
    if (ips[k].len) L->bytes.insert(L->bytes.end(), (const uint8_t *)ips[k].ptr, (const uint8_t *)ips[k].ptr + ips[k].len);
    if (L->has_ip && ips[k].len == f.ip.len && (!f.ip.len || !memcmp(ips[k].ptr, f.ip.ptr, f.ip.len))) listed = true;
  }
  if (L->has_ip) {
    L->off.push_back((uint32_t)L->bytes.size());
    if (f.ip.len) L->bytes.insert(L->bytes.end(), (const uint8_t *)f.ip.ptr, (const uint8_t *)f.ip.ptr + f.ip.len);
  }
  L->off.push_back((uint32_t)L->bytes.size());
  L->restrict = L->has_ip || n_ips != 0;
  if (L->has_ip) {
    L->nothing = n_ips != 0 && !listed;
    L->sel_first = L->n_list;
    L->sel_count = 1;
  } else {
    L->sel_count = L->n_list;
  }
}

// The node's sum: an IP lives on one shard, so counts and bytes add up
// exactly; device_ms is the slowest shard's.
inline void add(bjx_remove_stats *t, const bjx_remove_stats &s) {
  t->states_before += s.states_before; t->states_dropped += s.states_dropped;
  t->ips_before += s.ips_before; t->ips_dropped += s.ips_dropped;
  t->ips_found += s.ips_found;
  t->arena_bytes_before += s.arena_bytes_before; t->arena_bytes_after += s.arena_bytes_after;
  t->device_bytes_before += s.device_bytes_before; t->device_bytes_after += s.device_bytes_after;
  if (s.device_ms > t->device_ms) t->device_ms = s.device_ms;
}

}  // namespace bjx_remove

#endif  // BJX_STATE_REMOVE_H
