// State snapshot, format version 1 (bjx_state_export / bjx_state_import,
// include/banjax_gpu.h; DESIGN.md §2 "Snapshot").  Host-only: the layout, the
// host part of the validation (header, section arithmetic, names) and the
// node's merge of its shards' snapshots.  engine.hip and node.cpp include it;
// tests/cpu/snapshot_host.cpp builds it without a GPU.
//
// Little-endian.  Header, 64 bytes:
//   magic[8] "BJXSTATE", u32 version = 1, u32 header_bytes = 64,
//   u64 total_bytes, n_names, names_bytes, n_ips, ip_bytes, n_states
// then five sections, each padded with zeros to 8 bytes:
//   u64 name_off[n_names + 1] | name bytes | u64 ip_off[n_ips + 1] | IP bytes |
//   n_states records {u32 ip, u32 name, i64 hits, i64 start}
// Canonical form: names sorted bytewise, distinct, each used by a record; every
// IP has a record; records strictly ascending by (ip, name).
#ifndef BJX_SNAPSHOT_H
#define BJX_SNAPSHOT_H

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

namespace bjx_snap {

constexpr uint32_t kVersion = 1, kHeaderBytes = 64, kRecBytes = 24;
constexpr uint64_t kMaxNames = 1ull << 24, kMaxIps = 0x7FFFFFFFull, kMaxStates = 0x7FFFFFFFull;
static const char kMagic[9] = "BJXSTATE";

struct Rec {
  uint32_t ip, name;
  int64_t hits, start;
};
static_assert(sizeof(Rec) == kRecBytes, "snapshot record is 24 bytes");

inline uint64_t pad8(uint64_t x) { return (x + 7) & ~7ull; }
inline uint64_t rd64(const uint8_t *p) { uint64_t v; memcpy(&v, p, 8); return v; }
inline uint32_t rd32(const uint8_t *p) { uint32_t v; memcpy(&v, p, 4); return v; }
inline void wr64(uint8_t *p, uint64_t v) { memcpy(p, &v, 8); }
inline void wr32(uint8_t *p, uint32_t v) { memcpy(p, &v, 4); }

// section offsets of a snapshot with the given counts
struct Layout {
  uint64_t n_names = 0, names_bytes = 0, n_ips = 0, ip_bytes = 0, n_states = 0;
  uint64_t o_name_off = 0, o_names = 0, o_ip_off = 0, o_ips = 0, o_recs = 0, total = 0;
};

// false: a count over its limit or sizes that overflow u64 (*why names which)
inline bool make_layout(uint64_t n_names, uint64_t names_bytes, uint64_t n_ips, uint64_t ip_bytes, uint64_t n_states,
                        Layout *L, const char **why) {
  if (n_names >= kMaxNames) { *why = "n_names limit: 2^24 names or more"; return false; }
  if (n_ips >= kMaxIps) { *why = "n_ips limit: 2^31 IPs or more"; return false; }
  if (n_states >= kMaxStates) { *why = "n_states limit: 2^31 states or more"; return false; }
  // the three counted sections are below 2^36 bytes each; the byte sections may not wrap the sum
  const uint64_t fixed = kHeaderBytes + 8 * (n_names + 1) + 8 * (n_ips + 1) + kRecBytes * n_states;
  const uint64_t room = ~0ull - fixed - 16;
  if (names_bytes > room || ip_bytes > room - names_bytes) { *why = "section sizes overflow u64"; return false; }
  L->n_names = n_names; L->names_bytes = names_bytes; L->n_ips = n_ips; L->ip_bytes = ip_bytes; L->n_states = n_states;
  L->o_name_off = kHeaderBytes;
  L->o_names = L->o_name_off + 8 * (n_names + 1);
  L->o_ip_off = L->o_names + pad8(names_bytes);
  L->o_ips = L->o_ip_off + 8 * (n_ips + 1);
  L->o_recs = L->o_ips + pad8(ip_bytes);
  L->total = L->o_recs + kRecBytes * n_states;
  return true;
}

inline void write_header(uint8_t *out, const Layout &L) {
  memcpy(out, kMagic, 8);
  wr32(out + 8, kVersion);
  wr32(out + 12, kHeaderBytes);
  wr64(out + 16, L.total);
  wr64(out + 24, L.n_names);
  wr64(out + 32, L.names_bytes);
  wr64(out + 40, L.n_ips);
  wr64(out + 48, L.ip_bytes);
  wr64(out + 56, L.n_states);
}

// name_off section and the padded name bytes of `names` (sorted by the caller)
inline void write_names(uint8_t *out, const Layout &L, const std::vector<std::string> &names) {
  uint64_t off = 0;
  for (size_t k = 0; k < names.size(); ++k) {
    wr64(out + L.o_name_off + 8 * k, off);
    if (!names[k].empty()) memcpy(out + L.o_names + off, names[k].data(), names[k].size());
    off += names[k].size();
  }
  wr64(out + L.o_name_off + 8 * names.size(), off);
  memset(out + L.o_names + off, 0, pad8(off) - off);
}

// Host part of the validation: header, section arithmetic, names.  Returns
// NULL when it passes (L filled, names appended if asked for), else a message
// that names the failed check.  ip_off and the records are checked by the
// importer on the device (k_imp_check) or by check_body below.
inline const char *validate_host(const uint8_t *p, uint64_t len, Layout *L, std::vector<std::string> *names) {
  if (!p || len < kHeaderBytes) return "header: shorter than 64 bytes";
  if (memcmp(p, kMagic, 8) != 0) return "magic: not BJXSTATE";
  if (rd32(p + 8) != kVersion) return "version: not 1";
  if (rd32(p + 12) != kHeaderBytes) return "header_bytes: not 64";
  if (rd64(p + 16) != len) return "total_bytes: does not equal the length given";
  const char *why = nullptr;
  if (!make_layout(rd64(p + 24), rd64(p + 32), rd64(p + 40), rd64(p + 48), rd64(p + 56), L, &why)) return why;
  if (L->total != len) return "section sizes: do not add up to total_bytes";
  if (L->n_ips && !L->n_states) return "records: an IP without a record";
  if (!L->n_ips && L->n_states) return "records: a record without an IP";
  const uint8_t *no = p + L->o_name_off, *nb = p + L->o_names;
  if (rd64(no) != 0) return "name_off: does not start at 0";
  for (uint64_t k = 0; k < L->n_names; ++k) {
    const uint64_t a = rd64(no + 8 * k), b = rd64(no + 8 * (k + 1));
    if (b < a || b > L->names_bytes) return "name_off: not monotone inside names_bytes";
  }
  if (rd64(no + 8 * L->n_names) != L->names_bytes) return "name_off: does not end at names_bytes";
  for (uint64_t k = 1; k < L->n_names; ++k) {
    const uint64_t a = rd64(no + 8 * (k - 1)), b = rd64(no + 8 * k), c = rd64(no + 8 * (k + 1));
    const uint64_t la = b - a, lb = c - b;
    const int cmp = memcmp(nb + a, nb + b, (size_t)std::min(la, lb));
    if (cmp == 0 && la == lb) return "names: duplicate name";
    if (cmp > 0 || (cmp == 0 && la > lb)) return "names: not sorted";
  }
  for (uint64_t k = L->names_bytes; k < pad8(L->names_bytes); ++k)
    if (nb[k]) return "padding: name bytes not padded with zeros";
  for (uint64_t k = L->ip_bytes; k < pad8(L->ip_bytes); ++k)
    if (p[L->o_ips + k]) return "padding: IP bytes not padded with zeros";
  if (names) {
    names->clear();
    for (uint64_t k = 0; k < L->n_names; ++k) {
      const uint64_t a = rd64(no + 8 * k), b = rd64(no + 8 * (k + 1));
      names->emplace_back(reinterpret_cast<const char *>(nb + a), (size_t)(b - a));
    }
  }
  return nullptr;
}

// The checks the importer runs on the device, on the host (the node's merge
// reads its own engines' exports through it; tests compare the two).
inline const char *check_body(const uint8_t *p, const Layout &L) {
  const uint8_t *io = p + L.o_ip_off, *rc = p + L.o_recs;
  if (rd64(io) != 0) return "ip_off: does not start at 0";
  for (uint64_t k = 0; k < L.n_ips; ++k)
    if (rd64(io + 8 * (k + 1)) < rd64(io + 8 * k)) return "ip_off: not monotone";
  if (rd64(io + 8 * L.n_ips) != L.ip_bytes) return "ip_off: does not end at ip_bytes";
  std::vector<uint8_t> used(L.n_names, 0);
  uint32_t pi = 0, pn = 0;
  for (uint64_t j = 0; j < L.n_states; ++j) {
    const uint32_t ip = rd32(rc + kRecBytes * j), nm = rd32(rc + kRecBytes * j + 4);
    if (ip >= L.n_ips) return "records: ip index out of range";
    if (nm >= L.n_names) return "records: name index out of range";
    if (j && (ip < pi || (ip == pi && nm <= pn))) return "records: not strictly ascending by (ip, name)";
    if (j ? ip - pi > 1 : ip != 0) return "records: an IP without a record";
    used[nm] = 1;
    pi = ip; pn = nm;
  }
  if (L.n_states && pi != L.n_ips - 1) return "records: an IP without a record";
  for (uint64_t k = 0; k < L.n_names; ++k)
    if (!used[k]) return "names: a name no record uses";
  return nullptr;
}

// The node's merge: shards concatenated in the order given (engine-major),
// IP indices offset, names remapped to the sorted union.  The remap is
// monotone, so each shard's records stay sorted.  Returns NULL and fills out,
// or the failed check (*capacity: the merged snapshot is over a format limit).
inline const char *merge(const std::vector<std::pair<const uint8_t *, uint64_t>> &shards, std::vector<uint8_t> *out,
                         bool *capacity) {
  *capacity = false;
  std::vector<Layout> Ls(shards.size());
  std::vector<std::vector<std::string>> nm(shards.size());
  std::vector<std::string> all;
  uint64_t n_ips = 0, ip_bytes = 0, n_states = 0, names_bytes = 0;
  for (size_t s = 0; s < shards.size(); ++s) {
    if (const char *w = validate_host(shards[s].first, shards[s].second, &Ls[s], &nm[s])) return w;
    if (const char *w = check_body(shards[s].first, Ls[s])) return w;
    all.insert(all.end(), nm[s].begin(), nm[s].end());
    n_ips += Ls[s].n_ips; ip_bytes += Ls[s].ip_bytes; n_states += Ls[s].n_states;
  }
  std::sort(all.begin(), all.end());
  all.erase(std::unique(all.begin(), all.end()), all.end());
  for (auto &x : all) names_bytes += x.size();
  Layout L;
  const char *why = nullptr;
  if (!make_layout(all.size(), names_bytes, n_ips, ip_bytes, n_states, &L, &why)) { *capacity = true; return why; }
  out->assign(L.total, 0);
  uint8_t *o = out->data();
  write_header(o, L);
  write_names(o, L, all);
  uint64_t ip0 = 0, by0 = 0, st0 = 0;
  for (size_t s = 0; s < shards.size(); ++s) {
    const uint8_t *p = shards[s].first;
    const Layout &A = Ls[s];
    std::vector<uint32_t> remap(A.n_names);
    for (uint64_t k = 0; k < A.n_names; ++k)
      remap[k] = (uint32_t)(std::lower_bound(all.begin(), all.end(), nm[s][k]) - all.begin());
    for (uint64_t k = 0; k < A.n_ips; ++k) wr64(o + L.o_ip_off + 8 * (ip0 + k), by0 + rd64(p + A.o_ip_off + 8 * k));
    if (A.ip_bytes) memcpy(o + L.o_ips + by0, p + A.o_ips, A.ip_bytes);
    for (uint64_t j = 0; j < A.n_states; ++j) {
      const uint8_t *r = p + A.o_recs + kRecBytes * j;
      uint8_t *w = o + L.o_recs + kRecBytes * (st0 + j);
      wr32(w, (uint32_t)(ip0 + rd32(r)));
      wr32(w + 4, remap[rd32(r + 4)]);
      memcpy(w + 8, r + 8, 16);
    }
    ip0 += A.n_ips; by0 += A.ip_bytes; st0 += A.n_states;
  }
  wr64(o + L.o_ip_off + 8 * n_ips, ip_bytes);
  return nullptr;
}

}  // namespace bjx_snap

#endif  // BJX_SNAPSHOT_H
