// State selection by network (bjx_state_query_nets / bjx_state_remove_nets and
// their node forms, include/banjax_gpu.h; DESIGN.md §2 "Nets").  The argument
// checks, the entries parsed through parse_allow_entry and canonicalised into
// the net table the engine uploads, the membership rule on that table (host
// and device: k_net_sel / k_net_count in state_ops.h run it per held IP, the
// host runs it for a filter's ip), and the node's sum of net_ips.  engine.hip
// and node.cpp include it; tests/cpu/nets_host.cpp builds it without a GPU.
//
// Membership is scope_allows_addr's rule (engine.hip) for a global Allow list
// made of the entries: an address that is v4-mapped compares as IPv4, against
// 4-byte networks only; every other address against 16-byte networks only.  An
// entry is filed under (family, prefix length, masked network): an IPv4
// address is the /32 of its family, an IPv6 one the /128; an IPv6-text entry
// whose masked network is v4-mapped (::ffff:a.b.c.d/96+n) is the IPv4 /n.
#ifndef BJX_STATE_NETS_H
#define BJX_STATE_NETS_H

#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <string>
#include <vector>

#include "../../include/banjax_gpu.h"
#include "allow_entry.h"

namespace bjx_nets {

// one prefix length of one family: keys[first, first + count) of that family's
// array, sorted ascending and distinct, each masked to `bits`
struct Dir {
  uint32_t bits, first, count, _pad;
};
// the table as the membership code reads it (host or device pointers).  dir
// holds the IPv4 lengths first (n_dir4 of them, ascending), then the IPv6
// ones; k4 one u32 per IPv4 network, k6 two u64 (high, low) per IPv6 network.
// The canonical index of an IPv4 network is its index in k4, of an IPv6
// network n4 + its index in k6.
struct View {
  const Dir *dir;
  const uint32_t *k4;
  const uint64_t *k6;
  uint32_t n_dir4, n_dir6, n4, n6;
};

BJX_HD uint32_t mask32(uint32_t bits) { return bits ? ~0u << (32 - bits) : 0u; }
BJX_HD uint64_t mask64(uint32_t bits) { return bits >= 64 ? ~0ull : (bits ? ~0ull << (64 - bits) : 0ull); }
BJX_HD uint64_t be64(const uint8_t *a) {
  uint64_t v = 0;
  for (int k = 0; k < 8; ++k) v = (v << 8) | a[k];
  return v;
}

// For every network of V that holds the parsed address a (go_parse_addr's 16
// bytes), hit(canonical index) is called; hit returns true to stop.  Returns
// whether any network held it.  One binary search per prefix length present.
template <typename Hit>
BJX_HD bool member(const View &V, const uint8_t a[16], Hit hit) {
  bool any = false;
  if (bjx::is_v4_mapped(a)) {
    const uint32_t ip = ((uint32_t)a[12] << 24) | ((uint32_t)a[13] << 16) | ((uint32_t)a[14] << 8) | a[15];
    for (uint32_t d = 0; d < V.n_dir4; ++d) {
      const Dir D = V.dir[d];
      const uint32_t key = ip & mask32(D.bits);
      uint32_t lo = D.first, hi = D.first + D.count;
      while (lo < hi) {
        const uint32_t m = lo + ((hi - lo) >> 1);
        if (V.k4[m] < key) lo = m + 1; else hi = m;
      }
      if (lo < D.first + D.count && V.k4[lo] == key) {
        any = true;
        if (hit(lo)) return true;
      }
    }
    return any;
  }
  const uint64_t h = be64(a), l = be64(a + 8);
  for (uint32_t d = V.n_dir4; d < V.n_dir4 + V.n_dir6; ++d) {
    const Dir D = V.dir[d];
    const uint64_t kh = h & mask64(D.bits), kl = D.bits > 64 ? l & mask64(D.bits - 64) : 0ull;
    uint32_t lo = D.first, hi = D.first + D.count;
    while (lo < hi) {
      const uint32_t m = lo + ((hi - lo) >> 1);
      const uint64_t mh = V.k6[2 * (uint64_t)m], ml = V.k6[2 * (uint64_t)m + 1];
      if (mh < kh || (mh == kh && ml < kl)) lo = m + 1; else hi = m;
    }
    if (lo < D.first + D.count && V.k6[2 * (uint64_t)lo] == kh && V.k6[2 * (uint64_t)lo + 1] == kl) {
      any = true;
      if (hit(V.n4 + lo)) return true;
    }
  }
  return any;
}

// NULL when the call can be answered, else what is wrong with its arguments.
// Only the lengths are read: no entry's bytes are touched before this passes.
inline const char *check_args(const bjx_state_filter *f, const bjx_str *nets, size_t n_nets) {
  if (!f) return "no filter";
  if (f->ip.len && !f->ip.ptr) return "filter: ip with a length and no bytes";
  if (f->name.len && !f->name.ptr) return "filter: name with a length and no bytes";
  if (!nets) return "nets: no list";
  if (n_nets == 0) return "nets: an empty list (a nets call never means every IP)";
  if (n_nets > BJX_NETS_MAX) return "nets: more than BJX_NETS_MAX entries";
  for (size_t k = 0; k < n_nets; ++k)
    if (nets[k].len && !nets[k].ptr) return "nets: an entry with a length and no bytes";
  return nullptr;
}

struct Table {
  std::vector<Dir> dir;
  std::vector<uint32_t> k4;
  std::vector<uint64_t> k6;        // two words a network
  std::vector<uint32_t> entry;     // caller entry k -> canonical index
  uint32_t n_dir4 = 0, n_dir6 = 0;
  uint32_t n_canon() const { return (uint32_t)(k4.size() + k6.size() / 2); }
  View view() const {
    return View{dir.data(), k4.data(), k6.data(), n_dir4, n_dir6, (uint32_t)k4.size(), (uint32_t)(k6.size() / 2)};
  }
  // the table in one piece, as the engine uploads it: k6, dir, k4 (each
  // aligned for its type); the offsets of dir and k4 in it
  uint64_t image(std::vector<uint8_t> *img, uint64_t *o_dir, uint64_t *o_k4) const {
    *o_dir = k6.size() * 8;
    *o_k4 = *o_dir + dir.size() * sizeof(Dir);
    const uint64_t total = *o_k4 + k4.size() * 4;
    img->assign(total, 0);
    if (!k6.empty()) memcpy(img->data(), k6.data(), k6.size() * 8);
    if (!dir.empty()) memcpy(img->data() + *o_dir, dir.data(), dir.size() * sizeof(Dir));
    if (!k4.empty()) memcpy(img->data() + *o_k4, k4.data(), k4.size() * 4);
    return total;
  }
  // membership of one IP text (a filter's ip): parsed as a held IP is
  bool holds(const uint8_t *ip, uint32_t len, std::vector<uint32_t> *canon = nullptr) const {
    uint8_t a[16];
    bool is4;
    if (!bjx::go_parse_addr(ip, len, a, &is4)) return false;
    return member(view(), a, [&](uint32_t c) {
      if (canon) canon->push_back(c);
      return canon == nullptr;
    });
  }
};

// one entry -> (family 4 / 6, prefix length, masked network); false: it does not file
inline bool parse_entry(const std::string &s, int *family, uint32_t *bits, uint64_t *hi, uint64_t *lo) {
  std::vector<std::array<uint8_t, 16>> addrs;
  std::vector<bjx::Subnet> subs;
  if (!bjx::parse_allow_entry(s, addrs, subs)) return false;
  if (!addrs.empty()) {  // a single address: the last length of its family
    const uint8_t *a = addrs[0].data();
    if (bjx::is_v4_mapped(a)) { *family = 4; *bits = 32; *hi = 0; *lo = be64(a + 8) & 0xFFFFFFFFull; }
    else { *family = 6; *bits = 128; *hi = be64(a); *lo = be64(a + 8); }
    return true;
  }
  const bjx::Subnet &sn = subs[0];
  uint32_t n = 0;
  for (uint32_t k = 0; k < sn.netlen; ++k) n += (uint32_t)__builtin_popcount(sn.mask[k]);
  *bits = n;
  if (sn.netlen == 4) {
    *family = 4; *hi = 0;
    *lo = ((uint64_t)sn.net[0] << 24) | ((uint64_t)sn.net[1] << 16) | ((uint64_t)sn.net[2] << 8) | sn.net[3];
  } else {
    *family = 6; *hi = be64(sn.net); *lo = be64(sn.net + 8);
  }
  return true;
}

// check_args passed.  -1 when every entry files, else the index of the first
// one that does not (T is then unspecified).
inline int64_t build(const bjx_str *nets, size_t n_nets, Table *T) {
  *T = Table{};
  struct Key { uint32_t fam, bits; uint64_t hi, lo; };
  auto less = [](const Key &a, const Key &b) {
    if (a.fam != b.fam) return a.fam < b.fam;
    if (a.bits != b.bits) return a.bits < b.bits;
    if (a.hi != b.hi) return a.hi < b.hi;
    return a.lo < b.lo;
  };
  auto same = [](const Key &a, const Key &b) { return a.fam == b.fam && a.bits == b.bits && a.hi == b.hi && a.lo == b.lo; };
  std::vector<Key> given(n_nets);
  for (size_t k = 0; k < n_nets; ++k) {
    int fam = 0;
    Key &K = given[k];
    if (!parse_entry(std::string(nets[k].len ? nets[k].ptr : "", nets[k].len), &fam, &K.bits, &K.hi, &K.lo)) return (int64_t)k;
    K.fam = (uint32_t)fam;
  }
  std::vector<Key> canon(given);
  std::sort(canon.begin(), canon.end(), less);
  canon.erase(std::unique(canon.begin(), canon.end(), same), canon.end());
  // (family 4 sorts before 6, so a canonical index is the position in `canon`)
  for (const Key &K : canon) {
    const bool v4 = K.fam == 4;
    const uint32_t at = v4 ? (uint32_t)T->k4.size() : (uint32_t)(T->k6.size() / 2);
    if (T->dir.empty() || (T->dir.size() == T->n_dir4 && !v4) || T->dir.back().bits != K.bits) {
      T->dir.push_back(Dir{K.bits, at, 0, 0});
      ++(v4 ? T->n_dir4 : T->n_dir6);
    }
    ++T->dir.back().count;
    if (v4) T->k4.push_back((uint32_t)K.lo);
    else { T->k6.push_back(K.hi); T->k6.push_back(K.lo); }
  }
  T->entry.resize(n_nets);
  for (size_t k = 0; k < n_nets; ++k)
    T->entry[k] = (uint32_t)(std::lower_bound(canon.begin(), canon.end(), given[k], less) - canon.begin());
  return -1;
}

// what a call says about the first entry that does not file
inline std::string bad_entry(int64_t k) { return "nets: entry " + std::to_string(k) + " is not an address or address/bits"; }

// the caller's view of the canonical counters: net_ips[k] for entry k
inline void per_entry(const Table &T, const std::vector<uint32_t> &canon_count, std::vector<uint64_t> *net_ips) {
  net_ips->assign(T.entry.size(), 0);
  for (size_t k = 0; k < T.entry.size(); ++k)
    if (T.entry[k] < canon_count.size()) (*net_ips)[k] = canon_count[T.entry[k]];
}

// The node's sum: an IP lives on one shard, so each entry's counts add up.
inline void add(std::vector<uint64_t> *t, const uint64_t *s, size_t n_nets) {
  if (t->size() < n_nets) t->resize(n_nets, 0);
  if (s)
    for (size_t k = 0; k < n_nets; ++k) (*t)[k] += s[k];
}

}  // namespace bjx_nets

#endif  // BJX_STATE_NETS_H
