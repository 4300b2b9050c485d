// One Allow entry of a decision list as ipfilter's ToggleIP files it (host
// only: bind_ruleset builds the per-scope address and subnet tables from it;
// tests/cpu/header_fields.cpp checks it against a model of net.ParseCIDR and
// IPNet.Contains).
#pragma once
#include <stdint.h>
#include <string.h>

#include <array>
#include <string>
#include <vector>

#include "bjx_common.h"

namespace bjx {

// a subnet as scope_allows_addr compares it: netlen bytes of net and mask
struct Subnet {
  uint8_t net[16];
  uint8_t mask[16];
  uint32_t netlen;  // 4 (IPv4 compare, To4 semantics) or 16
  uint32_t _pad;
};

// net.ParseCIDR + IPNet/To4 handling of ipfilter's ToggleIP (allow entries)
inline bool parse_allow_entry(const std::string &s, std::vector<std::array<uint8_t, 16>> &addrs, std::vector<Subnet> &subs) {
  auto slash = s.find('/');
  const uint8_t *p = reinterpret_cast<const uint8_t *>(s.data());
  if (slash != std::string::npos) {
    uint8_t a[16];
    bool is4;
    std::string addr = s.substr(0, slash), mask = s.substr(slash + 1);
    if (!go_parse_addr(reinterpret_cast<const uint8_t *>(addr.data()), (uint32_t)addr.size(), a, &is4)) return false;
    if (addr.find('%') != std::string::npos) return false;
    long bits = 0;
    size_t i = 0;
    for (; i < mask.size() && mask[i] >= '0' && mask[i] <= '9'; ++i) {
      bits = bits * 10 + (mask[i] - '0');
      if (bits >= 0xFFFFFF) return false;
    }
    if (i == 0 || i != mask.size()) return false;
    const int bitlen = is4 ? 32 : 128;
    if (bits > bitlen) return false;
    if (bits == bitlen) {  // single address
      std::array<uint8_t, 16> x;
      memcpy(x.data(), a, 16);
      addrs.push_back(x);
      return true;
    }
    Subnet sn;
    memset(&sn, 0, sizeof sn);
    auto mk = [&](int k) -> uint8_t {
      int b = (int)bits - 8 * k;
      return b >= 8 ? 0xFF : (b <= 0 ? 0 : (uint8_t)(0xFF << (8 - b)));
    };
    if (is4) {
      sn.netlen = 4;
      for (int k = 0; k < 4; ++k) { sn.mask[k] = mk(k); sn.net[k] = a[12 + k] & sn.mask[k]; }
    } else {
      uint8_t net[16], m[16];
      for (int k = 0; k < 16; ++k) { m[k] = mk(k); net[k] = a[k] & m[k]; }
      if (is_v4_mapped(net)) { sn.netlen = 4; memcpy(sn.net, net + 12, 4); memcpy(sn.mask, m + 12, 4); }
      else { sn.netlen = 16; memcpy(sn.net, net, 16); memcpy(sn.mask, m, 16); }
    }
    subs.push_back(sn);
    return true;
  }
  uint8_t a[16];
  bool is4;
  if (go_parse_addr(p, (uint32_t)s.size(), a, &is4)) {
    std::array<uint8_t, 16> x;
    memcpy(x.data(), a, 16);
    addrs.push_back(x);
    return true;
  }
  return false;
}

}  // namespace bjx
