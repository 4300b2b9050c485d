// CPU harness for the header-field parsers the kernels share with the host
// (banjax_amd/csrc/bjx_common.h: go_parse_float, parse_float_fast,
// ns_from_seconds, go_parse_addr) and for the allow-entry parser that builds
// the per-scope tables scope_allows_addr reads (allow_entry.h).  Batched: the
// tokens lie end to end in buf, token k is [off[k], off[k + 1]).
// tests/test_header_fields_cpu.py compares every output with the references
// of tests/header_fields.py and with the oracle.
#include <stdint.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../banjax_amd/csrc/allow_entry.h"
#include "../../banjax_amd/csrc/bjx_common.h"

namespace {
uint64_t bits_of(double f) {
  uint64_t u;
  memcpy(&u, &f, 8);
  return u;
}
}  // namespace

extern "C" {

// fast = 0: go_parse_float (rc 0, -1 syntax, -2 range); fast = 1: parse_float_fast (rc 0, 1 declined).
// bits: the value (0 where none); ns: ns_from_seconds of it where rc == 0.
void bjx_test_parse_floats(const uint8_t *buf, const uint64_t *off, uint64_t n, int fast, int32_t *rc, uint64_t *bits,
                           int64_t *ns) {
  static bjx::Decimal dec;
  for (uint64_t k = 0; k < n; ++k) {
    double f = 0.0;
    const uint8_t *s = buf + off[k];
    const uint32_t len = (uint32_t)(off[k + 1] - off[k]);
    rc[k] = fast ? bjx::parse_float_fast(s, len, &f) : bjx::go_parse_float(s, len, &f, &dec);
    const bool has = rc[k] == 0 || rc[k] == -2;
    bits[k] = has ? bits_of(f) : 0;
    ns[k] = rc[k] == 0 ? bjx::ns_from_seconds(f) : 0;
  }
}

void bjx_test_ns_from_seconds(const uint64_t *bits, uint64_t n, int64_t *ns) {
  for (uint64_t k = 0; k < n; ++k) {
    double f;
    memcpy(&f, &bits[k], 8);
    ns[k] = bjx::ns_from_seconds(f);
  }
}

// go_parse_addr: ok[k], the 16 bytes and the IPv4-text flag (0 where refused)
void bjx_test_parse_addrs(const uint8_t *buf, const uint64_t *off, uint64_t n, uint8_t *ok, uint8_t *out16, uint8_t *is4) {
  for (uint64_t k = 0; k < n; ++k) {
    uint8_t a[16];
    bool v4 = false;
    const bool r = bjx::go_parse_addr(buf + off[k], (uint32_t)(off[k + 1] - off[k]), a, &v4);
    ok[k] = r ? 1 : 0;
    is4[k] = r && v4 ? 1 : 0;
    if (r) memcpy(out16 + 16 * k, a, 16);
    else memset(out16 + 16 * k, 0, 16);
  }
}

// parse_allow_entry of one entry: 0 not filed, 1 a single address (net), 2 a subnet (net, mask, netlen);
// -1 if its return value and what it appended disagree
int bjx_test_allow_entry(const char *s, uint32_t n, uint8_t net[16], uint8_t mask[16], uint32_t *netlen) {
  std::vector<std::array<uint8_t, 16>> addrs;
  std::vector<bjx::Subnet> subs;
  const bool r = bjx::parse_allow_entry(std::string(s, n), addrs, subs);
  if (addrs.size() + subs.size() != (r ? 1u : 0u)) return -1;
  memset(net, 0, 16);
  memset(mask, 0, 16);
  *netlen = 0;
  if (!r) return 0;
  if (!addrs.empty()) {
    memcpy(net, addrs[0].data(), 16);
    return 1;
  }
  memcpy(net, subs[0].net, 16);
  memcpy(mask, subs[0].mask, 16);
  *netlen = subs[0].netlen;
  return 2;
}

}  // extern "C"
