// Budgeted trim (bjx_state_trim / bjx_node_state_trim, include/banjax_gpu.h;
// DESIGN.md §2 "Trim").  Host-only: the budget's checks, the radix select's
// host step (a digit histogram plus the remaining rank give the chosen digit
// and the new rank, from the top digit down), the biased key and the
// saturating + 1, the cutoff, bound and budget_met from the three candidate
// cutoffs, and the node's max and sum.  engine.hip and node.cpp include it (the
// kernels that count the digits use its digit geometry);
// tests/cpu/trim_host.cpp builds it without a GPU.
#ifndef BJX_STATE_TRIM_H
#define BJX_STATE_TRIM_H

#include <stdint.h>

#include "../../include/banjax_gpu.h"

#ifdef __HIPCC__
#define BJX_TRIM_HD __host__ __device__
#else
#define BJX_TRIM_HD
#endif

namespace bjx_trim {

// NULL when the call can be answered, else what is wrong with its arguments
inline const char *check_budget(const bjx_trim_budget *b) {
  if (!b) return "no budget";
  if (b->flags & ~(uint32_t)BJX_TRIM_DRY_RUN) return "budget: unknown flag bits";
  return nullptr;
}

// ---- the key.  int64 -> u64 of the same order (the sign bit flipped), read
// as kDigits digits from the top: four of 13 bits and a last one of 12.
constexpr uint32_t kDigits = 5, kDigitBits = 13, kBins = 1u << kDigitBits;
BJX_TRIM_HD inline uint64_t key_of(int64_t v) { return (uint64_t)v ^ 0x8000000000000000ull; }
BJX_TRIM_HD inline int64_t value_of(uint64_t key) { return (int64_t)(key ^ 0x8000000000000000ull); }
BJX_TRIM_HD inline uint32_t digit_shift(uint32_t p) { return p + 1 < kDigits ? 64 - kDigitBits * (p + 1) : 0; }
BJX_TRIM_HD inline uint32_t digit_bins(uint32_t p) { return p + 1 < kDigits ? kBins : 1u << (64 - kDigitBits * (kDigits - 1)); }
BJX_TRIM_HD inline uint32_t digit(uint64_t key, uint32_t p) { return (uint32_t)(key >> digit_shift(p)) & (digit_bins(p) - 1); }
// key has the digits above p that prefix has (p == 0: every key)
BJX_TRIM_HD inline bool under(uint64_t key, uint64_t prefix, uint32_t p) {
  return p == 0 || ((key ^ prefix) >> digit_shift(p - 1)) == 0;
}
static_assert(kDigitBits * (kDigits - 1) < 64 && kDigitBits * kDigits >= 64, "the digits cover 64 bits");

// ---- the select: the rank-th largest key (rank from 1) of a multiset, found
// digit by digit.  Before pass p the keys still in play are those under
// `prefix`; hist[d] counts them by digit p.
struct Select {
  uint64_t rank = 0, prefix = 0;
  uint32_t p = 0;
  bool done() const { return p == kDigits; }
};
// false when the histogram holds fewer than rank keys (not from a count of the
// keys under prefix: never taken)
inline bool step(Select *s, const uint64_t *hist) {
  uint64_t above = 0;
  for (uint32_t d = digit_bins(s->p); d-- > 0;) {
    if (hist[d] >= s->rank - above) {
      s->rank -= above;
      s->prefix |= (uint64_t)d << digit_shift(s->p);
      ++s->p;
      return true;
    }
    above += hist[d];
  }
  return false;
}

// ---- cut(V, k): the smallest C with #{v in V : v >= C} <= k
struct Cut {
  int64_t c = INT64_MIN;
  bool saturated = false;  // more than k values equal INT64_MAX: they stay
};
// k == 0 (no bound) or |V| <= k
inline bool unbounded(uint64_t k, uint64_t n_values) { return k == 0 || n_values <= k; }
// from v, the (k + 1)-th largest value: v + 1, saturating
inline Cut cut_after(int64_t v) {
  Cut c;
  c.saturated = v == INT64_MAX;
  c.c = c.saturated ? INT64_MAX : v + 1;
  return c;
}

// ---- what one engine's selection found
struct Picked {
  int64_t cutoff = INT64_MIN;
  uint32_t bound = BJX_TRIM_BY_NONE, budget_met = 1;
  double select_ms = 0;
};
inline Picked pick(int64_t floor_cutoff, const Cut &states, const Cut &ips) {
  Picked P;
  P.cutoff = floor_cutoff;
  if (states.c > P.cutoff) P.cutoff = states.c;
  if (ips.c > P.cutoff) P.cutoff = ips.c;
  if (ips.c == P.cutoff && ips.c > INT64_MIN) P.bound = BJX_TRIM_BY_IPS;
  else if (states.c == P.cutoff && states.c > INT64_MIN) P.bound = BJX_TRIM_BY_STATES;
  else if (floor_cutoff > INT64_MIN) P.bound = BJX_TRIM_BY_FLOOR;
  P.budget_met = states.saturated || ips.saturated ? 0u : 1u;
  return P;
}

// ---- the node: one cutoff, the largest; its bound is that of the first
// engine that gave it; budget_met is the AND, select_ms the slowest engine's
inline Picked node_pick(const Picked *p, size_t n) {
  Picked N;
  for (size_t k = 0; k < n; ++k) {
    if (k == 0 || p[k].cutoff > N.cutoff) { N.cutoff = p[k].cutoff; N.bound = p[k].bound; }
    N.budget_met &= p[k].budget_met;
    if (p[k].select_ms > N.select_ms) N.select_ms = p[k].select_ms;
  }
  return N;
}
// an IP lives on one engine, so counts and bytes add up exactly; the times are
// the slowest engine's; cutoff_ns, bound and budget_met are node_pick's
inline void add(bjx_trim_stats *t, const bjx_trim_stats &s) {
  t->states_before += s.states_before; t->states_dropped += s.states_dropped; t->states_dropped_live += s.states_dropped_live;
  t->ips_before += s.ips_before; t->ips_dropped += s.ips_dropped;
  t->arena_bytes_before += s.arena_bytes_before; t->arena_bytes_after += s.arena_bytes_after;
  t->device_bytes_before += s.device_bytes_before; t->device_bytes_after += s.device_bytes_after;
  if (s.select_ms > t->select_ms) t->select_ms = s.select_ms;
  if (s.device_ms > t->device_ms) t->device_ms = s.device_ms;
}

}  // namespace bjx_trim

// The two halves of bjx_state_trim as the node calls them (engine.hip; not part
// of the C ABI): the selection alone, and the trim at a given cutoff --
// bjx_state_expire(cutoff_ns) with the trim's no-op rule, dry run and stats,
// states_dropped_live counted against live_floor_ns.  Both take the engine lock.
int bjx_trim_select(bjx_engine *e, const bjx_trim_budget *b, bjx_trim::Picked *out);
int bjx_trim_apply(bjx_engine *e, int64_t cutoff_ns, int64_t live_floor_ns, uint32_t flags, bjx_trim_stats *out);

#endif  // BJX_STATE_TRIM_H
