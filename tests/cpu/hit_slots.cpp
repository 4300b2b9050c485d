// CPU harness for the literal-hit slot arithmetic shared with the device
// (bjx::slot_lead_start / slot_certain / lead_bound in
// banjax_amd/csrc/bjx_common.h; called by l2_job_rec in lines2.h and by
// lead_start / eq_certain in engine.hip).
//
// A long line's hits reach the scan's four slots in any order, so for a set of
// hits this enumerates every choice and order of the min(n, 4) that get slots,
// folds the others into the summary the way engine_types.h CandMeta documents
// (and k_scan does), and checks what a job may conclude:
//   - the start bound never exceeds max(0, first own hit at or past rs - rs -
//     back), and equals rl only when there is no such hit;
//   - certainty implies a verified own hit at or past rs;
//   - with n <= 4 (no overflow) every order gives the same, exact, answer.
// "far" (verified and 256 bytes or more into the line) is only ever set on a
// hit that lies there; k_scan may leave it off one that does.
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include "../../banjax_amd/csrc/bjx_common.h"

namespace {

constexpr uint32_t kOwn = 5, kOther = 9, kAlias = kOwn + 32;
constexpr uint64_t kRs = 1042;  // not a multiple of 8: a hit just past rs rounds down to before it
constexpr uint32_t kRl = 400;

struct Hit { uint32_t pos, lit; bool ver, far; };
struct Env { uint32_t rest_off, back; bool lits_small; };
struct Res { uint32_t start; bool certain; };

struct Run {
  Env E;
  const Hit *types;
  uint32_t n_types;
  uint64_t sets = 0, evals = 0, bad = 0;
  char first_bad[512] = "";
};

bool mine(uint64_t v) { return (uint32_t)(v & 0x7FFFFF) == kOwn; }

Res eval(const Hit *h, uint32_t n, const uint32_t *slot, uint32_t ns, const Env &E) {
  uint64_t cv[bjx::kSlots] = {0, 0, 0, 0};
  bool used[8] = {false, false, false, false, false, false, false, false};
  for (uint32_t c = 0; c < ns; ++c) {
    const Hit &x = h[slot[c]];
    cv[c] = ((uint64_t)x.pos << 24) | (x.ver ? bjx::kSlotVerified : 0ull) | x.lit;
    used[slot[c]] = true;
  }
  uint64_t bits = 0;
  uint32_t first_inv = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (used[i]) continue;
    const uint64_t bit = 1ull << (h[i].lit & 31);
    bits |= (h[i].ver && h[i].far) ? bit | (bit << 32) : bit;
    const uint32_t inv = ~(h[i].pos >> 3);
    first_inv = inv > first_inv ? inv : first_inv;
  }
  Res r;
  r.start = bjx::slot_lead_start(cv, n, first_inv, kRs, kRl, E.back, mine);
  r.certain = bjx::slot_certain(cv, n, bits, 1u << (kOwn & 31), E.lits_small, E.rest_off, kRs, mine);
  return r;
}

void fail(Run &R, const Hit *h, uint32_t n, const uint32_t *slot, uint32_t ns, const Res &r, const char *what) {
  if (R.bad++ != 0) return;
  int o = snprintf(R.first_bad, sizeof R.first_bad, "%s: start %u certain %d; hits", what, r.start, (int)r.certain);
  for (uint32_t i = 0; i < n && o < (int)sizeof R.first_bad - 40; ++i)
    o += snprintf(R.first_bad + o, sizeof R.first_bad - o, " (%u,%u,%d,%d)", h[i].pos, h[i].lit, (int)h[i].ver, (int)h[i].far);
  o += snprintf(R.first_bad + o, sizeof R.first_bad - o, " slots");
  for (uint32_t c = 0; c < ns && o < (int)sizeof R.first_bad - 8; ++c) o += snprintf(R.first_bad + o, sizeof R.first_bad - o, " %u", slot[c]);
}

void check_set(Run &R, const Hit *h, uint32_t n) {
  ++R.sets;
  // what is true of the set, whichever hits got slots
  uint32_t first_own = ~0u;
  bool ver_own = false;
  for (uint32_t i = 0; i < n; ++i) {
    if (h[i].lit != kOwn || h[i].pos < kRs) continue;
    if (h[i].pos < first_own) first_own = h[i].pos;
    ver_own = ver_own || h[i].ver;
  }
  uint32_t limit = kRl;
  if (first_own != ~0u) {
    const uint32_t o = first_own - (uint32_t)kRs < kRl ? first_own - (uint32_t)kRs : kRl;
    limit = o > R.E.back ? o - R.E.back : 0u;
  }
  const uint32_t ns = n < bjx::kSlots ? n : bjx::kSlots;
  uint32_t slot[4] = {0, 0, 0, 0};
  Res ref{0, false};
  bool have_ref = false;
  // every ordered choice of ns distinct hits
  uint32_t idx[4] = {0, 0, 0, 0};
  int depth = 0;
  if (ns == 0) {
    const Res r = eval(h, n, slot, 0, R.E);
    ++R.evals;
    if (r.start != kRl || r.certain) fail(R, h, n, slot, 0, r, "no hits");
    return;
  }
  idx[0] = 0;
  while (depth >= 0) {
    if (idx[depth] >= n) { --depth; if (depth >= 0) ++idx[depth]; continue; }
    bool dup = false;
    for (int d = 0; d < depth; ++d) dup = dup || idx[d] == idx[depth];
    if (dup) { ++idx[depth]; continue; }
    if (depth + 1 < (int)ns) { ++depth; idx[depth] = 0; continue; }
    for (uint32_t c = 0; c < ns; ++c) slot[c] = idx[c];
    const Res r = eval(h, n, slot, ns, R.E);
    ++R.evals;
    if (r.start > limit) fail(R, h, n, slot, ns, r, "start past the first own hit");
    if (r.start == kRl && first_own != ~0u) fail(R, h, n, slot, ns, r, "no-match start with an own hit in rest");
    if (r.certain && !ver_own) fail(R, h, n, slot, ns, r, "certain without a verified own hit in rest");
    if (n <= bjx::kSlots) {
      if (r.start != limit || r.certain != ver_own) fail(R, h, n, slot, ns, r, "not exact without overflow");
      if (have_ref && (r.start != ref.start || r.certain != ref.certain)) fail(R, h, n, slot, ns, r, "order changes the answer");
      ref = r;
      have_ref = true;
    }
    ++idx[depth];
  }
}

void sets_of(Run &R, Hit *h, uint32_t n, uint32_t k, uint32_t from) {
  if (k == n) { check_set(R, h, n); return; }
  for (uint32_t t = from; t < R.n_types; ++t) {
    h[k] = R.types[t];
    sets_of(R, h, n, k + 1, t);
  }
}

}  // namespace

// Every multiset of n_lo .. n_hi hits over the grid positions x {own, other, own + 32
// (only when !lits_small)} x {unverified, verified, verified and far (only where the
// hit lies 256 bytes or more into the line)}.  flags: 1 lits_small.  Returns the
// number of violations; out = {sets, evaluations}; msg = the first violation.
extern "C" uint64_t bjx_test_hit_slots(const uint32_t *positions, uint32_t n_pos, uint32_t n_lo, uint32_t n_hi, uint32_t rest_off,
                                       uint32_t back, uint32_t flags, uint32_t own_only_verified, uint64_t *out, char *msg,
                                       uint32_t msg_len) {
  Run R;
  R.E = Env{rest_off, back, (flags & 1u) != 0};
  Hit types[256];
  uint32_t nt = 0;
  const uint64_t line_start = kRs - rest_off;
  const uint32_t lits[3] = {kOwn, kOther, kAlias};
  for (uint32_t p = 0; p < n_pos; ++p)
    for (uint32_t l = 0; l < 3; ++l) {
      if (lits[l] == kAlias && R.E.lits_small) continue;
      const bool can_far = positions[p] - line_start >= bjx::kSlotCertainGap;
      for (uint32_t f = 0; f < 3; ++f) {
        if (f == 2 && !can_far) continue;
        // the reduced grid keeps one state per (position, literal) beside the own literal's
        if (own_only_verified && lits[l] != kOwn && f != (can_far ? 2u : 1u)) continue;
        if (nt < 256) types[nt++] = Hit{positions[p], lits[l], f >= 1, f == 2};
      }
    }
  R.types = types;
  R.n_types = nt;
  Hit h[8];
  for (uint32_t n = n_lo; n <= n_hi && n <= 7; ++n) sets_of(R, h, n, 0, 0);
  out[0] = R.sets;
  out[1] = R.evals;
  out[2] = nt;
  if (msg && msg_len) { strncpy(msg, R.first_bad, msg_len - 1); msg[msg_len - 1] = 0; }
  return R.bad;
}

// one evaluation, for spot checks: hits as (pos, lit, ver, far) quadruples, the first ns in slot order
extern "C" uint32_t bjx_test_hit_slots_eval(const uint32_t *quads, uint32_t n, uint32_t ns, uint32_t rest_off, uint32_t back,
                                            uint32_t lits_small, uint32_t *certain) {
  Hit h[8];
  uint32_t slot[4] = {0, 1, 2, 3};
  for (uint32_t i = 0; i < n && i < 8; ++i) h[i] = Hit{quads[4 * i], quads[4 * i + 1], quads[4 * i + 2] != 0, quads[4 * i + 3] != 0};
  const Res r = eval(h, n, slot, ns, Env{rest_off, back, lits_small != 0});
  *certain = r.certain;
  return r.start;
}
