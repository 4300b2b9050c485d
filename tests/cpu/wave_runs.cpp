// CPU harness for the wave-per-run path of k_bucket_apply (bucket_wave_run in
// banjax_amd/csrc/engine.hip): one run of one (ip, rule name) state, taken in
// chunks of 64 events with the state carried between them, against the
// event-by-event walk (bjx::window_step, Apply as the reference writes it).
// The wave is simulated sequentially, as block_search.cpp simulates the block:
// a ballot is a loop over the lanes, a shuffle an array read.  The window rule
// (bjx::window_past) and the closed form (bjx::window_hits) are the device's
// own, from banjax_amd/csrc/bjx_common.h.
//
// An event is (ts, interval, limit): the interval and limit of its own rule
// (rules sharing a name share the state but not their limits).  Outcomes are
// MatchType | Exceeded << 2.
//
// -DWAVE_RUNS_MAIN builds a stand-alone self-test (for sanitizer runs).
#include <stdint.h>
#include "../../banjax_amd/csrc/bjx_common.h"

namespace {

constexpr uint32_t kLanes = 64;

struct WState {
  bool valid;
  int64_t hits, start;
};

void run_serial(uint32_t n, const int64_t *ts, const int64_t *iv, const int64_t *lim, WState &s, uint8_t *out) {
  for (uint32_t i = 0; i < n; ++i) {
    uint32_t mt;
    const bool ex = bjx::window_step(ts[i], iv[i], lim[i], s.valid, s.hits, s.start, mt);
    out[i] = (uint8_t)(mt | (ex ? 4 : 0));
  }
}

// chunks: 0 for the serial walk inside every chunk, 1 closed form where the chunk allows it
void run_chunked(uint32_t n, const int64_t *ts, const int64_t *iv, const int64_t *lim, WState &s, uint8_t *out,
                 uint32_t *n_closed) {
  const int64_t I = iv[0], Lim = lim[0];  // the head's rule
  for (uint32_t c = 0; c < n; c += kLanes) {
    const uint32_t na = n - c < kLanes ? n - c : kLanes;
    const int64_t *t = ts + c;
    bool same = true;
    for (uint32_t l = 0; l < na; ++l) same = same && iv[c + l] == I && lim[c + l] == Lim;
    if (same) {
      ++*n_closed;
      int32_t a = s.valid ? -1 : 0;
      int64_t Tw = s.valid ? s.start : t[0];
      uint32_t wa[kLanes], wmt[kLanes];
      int64_t wh0[kLanes];
      for (uint32_t l = 0; l < na; ++l) { wa[l] = 0; wmt[l] = s.valid ? 2 : 0; wh0[l] = s.valid ? s.hits : 0; }
      for (;;) {
        int32_t f = -1;  // ballot + find first
        for (uint32_t l = 0; l < na; ++l)
          if ((int32_t)l > a && bjx::window_past(t[l], Tw, I)) { f = (int32_t)l; break; }
        if (f < 0) break;
        a = f;
        Tw = t[a];
        for (uint32_t l = (uint32_t)a; l < na; ++l) { wa[l] = (uint32_t)a; wh0[l] = 0; wmt[l] = 1; }
      }
      int64_t hh = 0;
      for (uint32_t l = 0; l < na; ++l) {
        hh = bjx::window_hits(wh0[l], (int64_t)(l - wa[l]) + 1, Lim);
        out[c + l] = (uint8_t)((l == wa[l] ? wmt[l] : 2u) | (hh == 0 ? 4 : 0));
      }
      s.hits = hh;  // the last lane's
      s.start = Tw;
      s.valid = true;
    } else {
      run_serial(na, t, iv + c, lim + c, s, out + c);
    }
  }
}

}  // namespace

// returns the number of chunks that took the closed form; out_* have n bytes,
// st_* = {valid, hits, start} in and out
extern "C" uint32_t bjx_test_wave_run(uint32_t n, const int64_t *ts, const int64_t *iv, const int64_t *lim, int64_t *st_serial,
                                      int64_t *st_chunked, uint8_t *out_serial, uint8_t *out_chunked) {
  WState a = {st_serial[0] != 0, st_serial[1], st_serial[2]}, b = {st_chunked[0] != 0, st_chunked[1], st_chunked[2]};
  uint32_t n_closed = 0;
  run_serial(n, ts, iv, lim, a, out_serial);
  run_chunked(n, ts, iv, lim, b, out_chunked, &n_closed);
  st_serial[0] = a.valid; st_serial[1] = a.hits; st_serial[2] = a.start;
  st_chunked[0] = b.valid; st_chunked[1] = b.hits; st_chunked[2] = b.start;
  return n_closed;
}

#ifdef WAVE_RUNS_MAIN
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>

int main() {
  uint64_t x = 0x9E3779B97F4A7C15ull;
  auto rnd = [&](uint64_t m) { x = bjx::mix64(x + 0x632BE59BD9B4E019ull); return x % m; };
  const int64_t lims[] = {-1, 0, 1, 5, 800};
  uint64_t bad = 0, closed = 0;
  for (uint32_t it = 0; it < 20000; ++it) {
    const uint32_t n = 1 + (uint32_t)rnd(300);
    const int64_t I = (int64_t)(1 + rnd(4)) * 250000000ll, L = lims[rnd(5)], L2 = rnd(4) ? L : lims[rnd(5)];
    std::vector<int64_t> ts(n), iv(n, I), lim(n);
    int64_t t = 1700000000000000000ll;
    for (uint32_t i = 0; i < n; ++i) {
      t += (int64_t)rnd(3) * 1000000ll * (int64_t)(1 + rnd(40));
      ts[i] = rnd(97) ? t : t - 5000000000ll;
      lim[i] = rnd(7) ? L : L2;
    }
    int64_t s0[3] = {(int64_t)rnd(2), (int64_t)rnd(900), ts[0] - (int64_t)rnd(3) * I / 2}, s1[3];
    memcpy(s1, s0, sizeof s0);
    std::vector<uint8_t> o0(n), o1(n);
    closed += bjx_test_wave_run(n, ts.data(), iv.data(), lim.data(), s0, s1, o0.data(), o1.data());
    if (memcmp(s0, s1, sizeof s0) || memcmp(o0.data(), o1.data(), n)) ++bad;
  }
  printf("wave_runs: 20000 runs, %llu closed-form chunks, %llu mismatches\n", (unsigned long long)closed, (unsigned long long)bad);
  return bad ? 1 : 0;
}
#endif
