// Per-rule statistics of a batch (BJX_RULE_STATS, bjx_batch_rule_stats /
// bjx_rule_stats_total; include/banjax_gpu.h, DESIGN.md §2 "Rule statistics").
//
// Included by engine.hip at file scope (the same translation unit), after
// bjx_engine, guarded() and the rate-limit stage, before finish_phase, which
// calls rule_stats_launch once the trips are built and rule_stats_collect
// after its stream wait.  It relies on Bind / Lines (engine_types.h), is_skip
// and kBlock.
//
// A batch's RuleResults exist as one mask of rule positions per line
// (Lines::mword) and its trips as bjx_trip records; both are counted where
// they lie and 3 x 8 B per rule come back:
//   k_rule_hist        one pass over the lines with results: matches and
//                      SkipHost matches per rule
//   k_rule_hist_trips  one pass over the built trips: trips per rule
// Both bin into u32 counters in LDS (a block sees fewer than 2^32 lines, so a
// bin cannot wrap) and flush their non-zero bins to the u64 global counters
// with one atomic each; a ruleset whose bins do not fit the LDS a block may
// have (or bjx_debug_set_rule_stats_lds) adds straight to the global counters.
//
// What decides the design is one bin hit by every lane: a global `.*` rule
// matches every line, and most trips of a burst name one rule, so a lane per
// set bit would serialise its LDS atomics 64-way.  Global positions are the
// same rule for every line once shifted by the line's nsite, so a wave takes
// each global rule some lane has set with one ballot and a popcount and one
// lane adds the sums: one LDS operation per distinct rule of the wave, not per
// match.  Per-site positions are sparse and host-dependent: lane-private
// atomics.  The trips are grouped by rule in the wave the same way.
#pragma once

namespace {

constexpr uint32_t kRuleHistLdsMax = 128 * 1024;             // dynamic LDS a block may ask for (of gfx950's 160 KiB)
constexpr uint32_t kRuleHistMaxRules = kRuleHistLdsMax / 8;  // two u32 bins per rule
constexpr unsigned kRuleHistGrid = 2048;                     // blocks at most (each flushes its bins once)

// A line's scope: which rules its mask positions mean and which of them are
// HostsToSkip for its host.  Positions resolve as k_emit resolves them: the
// host's per-site rules first, then the global ones; skip from the scope's
// sc_skip words below position 128, from is_skip past it.  This is a second
// copy of that rule, not a shared one: k_emit keeps its own lines (it is not
// to be touched here) and the two can drift apart.  What binds them is the
// host's check of the sums against the batch's n_results / n_events, which
// k_emit's side of the pipeline produced, and the tests against the oracle.
// One difference on purpose: k_rule_hist masks off bits at or past the scope
// (nsite for the site part, n_global for the global part) before it indexes
// site_rules / global_rules; k_emit trusts the mask words to be clear there.
struct LineScope {
  int32_t hid;
  uint32_t s_begin, nsite, napp;
  uint64_t k0, k1;
};
__device__ __forceinline__ LineScope line_scope(const Bind &B, const Lines &L, uint64_t j) {
  LineScope S;
  S.hid = L.host_id[j];
  uint32_t s_end = 0;
  S.s_begin = 0;
  if (S.hid >= 0) { S.s_begin = B.site_off[S.hid]; s_end = B.site_off[S.hid + 1]; }
  S.nsite = s_end - S.s_begin;
  S.napp = S.nsite + B.n_global;
  const uint32_t sc = S.hid >= 0 ? (uint32_t)S.hid : B.n_hosts;
  S.k0 = B.sc_skip[2 * sc];
  S.k1 = B.sc_skip[2 * sc + 1];
  return S;
}
__device__ __forceinline__ bool scope_skip(const Bind &B, const LineScope &S, uint32_t pos, uint32_t r) {
  return pos < 128 ? (((pos < 64 ? S.k0 >> pos : S.k1 >> (pos - 64)) & 1) != 0) : is_skip(B, r, S.hid);
}

// the bins of one block: u32 in LDS, or the u64 global counters themselves
template <bool LDS>
struct RuleBins;
template <>
struct RuleBins<true> {
  uint32_t *b;
  __device__ __forceinline__ void add(uint32_t i, uint32_t v) const { atomicAdd(&b[i], v); }
};
template <>
struct RuleBins<false> {
  unsigned long long *b;
  __device__ __forceinline__ void add(uint32_t i, uint32_t v) const { atomicAdd(&b[i], (unsigned long long)v); }
};

template <bool LDS>
__device__ __forceinline__ RuleBins<LDS> bins_open(uint32_t *lds, unsigned long long *g, uint32_t n) {
  RuleBins<LDS> R;
  if constexpr (LDS) {
    for (uint32_t i = threadIdx.x; i < n; i += kBlock) lds[i] = 0;
    __syncthreads();
    R.b = lds;
  } else {
    R.b = g;
  }
  return R;
}
template <bool LDS>
__device__ __forceinline__ void bins_flush(const uint32_t *lds, unsigned long long *g, uint32_t n) {
  if constexpr (LDS) {
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += kBlock) {
      const uint32_t v = lds[i];
      if (v) atomicAdd(&g[i], (unsigned long long)v);
    }
  }
}

// g[r] += RuleResults of rule r, g[n_rules + r] += the SkipHost ones among
// them, over the lines with results.  Nothing is written per line.  Every
// lane of a wave runs the same rounds (the ballots need the whole wave); a
// lane past the last line, or whose line has no result, holds an empty mask.
template <bool LDS>
__global__ __launch_bounds__(kBlock) void k_rule_hist(Bind B, uint64_t n_lines, Lines L, unsigned long long *__restrict__ g) {
  extern __shared__ uint32_t rh_bins[];
  const uint32_t nr = B.n_rules;
  const RuleBins<LDS> R = bins_open<LDS>(rh_bins, g, 2 * nr);
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t base = (uint64_t)blockIdx.x * kBlock + (threadIdx.x & ~63u); base < n_lines; base += stride) {
    const uint64_t j = base + lane;
    const bool live = j < n_lines && L.counts[j] != 0;
    LineScope S{};
    if (live) {
      S = line_scope(B, L, j);
      // per-site positions: sparse and host-dependent, one atomic per match
      for (uint32_t w = 0; w * 64 < S.nsite; ++w) {
        uint64_t m = L.mword(j, w);
        if (S.nsite - w * 64 < 64) m &= (1ull << (S.nsite - w * 64)) - 1;
        while (m) {
          const uint32_t pos = w * 64 + (uint32_t)__ffsll((unsigned long long)m) - 1;
          m &= m - 1;
          const uint32_t r = B.site_rules[S.s_begin + pos];
          if (r >= nr) continue;  // (never: the host check of the sums would tell)
          R.add(r, 1);
          if (scope_skip(B, S, pos, r)) R.add(nr + r, 1);
        }
      }
    }
    // global positions, 64 at a time: bit b of gm is global rule g0 + b for
    // every lane, whatever the line's nsite
    for (uint32_t g0 = 0; g0 < B.n_global; g0 += 64) {
      uint64_t gm = 0;
      if (live) {
        const uint32_t p0 = S.nsite + g0, w = p0 >> 6, s = p0 & 63;
        gm = L.mword(j, w) >> s;
        if (s && (w + 1) * 64 < S.napp) gm |= L.mword(j, w + 1) << (64 - s);
        if (B.n_global - g0 < 64) gm &= (1ull << (B.n_global - g0)) - 1;
      }
      for (;;) {
        const uint64_t any = __ballot(gm != 0);
        if (!any) break;
        const uint32_t lead = (uint32_t)__ffsll((unsigned long long)any) - 1;
        const uint32_t b = (uint32_t)__shfl((int)((uint32_t)__ffsll((unsigned long long)gm) - 1), (int)lead) & 63;
        const bool has = ((gm >> b) & 1) != 0;
        const uint32_t r = B.global_rules[g0 + b];
        const bool skip = has && scope_skip(B, S, S.nsite + g0 + b, r);
        const uint64_t hm = __ballot(has), sm = __ballot(skip);
        if (lane == lead && r < nr) {
          R.add(r, (uint32_t)__popcll((unsigned long long)hm));
          if (sm) R.add(nr + r, (uint32_t)__popcll((unsigned long long)sm));
        }
        gm &= ~(1ull << b);
      }
    }
  }
  bins_flush<LDS>(rh_bins, g, 2 * nr);
}

// g[r] += trips of rule r.  A wave groups its trips by rule: the first live
// lane's rule, a ballot of the lanes that hold the same one, one add.
template <bool LDS>
__global__ __launch_bounds__(kBlock) void k_rule_hist_trips(uint64_t n, const bjx_trip *__restrict__ t, uint32_t nr,
                                                            unsigned long long *__restrict__ g) {
  extern __shared__ uint32_t rh_bins[];
  const RuleBins<LDS> R = bins_open<LDS>(rh_bins, g, nr);
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t stride = (uint64_t)gridDim.x * kBlock;
  for (uint64_t base = (uint64_t)blockIdx.x * kBlock + (threadIdx.x & ~63u); base < n; base += stride) {
    const uint64_t i = base + lane;
    const uint32_t r = i < n ? t[i].rule_idx : nr;
    bool live = r < nr;  // (a rule past the ruleset: never; the host check of the sums would tell)
    for (;;) {
      const uint64_t any = __ballot(live);
      if (!any) break;
      const uint32_t lead = (uint32_t)__ffsll((unsigned long long)any) - 1;
      const uint32_t rr = (uint32_t)__shfl((int)r, (int)lead);
      const bool same = live && r == rr;
      const uint64_t sm = __ballot(same);
      if (lane == lead) R.add(rr, (uint32_t)__popcll((unsigned long long)sm));
      live = live && !same;
    }
  }
  bins_flush<LDS>(rh_bins, g, nr);
}

// ------------------------------------------------------------------ host

// finish_phase, the trips built and the masks still current: zero the
// counters, count, queue the copy.  Only for a batch with results.
void rule_stats_launch(bjx_engine *e, uint64_t n_trips) {
  const Bind &B = e->bind;
  const BatchCtx &c = e->bc;
  hipStream_t st = e->stream;
  const uint32_t nr = c.rs_rules;
  if (B.n_rules != nr) throw BjxError(BJX_ERR_DEVICE, "internal: rule stats: the bound ruleset is not the batch's");
  if (!e->rs_ev[0])
    for (auto &x : e->rs_ev) HIP_OK(hipEventCreate(&x));
  e->rs_cnt.ensure(3 * (size_t)nr);
  e->rs_pin.resize(3 * (size_t)nr);
  unsigned long long *g = e->rs_cnt.p;
  HIP_OK(hipEventRecord(e->rs_ev[0], st));
  HIP_OK(hipMemsetAsync(g, 0, 3 * (size_t)nr * 8, st));
  const uint32_t max_rules = e->rs_lds_rules ? std::min(e->rs_lds_rules, kRuleHistMaxRules) : kRuleHistMaxRules;
  const bool lds = nr <= max_rules;
  e->rs_path = lds ? 1 : 2;
  {
    const unsigned grid = (unsigned)std::min<uint64_t>(grid_for(c.n_lines), kRuleHistGrid);
    if (lds) {
      const uint32_t bytes = 8 * nr;
      if (bytes > 64 * 1024 && bytes > e->rs_lds_set) {  // past the 64 KB of dynamic LDS a kernel has by default
        HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_rule_hist<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                   (int)bytes));
        e->rs_lds_set = bytes;
      }
      hipLaunchKernelGGL(k_rule_hist<true>, dim3(grid), dim3(kBlock), bytes, st, B, c.n_lines, c.L, g);
    } else {
      hipLaunchKernelGGL(k_rule_hist<false>, dim3(grid), dim3(kBlock), 0, st, B, c.n_lines, c.L, g);
    }
    HIP_OK(hipGetLastError());
  }
  if (n_trips) {
    const unsigned grid = (unsigned)std::min<uint64_t>(grid_for(n_trips), kRuleHistGrid);
    if (lds) {  // 4 B per rule: never past the 64 KB a kernel has by default
      hipLaunchKernelGGL(k_rule_hist_trips<true>, dim3(grid), dim3(kBlock), 4 * nr, st, n_trips, e->d_trips.p, nr, g + 2 * (size_t)nr);
    } else {
      hipLaunchKernelGGL(k_rule_hist_trips<false>, dim3(grid), dim3(kBlock), 0, st, n_trips, e->d_trips.p, nr, g + 2 * (size_t)nr);
    }
    HIP_OK(hipGetLastError());
  }
  HIP_OK(hipEventRecord(e->rs_ev[1], st));
  if (nr) HIP_OK(hipMemcpyAsync(e->rs_pin.data(), g, 3 * (size_t)nr * 8, hipMemcpyDeviceToHost, st));
}

// After the stream wait: the rows of the batch (zeros when nothing was
// launched: no results), their sums against the batch's own counts, then the
// totals.  rs_counted is set last: a failed check leaves no answer behind.
void rule_stats_collect(bjx_engine *e, bool launched, uint64_t n_trips) {
  const BatchCtx &c = e->bc;
  const size_t nr = c.rs_rules;
  e->rs_last.assign(nr, bjx_rule_stat{});
  double ms = 0;
  uint64_t sm = 0, ss = 0, stp = 0;
  if (launched) {
    float x = 0;
    HIP_OK(hipEventElapsedTime(&x, e->rs_ev[0], e->rs_ev[1]));
    ms = x;
    const uint64_t *m = e->rs_pin.data(), *s = m + nr, *t = s + nr;
    for (size_t r = 0; r < nr; ++r) {
      e->rs_last[r] = bjx_rule_stat{m[r], s[r], t[r]};
      sm += m[r]; ss += s[r]; stp += t[r];
    }
  }
  if (sm != c.n_res || sm - ss != c.n_ev || stp != n_trips) {
    char msg[256];
    snprintf(msg, sizeof msg, "internal: rule stats count %llu matches, %llu events, %llu trips; the batch has %llu RuleResults, "
             "%llu events, %llu trips", (unsigned long long)sm, (unsigned long long)(sm - ss), (unsigned long long)stp,
             (unsigned long long)c.n_res, (unsigned long long)c.n_ev, (unsigned long long)n_trips);
    throw BjxError(BJX_ERR_DEVICE, msg);
  }
  if (!launched) e->rs_path = 0;
  e->rs_last_ms = ms;
  e->rs_last_lines = c.n_lines;
  if (e->rs_uid != c.rs_uid || e->rs_total.size() != nr) {  // another ruleset: its rule indices are another thing
    e->rs_total.assign(nr, bjx_rule_stat{});
    e->rs_uid = c.rs_uid;
    e->rs_batches = e->rs_lines = 0;
    e->rs_ms = 0;
  }
  for (size_t r = 0; r < nr; ++r) {
    e->rs_total[r].matches += e->rs_last[r].matches;
    e->rs_total[r].skip_host += e->rs_last[r].skip_host;
    e->rs_total[r].trips += e->rs_last[r].trips;
  }
  ++e->rs_batches;
  e->rs_lines += c.n_lines;
  e->rs_ms += ms;
  e->rs_counted = true;
}

// a batch closed without reaching finish_phase (no bytes, no complete line)
void rule_stats_close_empty(bjx_engine *e, uint32_t flags) {
  e->rs_counted = false;
  if (flags & BJX_RULE_STATS) rule_stats_collect(e, false, 0);
}

}  // namespace

extern "C" int bjx_batch_rule_stats(bjx_engine *e, bjx_rule_stats *out) {
  if (!out) return BJX_ERR_ARG;
  return guarded(e, [&]() -> int {
    memset(out, 0, sizeof *out);
    if (!e->rs_counted) throw BjxError(BJX_ERR_ARG, "bjx_batch_rule_stats: the last batch ran without BJX_RULE_STATS");
    out->n_rules = e->rs_last.size();
    out->rules = out->n_rules ? e->rs_last.data() : nullptr;
    out->n_batches = 1;
    out->n_lines = e->rs_last_lines;
    out->device_ms = e->rs_last_ms;
    return BJX_OK;
  });
}

extern "C" int bjx_rule_stats_total(bjx_engine *e, bjx_rule_stats *out) {
  if (!out) return BJX_ERR_ARG;
  return guarded(e, [&]() -> int {
    memset(out, 0, sizeof *out);
    if (!e->rs_uid) return BJX_OK;  // no flagged batch yet
    out->n_rules = e->rs_total.size();
    out->rules = out->n_rules ? e->rs_total.data() : nullptr;
    out->n_batches = e->rs_batches;
    out->n_lines = e->rs_lines;
    out->device_ms = e->rs_ms;
    return BJX_OK;
  });
}

extern "C" int bjx_rule_stats_reset(bjx_engine *e) {
  return guarded(e, [&]() -> int {
    e->rs_total.clear();
    e->rs_uid = 0;
    e->rs_batches = e->rs_lines = 0;
    e->rs_ms = 0;
    return BJX_OK;
  });
}
