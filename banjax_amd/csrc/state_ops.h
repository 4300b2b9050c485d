// The state path around the hot one: everything that replaces or walks the
// rate-limit tables in HBM outside a batch's claim / apply kernels -- rollback,
// growth, clear, expiry, snapshot export / import, query, Get, dump.
//
// Included by engine.hip at file scope (the same translation unit), after
// bjx_engine, the pinned reads (pin_get / pin_sync / read_counters), cub_call
// and guarded(), and before bjx_engine_create and the rate-limit stage, which
// call alloc_state / free_state, ensure_capacity and grow_*.  It relies on
// engine.hip's device helpers (bytes_eq, ip_key16_bytes, key16_eq,
// block_alloc, block_sum2), on State / IpSlot / StSlot (engine_types.h), the
// sizing rule (bjx_common.h), snapshot.h and state_query.h.
//
// Every rebuild of the tables goes through the same pieces:
//   fresh_put_ip / fresh_put_st   insert into a table only this rebuild writes
//   copy_ip_bytes                 one kept IP's bytes under its new id
//   mark_and_scan / scan_kept     keep[], dense new ids, arena offsets, totals
//   NewTables                     the new arrays, owned until installed
//   install                       the swap and everything it resets
//   rebuild_kept                  expiry's and removal's second half: new tables, kept IPs and states, the swap
#pragma once

namespace {

// ------------------------------------------------------------------ kernels

// Insert into a fresh table: every slot starts empty and only this rebuild
// writes it, so a CAS on the first word claims a slot and plain stores fill
// the rest (nothing reads the table before the rebuild's kernels have ended).
// Equal hashes of distinct IPs take successive slots.
__device__ __forceinline__ void fresh_put_ip(IpSlot *__restrict__ nt, uint64_t nmask, uint64_t hash, uint32_t id, uint32_t born,
                                             const uint4 &key16) {
  for (uint64_t j = hash & nmask;; j = (j + 1) & nmask)
    if (atomicCAS((unsigned long long *)&nt[j].hash, 0ull, (unsigned long long)hash) == 0) {
      nt[j].id = id; nt[j].born = born; nt[j].key16 = key16;
      return;
    }
}
__device__ __forceinline__ void fresh_put_st(StSlot *__restrict__ nt, uint64_t nmask, uint64_t key, int64_t hits, int64_t start,
                                             uint64_t valid) {
  for (uint64_t j = mix64(key) & nmask;; j = (j + 1) & nmask)
    if (atomicCAS((unsigned long long *)&nt[j].key, 0ull, (unsigned long long)key) == 0) {
      nt[j].hits = hits; nt[j].start = start; nt[j].valid = valid;
      return;
    }
}
// src[so, so + len) -> dst[d, d + len); false, and nothing written, when
// either range leaves its buffer (not from a finished batch / a checked
// snapshot: never taken)
__device__ __forceinline__ bool copy_ip_bytes(uint8_t *__restrict__ dst, uint64_t d, uint64_t dst_cap,
                                              const uint8_t *__restrict__ src, uint64_t so, uint64_t src_used, uint32_t len) {
  if (so + len > src_used || d + len > dst_cap) return false;
  for (uint32_t k = 0; k < len; ++k) dst[d + k] = src[so + k];
  return true;
}

// undo one batch's claims (table overflow): its slots were empty before the
// batch and no earlier key's probe chain runs through them
__global__ void k_ip_rollback(uint64_t cap, State S, uint32_t epoch) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap) return;
  const IpSlot v = S.ip[i];
  if (v.hash != 0 && (v.born == epoch || v.born == 0)) {
    S.ip[i] = IpSlot{};
    S.ip_first[i] = 0xFFFFFFFFu;
  }
}
__global__ void k_st_rollback(uint64_t cap, State S) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cap) return;
  const bool live = S.st[i].key != 0 && S.st[i].valid != 0;
  if (S.st[i].key != 0 && !live) S.st[i] = StSlot{};
  const uint64_t m = __ballot(live);
  if (m && (threadIdx.x & 63) == (uint32_t)(__ffsll((unsigned long long)m) - 1))
    atomicAdd((unsigned long long *)&S.counters[2], (unsigned long long)__popcll(m));
}

// rehash (table growth)
__global__ void k_rehash_ip(uint64_t old_cap, const IpSlot *__restrict__ o, IpSlot *__restrict__ nt, uint64_t nmask) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= old_cap || o[i].hash == 0) return;
  const IpSlot v = o[i];
  fresh_put_ip(nt, nmask, v.hash, v.id, v.born, v.key16);
}
__global__ void k_rehash_st(uint64_t old_cap, const StSlot *__restrict__ o, StSlot *__restrict__ nt, uint64_t nmask) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= old_cap || o[i].key == 0) return;
  const StSlot v = o[i];
  fresh_put_st(nt, nmask, v.key, v.hits, v.start, v.valid);
}

// expiry (bjx_state_expire): a rebuild into fresh tables that drops every
// state whose window started before the cutoff and every IP left without one.
// IP ids stay dense and in first-seen order: keep[id] marks the IPs with a
// surviving state, its exclusive scan is the new id, the scan of the kept
// lengths the new arena offset.
__device__ __forceinline__ bool st_survives(const StSlot &v, int64_t cutoff, uint64_t n_ips) {
  // (an id past n_ips cannot come from a finished batch: never followed)
  return v.key != 0 && v.valid != 0 && v.start >= cutoff && (v.key >> 24) - 1 < n_ips;
}
// grid-stride; cnt[0] += surviving states (one atomic per block)
__global__ __launch_bounds__(kBlock) void k_exp_mark(uint64_t st_cap, const StSlot *__restrict__ st, int64_t cutoff,
                                                     uint64_t n_ips, uint32_t *__restrict__ keep,
                                                     unsigned long long *__restrict__ cnt) {
  uint64_t n = 0, z = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < st_cap; i += (uint64_t)gridDim.x * blockDim.x) {
    const StSlot v = st[i];
    if (st_survives(v, cutoff, n_ips)) {
      keep[(v.key >> 24) - 1] = 1u;  // every writer stores the same value
      ++n;
    }
  }
  block_sum2(n, z);
  if (threadIdx.x == 0 && n) atomicAdd(&cnt[0], (unsigned long long)n);
}
// klen[id] = the arena bytes IP id keeps, over [0, n_ips] (the last entry 0:
// the scans' totals land there)
__global__ void k_exp_len(uint64_t n_ips, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ ip_len,
                          uint64_t *__restrict__ klen) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n_ips) return;
  klen[i] = i < n_ips && keep[i] ? ip_len[i] : 0;
}
// kept IP id -> its bytes, offset and length under the new id
__global__ void k_exp_arena(uint64_t n_ips, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ nid,
                            const uint64_t *__restrict__ noff, const uint64_t *__restrict__ o_off,
                            const uint32_t *__restrict__ o_len, const uint8_t *__restrict__ o_arena, uint64_t o_used,
                            uint8_t *__restrict__ n_arena, uint64_t n_arena_cap, uint64_t *__restrict__ n_off,
                            uint32_t *__restrict__ n_len) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ips || !keep[i]) return;
  const uint32_t len = o_len[i];
  const uint64_t d = noff[i];
  if (!copy_ip_bytes(n_arena, d, n_arena_cap, o_arena, o_off[i], o_used, len)) return;
  n_off[nid[i]] = d;
  n_len[nid[i]] = len;
}
__global__ void k_exp_st(uint64_t old_cap, const StSlot *__restrict__ o, int64_t cutoff, uint64_t n_ips,
                         const uint32_t *__restrict__ nid, StSlot *__restrict__ nt, uint64_t nmask) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= old_cap) return;
  const StSlot v = o[i];
  if (!st_survives(v, cutoff, n_ips)) return;
  const uint64_t key = ((uint64_t)(nid[(v.key >> 24) - 1] + 1) << 24) | (v.key & 0xFFFFFFull);
  fresh_put_st(nt, nmask, key, v.hits, v.start, v.valid);
}
__global__ void k_exp_ip(uint64_t old_cap, const IpSlot *__restrict__ o, uint64_t n_ips, const uint32_t *__restrict__ keep,
                         const uint32_t *__restrict__ nid, IpSlot *__restrict__ nt, uint64_t nmask) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= old_cap) return;
  const IpSlot v = o[i];
  if (v.hash == 0 || v.id >= n_ips || !keep[v.id]) return;
  fresh_put_ip(nt, nmask, v.hash, nid[v.id], v.born, v.key16);
}
__global__ void k_exp_counters(uint64_t *__restrict__ counters, uint64_t ips, uint64_t bytes, uint64_t states) {
  if (blockIdx.x || threadIdx.x) return;
  counters[0] = ips;
  counters[1] = bytes;
  counters[2] = states;
}

// snapshot export (bjx_state_export; format: snapshot.h).  keep / nid / noff
// come from expiry's mark, length and scan passes with min_start_ns as the
// cutoff.  k_snap_compact gathers the surviving slots, in any order, as
// (key = new IP id << 24 | name id, index, {hits, start}) and marks the name
// ids in use; the host sorts the used names and k_snap_remap rewrites the name
// bits to the canonical index; a radix sort over the key bits in use orders the
// records by (ip, name); k_snap_gather writes them, k_snap_ips the IP section.
// One atomic per block and pass (block_alloc); every block runs the same
// number of passes.
__global__ __launch_bounds__(kBlock) void k_snap_compact(uint64_t st_cap, const StSlot *__restrict__ st, int64_t cutoff,
                                                         uint64_t n_ips, const uint32_t *__restrict__ nid, uint32_t n_names,
                                                         uint32_t *__restrict__ used, unsigned long long *__restrict__ ctr,
                                                         uint64_t room, uint64_t *__restrict__ keys,
                                                         uint32_t *__restrict__ idx, int64_t *__restrict__ pay) {
  for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < st_cap; base += (uint64_t)gridDim.x * kBlock) {
    const uint64_t i = base + threadIdx.x;
    StSlot v{};
    bool live = false;
    if (i < st_cap) {
      v = st[i];
      live = st_survives(v, cutoff, n_ips) && (v.key & 0xFFFFFFull) < n_names;
    }
    const uint64_t k = block_alloc(ctr, live ? 1 : 0);
    if (live && k < room) {
      const uint32_t name = (uint32_t)(v.key & 0xFFFFFFull);
      used[name] = 1u;  // every writer stores the same value
      keys[k] = ((uint64_t)nid[(v.key >> 24) - 1] << 24) | name;
      idx[k] = (uint32_t)k;
      pay[2 * k] = v.hits;
      pay[2 * k + 1] = v.start;
    }
  }
}
__global__ void k_snap_remap(uint64_t n, uint64_t *__restrict__ keys, const uint32_t *__restrict__ remap) {
  const uint64_t k = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n) return;
  const uint64_t v = keys[k];
  keys[k] = (v & ~0xFFFFFFull) | remap[v & 0xFFFFFFull];
}
// sorted (key, index) -> the 24-byte record {u32 ip, u32 name, i64 hits, i64 start} as three words
__global__ void k_snap_gather(uint64_t n, const uint64_t *__restrict__ keys, const uint32_t *__restrict__ idx,
                              const int64_t *__restrict__ pay, uint64_t *__restrict__ recs) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint64_t key = keys[j], s = idx[j];
  if (s >= n) return;  // (a permutation of [0, n): never taken)
  recs[3 * j] = (key >> 24) | ((key & 0xFFFFFFull) << 32);
  recs[3 * j + 1] = (uint64_t)pay[2 * s];
  recs[3 * j + 2] = (uint64_t)pay[2 * s + 1];
}
// kept IP id -> its bytes and offset under the new id (k_exp_arena's shape); i = n_ips writes the end offset
__global__ void k_snap_ips(uint64_t n_ips, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ nid,
                           const uint64_t *__restrict__ noff, const uint64_t *__restrict__ o_off,
                           const uint32_t *__restrict__ o_len, const uint8_t *__restrict__ o_arena, uint64_t o_used,
                           uint64_t kept_ips, uint64_t kept_bytes, uint64_t *__restrict__ out_off,
                           uint8_t *__restrict__ out_bytes) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n_ips) return;
  if (i == n_ips) { out_off[kept_ips] = kept_bytes; return; }
  if (!keep[i]) return;
  const uint64_t d = noff[i];
  if (nid[i] >= kept_ips) return;  // (not from a finished batch)
  if (!copy_ip_bytes(out_bytes, d, kept_bytes, o_arena, o_off[i], o_used, o_len[i])) return;
  out_off[nid[i]] = d;
}

// state query (bjx_state_query; filter checks, sort key, name ranks, node
// merge: state_query.h).  A state that passes the filter becomes a 16-byte
// candidate {key_desc(primary), ip id << 24 | rank(name)}: ascending order of
// that 128-bit key is the order of the rows.  k_qry_scan reads the state table
// once (no ip filter), k_qry_ip probes one key per interned name (ip filter).
// Selection is an MSB-first radix select, 8 bits a pass: k_qry_hist counts the
// digits, the host picks the bucket the limit falls into, k_qry_filter moves
// the buckets below it to the selected rows and that bucket to the next pass's
// set.  What is left is sorted (two stable 64-bit sorts through an index) and
// k_qry_rows / k_qry_bytes write the rows.  One atomic per block and pass
// (block_alloc); every block runs the same number of passes.
constexpr int kQryItems = 4;  // k_qry_scan: state slots per thread and pass
struct QFilter {
  int64_t min_hits, min_start, max_start;
  uint32_t name;      // name id, kNone: every name
  uint32_t by_start;  // primary key: 0 hits, 1 start
};
// (an id past n_ips or n_names cannot come from a finished batch: never followed, as st_survives)
__device__ __forceinline__ bool q_pass(const StSlot &v, const QFilter &F, uint64_t n_ips, uint32_t n_names) {
  const uint32_t name = (uint32_t)(v.key & 0xFFFFFFull);
  return v.key != 0 && v.valid != 0 && (v.key >> 24) - 1 < n_ips && name < n_names && (F.name == kNone || name == F.name) &&
         v.hits >= F.min_hits && v.start >= F.min_start && v.start <= F.max_start;
}
__device__ __forceinline__ ulonglong2 q_cand(const StSlot &v, const QFilter &F, const uint32_t *__restrict__ rank) {
  return make_ulonglong2(bjx_query::key_desc(F.by_start ? v.start : v.hits),
                         (((v.key >> 24) - 1) << 24) | rank[v.key & 0xFFFFFFull]);
}
// grid-stride; cnt[0] += passing states (one atomic per block), keep[ip id] = 1;
// room != 0: the candidates appended at cnt[1].  sel != NULL (a nets query): a
// state passes only when sel[its IP id] is set, as rm_selected reads it
__global__ __launch_bounds__(kBlock) void k_qry_scan(uint64_t st_cap, const StSlot *__restrict__ st, QFilter F, uint64_t n_ips,
                                                     uint32_t n_names, const uint32_t *__restrict__ rank,
                                                     const uint32_t *__restrict__ sel, uint32_t *__restrict__ keep,
                                                     unsigned long long *__restrict__ cnt, uint64_t room,
                                                     ulonglong2 *__restrict__ cand) {
  uint64_t n = 0, z = 0;
  constexpr uint64_t kTile = (uint64_t)kBlock * kQryItems;  // slots per block and pass: one block_alloc for all of them
  for (uint64_t base = (uint64_t)blockIdx.x * kTile; base < st_cap; base += (uint64_t)gridDim.x * kTile) {
    ulonglong2 c[kQryItems];
    uint32_t mask = 0;  // bit j: slot j of this thread passes (c[j] set)
#pragma unroll
    for (int j = 0; j < kQryItems; ++j) {
      const uint64_t i = base + (uint64_t)j * kBlock + threadIdx.x;
      c[j] = make_ulonglong2(0, 0);
      if (i >= st_cap) continue;
      const StSlot v = st[i];
      if (!q_pass(v, F, n_ips, n_names) || (sel && !sel[(v.key >> 24) - 1])) continue;
      keep[(v.key >> 24) - 1] = 1u;  // every writer stores the same value
      if (room) c[j] = q_cand(v, F, rank);
      mask |= 1u << j;
    }
    n += __popc(mask);
    if (room) {
      uint64_t k = block_alloc(&cnt[1], __popc(mask));
#pragma unroll
      for (int j = 0; j < kQryItems; ++j)
        if ((mask >> j) & 1u) {
          if (k < room) cand[k] = c[j];
          ++k;
        }
    }
  }
  block_sum2(n, z);
  if (threadIdx.x == 0 && n) atomicAdd(&cnt[0], (unsigned long long)n);
}
// Get(ip): the IP as k_state_get finds it (hash, probe chain, length and arena
// bytes), then one lane per interned name id probes ((id + 1) << 24) | name
__global__ __launch_bounds__(kBlock) void k_qry_ip(State S, uint64_t h, const uint8_t *__restrict__ ip, uint32_t len, QFilter F,
                                                   uint64_t n_ips, uint32_t n_names, const uint32_t *__restrict__ rank,
                                                   unsigned long long *__restrict__ cnt, uint64_t room,
                                                   ulonglong2 *__restrict__ cand) {
  __shared__ uint32_t s_id;
  if (threadIdx.x == 0) {
    uint32_t id = kNone;
    for (uint64_t i = h & S.ip_mask;; i = (i + 1) & S.ip_mask) {
      const uint64_t cur = S.ip[i].hash;
      if (cur == 0) break;
      if (cur == h) {
        const uint32_t c = S.ip[i].id;
        if (c < n_ips && S.ip_len[c] == len && bytes_eq(S.arena + S.ip_off[c], ip, len)) { id = c; break; }
      }
    }
    s_id = id;
  }
  __syncthreads();
  const uint32_t id = s_id;
  uint64_t n = 0, z = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < n_names; base += (uint64_t)gridDim.x * kBlock) {
    const uint64_t name = base + threadIdx.x;
    StSlot v{};
    bool ok = false;
    if (id != kNone && name < n_names && (F.name == kNone || name == F.name)) {
      const uint64_t key = ((uint64_t)(id + 1) << 24) | name;
      for (uint64_t j = mix64(key) & S.st_mask;; j = (j + 1) & S.st_mask) {
        const uint64_t k = S.st[j].key;
        if (k == 0) break;
        if (k == key) {
          v = S.st[j];
          ok = q_pass(v, F, n_ips, n_names);
          break;
        }
      }
    }
    if (ok) ++n;
    if (room) {
      const uint64_t k = block_alloc(&cnt[1], ok ? 1 : 0);
      if (ok && k < room) cand[k] = q_cand(v, F, rank);
    }
  }
  block_sum2(n, z);
  if (threadIdx.x == 0 && n) atomicAdd(&cnt[0], (unsigned long long)n);
}
__device__ __forceinline__ uint32_t q_digit(const ulonglong2 &c, uint32_t word, uint32_t shift) {
  return (uint32_t)(((word ? c.y : c.x) >> shift) & 0xFFu);
}
// hist[d] += candidates whose digit (8 bits at `shift` of word 0 primary / 1
// tie) is d.  A thread counts a run of equal digits before it touches LDS: the
// high bytes of small hit counts are all one value.
__global__ __launch_bounds__(kBlock) void k_qry_hist(const ulonglong2 *__restrict__ c, uint64_t n, uint32_t word, uint32_t shift,
                                                     unsigned long long *__restrict__ hist) {
  static_assert(kBlock == 256, "one histogram bin per thread");
  __shared__ uint32_t s_h[256];
  s_h[threadIdx.x] = 0;
  __syncthreads();
  uint32_t run_d = 0, run_n = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (uint64_t)gridDim.x * kBlock) {
    const uint32_t d = q_digit(c[i], word, shift);
    if (d != run_d && run_n) {
      atomicAdd(&s_h[run_d], run_n);
      run_n = 0;
    }
    run_d = d;
    ++run_n;
  }
  if (run_n) atomicAdd(&s_h[run_d], run_n);
  __syncthreads();
  if (s_h[threadIdx.x]) atomicAdd(&hist[threadIdx.x], (unsigned long long)s_h[threadIdx.x]);
}
// digit < b: selected (appended at ctr[0]); digit == b: the next pass's set (at ctr[1]); above: dropped
__global__ __launch_bounds__(kBlock) void k_qry_filter(const ulonglong2 *__restrict__ c, uint64_t n, uint32_t word, uint32_t shift,
                                                       uint32_t b, ulonglong2 *__restrict__ sel, uint64_t sel_room,
                                                       ulonglong2 *__restrict__ nxt, uint64_t nxt_room,
                                                       unsigned long long *__restrict__ ctr) {
  for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < n; base += (uint64_t)gridDim.x * kBlock) {
    const uint64_t i = base + threadIdx.x;
    ulonglong2 v = make_ulonglong2(0, 0);
    uint32_t d = 256;
    if (i < n) {
      v = c[i];
      d = q_digit(v, word, shift);
    }
    const uint64_t k0 = block_alloc(&ctr[0], d < b ? 1 : 0);
    if (d < b && k0 < sel_room) sel[k0] = v;
    const uint64_t k1 = block_alloc(&ctr[1], d == b ? 1 : 0);
    if (d == b && k1 < nxt_room) nxt[k1] = v;
  }
}
__global__ void k_qry_split(uint64_t n, const ulonglong2 *__restrict__ c, uint64_t *__restrict__ tie, uint32_t *__restrict__ idx) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  tie[i] = c[i].y;
  idx[i] = (uint32_t)i;
}
__global__ void k_qry_prim(uint64_t n, const ulonglong2 *__restrict__ c, const uint32_t *__restrict__ idx,
                           uint64_t *__restrict__ prim) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t s = idx[j];
  prim[j] = s < n ? c[s].x : ~0ull;  // (a permutation of [0, n): always inside)
}
// row r = the r-th candidate in order: its state read back from the table,
// the lengths of its IP and name; lens[r] = the bytes it takes ([0, n_rows]:
// the last entry 0, the scan's total lands there)
__global__ void k_qry_rows(uint64_t n_rows, uint64_t n_cand, const ulonglong2 *__restrict__ c, const uint32_t *__restrict__ idx,
                           State S, uint64_t n_ips, uint32_t n_names, const uint32_t *__restrict__ by_rank,
                           const uint64_t *__restrict__ name_off, bjx_state_row *__restrict__ rows,
                           uint64_t *__restrict__ lens) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r > n_rows) return;
  if (r == n_rows) { lens[r] = 0; return; }
  bjx_state_row o{};
  const uint32_t s = idx[r];
  if (s < n_cand) {
    const uint64_t tie = c[s].y, id = tie >> 24;
    const uint32_t rk = (uint32_t)(tie & 0xFFFFFFull);
    if (id < n_ips && rk < n_names) {
      const uint64_t key = ((id + 1) << 24) | by_rank[rk];
      for (uint64_t j = mix64(key) & S.st_mask;; j = (j + 1) & S.st_mask) {
        const uint64_t k = S.st[j].key;
        if (k == 0) break;
        if (k == key) { o.hits = S.st[j].hits; o.start_ns = S.st[j].start; break; }
      }
      o.ip_len = S.ip_len[id];
      o.name_len = (uint32_t)(name_off[rk + 1] - name_off[rk]);
    }
  }
  rows[r] = o;
  lens[r] = (uint64_t)o.ip_len + o.name_len;
}
// the rows' offsets and their bytes: IP, then name, at offs[r]
__global__ void k_qry_bytes(uint64_t n_rows, uint64_t n_cand, const ulonglong2 *__restrict__ c, const uint32_t *__restrict__ idx,
                            State S, uint64_t n_ips, uint64_t arena_used, const uint64_t *__restrict__ name_off,
                            const uint8_t *__restrict__ name_bytes, const uint64_t *__restrict__ offs, uint64_t total,
                            bjx_state_row *__restrict__ rows, uint8_t *__restrict__ out) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  const uint32_t s = idx[r];
  const uint32_t il = rows[r].ip_len, nl = rows[r].name_len;
  const uint64_t d = offs[r];
  rows[r].ip_off = d;
  rows[r].name_off = d + il;
  if (s >= n_cand || d + il + nl > total) return;  // (not from a finished batch)
  const uint64_t tie = c[s].y, id = tie >> 24;
  if (id >= n_ips) return;
  const uint64_t so = S.ip_off[id];
  if (so + il > arena_used) return;
  for (uint32_t k = 0; k < il; ++k) out[d + k] = S.arena[so + k];
  if (!nl) return;  // (nl != 0: k_qry_rows found the rank inside the table)
  const uint64_t no = name_off[tie & 0xFFFFFFull];
  for (uint32_t k = 0; k < nl; ++k) out[d + il + k] = name_bytes[no + k];
}

// removal (bjx_state_remove; argument checks, the packed list, the node's sum:
// state_remove.h): the expiry's rebuild with another predicate.  A state goes
// when the query's filter passes it and, with a list, sel[its IP id] is set;
// k_rm_ips sets sel[] from the listed bytes, k_rm_mark is k_exp_mark and
// k_rm_st is k_exp_st with that predicate.  Everything between them is the
// expiry's own (k_exp_len, scan_kept, k_exp_arena, k_exp_ip, install).
//
// One lane per listed IP, entries [first, first + n_list) of the packed list
// (entry k: bytes[off[k], off[k + 1]); 4 readable bytes past the last one for
// hash_bytes' word loads).  The IP is looked up as ip_claim_line looks up an IP
// of an earlier batch and k_imp_verify checks one: hash (under the debug mask
// as k_imp_place applies it), key16, arena bytes past 15 bytes, id < n_ips.
// sel[id] = 1: every writer stores the same value.
__global__ void k_rm_ips(uint32_t first, uint32_t n_list, const uint32_t *__restrict__ off, const uint8_t *__restrict__ bytes,
                         uint64_t hmask, const IpSlot *__restrict__ ipt, uint64_t ip_mask, uint64_t n_ips,
                         const uint64_t *__restrict__ ip_off, const uint32_t *__restrict__ ip_len,
                         const uint8_t *__restrict__ arena, uint64_t arena_used, uint32_t *__restrict__ sel) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_list) return;
  const uint32_t a = off[first + i], len = off[first + i + 1] - a;
  const uint8_t *src = bytes + a;
  const uint4 k16 = ip_key16_bytes(src, len);
  uint64_t h = hash_bytes(src, len);
  if (hmask) h = (h & hmask) | 1ull;
  uint64_t j = h & ip_mask;
  for (uint64_t step = 0; step <= ip_mask; ++step) {
    const IpSlot v = ipt[j];
    if (v.hash == 0) return;
    if (v.hash == h && v.id < n_ips && key16_eq(v.key16, k16)) {
      bool same = len <= 15;
      if (!same && ip_len[v.id] == len) {
        const uint64_t so = ip_off[v.id];
        same = so + len <= arena_used && bytes_eq(arena + so, src, len);
      }
      if (same) {
        sel[v.id] = 1u;
        return;  // (an IP has one slot)
      }
    }
    j = (j + 1) & ip_mask;
  }
}
// the one predicate of the mark and the re-insert: v (live) is to be dropped
__device__ __forceinline__ bool rm_selected(const StSlot &v, const QFilter &F, uint64_t n_ips, uint32_t n_names,
                                            const uint32_t *__restrict__ sel) {
  return q_pass(v, F, n_ips, n_names) && (!sel || sel[(v.key >> 24) - 1]);
}
// grid-stride; a live slot that is not selected keeps its IP (keep[id] = 1);
// cnt[0] += states kept, cnt[1] += states selected (one atomic each per block)
__global__ __launch_bounds__(kBlock) void k_rm_mark(uint64_t st_cap, const StSlot *__restrict__ st, QFilter F, uint64_t n_ips,
                                                    uint32_t n_names, const uint32_t *__restrict__ sel,
                                                    uint32_t *__restrict__ keep, unsigned long long *__restrict__ cnt) {
  uint64_t kept = 0, gone = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < st_cap; i += (uint64_t)gridDim.x * blockDim.x) {
    const StSlot v = st[i];
    if (!st_survives(v, INT64_MIN, n_ips)) continue;
    if (rm_selected(v, F, n_ips, n_names, sel)) {
      ++gone;
    } else {
      keep[(v.key >> 24) - 1] = 1u;  // every writer stores the same value
      ++kept;
    }
  }
  block_sum2(kept, gone);
  if (threadIdx.x == 0 && kept) atomicAdd(&cnt[0], (unsigned long long)kept);
  if (threadIdx.x == 0 && gone) atomicAdd(&cnt[1], (unsigned long long)gone);
}
// the live, unselected slots under their IPs' new ids (k_exp_st's shape: the
// payload stores stay outside fresh_put_st's probe loop)
__global__ void k_rm_st(uint64_t old_cap, const StSlot *__restrict__ o, QFilter F, uint64_t n_ips, uint32_t n_names,
                        const uint32_t *__restrict__ sel, const uint32_t *__restrict__ nid, StSlot *__restrict__ nt,
                        uint64_t nmask) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= old_cap) return;
  const StSlot v = o[i];
  if (!st_survives(v, INT64_MIN, n_ips) || rm_selected(v, F, n_ips, n_names, sel)) return;
  const uint64_t key = ((uint64_t)(nid[(v.key >> 24) - 1] + 1) << 24) | (v.key & 0xFFFFFFull);
  fresh_put_st(nt, nmask, key, v.hits, v.start, v.valid);
}

// selection by network (bjx_state_query_nets / bjx_state_remove_nets; the
// argument checks, the net table and the membership rule: state_nets.h).  One
// lane per held IP: its bytes are read in place from the arena (byte loads, no
// alignment and no length assumed: go_parse_addr reads [0, len) and nothing
// else) and parsed as check_is_allowed parses a line's IP; bjx_nets::member
// then runs one binary search per prefix length of the address's family over
// the table in global memory (1 MiB at BJX_NETS_MAX entries, L2-resident).
// An id past n_ips or bytes past arena_used cannot come from a finished batch
// and select nothing.
__device__ __forceinline__ bool net_ip_addr(uint64_t id, const uint64_t *__restrict__ ip_off, const uint32_t *__restrict__ ip_len,
                                            const uint8_t *__restrict__ arena, uint64_t arena_used, uint8_t a[16]) {
  const uint64_t so = ip_off[id];
  const uint32_t len = ip_len[id];
  if (so > arena_used || len > arena_used - so) return false;
  bool is4;
  return go_parse_addr(arena + so, len, a, &is4);
}
// grid-stride; sel[id] = 1 when a network holds IP id (sel[] zeroed before),
// cnt[0] += those IPs (one atomic per block)
__global__ __launch_bounds__(kBlock) void k_net_sel(uint64_t n_ips, const uint64_t *__restrict__ ip_off,
                                                    const uint32_t *__restrict__ ip_len, const uint8_t *__restrict__ arena,
                                                    uint64_t arena_used, bjx_nets::View V, uint32_t *__restrict__ sel,
                                                    unsigned long long *__restrict__ cnt) {
  uint64_t n = 0, z = 0;
  for (uint64_t id = (uint64_t)blockIdx.x * kBlock + threadIdx.x; id < n_ips; id += (uint64_t)gridDim.x * kBlock) {
    uint8_t a[16];
    if (!net_ip_addr(id, ip_off, ip_len, arena, arena_used, a)) continue;
    if (bjx_nets::member(V, a, [](uint32_t) { return true; })) {
      sel[id] = 1u;
      ++n;
    }
  }
  block_sum2(n, z);
  if (threadIdx.x == 0 && n) atomicAdd(&cnt[0], (unsigned long long)n);
}
// after the state scan: every IP with a selected state (keep[id], which the
// scan sets only where sel[id] is set) adds 1 to each canonical network that
// holds it (cnt[] has n_canon counters, zeroed before).  A wide network holds
// a large share of the IPs, and one global atomic per IP on its counter runs
// at the rate of one address; so a block counts in LDS first -- an
// open-addressed table of kNetLds (network, count) slots, claimed by CAS --
// over all the IPs it walks (few blocks, grid-stride) and adds each slot to the
// global counter once at the end.  A network that finds no slot within
// kNetProbe steps (more distinct networks in one block than the table holds:
// narrow ones, each with few IPs) is counted in global memory directly.
constexpr uint32_t kNetLds = 2048, kNetProbe = 16;
constexpr uint64_t kNetCountIps = 4096;  // held IPs per block of k_net_count (the grid is sized by it)
__global__ __launch_bounds__(kBlock) void k_net_count(uint64_t n_ips, const uint32_t *__restrict__ keep,
                                                      const uint64_t *__restrict__ ip_off, const uint32_t *__restrict__ ip_len,
                                                      const uint8_t *__restrict__ arena, uint64_t arena_used, bjx_nets::View V,
                                                      uint32_t n_canon, uint32_t *__restrict__ cnt) {
  __shared__ uint32_t s_key[kNetLds], s_cnt[kNetLds];
  for (uint32_t k = threadIdx.x; k < kNetLds; k += kBlock) {
    s_key[k] = kNone;
    s_cnt[k] = 0;
  }
  __syncthreads();
  for (uint64_t id = (uint64_t)blockIdx.x * kBlock + threadIdx.x; id < n_ips; id += (uint64_t)gridDim.x * kBlock) {
    if (!keep[id]) continue;
    uint8_t a[16];
    if (!net_ip_addr(id, ip_off, ip_len, arena, arena_used, a)) continue;
    bjx_nets::member(V, a, [&](uint32_t c) {
      if (c >= n_canon) return false;
      uint32_t h = (c * 2654435761u) >> 21;  // 11 bits: kNetLds slots
      for (uint32_t step = 0; step < kNetProbe; ++step, h = (h + 1) & (kNetLds - 1)) {
        const uint32_t was = atomicCAS(&s_key[h], kNone, c);
        if (was == kNone || was == c) {
          atomicAdd(&s_cnt[h], 1u);
          return false;
        }
      }
      atomicAdd(&cnt[c], 1u);
      return false;
    });
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < kNetLds; k += kBlock)
    if (s_key[k] != kNone && s_cnt[k]) atomicAdd(&cnt[s_key[k]], s_cnt[k]);
}
static_assert(kNetLds == 1u << 11, "k_net_count hashes to 11 bits");

// snapshot import (bjx_state_import).  err[c] = 1 (plain stores of one value)
// when check c fails: 1 ip_off not monotone from 0, 2 ip_off[n_ips] !=
// ip_bytes, 3 record ip >= n_ips, 4 record name >= n_names, 5 records not
// strictly ascending, 6 an IP without a record (the records are sorted by IP,
// so that is a first IP other than 0, a step over an index, or a last IP other
// than n_ips - 1), 0 (k_imp_verify) an IP found twice or not under its own id.
__global__ void k_imp_check(uint64_t n_ips, const uint64_t *__restrict__ ip_off, uint64_t ip_bytes, uint64_t n_states,
                            const uint64_t *__restrict__ recs, uint32_t n_names, uint32_t *__restrict__ used,
                            uint32_t *__restrict__ err) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i <= n_ips) {
    const uint64_t a = ip_off[i];
    if (i == 0 && a != 0) err[1] = 1u;
    if (i == n_ips) {
      if (a != ip_bytes) err[2] = 1u;
    } else {
      const uint64_t b = ip_off[i + 1];
      if (b < a || b - a > 0x7FFFFFFFull) err[1] = 1u;
    }
  }
  if (i < n_states) {
    const uint64_t w = recs[3 * i];
    const uint32_t ip = (uint32_t)w, nm = (uint32_t)(w >> 32);
    if (ip >= n_ips) err[3] = 1u;
    if (nm >= n_names) err[4] = 1u;
    else used[nm] = 1u;
    if (i) {
      const uint64_t pw = recs[3 * (i - 1)];
      const uint32_t pip = (uint32_t)pw, pnm = (uint32_t)(pw >> 32);
      if (ip < pip || (ip == pip && nm <= pnm)) err[5] = 1u;
      else if (ip - pip > 1) err[6] = 1u;
    } else if (ip != 0) {
      err[6] = 1u;
    }
    if (i == n_states - 1 && (uint64_t)ip + 1 != n_ips) err[6] = 1u;
  }
}
// per IP: hash_bytes of its bytes, the owner filter, the arena bytes it keeps ([0, n_ips]: the last entry 0)
__global__ void k_imp_ip(uint64_t n_ips, const uint64_t *__restrict__ ip_off, const uint8_t *__restrict__ bytes,
                         uint32_t part, uint32_t n_parts, uint32_t *__restrict__ keep, uint64_t *__restrict__ klen,
                         uint64_t *__restrict__ hash) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i > n_ips) return;
  if (i == n_ips) { keep[i] = 0; klen[i] = 0; hash[i] = 0; return; }
  const uint64_t a = ip_off[i];
  const uint32_t len = (uint32_t)(ip_off[i + 1] - a);
  const uint64_t h = hash_bytes(bytes + a, len);
  const bool mine = (uint32_t)((h >> 32) % n_parts) == part;  // the node's owner function (part_line)
  keep[i] = mine ? 1u : 0u;
  klen[i] = mine ? len : 0;
  hash[i] = h;
}
// cnt[0] += records of kept IPs (one atomic per block)
__global__ __launch_bounds__(kBlock) void k_imp_count(uint64_t n_states, const uint64_t *__restrict__ recs,
                                                      const uint32_t *__restrict__ keep,
                                                      unsigned long long *__restrict__ cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t n = i < n_states && keep[(uint32_t)recs[3 * i]] ? 1 : 0, z = 0;
  block_sum2(n, z);
  if (threadIdx.x == 0 && n) atomicAdd(&cnt[0], (unsigned long long)n);
}
// kept IP -> arena bytes, offset, length and its IpSlot (CAS on an empty slot,
// as k_exp_ip: equal hashes of distinct IPs take successive slots)
__global__ void k_imp_place(uint64_t n_ips, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ nid,
                            const uint64_t *__restrict__ noff, const uint64_t *__restrict__ hash, uint64_t hmask,
                            const uint64_t *__restrict__ ip_off, const uint8_t *__restrict__ bytes, uint32_t born,
                            uint64_t kept_ips, uint8_t *__restrict__ n_arena, uint64_t n_arena_cap,
                            uint64_t *__restrict__ n_off, uint32_t *__restrict__ n_len, IpSlot *__restrict__ nt,
                            uint64_t nmask) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ips || !keep[i]) return;
  const uint64_t a = ip_off[i], d = noff[i];
  const uint32_t len = (uint32_t)(ip_off[i + 1] - a), id = nid[i];
  if (id >= kept_ips) return;  // (the scans' totals sized the tables: never taken)
  // (the source range ends inside the IP section: k_imp_check saw ip_off monotone up to ip_off[n_ips])
  if (!copy_ip_bytes(n_arena, d, n_arena_cap, bytes, a, ip_off[n_ips], len)) return;
  n_off[id] = d;
  n_len[id] = len;
  const uint64_t h = hmask ? (hash[i] & hmask) | 1ull : hash[i];
  fresh_put_ip(nt, nmask, h, id, born, ip_key16_bytes(bytes + a, len));
}
// one lane per record of a kept IP (CAS on the key, as k_exp_st)
__global__ void k_imp_st(uint64_t n_states, const uint64_t *__restrict__ recs, const uint32_t *__restrict__ keep,
                         const uint32_t *__restrict__ nid, const uint32_t *__restrict__ remap, StSlot *__restrict__ nt,
                         uint64_t nmask) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_states) return;
  const uint64_t w = recs[3 * i];
  const uint32_t ip = (uint32_t)w;
  if (!keep[ip]) return;
  const uint64_t key = ((uint64_t)(nid[ip] + 1) << 24) | remap[w >> 32];
  fresh_put_st(nt, nmask, key, (int64_t)recs[3 * i + 1], (int64_t)recs[3 * i + 2], 1);
}
// every imported IP looked up as ip_claim_line looks up an IP of an earlier
// batch (hash, key16, arena bytes past 15), along its whole probe chain: it
// must match one slot, the one with its own id
__global__ void k_imp_verify(uint64_t n_ips, const uint32_t *__restrict__ keep, const uint32_t *__restrict__ nid,
                             const uint64_t *__restrict__ hash, uint64_t hmask, const uint64_t *__restrict__ ip_off,
                             const uint8_t *__restrict__ bytes, uint64_t kept_ips, const IpSlot *__restrict__ nt,
                             uint64_t nmask, const uint64_t *__restrict__ n_off, const uint32_t *__restrict__ n_len,
                             const uint8_t *__restrict__ n_arena, uint32_t *__restrict__ err) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ips || !keep[i]) return;
  const uint64_t a = ip_off[i];
  const uint32_t len = (uint32_t)(ip_off[i + 1] - a);
  const uint8_t *src = bytes + a;
  const uint4 k16 = ip_key16_bytes(src, len);
  const uint64_t h = hmask ? (hash[i] & hmask) | 1ull : hash[i];
  uint32_t found = 0;
  bool own = false;
  uint64_t j = h & nmask;
  for (uint64_t step = 0; step <= nmask; ++step) {
    const IpSlot v = nt[j];
    if (v.hash == 0) break;
    if (v.hash == h && v.id < kept_ips && key16_eq(v.key16, k16) &&
        (len <= 15 || (n_len[v.id] == len && bytes_eq(n_arena + n_off[v.id], src, len)))) {
      ++found;
      own = own || v.id == nid[i];
    }
    j = (j + 1) & nmask;
  }
  if (found != 1 || !own) err[0] = 1u;
}

// snapshot merge (bjx_state_merge): the import's checks and owner filter, then
// every kept snapshot IP is looked up in the live IP table and every record of
// one in the live state table, which gives each record a verdict.  The new IPs
// (not held, bringing a record) are scanned into the ids and arena offsets
// after the engine's; the union is built into new tables: the engine's slots
// re-put as growth does, the new IPs placed as import does, the records put
// or written over their key's slot by their verdict.
constexpr uint8_t kMrgSkip = 0, kMrgAdd = 1, kMrgReplace = 2, kMrgKeep = 3, kMrgFill = 4;  // Fill: the key is held with valid == 0
// per snapshot IP: eid[i] = the engine's id of a kept IP, kNone when it holds
// none (k_imp_verify's lookup on the live table: masked hash, key16, arena
// bytes past 15).  claim[id] takes the first snapshot index that finds id; a
// second one is an IP twice in the snapshot: err[0]
__global__ void k_mrg_find(uint64_t n_ips, const uint32_t *__restrict__ keep, const uint64_t *__restrict__ hash, uint64_t hmask,
                           const uint64_t *__restrict__ ip_off, const uint8_t *__restrict__ bytes, State S, uint64_t e_ips,
                           uint32_t *__restrict__ eid, uint32_t *__restrict__ claim, uint32_t *__restrict__ err) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ips) return;
  uint32_t id = kNone;
  if (keep[i] && e_ips) {
    const uint64_t a = ip_off[i];
    const uint32_t len = (uint32_t)(ip_off[i + 1] - a);
    const uint8_t *src = bytes + a;
    const uint4 k16 = ip_key16_bytes(src, len);
    const uint64_t h = hmask ? (hash[i] & hmask) | 1ull : hash[i];
    uint64_t j = h & S.ip_mask;
    for (uint64_t step = 0; step <= S.ip_mask; ++step) {
      const IpSlot v = S.ip[j];
      if (v.hash == 0) break;
      if (v.hash == h && v.id < e_ips && key16_eq(v.key16, k16) &&
          (len <= 15 || (S.ip_len[v.id] == len && bytes_eq(S.arena + S.ip_off[v.id], src, len)))) {
        id = v.id;
        break;
      }
      j = (j + 1) & S.ip_mask;
    }
    if (id != kNone && atomicCAS(&claim[id], kNone, (uint32_t)i) != kNone) err[0] = 1u;
  }
  eid[i] = id;
}
// per record: the owner and min_start filters, the live state of its key (the
// probe stops at an empty key; valid == 0 is absent), the policy -> verdict[i];
// brings[ip] = 1 for an IP with a record that is not skipped.  cnt[0..4] +=
// skipped, added, replaced, kept, and the added ones that take a new slot (one
// atomic per block and counter).  remap: snapshot name -> engine name id, ids
// from e_names on are names the engine has not interned
__global__ __launch_bounds__(kBlock) void k_mrg_rec(uint64_t n_states, const uint64_t *__restrict__ recs,
                                                    const uint32_t *__restrict__ keep, const uint32_t *__restrict__ eid,
                                                    const uint32_t *__restrict__ remap, uint32_t e_names, State S,
                                                    int64_t min_start, uint32_t policy, uint8_t *__restrict__ verdict,
                                                    uint32_t *__restrict__ brings, unsigned long long *__restrict__ cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t v = kMrgSkip;
  if (i < n_states) {
    const uint64_t w = recs[3 * i];
    const uint32_t ip = (uint32_t)w;
    const int64_t hits = (int64_t)recs[3 * i + 1], start = (int64_t)recs[3 * i + 2];
    if (keep[ip] && start >= min_start) {
      brings[ip] = 1u;  // every writer stores the same value
      v = kMrgAdd;
      const uint32_t id = eid[ip], nm = remap[w >> 32];
      if (id != kNone && nm < e_names) {
        const uint64_t key = ((uint64_t)(id + 1) << 24) | nm;
        uint64_t j = mix64(key) & S.st_mask;
        for (uint64_t step = 0; step <= S.st_mask; ++step, j = (j + 1) & S.st_mask) {
          const StSlot s = S.st[j];
          if (s.key == 0) break;
          if (s.key != key) continue;
          if (!s.valid) {
            v = kMrgFill;
          } else {
            const bool differs = s.hits != hits || s.start != start;
            const bool wins = policy == BJX_MERGE_REPLACE ? differs
                              : policy == BJX_MERGE_KEEP  ? false
                                                          : start > s.start || (start == s.start && hits > s.hits);
            v = wins ? kMrgReplace : kMrgKeep;
          }
          break;
        }
      }
    }
    verdict[i] = (uint8_t)v;
  }
  const bool in = i < n_states;
  uint64_t n_skip = in && v == kMrgSkip, n_add = in && (v == kMrgAdd || v == kMrgFill), n_rep = in && v == kMrgReplace,
           n_keep = in && v == kMrgKeep, n_slot = in && v == kMrgAdd, z = 0;
  block_sum2(n_skip, n_add);
  __syncthreads();  // thread 0 has read the first pair's partial sums
  block_sum2(n_rep, n_keep);
  __syncthreads();
  block_sum2(n_slot, z);
  if (threadIdx.x == 0) {
    if (n_skip) atomicAdd(&cnt[0], (unsigned long long)n_skip);
    if (n_add) atomicAdd(&cnt[1], (unsigned long long)n_add);
    if (n_rep) atomicAdd(&cnt[2], (unsigned long long)n_rep);
    if (n_keep) atomicAdd(&cnt[3], (unsigned long long)n_keep);
    if (n_slot) atomicAdd(&cnt[4], (unsigned long long)n_slot);
  }
}
// per snapshot IP over [0, n_ips] (the last entry 0): is[i] = 1 and klen[i] =
// its bytes for an IP the engine does not hold that brings a record; cnt[5] +=
// the IPs that bring one, held or not
__global__ __launch_bounds__(kBlock) void k_mrg_new(uint64_t n_ips, const uint64_t *__restrict__ ip_off,
                                                    const uint32_t *__restrict__ keep, const uint32_t *__restrict__ brings,
                                                    const uint32_t *__restrict__ eid, uint32_t *__restrict__ is,
                                                    uint64_t *__restrict__ klen, unsigned long long *__restrict__ cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t n = 0, z = 0;
  if (i <= n_ips) {
    const bool br = i < n_ips && keep[i] && brings[i];
    const bool nw = br && eid[i] == kNone;
    is[i] = nw ? 1u : 0u;
    klen[i] = nw ? ip_off[i + 1] - ip_off[i] : 0;
    n = br ? 1 : 0;
  }
  block_sum2(n, z);
  if (threadIdx.x == 0 && n) atomicAdd(&cnt[5], (unsigned long long)n);
}
// the scans' ranks -> final ids and arena offsets: nid[i] = the engine's id of
// a held IP, e_ips + rank for a new one, kNone for the others; noff[i] += used
__global__ void k_mrg_ids(uint64_t n_ips, const uint32_t *__restrict__ is, const uint32_t *__restrict__ eid, uint64_t e_ips,
                          uint64_t used, uint32_t *__restrict__ nid, uint64_t *__restrict__ noff) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_ips) return;
  nid[i] = eid[i] != kNone ? eid[i] : is[i] ? (uint32_t)(e_ips + nid[i]) : kNone;
  noff[i] += used;
}
// per record, after the engine's states are in the new table: an added record
// takes a slot (k_imp_st), a replacing or filling one is written over the slot
// of its key; err[7]: that key is not there (never: k_mrg_rec found it)
__global__ void k_mrg_put(uint64_t n_states, const uint64_t *__restrict__ recs, const uint8_t *__restrict__ verdict,
                          const uint32_t *__restrict__ nid, const uint32_t *__restrict__ remap, StSlot *__restrict__ nt,
                          uint64_t nmask, uint32_t *__restrict__ err) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_states) return;
  const uint32_t v = verdict[i];
  if (v == kMrgSkip || v == kMrgKeep) return;
  const uint64_t w = recs[3 * i];
  const uint32_t id = nid[(uint32_t)w];
  if (id == kNone) { err[7] = 1u; return; }  // (a record that is not skipped made its IP held or new)
  const uint64_t key = ((uint64_t)(id + 1) << 24) | remap[w >> 32];
  const int64_t hits = (int64_t)recs[3 * i + 1], start = (int64_t)recs[3 * i + 2];
  if (v == kMrgAdd) {
    fresh_put_st(nt, nmask, key, hits, start, 1);
    return;
  }
  uint64_t j = mix64(key) & nmask;
  for (uint64_t step = 0; step <= nmask; ++step, j = (j + 1) & nmask) {
    const uint64_t k = nt[j].key;
    if (k == 0) break;
    if (k == key) {
      nt[j].hits = hits; nt[j].start = start; nt[j].valid = 1;
      return;
    }
  }
  err[7] = 1u;
}

// state query (RegexRateLimitStates.Get for one (ip, name))
__global__ void k_state_get(State S, uint64_t h, const uint8_t *ip, uint32_t len, uint32_t name_id, int64_t *out) {
  out[0] = 0;
  uint64_t i = h & S.ip_mask;
  for (;;) {
    const uint64_t cur = S.ip[i].hash;
    if (cur == 0) return;
    if (cur == h) {
      const uint32_t id = S.ip[i].id;
      if (S.ip_len[id] == len && bytes_eq(S.arena + S.ip_off[id], ip, len)) {
        const uint64_t key = ((uint64_t)(id + 1) << 24) | name_id;
        uint64_t j = mix64(key) & S.st_mask;
        for (;;) {
          const uint64_t k = S.st[j].key;
          if (k == 0) { out[0] = 1; return; }  // ip known, rule state absent
          if (k == key) {
            if (!S.st[j].valid) { out[0] = 1; return; }
            out[0] = 2; out[1] = S.st[j].hits; out[2] = S.st[j].start;
            return;
          }
          j = (j + 1) & S.st_mask;
        }
      }
    }
    i = (i + 1) & S.ip_mask;
  }
}

// bjx_debug_state_slots: k_state_get's lookup for a whole list, one lane per
// (ip, name id) pair of the packed list (entry i: bytes[off[i], off[i + 1]),
// 4 readable bytes past the last one for hash_bytes' word loads); out[i] = the
// state-table slot (k_state_get's j) of a live state, -1 where it finds none
__global__ __launch_bounds__(kBlock) void k_state_slots(State S, uint64_t hmask, uint64_t n, uint64_t n_ips,
                                                        const uint32_t *__restrict__ off, const uint32_t *__restrict__ name_id,
                                                        const uint8_t *__restrict__ bytes, int64_t *__restrict__ out) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n) return;
  int64_t slot = -1;
  const uint32_t a = off[t], len = off[t + 1] - a, name = name_id[t];
  const uint8_t *src = bytes + a;
  uint64_t h = hash_bytes(src, len);
  if (hmask) h = (h & hmask) | 1ull;
  uint64_t i = h & S.ip_mask;
  for (uint64_t step = 0; step <= S.ip_mask && name != kNone; ++step, i = (i + 1) & S.ip_mask) {
    const uint64_t cur = S.ip[i].hash;
    if (cur == 0) break;
    if (cur != h) continue;
    const uint32_t id = S.ip[i].id;
    if (id >= n_ips || S.ip_len[id] != len || !bytes_eq(S.arena + S.ip_off[id], src, len)) continue;
    const uint64_t key = ((uint64_t)(id + 1) << 24) | name;
    uint64_t j = mix64(key) & S.st_mask;
    for (uint64_t s2 = 0; s2 <= S.st_mask; ++s2, j = (j + 1) & S.st_mask) {
      const uint64_t k = S.st[j].key;
      if (k == 0) break;
      if (k == key) {
        if (S.st[j].valid) slot = (int64_t)j;
        break;
      }
    }
    break;
  }
  out[t] = slot;
}

// live keys left in the state / IP tables (bjx_state_clear's check)
__global__ void k_count_live(const StSlot *__restrict__ st, uint64_t st_cap, const IpSlot *__restrict__ ip, uint64_t ip_cap,
                             unsigned long long *__restrict__ cnt) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < st_cap && st[i].key != 0) atomicAdd(&cnt[0], 1ull);
  if (i < ip_cap && ip[i].hash != 0) atomicAdd(&cnt[1], 1ull);
}

// ------------------------------------------------------------------ host side

uint64_t state_device_bytes(uint64_t ip_cap, uint64_t st_cap, uint64_t arena_cap) {
  return ip_cap * (sizeof(IpSlot) + 4 + 8 + 4) + st_cap * sizeof(StSlot) + arena_cap;
}

// device allocations owned until taken: freed on every way out
struct ExpAlloc {
  std::vector<void *> ptrs;
  bool nomem = false;
  template <typename T>
  T *get(uint64_t n) {
    void *p = nullptr;
    if (nomem) return nullptr;
    if (hipMalloc(&p, std::max<uint64_t>(n, 1) * sizeof(T)) != hipSuccess) {
      (void)hipGetLastError();  // the failed allocation is reported as BJX_ERR_NOMEM, not left pending
      nomem = true;
      return nullptr;
    }
    ptrs.push_back(p);
    return static_cast<T *>(p);
  }
  void take() { ptrs.clear(); }
  ~ExpAlloc() {
    for (void *p : ptrs) (void)hipFree(p);
  }
};

// Tables nothing has been inserted into: ip and st all 0 (empty slots),
// ip_first and the ip_st slot cache all ~0.  A null pointer is skipped.
void clear_tables(hipStream_t s, IpSlot *ip, uint32_t *ip_first, uint32_t *ip_st, uint64_t ip_cap, StSlot *st, uint64_t st_cap) {
  if (ip) HIP_OK(hipMemsetAsync(ip, 0, ip_cap * sizeof(IpSlot), s));
  if (ip_first) HIP_OK(hipMemsetAsync(ip_first, 0xFF, ip_cap * 4, s));
  if (ip_st) HIP_OK(hipMemsetAsync(ip_st, 0xFF, ip_cap * 4, s));
  if (st) HIP_OK(hipMemsetAsync(st, 0, st_cap * sizeof(StSlot), s));
}

// New arrays for the state, owned until install() hands them to the engine:
// every way out before that frees them and leaves the engine untouched.
// ip_cap covers ip, ip_first, ip_off, ip_len and ip_st, arena_cap the arena,
// st_cap st; a capacity of 0 keeps that part of the engine's state.
struct NewTables {
  ExpAlloc own;
  IpSlot *ip = nullptr;
  uint32_t *ip_first = nullptr, *ip_len = nullptr, *ip_st = nullptr;
  uint64_t *ip_off = nullptr;
  uint8_t *arena = nullptr;
  StSlot *st = nullptr;
  uint64_t ip_cap, st_cap, arena_cap;
  NewTables(uint64_t ip_cap_, uint64_t st_cap_, uint64_t arena_cap_, const char *nomem_msg)
      : ip_cap(ip_cap_), st_cap(st_cap_), arena_cap(arena_cap_) {
    if (ip_cap) {
      ip = own.get<IpSlot>(ip_cap);
      ip_first = own.get<uint32_t>(ip_cap);
      ip_off = own.get<uint64_t>(ip_cap);
      ip_len = own.get<uint32_t>(ip_cap);
      ip_st = own.get<uint32_t>(ip_cap);
    }
    if (arena_cap) arena = own.get<uint8_t>(arena_cap);
    if (st_cap) st = own.get<StSlot>(st_cap);
    if (own.nomem) throw BjxError(BJX_ERR_NOMEM, nomem_msg);
  }
  void clear(hipStream_t s) { clear_tables(s, ip, ip_first, ip_st, ip_cap, st, st_cap); }
};

// The swap, and the one place that says what a change of tables resets.  Waits
// for the stream (the kernels that filled nw, the last readers of the old
// arrays), frees the old arrays and takes nw's.  What is keyed by slot index
// or IP id came new with the tables (ip_first, the ip_st slot cache); past 2^32
// state slots the slot cache is off, and coming back under them makes the next
// batch bind again so that it may cache again.
// totals != nullptr (a rebuild: expiry, import): the entries changed too, so
// the counters {ips, arena bytes, states} are set on the device and the host
// and sort2_hold and rec_hold start over, as bjx_state_clear does.  nullptr (growth): the
// same entries under the same ids, the counters stand.
void install(bjx_engine *e, NewTables &nw, const uint64_t *totals) {
  State &S = e->S;
  HIP_OK(hipStreamSynchronize(e->stream));
  if (nw.ip) {
    for (void *p : {(void *)S.ip, (void *)S.ip_first, (void *)S.ip_off, (void *)S.ip_len, (void *)S.ip_st}) (void)hipFree(p);
    S.ip = nw.ip; S.ip_first = nw.ip_first; S.ip_off = nw.ip_off; S.ip_len = nw.ip_len; S.ip_st = nw.ip_st;
    S.ip_mask = nw.ip_cap - 1;
    S.ip_st_cap = e->ip_cap = nw.ip_cap;
  }
  if (nw.arena) {
    (void)hipFree(S.arena);
    S.arena = nw.arena;
    S.arena_cap = nw.arena_cap;
  }
  if (nw.st) {
    (void)hipFree(S.st);
    S.st = nw.st;
    S.st_mask = nw.st_cap - 1;
    if (nw.st_cap > (1ull << 32)) S.hot_name = kNone;
    else if (e->st_cap > (1ull << 32)) e->bound_uid = 0;
    e->st_cap = nw.st_cap;
  }
  nw.own.take();
  if (!totals) return;
  e->sort2_hold = 0;
  e->rec_hold = 0;
  hipLaunchKernelGGL(k_exp_counters, dim3(1), dim3(64), 0, e->stream, S.counters, totals[0], totals[1], totals[2]);
  HIP_OK(hipGetLastError());
  HIP_OK(hipStreamSynchronize(e->stream));
  for (int k = 0; k < 3; ++k) e->host_counters[k] = totals[k];
  e->counters_fresh = false;  // the next stage reads them again
}

void alloc_state(bjx_engine *e, uint64_t ip_cap, uint64_t st_cap, uint64_t arena_cap) {
  NewTables nw(ip_cap, st_cap, arena_cap, "no device memory for the state tables");
  ExpAlloc ctr;
  uint64_t *counters = ctr.get<uint64_t>(kCounterBytes / 8);
  if (ctr.nomem) throw BjxError(BJX_ERR_NOMEM, "no device memory for the state counters");
  HIP_OK(hipMemsetAsync(counters, 0, kCounterBytes, e->stream));
  nw.clear(e->stream);
  e->S.hot_name = kNone;
  install(e, nw, nullptr);
  e->S.counters = counters;
  ctr.take();
}

void free_state(bjx_engine *e) {
  State &S = e->S;
  for (void *p : {(void *)S.ip, (void *)S.ip_first, (void *)S.ip_off, (void *)S.ip_len, (void *)S.arena, (void *)S.st,
                  (void *)S.counters, (void *)S.ip_st})
    if (p) (void)hipFree(p);
  S = State{};
}

// rehash the IP table into one that holds `want` IPs under a 3/4 load factor;
// the arena and the ids stay
void grow_ip(bjx_engine *e, uint64_t want) {
  State &S = e->S;
  const uint64_t n_ips = e->host_counters[0];
  const uint64_t cap = table_cap_for(want);
  if (cap <= e->ip_cap) return;
  NewTables nw(cap, 0, 0, "no device memory to grow the IP table");
  nw.clear(e->stream);
  HIP_OK(hipMemcpyAsync(nw.ip_off, S.ip_off, n_ips * 8, hipMemcpyDeviceToDevice, e->stream));
  HIP_OK(hipMemcpyAsync(nw.ip_len, S.ip_len, n_ips * 4, hipMemcpyDeviceToDevice, e->stream));
  hipLaunchKernelGGL(k_rehash_ip, dim3(grid_for(e->ip_cap)), dim3(kBlock), 0, e->stream, e->ip_cap, S.ip, nw.ip, cap - 1);
  HIP_OK(hipGetLastError());
  install(e, nw, nullptr);
  ++e->rehashes;
}

// rehash the state table into one that holds `want` states under a 3/4 load factor
void grow_st(bjx_engine *e, uint64_t want) {
  State &S = e->S;
  const uint64_t cap = table_cap_for(want);
  if (cap <= e->st_cap) return;
  NewTables nw(0, cap, 0, "no device memory to grow the state table");
  nw.clear(e->stream);
  hipLaunchKernelGGL(k_rehash_st, dim3(grid_for(e->st_cap)), dim3(kBlock), 0, e->stream, e->st_cap, S.st, nw.st, cap - 1);
  HIP_OK(hipGetLastError());
  install(e, nw, nullptr);
  clear_tables(e->stream, nullptr, nullptr, S.ip_st, S.ip_st_cap, nullptr, 0);  // slots moved: the cache of them starts over
  ++e->rehashes;
}

// Tables sized for the steady state, not for every batch's worst case: the
// IP and state tables keep room for `new_ips` / `new_states` more entries
// (claims beyond that roll back and grow, see rate_limit_stage); the arena
// always fits the batch's IP bytes.  Small tables keep the random probes in
// cache and the state-slot sort short.
// (e->host_counters current: the caller has just read them)
void ensure_capacity(bjx_engine *e, uint64_t new_ips, uint64_t new_bytes, uint64_t new_states) {
  State &S = e->S;
  const uint64_t n_ips = e->host_counters[0], used = e->host_counters[1], n_st = e->host_counters[2];
  if ((n_ips + new_ips) * 4 > e->ip_cap * 3) grow_ip(e, 2 * (n_ips + new_ips));
  if (used + new_bytes > S.arena_cap) {
    NewTables nw(0, 0, std::max<uint64_t>(S.arena_cap * 2, used + new_bytes + (1 << 20)), "no device memory to grow the IP arena");
    HIP_OK(hipMemcpyAsync(nw.arena, S.arena, used, hipMemcpyDeviceToDevice, e->stream));
    install(e, nw, nullptr);
  }
  if ((n_st + new_states) * 4 > e->st_cap * 3) grow_st(e, 2 * (n_st + new_states));
}

// What a rebuild keeps: keep[id] = 1 for the IPs that stay and klen[id] their
// arena bytes, over [0, n_ips] with the last entry 0; nid / noff their
// exclusive scans, the dense new id (order kept) and the new arena offset, the
// totals landing in the last entry; ips / bytes / states the three totals.
struct Kept {
  uint32_t *keep, *nid;
  uint64_t *klen, *noff;
  uint64_t ips = 0, bytes = 0, states = 0;
  Kept(ExpAlloc &tmp, uint64_t n_ips)
      : keep(tmp.get<uint32_t>(n_ips + 1)), nid(tmp.get<uint32_t>(n_ips + 1)), klen(tmp.get<uint64_t>(n_ips + 1)),
        noff(tmp.get<uint64_t>(n_ips + 1)) {}
};
// keep[] and klen[] filled and the kept states counted into chk[0] by kernels
// already queued: the two scans, ev_end, then the totals read back and checked
// against what they were taken from (`what` names the failure)
void scan_kept(bjx_engine *e, Kept &K, uint64_t n_ips, uint64_t max_bytes, uint64_t max_states, hipEvent_t ev_end,
               const char *what) {
  hipStream_t st = e->stream;
  cub_call(e, [&](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, K.keep, K.nid, (int)(n_ips + 1), st); });
  cub_call(e, [&](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, K.klen, K.noff, (int)(n_ips + 1), st); });
  HIP_OK(hipEventRecord(ev_end, st));
  unsigned long long kept_st = 0;
  uint32_t kept_ips32 = 0;
  pin_get(e, &kept_st, e->chk.p, 8);
  pin_get(e, &kept_ips32, K.nid + n_ips, 4);
  pin_get(e, &K.bytes, K.noff + n_ips, 8);
  pin_sync(e);
  K.ips = kept_ips32;
  K.states = kept_st;
  if (K.ips > n_ips || K.bytes > max_bytes || K.states > max_states) throw BjxError(BJX_ERR_DEVICE, what);
}
// Expiry's and export's first half, between ev_begin and ev_end: the IPs with a
// state whose window started at or after the cutoff, then scan_kept.  chk[0]
// and chk[1] start at 0.  (e->host_counters current, n_ips < 2^31)
void mark_and_scan(bjx_engine *e, Kept &K, int64_t cutoff, hipEvent_t ev_begin, hipEvent_t ev_end, const char *what) {
  const uint64_t n_ips = e->host_counters[0], used = e->host_counters[1];
  hipStream_t st = e->stream;
  e->chk.ensure(8);
  HIP_OK(hipEventRecord(ev_begin, st));
  HIP_OK(hipMemsetAsync(K.keep, 0, (n_ips + 1) * 4, st));
  HIP_OK(hipMemsetAsync(e->chk.p, 0, 16, st));
  hipLaunchKernelGGL(k_exp_mark, dim3((unsigned)std::min<uint64_t>(grid_for(e->st_cap), 8192)), dim3(kBlock), 0, st, e->st_cap,
                     e->S.st, cutoff, n_ips, K.keep, e->chk.p);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(k_exp_len, dim3(grid_for(n_ips + 1)), dim3(kBlock), 0, st, n_ips, K.keep, e->S.ip_len, K.klen);
  HIP_OK(hipGetLastError());
  scan_kept(e, K, n_ips, used, e->st_cap, ev_end, what);
}

// Expiry's and removal's second half, between ev_begin and ev_end: the new
// tables by growth's sizing rule on what K keeps (never below the capacity the
// engine was created with, never above the present one; allocated before the
// old ones go, so BJX_ERR_NOMEM leaves the state untouched), the kept IPs'
// bytes and slots under their new ids, the kept states through put_states(nw)
// -- the caller's kernel, which knows what survives -- and the swap.
// (n_ips, used: the counters K was taken from)
template <typename PutStates>
void rebuild_kept(bjx_engine *e, const Kept &K, uint64_t n_ips, uint64_t used, hipEvent_t ev_begin, hipEvent_t ev_end,
                  const char *nomem_msg, PutStates put_states) {
  State &S = e->S;
  hipStream_t st = e->stream;
  NewTables nw(clamp_cap(table_cap_for(K.ips), e->ip_cap0, e->ip_cap), clamp_cap(table_cap_for(K.states), e->st_cap0, e->st_cap),
               clamp_cap(arena_cap_for(K.bytes), e->arena_cap0, S.arena_cap), nomem_msg);
  HIP_OK(hipEventRecord(ev_begin, st));
  nw.clear(st);
  if (n_ips) {
    hipLaunchKernelGGL(k_exp_arena, dim3(grid_for(n_ips)), dim3(kBlock), 0, st, n_ips, K.keep, K.nid, K.noff, S.ip_off, S.ip_len,
                       S.arena, used, nw.arena, nw.arena_cap, nw.ip_off, nw.ip_len);
    HIP_OK(hipGetLastError());
  }
  put_states(nw);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(k_exp_ip, dim3(grid_for(e->ip_cap)), dim3(kBlock), 0, st, e->ip_cap, S.ip, n_ips, K.keep, K.nid, nw.ip,
                     nw.ip_cap - 1);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(ev_end, st));
  const uint64_t totals[3] = {K.ips, K.bytes, K.states};
  install(e, nw, totals);
}

// ---- snapshot: bjx_state_export / bjx_state_import (format and host checks: snapshot.h)
struct SnapEvents {
  hipEvent_t ev[8] = {};
  void create() {
    for (auto &x : ev) HIP_OK(hipEventCreate(&x));
  }
  ~SnapEvents() {
    for (auto &x : ev)
      if (x) (void)hipEventDestroy(x);
  }
  double ms(int a, int b) {
    float t = 0;
    HIP_OK(hipEventElapsedTime(&t, ev[a], ev[b]));
    return (double)t;
  }
};
constexpr size_t kSnapChunk = 8u << 20;
// device memory <-> the caller's in chunks through two pinned buffers, the copy
// of one chunk running while the host moves the other
void snap_copy_out(bjx_engine *e, uint8_t *dst, const uint8_t *d_src, uint64_t n) {
  e->snap_pin.reserve(2 * kSnapChunk);
  SnapEvents E;
  E.create();
  const uint64_t nc = (n + kSnapChunk - 1) / kSnapChunk;
  auto land = [&](uint64_t c) {
    HIP_OK(hipEventSynchronize(E.ev[c & 1]));
    memcpy(dst + c * kSnapChunk, e->snap_pin.p + (c & 1) * kSnapChunk, (size_t)std::min<uint64_t>(kSnapChunk, n - c * kSnapChunk));
  };
  for (uint64_t c = 0; c < nc; ++c) {
    HIP_OK(hipMemcpyAsync(e->snap_pin.p + (c & 1) * kSnapChunk, d_src + c * kSnapChunk,
                          (size_t)std::min<uint64_t>(kSnapChunk, n - c * kSnapChunk), hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipEventRecord(E.ev[c & 1], e->stream));
    if (c) land(c - 1);
  }
  if (nc) land(nc - 1);
}
void snap_copy_in(bjx_engine *e, uint8_t *d_dst, const uint8_t *src, uint64_t n) {
  e->snap_pin.reserve(2 * kSnapChunk);
  SnapEvents E;
  E.create();
  const uint64_t nc = (n + kSnapChunk - 1) / kSnapChunk;
  for (uint64_t c = 0; c < nc; ++c) {
    const size_t m = (size_t)std::min<uint64_t>(kSnapChunk, n - c * kSnapChunk);
    if (c >= 2) HIP_OK(hipEventSynchronize(E.ev[c & 1]));  // the chunk that used this buffer has left it
    memcpy(e->snap_pin.p + (c & 1) * kSnapChunk, src + c * kSnapChunk, m);
    HIP_OK(hipMemcpyAsync(d_dst + c * kSnapChunk, e->snap_pin.p + (c & 1) * kSnapChunk, m, hipMemcpyHostToDevice, e->stream));
    HIP_OK(hipEventRecord(E.ev[c & 1], e->stream));
  }
  HIP_OK(hipStreamSynchronize(e->stream));
}

// ---- query: bjx_state_query (filter checks, sort key, name ranks: state_query.h)
// the radix select stops at this many candidates for `need` rows still
// wanted: what is left is sorted, so the sort stays O(limit)
inline uint64_t qry_small(uint64_t need) { return 2 * need + 256; }

}  // namespace

// ------------------------------------------------------------------ entry points

extern "C" int bjx_state_get(bjx_engine *e, const char *ip, size_t ip_len, const char *name, size_t name_len,
                             int64_t *num_hits, int64_t *start_ns) {
  if (ip_len && !ip) return BJX_ERR_ARG;
  return guarded(e, [&]() -> int {  // 1 found, 0 not, a negative code
    auto it = e->name_ids.find(std::string(name ? name : "", name_len));
    if (it == e->name_ids.end()) return 0;
    e->q_ip.ensure(ip_len + 1);
    e->q_out.ensure(4);
    if (ip_len) HIP_OK(hipMemcpyAsync(e->q_ip.p, ip, ip_len, hipMemcpyHostToDevice, e->stream));
    uint64_t h = hash_bytes(reinterpret_cast<const uint8_t *>(ip), (uint32_t)ip_len);
    if (e->dbg_hash_mask) h = (h & e->dbg_hash_mask) | 1;
    hipLaunchKernelGGL(k_state_get, dim3(1), dim3(1), 0, e->stream, e->S, h, e->q_ip.p, (uint32_t)ip_len, it->second, e->q_out.p);
    HIP_OK(hipGetLastError());
    int64_t o[3];
    HIP_OK(hipMemcpyAsync(o, e->q_out.p, 24, hipMemcpyDeviceToHost, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    if (o[0] != 2) return 0;
    if (num_hits) *num_hits = o[1];
    if (start_ns) *start_ns = o[2];
    return 1;
  });
}

extern "C" int64_t bjx_state_len(bjx_engine *e) {
  int64_t n_ips = 0;
  const int rc = guarded(e, [&]() -> int {
    read_counters(e);
    n_ips = (int64_t)e->host_counters[0];
    return BJX_OK;
  });
  return rc == BJX_OK ? n_ips : rc;  // the IPs, or a negative code
}

extern "C" int bjx_state_stats_get(bjx_engine *e, bjx_state_stats *out) {
  if (!out) return BJX_ERR_ARG;
  return guarded(e, [&]() -> int {
    read_counters(e);
    out->ips = e->host_counters[0];
    out->ip_slots = e->ip_cap;
    out->states = e->host_counters[2];
    out->state_slots = e->st_cap;
    out->arena_bytes = e->host_counters[1];
    out->arena_capacity = e->S.arena_cap;
    out->device_bytes = state_device_bytes(e->ip_cap, e->st_cap, e->S.arena_cap);
    out->rehashes = e->rehashes;
    return BJX_OK;
  });
}

extern "C" int bjx_state_clear(bjx_engine *e) {
  return guarded(e, [&]() -> int {
    State &S = e->S;
    HIP_OK(hipDeviceSynchronize());  // nothing of an earlier batch may land after the clear
    e->sort2_hold = 0;
    e->rec_hold = 0;
    clear_tables(e->stream, S.ip, S.ip_first, S.ip_st, e->ip_cap, S.st, e->st_cap);
    HIP_OK(hipMemsetAsync(S.counters, 0, kCounterBytes, e->stream));
    HIP_OK(hipStreamSynchronize(e->stream));
    {
      // the tables must read back empty: IP ids restart at 0, so a state slot
      // that survived would be found again by a new IP's key
      e->chk.ensure(8);
      HIP_OK(hipMemsetAsync(e->chk.p, 0, 16, e->stream));
      const uint64_t n = std::max(e->st_cap, e->ip_cap);
      hipLaunchKernelGGL(k_count_live, dim3(grid_for(n)), dim3(kBlock), 0, e->stream, S.st, e->st_cap, S.ip, e->ip_cap, e->chk.p);
      HIP_OK(hipGetLastError());
      unsigned long long live[2] = {0, 0};
      HIP_OK(hipMemcpyAsync(live, e->chk.p, 16, hipMemcpyDeviceToHost, e->stream));
      HIP_OK(hipStreamSynchronize(e->stream));
      if (live[0] | live[1]) {
        fprintf(stderr, "[bjx] state_clear: %llu state slots and %llu IP slots survived the clear; clearing again\n", live[0],
                live[1]);
        HIP_OK(hipDeviceSynchronize());
        HIP_OK(hipMemset(S.st, 0, e->st_cap * sizeof(StSlot)));
        HIP_OK(hipMemset(S.ip, 0, e->ip_cap * sizeof(IpSlot)));
        HIP_OK(hipDeviceSynchronize());
      }
    }
    return BJX_OK;
  });
}

// Expiry: mark the IPs that keep a state, scan them into new dense ids (order
// kept) and arena offsets, then build new tables from the survivors and
// install them.  The old tables are only read until then, so every failure
// before it leaves the state as it was.
extern "C" int bjx_state_expire(bjx_engine *e, int64_t cutoff_ns, bjx_expire_stats *out) {
  return guarded(e, [&]() -> int {
    if (e->batch_open) throw BjxError(BJX_ERR_ARG, "bjx_state_expire between bjx_match_batch and its bjx_finish_batch");
    HIP_OK(hipDeviceSynchronize());  // nothing of an earlier batch may land after the rebuild
    State &S = e->S;
    hipStream_t st = e->stream;
    SnapEvents E;
    E.create();
    read_counters(e);
    e->counters_fresh = false;
    const uint64_t n_ips = e->host_counters[0], used = e->host_counters[1], n_st = e->host_counters[2];
    if (n_ips >= 0x7FFFFFFFull) throw BjxError(BJX_ERR_CAPACITY, "more than 2^31 distinct IPs");
    const uint64_t bytes_before = state_device_bytes(e->ip_cap, e->st_cap, S.arena_cap);

    ExpAlloc tmp;
    Kept K(tmp, n_ips);
    if (tmp.nomem) throw BjxError(BJX_ERR_NOMEM, "bjx_state_expire: no device memory for the scan buffers");
    mark_and_scan(e, K, cutoff_ns, E.ev[0], E.ev[1], "internal: expiry counts exceed the tables");

    rebuild_kept(e, K, n_ips, used, E.ev[2], E.ev[3], "bjx_state_expire: no device memory for the new tables (state unchanged)",
                 [&](NewTables &nw) {
                   hipLaunchKernelGGL(k_exp_st, dim3(grid_for(e->st_cap)), dim3(kBlock), 0, st, e->st_cap, S.st, cutoff_ns, n_ips,
                                      K.nid, nw.st, nw.st_cap - 1);
                 });
    if (out) {
      out->states_before = n_st; out->states_dropped = n_st - std::min<uint64_t>(n_st, K.states);
      out->ips_before = n_ips; out->ips_dropped = n_ips - K.ips;
      out->arena_bytes_before = used; out->arena_bytes_after = K.bytes;
      out->device_bytes_before = bytes_before;
      out->device_bytes_after = state_device_bytes(e->ip_cap, e->st_cap, S.arena_cap);
      out->device_ms = E.ms(0, 1) + E.ms(2, 3);
    }
    return BJX_OK;
  });
}

// Removal: the listed IPs are found on the device (sel[]), one pass over the
// state table marks the IPs that keep a state and counts the states kept and
// selected, and when any state is selected the expiry's rebuild follows with
// k_rm_st in k_exp_st's place.  Nothing selected: the tables were only read and
// stay as they are.
//
// With nets (bjx_state_remove_nets) k_net_sel sets sel[] in k_rm_ips' place:
// every held IP a network holds.  A filter ip is tested against the table on
// the host and, when a network holds it, looked up as the list form's.
static int state_remove_impl(bjx_engine *e, const bjx_state_filter *f, const bjx_str *ips, size_t n_ips, const bjx_str *nets,
                             size_t n_nets, bool by_nets, bjx_remove_stats *out) {
  const std::string who = by_nets ? "bjx_state_remove_nets" : "bjx_state_remove";
  return guarded(e, [&]() -> int {
    bjx_nets::Table T;
    if (by_nets) {
      if (const char *why = bjx_nets::check_args(f, nets, n_nets)) throw BjxError(BJX_ERR_ARG, who + ": " + why);
      const int64_t bad = bjx_nets::build(nets, n_nets, &T);
      if (bad >= 0) throw BjxError(BJX_ERR_ARG, who + ": " + bjx_nets::bad_entry(bad));
    } else if (const char *why = bjx_remove::check_args(f, ips, n_ips)) {
      throw BjxError(BJX_ERR_ARG, who + ": " + why);
    }
    if (e->batch_open) throw BjxError(BJX_ERR_ARG, who + " between bjx_match_batch and its bjx_finish_batch");
    bjx_remove::List L;
    bjx_remove::pack(*f, by_nets ? nullptr : ips, by_nets ? 0 : n_ips, &L);
    if (by_nets && L.has_ip && !T.holds(reinterpret_cast<const uint8_t *>(f->ip.ptr), (uint32_t)f->ip.len)) L.nothing = true;
    HIP_OK(hipDeviceSynchronize());  // nothing of an earlier batch may land after the rebuild
    State &S = e->S;
    hipStream_t st = e->stream;
    SnapEvents E;
    E.create();
    read_counters(e);
    const uint64_t n_ips_held = e->host_counters[0], used = e->host_counters[1], n_st = e->host_counters[2];
    if (n_ips_held >= 0x7FFFFFFFull) throw BjxError(BJX_ERR_CAPACITY, "more than 2^31 distinct IPs");
    const uint32_t n_names = (uint32_t)e->names.size();
    bjx_remove_stats R{};
    R.states_before = n_st; R.ips_before = n_ips_held;
    R.arena_bytes_before = R.arena_bytes_after = used;
    R.device_bytes_before = R.device_bytes_after = state_device_bytes(e->ip_cap, e->st_cap, S.arena_cap);

    // what no state can pass (not errors): an empty window, a name never
    // interned, a filter ip the list does not hold, an engine without state
    QFilter F{f->min_hits, f->min_start_ns, f->max_start_ns, kNone, 0u};
    bool nothing = L.nothing || bjx_query::empty_window(*f) || !n_ips_held || !n_st;
    if (f->name.ptr) {
      auto it = e->name_ids.find(std::string(f->name.ptr, f->name.len));
      if (it == e->name_ids.end()) nothing = true;
      else F.name = it->second;
    }
    const bool count_found = (by_nets || L.n_list != 0) && n_ips_held != 0;  // ips_found is asked for
    if (nothing && !count_found) {
      if (out) *out = R;
      return BJX_OK;
    }

    ExpAlloc tmp;
    Kept K(tmp, n_ips_held);
    uint32_t *sel = L.restrict || by_nets ? tmp.get<uint32_t>(n_ips_held + 1) : nullptr;
    uint32_t *d_sum = tmp.get<uint32_t>(4);
    // the net table on the device: one image (state_nets.h)
    std::vector<uint8_t> net_img;
    uint64_t o_dir = 0, o_k4 = 0;
    const uint64_t net_bytes = by_nets ? T.image(&net_img, &o_dir, &o_k4) : 0;
    uint8_t *d_net = by_nets ? tmp.get<uint8_t>(net_bytes + 16) : nullptr;
    unsigned long long *d_found = by_nets ? tmp.get<unsigned long long>(2) : nullptr;
    // the list on the device: u32 off[entries + 1], then the bytes (word aligned, 4 readable bytes past them)
    const uint64_t off_bytes = ((uint64_t)L.n_entries() + 1) * 4;
    const uint64_t list_bytes = L.restrict ? off_bytes + L.bytes.size() : 0;
    uint8_t *d_list = L.restrict ? tmp.get<uint8_t>(((list_bytes + 3) & ~3ull) + 16) : nullptr;
    if (tmp.nomem) throw BjxError(BJX_ERR_NOMEM, who + ": no device memory for the scan buffers");
    if (by_nets) snap_copy_in(e, d_net, net_img.data(), net_bytes);
    if (L.restrict) {
      std::vector<uint8_t> img(list_bytes);
      memcpy(img.data(), L.off.data(), off_bytes);
      if (!L.bytes.empty()) memcpy(img.data() + off_bytes, L.bytes.data(), L.bytes.size());
      snap_copy_in(e, d_list, img.data(), list_bytes);  // one upload; waits for the stream
    }
    const uint32_t *d_off = reinterpret_cast<const uint32_t *>(d_list);
    const uint8_t *d_bytes = d_list ? d_list + off_bytes : nullptr;
    auto find_ips = [&](uint32_t first, uint32_t count) {
      HIP_OK(hipMemsetAsync(sel, 0, (n_ips_held + 1) * 4, st));
      if (!count) return;
      hipLaunchKernelGGL(k_rm_ips, dim3(grid_for(count)), dim3(kBlock), 0, st, first, count, d_off, d_bytes, e->dbg_hash_mask, S.ip,
                         S.ip_mask, n_ips_held, S.ip_off, S.ip_len, S.arena, used, sel);
      HIP_OK(hipGetLastError());
    };

    // 1. sel[]: the caller's list first (ips_found), then, when the filter
    // names an IP, that IP alone
    e->chk.ensure(8);
    uint32_t found = 0;
    HIP_OK(hipEventRecord(E.ev[0], st));
    HIP_OK(hipMemsetAsync(e->chk.p, 0, 16, st));
    unsigned long long found_nets = 0;
    if (count_found && by_nets) {
      bjx_nets::View V = T.view();
      V.k6 = reinterpret_cast<const uint64_t *>(d_net);
      V.dir = reinterpret_cast<const bjx_nets::Dir *>(d_net + o_dir);
      V.k4 = reinterpret_cast<const uint32_t *>(d_net + o_k4);
      HIP_OK(hipMemsetAsync(d_found, 0, 16, st));
      HIP_OK(hipMemsetAsync(sel, 0, (n_ips_held + 1) * 4, st));
      hipLaunchKernelGGL(k_net_sel, dim3((unsigned)std::min<uint64_t>(grid_for(n_ips_held), 8192)), dim3(kBlock), 0, st, n_ips_held,
                         S.ip_off, S.ip_len, S.arena, used, V, sel, d_found);
      HIP_OK(hipGetLastError());
      pin_get(e, &found_nets, d_found, 8);
    } else if (count_found) {
      HIP_OK(hipMemsetAsync(d_sum, 0, 16, st));
      find_ips(0, L.n_list);
      cub_call(e, [&](void *t, size_t &b) { return hipcub::DeviceReduce::Sum(t, b, sel, d_sum, (int)n_ips_held, st); });
      pin_get(e, &found, d_sum, 4);
    }
    if (nothing) {
      HIP_OK(hipEventRecord(E.ev[1], st));
      pin_sync(e);
      R.ips_found = by_nets ? found_nets : found;
      R.device_ms = E.ms(0, 1);
      if (out) *out = R;
      return BJX_OK;
    }
    if (L.restrict && (L.has_ip || !count_found)) find_ips(L.sel_first, L.sel_count);

    // 2. the IPs that keep a state, the states kept and selected, the scans
    unsigned long long selected = 0;
    HIP_OK(hipMemsetAsync(K.keep, 0, (n_ips_held + 1) * 4, st));
    hipLaunchKernelGGL(k_rm_mark, dim3((unsigned)std::min<uint64_t>(grid_for(e->st_cap), 8192)), dim3(kBlock), 0, st, e->st_cap,
                       S.st, F, n_ips_held, n_names, sel, K.keep, e->chk.p);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(k_exp_len, dim3(grid_for(n_ips_held + 1)), dim3(kBlock), 0, st, n_ips_held, K.keep, S.ip_len, K.klen);
    HIP_OK(hipGetLastError());
    pin_get(e, &selected, e->chk.p + 1, 8);  // lands with scan_kept's reads
    scan_kept(e, K, n_ips_held, used, e->st_cap, E.ev[1], "internal: removal counts exceed the tables");
    R.ips_found = by_nets ? found_nets : found;
    R.device_ms = E.ms(0, 1);
    if (!selected) {  // the tables were only read
      if (out) *out = R;
      return BJX_OK;
    }
    e->counters_fresh = false;

    // 3. the expiry's rebuild, with k_rm_st in k_exp_st's place
    const std::string nomem = who + ": no device memory for the new tables (state unchanged)";
    rebuild_kept(e, K, n_ips_held, used, E.ev[2], E.ev[3], nomem.c_str(),
                 [&](NewTables &nw) {
                   hipLaunchKernelGGL(k_rm_st, dim3(grid_for(e->st_cap)), dim3(kBlock), 0, st, e->st_cap, S.st, F, n_ips_held,
                                      n_names, sel, K.nid, nw.st, nw.st_cap - 1);
                 });
    R.states_dropped = n_st - std::min<uint64_t>(n_st, K.states);
    R.ips_dropped = n_ips_held - K.ips;
    R.arena_bytes_after = K.bytes;
    R.device_bytes_after = state_device_bytes(e->ip_cap, e->st_cap, S.arena_cap);
    R.device_ms += E.ms(2, 3);
    if (out) *out = R;
    return BJX_OK;
  });
}

extern "C" int bjx_state_remove(bjx_engine *e, const bjx_state_filter *f, const bjx_str *ips, size_t n_ips,
                                bjx_remove_stats *out) {
  return state_remove_impl(e, f, ips, n_ips, nullptr, 0, false, out);
}

extern "C" int bjx_state_remove_nets(bjx_engine *e, const bjx_state_filter *f, const bjx_str *nets, size_t n_nets,
                                     bjx_remove_stats *out) {
  return state_remove_impl(e, f, nullptr, 0, nets, n_nets, true, out);
}

extern "C" uint64_t bjx_state_export_bound(bjx_engine *e) {
  uint64_t total = 0;  // stays 0 on every failure
  guarded(e, [&]() -> int {
    read_counters(e);
    uint64_t nb = 0;
    for (auto &x : e->names) nb += x.size();
    bjx_snap::Layout L;
    const char *why = nullptr;
    if (!bjx_snap::make_layout(e->names.size(), nb, e->host_counters[0], e->host_counters[1], e->host_counters[2], &L, &why))
      throw BjxError(BJX_ERR_CAPACITY, std::string("bjx_state_export_bound: ") + why);
    total = L.total;
    return BJX_OK;
  });
  return total;
}

// Export: expiry's mark / scan passes with min_start_ns as the cutoff, then
// the records compacted, sorted by (ip, name) and written with the IP section
// into one device buffer laid out as the snapshot's tail, which is copied out.
// The tables are only read.
extern "C" int bjx_state_export(bjx_engine *e, int64_t min_start_ns, uint8_t *out, uint64_t cap, uint64_t *len,
                                bjx_snapshot_stats *stats) {
  return guarded(e, [&]() -> int {
    if (len) *len = 0;
    if (cap && !out) throw BjxError(BJX_ERR_ARG, "bjx_state_export: no output buffer");
    if (e->batch_open) throw BjxError(BJX_ERR_ARG, "bjx_state_export between bjx_match_batch and its bjx_finish_batch");
    HIP_OK(hipDeviceSynchronize());
    State &S = e->S;
    hipStream_t st = e->stream;
    SnapEvents E;
    E.create();
    read_counters(e);
    const uint64_t n_ips = e->host_counters[0], used = e->host_counters[1], n_st = e->host_counters[2];
    if (n_ips >= bjx_snap::kMaxIps) throw BjxError(BJX_ERR_CAPACITY, "bjx_state_export: 2^31 distinct IPs or more");
    const uint32_t n_all = (uint32_t)e->names.size();

    ExpAlloc tmp;
    Kept K(tmp, n_ips);
    uint32_t *d_used = tmp.get<uint32_t>(n_all + 1), *d_remap = tmp.get<uint32_t>(n_all + 1);
    if (tmp.nomem) throw BjxError(BJX_ERR_NOMEM, "bjx_state_export: no device memory for the scan buffers");
    mark_and_scan(e, K, min_start_ns, E.ev[0], E.ev[1], "internal: export counts exceed the tables");
    const uint64_t kept_ips = K.ips, kept_bytes = K.bytes, kept_st = K.states;
    if (kept_st >=bjx_snap::kMaxStates) throw BjxError(BJX_ERR_CAPACITY, "bjx_state_export: 2^31 states or more");

    // records, unsorted, with the engine's name ids; the names in use
    uint64_t *keys = tmp.get<uint64_t>(kept_st), *keys2 = tmp.get<uint64_t>(kept_st);
    uint32_t *idx = tmp.get<uint32_t>(kept_st), *idx2 = tmp.get<uint32_t>(kept_st);
    int64_t *pay = tmp.get<int64_t>(2 * kept_st);
    if (tmp.nomem) throw BjxError(BJX_ERR_NOMEM, "bjx_state_export: no device memory for the records");
    HIP_OK(hipEventRecord(E.ev[2], st));
    HIP_OK(hipMemsetAsync(d_used, 0, (n_all + 1) * 4, st));
    if (kept_st) {
      hipLaunchKernelGGL(k_snap_compact, dim3((unsigned)std::min<uint64_t>(grid_for(e->st_cap), 8192)), dim3(kBlock), 0, st,
                         e->st_cap, S.st, min_start_ns, n_ips, K.nid, n_all, d_used, e->chk.p + 1, (uint64_t)kept_st, keys, idx, pay);
      HIP_OK(hipGetLastError());
    }
    HIP_OK(hipEventRecord(E.ev[3], st));
    unsigned long long packed = 0;
    std::vector<uint32_t> h_used(n_all + 1, 0);
    pin_get(e, &packed, e->chk.p + 1, 8);
    pin_sync(e);
    HIP_OK(hipMemcpy(h_used.data(), d_used, (n_all + 1) * 4, hipMemcpyDeviceToHost));
    if (packed != kept_st) throw BjxError(BJX_ERR_DEVICE, "internal: export passes disagree on the surviving states");

    // canonical names: the used ones sorted bytewise; old id -> canonical index
    std::vector<std::string> canon;
    for (uint32_t k = 0; k < n_all; ++k)
      if (h_used[k]) canon.push_back(e->names[k]);
    std::sort(canon.begin(), canon.end());
    std::vector<uint32_t> remap(n_all + 1, 0);
    uint64_t names_bytes = 0;
    for (auto &x : canon) names_bytes += x.size();
    for (uint32_t k = 0; k < n_all; ++k)
      if (h_used[k]) remap[k] = (uint32_t)(std::lower_bound(canon.begin(), canon.end(), e->names[k]) - canon.begin());
    bjx_snap::Layout L;
    const char *why = nullptr;
    if (!bjx_snap::make_layout(canon.size(), names_bytes, kept_ips, kept_bytes, kept_st, &L, &why))
      throw BjxError(BJX_ERR_CAPACITY, std::string("bjx_state_export: ") + why);
    if (len) *len = L.total;
    if (cap < L.total)
      throw BjxError(BJX_ERR_CAPACITY, "bjx_state_export: the snapshot takes " + std::to_string(L.total) + " bytes, cap is " +
                                           std::to_string(cap));

    // the snapshot from ip_off on, built in device memory
    const uint64_t body = L.total - L.o_ip_off;
    uint8_t *d_body = tmp.get<uint8_t>(body + 16);
    if (tmp.nomem) throw BjxError(BJX_ERR_NOMEM, "bjx_state_export: no device memory for the snapshot");
    uint64_t *d_ipoff = reinterpret_cast<uint64_t *>(d_body);
    uint8_t *d_ipb = d_body + (L.o_ips - L.o_ip_off);
    uint64_t *d_recs = reinterpret_cast<uint64_t *>(d_body + (L.o_recs - L.o_ip_off));
    HIP_OK(hipMemcpyAsync(d_remap, remap.data(), (n_all + 1) * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipEventRecord(E.ev[4], st));
    HIP_OK(hipMemsetAsync(d_body, 0, L.o_recs - L.o_ip_off, st));  // the padding after the IP bytes
    if (kept_st) {
      hipLaunchKernelGGL(k_snap_remap, dim3(grid_for(kept_st)), dim3(kBlock), 0, st, (uint64_t)kept_st, keys, d_remap);
      HIP_OK(hipGetLastError());
      const int end_bit = 24 + std::max(1, bit_width(kept_ips));
      cub_call(e, [&](void *t, size_t &b) {
        return hipcub::DeviceRadixSort::SortPairs(t, b, keys, keys2, idx, idx2, (int)kept_st, 0, end_bit, st);
      });
      hipLaunchKernelGGL(k_snap_gather, dim3(grid_for(kept_st)), dim3(kBlock), 0, st, (uint64_t)kept_st, keys2, idx2, pay, d_recs);
      HIP_OK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_snap_ips, dim3(grid_for(n_ips + 1)), dim3(kBlock), 0, st, n_ips, K.keep, K.nid, K.noff, S.ip_off,
                       S.ip_len, S.arena, used, kept_ips, kept_bytes, d_ipoff, d_ipb);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(E.ev[5], st));
    HIP_OK(hipStreamSynchronize(st));

    bjx_snap::write_header(out, L);
    bjx_snap::write_names(out, L, canon);
    snap_copy_out(e, out + L.o_ip_off, d_body, body);
    if (stats) {
      stats->ips = kept_ips; stats->states = kept_st; stats->names = canon.size(); stats->bytes = L.total;
      stats->ips_skipped = n_ips - kept_ips;
      stats->states_skipped = n_st - std::min<uint64_t>(n_st, kept_st);
      stats->device_ms = E.ms(0, 1) + E.ms(2, 3) + E.ms(4, 5);
    }
    return BJX_OK;
  });
}

// Import into an empty engine: the snapshot's tail is uploaded and checked on
// the device, the IPs this part owns are scanned into dense ids and arena
// offsets, and new tables are built from them and installed.  Nothing of the
// engine changes before that, so every failure leaves it empty.
extern "C" int bjx_state_import(bjx_engine *e, const uint8_t *snap, uint64_t len, uint32_t part, uint32_t n_parts,
                                bjx_snapshot_stats *stats) {
  return guarded(e, [&]() -> int {
    if (e->batch_open) throw BjxError(BJX_ERR_ARG, "bjx_state_import between bjx_match_batch and its bjx_finish_batch");
    if (!snap) throw BjxError(BJX_ERR_ARG, "bjx_state_import: no snapshot");
    if (n_parts < 1 || n_parts > kMaxParts || part >= n_parts)
      throw BjxError(BJX_ERR_ARG, "bjx_state_import: part / n_parts out of range (n_parts 1..256, part < n_parts)");
    HIP_OK(hipDeviceSynchronize());
    hipStream_t st = e->stream;
    read_counters(e);
    if (e->host_counters[0] || e->host_counters[2])
      throw BjxError(BJX_ERR_ARG, "bjx_state_import: the engine holds state (import needs an empty engine)");
    bjx_snap::Layout L;
    std::vector<std::string> names;
    if (const char *why = bjx_snap::validate_host(snap, len, &L, &names))
      throw BjxError(BJX_ERR_ARG, std::string("bjx_state_import: ") + why);
    const uint64_t n_ips = L.n_ips, n_states = L.n_states;
    const uint32_t n_names = (uint32_t)L.n_names;
    SnapEvents E;
    E.create();

    const uint64_t body = L.total - L.o_ip_off;
    ExpAlloc tmp;
    uint8_t *d_body = tmp.get<uint8_t>(body + 16);
    Kept K(tmp, n_ips);
    uint64_t *hash = tmp.get<uint64_t>(n_ips + 1);
    uint32_t *d_used = tmp.get<uint32_t>(n_names + 1), *d_remap = tmp.get<uint32_t>(n_names + 1), *d_err = tmp.get<uint32_t>(8);
    if (tmp.nomem) throw BjxError(BJX_ERR_NOMEM, "bjx_state_import: no device memory for the snapshot");
    const uint64_t *d_ipoff = reinterpret_cast<const uint64_t *>(d_body);
    const uint8_t *d_ipb = d_body + (L.o_ips - L.o_ip_off);
    const uint64_t *d_recs = reinterpret_cast<const uint64_t *>(d_body + (L.o_recs - L.o_ip_off));
    snap_copy_in(e, d_body, snap + L.o_ip_off, body);

    // the device checks: nothing else runs before they pass
    HIP_OK(hipEventRecord(E.ev[0], st));
    HIP_OK(hipMemsetAsync(d_err, 0, 32, st));
    HIP_OK(hipMemsetAsync(d_used, 0, (n_names + 1) * 4, st));
    hipLaunchKernelGGL(k_imp_check, dim3(grid_for(std::max(n_ips + 1, n_states))), dim3(kBlock), 0, st, n_ips, d_ipoff, L.ip_bytes,
                       n_states, d_recs, n_names, d_used, d_err);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(E.ev[1], st));
    uint32_t err[8] = {};
    std::vector<uint32_t> h_used(n_names + 1, 0);
    pin_get(e, err, d_err, 32);
    pin_sync(e);
    HIP_OK(hipMemcpy(h_used.data(), d_used, (n_names + 1) * 4, hipMemcpyDeviceToHost));
    static const char *const kWhy[7] = {"", "ip_off: not monotone from 0", "ip_off: does not end at ip_bytes",
                                        "records: ip index out of range", "records: name index out of range",
                                        "records: not strictly ascending by (ip, name)", "records: an IP without a record"};
    for (int c = 1; c < 7; ++c)
      if (err[c]) throw BjxError(BJX_ERR_ARG, std::string("bjx_state_import: ") + kWhy[c]);
    for (uint32_t k = 0; k < n_names; ++k)
      if (!h_used[k]) throw BjxError(BJX_ERR_ARG, "bjx_state_import: names: a name no record uses");

    // names into this engine's ids
    std::vector<uint32_t> remap(n_names + 1, 0);
    for (uint32_t k = 0; k < n_names; ++k) remap[k] = intern_name(e, names[k]);
    HIP_OK(hipMemcpyAsync(d_remap, remap.data(), (n_names + 1) * 4, hipMemcpyHostToDevice, st));

    // per IP: hash, owner filter; dense ids and arena offsets of the kept ones
    e->chk.ensure(8);
    HIP_OK(hipEventRecord(E.ev[2], st));
    HIP_OK(hipMemsetAsync(e->chk.p, 0, 8, st));
    hipLaunchKernelGGL(k_imp_ip, dim3(grid_for(n_ips + 1)), dim3(kBlock), 0, st, n_ips, d_ipoff, d_ipb, part, n_parts, K.keep, K.klen,
                       hash);
    HIP_OK(hipGetLastError());
    if (n_states) {
      hipLaunchKernelGGL(k_imp_count, dim3(grid_for(n_states)), dim3(kBlock), 0, st, n_states, d_recs, K.keep, e->chk.p);
      HIP_OK(hipGetLastError());
    }
    scan_kept(e, K, n_ips, L.ip_bytes, n_states, E.ev[3], "internal: import counts exceed the snapshot");

    // the new tables: the growth rule on what this part keeps, never below the
    // capacities the engine was created with; allocated before the old go
    NewTables nw(clamp_cap(table_cap_for(K.ips), e->ip_cap0, kNoCeiling), clamp_cap(table_cap_for(K.states), e->st_cap0, kNoCeiling),
                 clamp_cap(arena_cap_for(K.bytes), e->arena_cap0, kNoCeiling),
                 "bjx_state_import: no device memory for the tables (the engine stays empty)");
    // born: non-zero and below every later batch's epoch (run_batch counts up before it claims)
    if (e->epoch == 0) e->epoch = 1;
    const uint32_t born = e->epoch;
    HIP_OK(hipEventRecord(E.ev[4], st));
    nw.clear(st);
    if (n_ips) {
      hipLaunchKernelGGL(k_imp_place, dim3(grid_for(n_ips)), dim3(kBlock), 0, st, n_ips, K.keep, K.nid, K.noff, hash,
                         e->dbg_hash_mask, d_ipoff, d_ipb, born, K.ips, nw.arena, nw.arena_cap, nw.ip_off, nw.ip_len, nw.ip,
                         nw.ip_cap - 1);
      HIP_OK(hipGetLastError());
    }
    if (n_states) {
      hipLaunchKernelGGL(k_imp_st, dim3(grid_for(n_states)), dim3(kBlock), 0, st, n_states, d_recs, K.keep, K.nid, d_remap, nw.st,
                         nw.st_cap - 1);
      HIP_OK(hipGetLastError());
    }
    if (n_ips) {
      hipLaunchKernelGGL(k_imp_verify, dim3(grid_for(n_ips)), dim3(kBlock), 0, st, n_ips, K.keep, K.nid, hash, e->dbg_hash_mask,
                         d_ipoff, d_ipb, K.ips, nw.ip, nw.ip_cap - 1, nw.ip_off, nw.ip_len, nw.arena, d_err);
      HIP_OK(hipGetLastError());
    }
    HIP_OK(hipEventRecord(E.ev[5], st));
    pin_get(e, err, d_err, 4);
    pin_sync(e);
    if (err[0]) throw BjxError(BJX_ERR_ARG, "bjx_state_import: ips: an IP appears twice in the snapshot");

    const uint64_t totals[3] = {K.ips, K.bytes, K.states};
    install(e, nw, totals);
    if (stats) {
      stats->ips = K.ips; stats->states = K.states; stats->names = n_names; stats->bytes = len;
      stats->ips_skipped = n_ips - K.ips;
      stats->states_skipped = n_states - K.states;
      stats->device_ms = E.ms(0, 1) + E.ms(2, 3) + E.ms(4, 5);
    }
    return BJX_OK;
  });
}

// Merge into an engine that holds state: import's upload, checks and owner
// filter; the lookups of the snapshot's IPs and keys against the live tables
// and the verdicts (k_mrg_find, k_mrg_rec); the ids and arena offsets of the
// new IPs behind the engine's; and, when a record is added or replaces one,
// the union built into new tables and installed.  The live tables are only
// read until then and nothing of the engine changes before every check has
// passed -- the names are interned last -- so every failure leaves it as it
// was.  A dry run builds and checks the new tables too and drops them.
static_assert(sizeof(bjx_merge_options) == 24 && sizeof(bjx_merge_stats) == 136, "the merge structs of the C ABI");
extern "C" int bjx_state_merge(bjx_engine *e, const uint8_t *snap, uint64_t len, const bjx_merge_options *o,
                               bjx_merge_stats *out) {
  if (!e || !snap || !o) return BJX_ERR_ARG;
  return guarded(e, [&]() -> int {
    if (e->batch_open) throw BjxError(BJX_ERR_ARG, "bjx_state_merge between bjx_match_batch and its bjx_finish_batch");
    if (o->policy > BJX_MERGE_REPLACE) throw BjxError(BJX_ERR_ARG, "bjx_state_merge: unknown policy");
    if (o->flags & ~(uint32_t)BJX_MERGE_DRY_RUN) throw BjxError(BJX_ERR_ARG, "bjx_state_merge: unknown flag bits");
    const uint32_t part = o->part, n_parts = o->n_parts;
    if (n_parts < 1 || n_parts > kMaxParts || part >= n_parts)
      throw BjxError(BJX_ERR_ARG, "bjx_state_merge: part / n_parts out of range (n_parts 1..256, part < n_parts)");
    const bool dry = (o->flags & BJX_MERGE_DRY_RUN) != 0;
    HIP_OK(hipDeviceSynchronize());  // nothing of an earlier batch may land after the rebuild
    State &S = e->S;
    hipStream_t st = e->stream;
    read_counters(e);
    const uint64_t e_ips = e->host_counters[0], used = e->host_counters[1], e_st = e->host_counters[2];
    if (e_ips >= bjx_snap::kMaxIps) throw BjxError(BJX_ERR_CAPACITY, "bjx_state_merge: the engine holds 2^31 distinct IPs or more");
    bjx_snap::Layout L;
    std::vector<std::string> names;
    if (const char *why = bjx_snap::validate_host(snap, len, &L, &names))
      throw BjxError(BJX_ERR_ARG, std::string("bjx_state_merge: ") + why);
    const uint64_t n_ips = L.n_ips, n_states = L.n_states;
    const uint32_t n_names = (uint32_t)L.n_names;
    SnapEvents E;
    E.create();

    const uint64_t body = L.total - L.o_ip_off;
    ExpAlloc tmp;
    uint8_t *d_body = tmp.get<uint8_t>(body + 16);
    Kept K(tmp, n_ips);  // keep[]: the new IPs
    uint64_t *hash = tmp.get<uint64_t>(n_ips + 1);
    uint32_t *own = tmp.get<uint32_t>(n_ips + 1), *eid = tmp.get<uint32_t>(n_ips + 1), *brings = tmp.get<uint32_t>(n_ips + 1);
    uint32_t *claim = tmp.get<uint32_t>(e_ips + 1);
    uint8_t *verdict = tmp.get<uint8_t>(n_states + 1);
    uint32_t *d_used = tmp.get<uint32_t>(n_names + 1), *d_remap = tmp.get<uint32_t>(n_names + 1), *d_err = tmp.get<uint32_t>(8);
    if (tmp.nomem) throw BjxError(BJX_ERR_NOMEM, "bjx_state_merge: no device memory for the snapshot");
    const uint64_t *d_ipoff = reinterpret_cast<const uint64_t *>(d_body);
    const uint8_t *d_ipb = d_body + (L.o_ips - L.o_ip_off);
    const uint64_t *d_recs = reinterpret_cast<const uint64_t *>(d_body + (L.o_recs - L.o_ip_off));
    snap_copy_in(e, d_body, snap + L.o_ip_off, body);

    // the device checks of import: nothing else runs before they pass
    HIP_OK(hipEventRecord(E.ev[0], st));
    HIP_OK(hipMemsetAsync(d_err, 0, 32, st));
    HIP_OK(hipMemsetAsync(d_used, 0, (n_names + 1) * 4, st));
    hipLaunchKernelGGL(k_imp_check, dim3(grid_for(std::max(n_ips + 1, n_states))), dim3(kBlock), 0, st, n_ips, d_ipoff, L.ip_bytes,
                       n_states, d_recs, n_names, d_used, d_err);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(E.ev[1], st));
    uint32_t err[8] = {};
    std::vector<uint32_t> h_used(n_names + 1, 0);
    pin_get(e, err, d_err, 32);
    pin_sync(e);
    HIP_OK(hipMemcpy(h_used.data(), d_used, (n_names + 1) * 4, hipMemcpyDeviceToHost));
    static const char *const kWhy[7] = {"", "ip_off: not monotone from 0", "ip_off: does not end at ip_bytes",
                                        "records: ip index out of range", "records: name index out of range",
                                        "records: not strictly ascending by (ip, name)", "records: an IP without a record"};
    for (int c = 1; c < 7; ++c)
      if (err[c]) throw BjxError(BJX_ERR_ARG, std::string("bjx_state_merge: ") + kWhy[c]);
    for (uint32_t k = 0; k < n_names; ++k)
      if (!h_used[k]) throw BjxError(BJX_ERR_ARG, "bjx_state_merge: names: a name no record uses");

    // names -> this engine's ids; one it has not interned gets the id it will
    // be interned under once everything has passed
    const uint32_t e_names = (uint32_t)e->names.size();
    std::vector<uint32_t> remap(n_names + 1, 0);
    std::vector<uint32_t> fresh_names;
    for (uint32_t k = 0; k < n_names; ++k) {
      auto it = e->name_ids.find(names[k]);
      if (it != e->name_ids.end()) {
        remap[k] = it->second;
      } else {
        remap[k] = e_names + (uint32_t)fresh_names.size();
        fresh_names.push_back(k);
      }
    }
    if ((uint64_t)e_names + fresh_names.size() >= bjx_snap::kMaxNames)
      throw BjxError(BJX_ERR_CAPACITY, "bjx_state_merge: the union would reach 2^24 rule names");
    HIP_OK(hipMemcpyAsync(d_remap, remap.data(), (n_names + 1) * 4, hipMemcpyHostToDevice, st));

    // per IP: hash, owner filter, the engine's id; per record: the verdict; the new IPs scanned
    e->chk.ensure(8);
    HIP_OK(hipEventRecord(E.ev[2], st));
    HIP_OK(hipMemsetAsync(e->chk.p, 0, 64, st));
    HIP_OK(hipMemsetAsync(brings, 0, (n_ips + 1) * 4, st));
    HIP_OK(hipMemsetAsync(claim, 0xFF, (e_ips + 1) * 4, st));
    hipLaunchKernelGGL(k_imp_ip, dim3(grid_for(n_ips + 1)), dim3(kBlock), 0, st, n_ips, d_ipoff, d_ipb, part, n_parts, own, K.klen,
                       hash);
    HIP_OK(hipGetLastError());
    if (n_ips) {
      hipLaunchKernelGGL(k_mrg_find, dim3(grid_for(n_ips)), dim3(kBlock), 0, st, n_ips, own, hash, e->dbg_hash_mask, d_ipoff, d_ipb,
                         S, e_ips, eid, claim, d_err);
      HIP_OK(hipGetLastError());
    }
    if (n_states) {
      hipLaunchKernelGGL(k_mrg_rec, dim3(grid_for(n_states)), dim3(kBlock), 0, st, n_states, d_recs, own, eid, d_remap, e_names, S,
                         o->min_start_ns, o->policy, verdict, brings, e->chk.p);
      HIP_OK(hipGetLastError());
    }
    hipLaunchKernelGGL(k_mrg_new, dim3(grid_for(n_ips + 1)), dim3(kBlock), 0, st, n_ips, d_ipoff, own, brings, eid, K.keep, K.klen,
                       e->chk.p);
    HIP_OK(hipGetLastError());
    cub_call(e, [&](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, K.keep, K.nid, (int)(n_ips + 1), st); });
    cub_call(e, [&](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, K.klen, K.noff, (int)(n_ips + 1), st); });
    HIP_OK(hipEventRecord(E.ev[3], st));
    unsigned long long cnt[6] = {};
    uint32_t new_ips32 = 0;
    uint64_t new_bytes = 0;
    pin_get(e, cnt, e->chk.p, 48);
    pin_get(e, &new_ips32, K.nid + n_ips, 4);
    pin_get(e, &new_bytes, K.noff + n_ips, 8);
    pin_get(e, err, d_err, 32);
    pin_sync(e);
    if (err[0]) throw BjxError(BJX_ERR_ARG, "bjx_state_merge: ips: an IP appears twice in the snapshot");
    const uint64_t new_ips = new_ips32, new_slots = cnt[4];
    if (cnt[0] + cnt[1] + cnt[2] + cnt[3] != n_states || new_ips > n_ips || new_bytes > L.ip_bytes || new_slots > cnt[1] ||
        cnt[5] > n_ips || cnt[5] < new_ips)
      throw BjxError(BJX_ERR_DEVICE, "internal: merge counts exceed the snapshot");
    if (e_ips + new_ips >= bjx_snap::kMaxIps) throw BjxError(BJX_ERR_CAPACITY, "bjx_state_merge: the union would reach 2^31 distinct IPs");

    const uint64_t bytes_before = state_device_bytes(e->ip_cap, e->st_cap, S.arena_cap);
    bjx_merge_stats r{};
    r.snap_ips = n_ips; r.snap_states = n_states; r.snap_names = n_names; r.snap_bytes = len;
    r.ips_before = e_ips; r.ips_added = new_ips; r.ips_skipped = n_ips - cnt[5];
    r.states_before = e_st; r.states_skipped = cnt[0]; r.states_added = cnt[1]; r.states_replaced = cnt[2]; r.states_kept = cnt[3];
    r.arena_bytes_before = used; r.arena_bytes_after = used + new_bytes;
    r.device_bytes_before = r.device_bytes_after = bytes_before;
    r.device_ms = E.ms(0, 1) + E.ms(2, 3);
    if (cnt[1] + cnt[2] == 0) {  // nothing to change: the tables were only read
      if (out) *out = r;
      return BJX_OK;
    }

    // the union in new tables: the growth rule on its counts, never below the
    // present capacities; allocated before the old go
    const uint64_t tot_ips = e_ips + new_ips, tot_bytes = used + new_bytes, tot_st = e_st + new_slots;
    NewTables nw(clamp_cap(table_cap_for(tot_ips), e->ip_cap, kNoCeiling), clamp_cap(table_cap_for(tot_st), e->st_cap, kNoCeiling),
                 clamp_cap(arena_cap_for(tot_bytes), S.arena_cap, kNoCeiling),
                 "bjx_state_merge: no device memory for the new tables (state unchanged)");
    // born: as import's, non-zero and below every later batch's epoch
    const uint32_t born = e->epoch ? e->epoch : 1;
    HIP_OK(hipEventRecord(E.ev[4], st));
    nw.clear(st);
    if (used) HIP_OK(hipMemcpyAsync(nw.arena, S.arena, used, hipMemcpyDeviceToDevice, st));
    if (e_ips) {
      HIP_OK(hipMemcpyAsync(nw.ip_off, S.ip_off, e_ips * 8, hipMemcpyDeviceToDevice, st));
      HIP_OK(hipMemcpyAsync(nw.ip_len, S.ip_len, e_ips * 4, hipMemcpyDeviceToDevice, st));
    }
    hipLaunchKernelGGL(k_rehash_ip, dim3(grid_for(e->ip_cap)), dim3(kBlock), 0, st, e->ip_cap, S.ip, nw.ip, nw.ip_cap - 1);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(k_rehash_st, dim3(grid_for(e->st_cap)), dim3(kBlock), 0, st, e->st_cap, S.st, nw.st, nw.st_cap - 1);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(k_mrg_ids, dim3(grid_for(n_ips)), dim3(kBlock), 0, st, n_ips, K.keep, eid, e_ips, used, K.nid, K.noff);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(k_imp_place, dim3(grid_for(n_ips)), dim3(kBlock), 0, st, n_ips, K.keep, K.nid, K.noff, hash, e->dbg_hash_mask,
                       d_ipoff, d_ipb, born, tot_ips, nw.arena, nw.arena_cap, nw.ip_off, nw.ip_len, nw.ip, nw.ip_cap - 1);
    HIP_OK(hipGetLastError());
    hipLaunchKernelGGL(k_mrg_put, dim3(grid_for(n_states)), dim3(kBlock), 0, st, n_states, d_recs, verdict, K.nid, d_remap, nw.st,
                       nw.st_cap - 1, d_err);
    HIP_OK(hipGetLastError());
    // the duplicate check for the IPs the engine did not hold: each is found once, under its own id
    hipLaunchKernelGGL(k_imp_verify, dim3(grid_for(n_ips)), dim3(kBlock), 0, st, n_ips, K.keep, K.nid, hash, e->dbg_hash_mask,
                       d_ipoff, d_ipb, tot_ips, nw.ip, nw.ip_cap - 1, nw.ip_off, nw.ip_len, nw.arena, d_err);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(E.ev[5], st));
    pin_get(e, err, d_err, 32);
    pin_sync(e);
    if (err[0]) throw BjxError(BJX_ERR_ARG, "bjx_state_merge: ips: an IP appears twice in the snapshot");
    if (err[7]) throw BjxError(BJX_ERR_DEVICE, "internal: merge lost the slot of a held key");
    r.device_ms += E.ms(4, 5);
    if (!dry) {
      for (uint32_t k : fresh_names)
        if (intern_name(e, names[k]) != remap[k]) throw BjxError(BJX_ERR_DEVICE, "internal: merge name ids moved");
      e->epoch = born;
      r.device_bytes_after = state_device_bytes(nw.ip_cap, nw.st_cap, nw.arena_cap);
      const uint64_t totals[3] = {tot_ips, tot_bytes, tot_st};
      install(e, nw, totals);
    }
    if (out) *out = r;
    return BJX_OK;
  });
}

// Query: one pass over the state table (or one probe per interned name of one
// IP) counts the passing states and appends them as 16-byte candidates; a
// radix select narrows them to the wanted rows plus a remainder of O(limit),
// which is sorted; the rows and their bytes are gathered on the device and
// copied out.  The tables are only read.  The candidate buffer is sized by the
// `states` counter (the most a scan can append).
//
// With nets (bjx_state_query_nets) k_net_sel marks the held IPs a network
// holds before the scan, which then passes only their states, and k_net_count
// adds every IP with a passing state to the networks that hold it.  With an ip
// filter the host tests that one IP against the table and the k_qry_ip path
// runs as it is, or nothing does.
static int state_query_impl(bjx_engine *e, const bjx_state_filter *f, const bjx_str *nets, size_t n_nets, bool by_nets,
                            bjx_state_rows *out, const uint64_t **net_ips) {
  if (!e || !f || !out) return BJX_ERR_ARG;
  const std::string who = by_nets ? "bjx_state_query_nets" : "bjx_state_query";
  return guarded(e, [&]() -> int {
    memset(out, 0, sizeof *out);
    if (net_ips) *net_ips = nullptr;
    if (const char *why = bjx_query::check_filter(f)) throw BjxError(BJX_ERR_ARG, who + ": " + why);
    bjx_nets::Table T;
    if (by_nets) {
      if (const char *why = bjx_nets::check_args(f, nets, n_nets)) throw BjxError(BJX_ERR_ARG, who + ": " + why);
      const int64_t bad = bjx_nets::build(nets, n_nets, &T);
      if (bad >= 0) throw BjxError(BJX_ERR_ARG, who + ": " + bjx_nets::bad_entry(bad));
    }
    if (e->batch_open) throw BjxError(BJX_ERR_ARG, who + " between bjx_match_batch and its bjx_finish_batch");
    if (by_nets) {
      e->qry_net_ips.assign(n_nets, 0);
      if (net_ips) *net_ips = e->qry_net_ips.data();
    }
    HIP_OK(hipDeviceSynchronize());
    State &S = e->S;
    hipStream_t st = e->stream;
    SnapEvents E;
    E.create();
    read_counters(e);
    const uint64_t n_ips = e->host_counters[0], used = e->host_counters[1], n_st = e->host_counters[2];
    const uint32_t n_names = (uint32_t)e->names.size();
    e->qry_rows.clear();
    e->qry_bytes.clear();
    QFilter F{f->min_hits, f->min_start_ns, f->max_start_ns, kNone, f->order == BJX_QUERY_BY_START ? 1u : 0u};
    if (f->name.ptr) {
      auto it = e->name_ids.find(std::string(f->name.ptr, f->name.len));
      if (it == e->name_ids.end()) return BJX_OK;  // never interned: no state can carry it
      F.name = it->second;
    }
    if (bjx_query::empty_window(*f) || !n_ips || !n_st || !n_names) return BJX_OK;
    if (n_ips >= bjx_snap::kMaxIps) throw BjxError(BJX_ERR_CAPACITY, who + ": 2^31 distinct IPs or more");
    const bool by_ip = f->ip.ptr != nullptr;
    std::vector<uint32_t> ip_canon;  // nets and an ip filter: the networks that hold it
    if (by_nets && by_ip && !T.holds(reinterpret_cast<const uint8_t *>(f->ip.ptr), (uint32_t)f->ip.len, &ip_canon)) return BJX_OK;
    const bool net_scan = by_nets && !by_ip;
    const uint64_t limit = f->limit;
    const uint64_t room = limit ? (by_ip ? (uint64_t)n_names : n_st) : 0;
    const uint64_t rows_max = std::min(limit, room);
    const uint64_t fin_cap = rows_max ? rows_max + qry_small(rows_max) : 0;

    // name ranks (tie word), rank -> id and the name bytes in rank order (the rows' names)
    std::vector<uint32_t> rank, by_rank;
    bjx_query::name_ranks(e->names, &rank, &by_rank);
    std::vector<uint64_t> noff(n_names + 1, 0);
    std::string nbytes;
    for (uint32_t r = 0; r < n_names; ++r) {
      noff[r] = nbytes.size();
      nbytes += e->names[by_rank[r]];
    }
    noff[n_names] = nbytes.size();

    // every buffer whose size is known now, before anything is launched
    ExpAlloc tmp;
    uint32_t *keep = by_ip ? nullptr : tmp.get<uint32_t>(n_ips + 1);
    uint32_t *d_sum = tmp.get<uint32_t>(4);
    // the net table in one image (state_nets.h), sel[], the canonical networks' counters
    std::vector<uint8_t> net_img;
    uint64_t o_dir = 0, o_k4 = 0;
    const uint64_t net_bytes = net_scan ? T.image(&net_img, &o_dir, &o_k4) : 0;
    const uint32_t n_canon = T.n_canon();
    uint8_t *d_net = net_scan ? tmp.get<uint8_t>(net_bytes + 16) : nullptr;
    uint32_t *sel = net_scan ? tmp.get<uint32_t>(n_ips + 1) : nullptr;
    uint32_t *d_ncnt = net_scan ? tmp.get<uint32_t>((uint64_t)n_canon + 1) : nullptr;
    unsigned long long *d_found = net_scan ? tmp.get<unsigned long long>(2) : nullptr;
    uint32_t *d_rank = tmp.get<uint32_t>(n_names), *d_by_rank = tmp.get<uint32_t>(n_names);
    uint64_t *d_noff = tmp.get<uint64_t>(n_names + 1);
    uint8_t *d_nbytes = tmp.get<uint8_t>(nbytes.size() + 16);
    unsigned long long *d_ctr = tmp.get<unsigned long long>(4 + 256);  // [0] matched [1] appended [2] selected [3] next set; the histogram
    ulonglong2 *cand = tmp.get<ulonglong2>(room), *fin = tmp.get<ulonglong2>(fin_cap);
    uint64_t *k0 = tmp.get<uint64_t>(fin_cap), *k1 = tmp.get<uint64_t>(fin_cap);
    uint32_t *i0 = tmp.get<uint32_t>(fin_cap), *i1 = tmp.get<uint32_t>(fin_cap);
    bjx_state_row *d_rows = tmp.get<bjx_state_row>(rows_max);
    uint64_t *d_lens = tmp.get<uint64_t>(rows_max + 1), *d_offs = tmp.get<uint64_t>(rows_max + 1);
    if (tmp.nomem) throw BjxError(BJX_ERR_NOMEM, who + ": no device memory for the candidates");
    if (net_scan) snap_copy_in(e, d_net, net_img.data(), net_bytes);
    HIP_OK(hipMemcpyAsync(d_rank, rank.data(), n_names * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_by_rank, by_rank.data(), n_names * 4, hipMemcpyHostToDevice, st));
    HIP_OK(hipMemcpyAsync(d_noff, noff.data(), (n_names + 1) * 8, hipMemcpyHostToDevice, st));
    if (!nbytes.empty()) HIP_OK(hipMemcpyAsync(d_nbytes, nbytes.data(), nbytes.size(), hipMemcpyHostToDevice, st));
    uint64_t h = 0;
    if (by_ip) {
      e->q_ip.ensure(f->ip.len + 1);
      if (f->ip.len) HIP_OK(hipMemcpyAsync(e->q_ip.p, f->ip.ptr, f->ip.len, hipMemcpyHostToDevice, st));
      h = hash_bytes(reinterpret_cast<const uint8_t *>(f->ip.ptr), (uint32_t)f->ip.len);
      if (e->dbg_hash_mask) h = (h & e->dbg_hash_mask) | 1;
    }
    HIP_OK(hipStreamSynchronize(st));  // the uploads read host vectors
    double ms = 0;

    // 1. the passing states: counts, keep[], candidates
    HIP_OK(hipEventRecord(E.ev[0], st));
    HIP_OK(hipMemsetAsync(d_ctr, 0, (4 + 256) * 8, st));
    HIP_OK(hipMemsetAsync(d_sum, 0, 16, st));
    if (by_ip) {
      hipLaunchKernelGGL(k_qry_ip, dim3((unsigned)std::min<uint64_t>(grid_for(n_names), 1024)), dim3(kBlock), 0, st, S, h,
                         e->q_ip.p, (uint32_t)f->ip.len, F, n_ips, n_names, d_rank, d_ctr, room, cand);
      HIP_OK(hipGetLastError());
    } else {
      bjx_nets::View V = T.view();
      if (net_scan) {
        V.k6 = reinterpret_cast<const uint64_t *>(d_net);
        V.dir = reinterpret_cast<const bjx_nets::Dir *>(d_net + o_dir);
        V.k4 = reinterpret_cast<const uint32_t *>(d_net + o_k4);
        HIP_OK(hipMemsetAsync(d_found, 0, 16, st));
        HIP_OK(hipMemsetAsync(sel, 0, (n_ips + 1) * 4, st));
        HIP_OK(hipMemsetAsync(d_ncnt, 0, ((uint64_t)n_canon + 1) * 4, st));
        hipLaunchKernelGGL(k_net_sel, dim3((unsigned)std::min<uint64_t>(grid_for(n_ips), 8192)), dim3(kBlock), 0, st, n_ips, S.ip_off,
                           S.ip_len, S.arena, used, V, sel, d_found);
        HIP_OK(hipGetLastError());
      }
      HIP_OK(hipMemsetAsync(keep, 0, (n_ips + 1) * 4, st));
      hipLaunchKernelGGL(k_qry_scan, dim3((unsigned)std::min<uint64_t>(grid_for(e->st_cap), 8192)), dim3(kBlock), 0, st, e->st_cap,
                         S.st, F, n_ips, n_names, d_rank, sel, keep, d_ctr, room, cand);
      HIP_OK(hipGetLastError());
      cub_call(e, [&](void *t, size_t &b) { return hipcub::DeviceReduce::Sum(t, b, keep, d_sum, (int)n_ips, st); });
      if (net_scan) {
        hipLaunchKernelGGL(k_net_count, dim3((unsigned)std::min<uint64_t>((n_ips + kNetCountIps - 1) / kNetCountIps, 2048)), dim3(kBlock),
                           0, st, n_ips, keep,
                           S.ip_off, S.ip_len, S.arena, used, V, n_canon, d_ncnt);
        HIP_OK(hipGetLastError());
      }
    }
    HIP_OK(hipEventRecord(E.ev[1], st));
    unsigned long long got[2] = {0, 0};
    uint32_t ips_matched = 0;
    pin_get(e, got, d_ctr, 16);
    pin_get(e, &ips_matched, d_sum, 4);
    pin_sync(e);
    ms += E.ms(0, 1);
    if (net_scan) {
      std::vector<uint32_t> canon_count(n_canon, 0);
      if (n_canon) HIP_OK(hipMemcpy(canon_count.data(), d_ncnt, (uint64_t)n_canon * 4, hipMemcpyDeviceToHost));
      bjx_nets::per_entry(T, canon_count, &e->qry_net_ips);
    } else if (by_nets && got[0]) {  // an ip filter: that IP is held and has a selected state
      std::vector<uint32_t> canon_count(n_canon, 0);
      for (uint32_t c : ip_canon) canon_count[c] = 1;
      bjx_nets::per_entry(T, canon_count, &e->qry_net_ips);
    }
    if (by_nets && net_ips) *net_ips = e->qry_net_ips.data();
    const uint64_t matched = got[0];
    if (matched > n_st || (room && got[1] != matched))
      throw BjxError(BJX_ERR_DEVICE, "internal: query counts disagree with the tables");
    out->n_matched = matched;
    out->n_ips_matched = by_ip ? (matched ? 1 : 0) : ips_matched;
    const uint64_t n_rows = std::min(limit, matched);
    if (!n_rows) {
      out->device_ms = ms;
      return BJX_OK;
    }

    // 2. radix select, most significant byte first: through the primary word
    // into the tie word while the bucket the limit falls into is still large
    ulonglong2 *cur = cand, *spare = nullptr;
    uint64_t n_cur = matched, n_sel = 0, spare_cap = 0;
    for (int pass = 0; pass < 16 && n_cur > qry_small(n_rows - n_sel); ++pass) {
      const uint32_t word = pass < 8 ? 0u : 1u, shift = 56u - 8u * (uint32_t)(pass & 7);
      const uint64_t need = n_rows - n_sel;
      const unsigned grid = (unsigned)std::min<uint64_t>(grid_for(n_cur), 4096);
      HIP_OK(hipEventRecord(E.ev[0], st));
      HIP_OK(hipMemsetAsync(d_ctr + 4, 0, 256 * 8, st));
      hipLaunchKernelGGL(k_qry_hist, dim3(grid), dim3(kBlock), 0, st, cur, n_cur, word, shift, d_ctr + 4);
      HIP_OK(hipGetLastError());
      HIP_OK(hipEventRecord(E.ev[1], st));
      unsigned long long hist[256];
      pin_get(e, hist, d_ctr + 4, sizeof hist);
      pin_sync(e);
      ms += E.ms(0, 1);
      uint64_t below = 0;
      uint32_t b = 0;
      for (; b < 256 && below + hist[b] < need; ++b) below += hist[b];
      if (b == 256) throw BjxError(BJX_ERR_DEVICE, "internal: query histogram does not add up");
      const uint64_t in_b = hist[b];
      if (in_b == n_cur) continue;  // every candidate has this digit: nothing to move
      ulonglong2 *nxt;
      if (cur == cand) {
        if (!spare) {
          spare = tmp.get<ulonglong2>(in_b);
          spare_cap = in_b;
          if (tmp.nomem) throw BjxError(BJX_ERR_NOMEM, who + ": no device memory for the selection");
        }
        nxt = spare;
      } else {
        nxt = cand;
      }
      const uint64_t nxt_cap = nxt == cand ? room : spare_cap;
      if (in_b > nxt_cap || n_sel + below > fin_cap) throw BjxError(BJX_ERR_DEVICE, "internal: query selection exceeds its buffers");
      HIP_OK(hipEventRecord(E.ev[0], st));
      HIP_OK(hipMemsetAsync(d_ctr + 3, 0, 8, st));
      hipLaunchKernelGGL(k_qry_filter, dim3(grid), dim3(kBlock), 0, st, cur, n_cur, word, shift, b, fin, fin_cap, nxt, nxt_cap,
                         d_ctr + 2);
      HIP_OK(hipGetLastError());
      HIP_OK(hipEventRecord(E.ev[1], st));
      unsigned long long moved[2] = {0, 0};
      pin_get(e, moved, d_ctr + 2, 16);
      pin_sync(e);
      ms += E.ms(0, 1);
      if (moved[0] != n_sel + below || moved[1] != in_b)
        throw BjxError(BJX_ERR_DEVICE, "internal: query selection disagrees with its histogram");
      n_sel += below;
      n_cur = in_b;
      cur = nxt;
    }
    const uint64_t m = n_sel + n_cur;
    if (m > fin_cap || m < n_rows) throw BjxError(BJX_ERR_DEVICE, "internal: query selection did not converge");

    // 3. sort the selected and the remainder by (primary, tie): two stable
    // sorts through an index, the tie word first; gather the rows
    HIP_OK(hipEventRecord(E.ev[0], st));
    HIP_OK(hipMemcpyAsync(fin + n_sel, cur, n_cur * sizeof(ulonglong2), hipMemcpyDeviceToDevice, st));
    hipLaunchKernelGGL(k_qry_split, dim3(grid_for(m)), dim3(kBlock), 0, st, m, fin, k0, i0);
    HIP_OK(hipGetLastError());
    const int tie_bits = std::min(64, 24 + std::max(1, bit_width(n_ips)));
    cub_call(e, [&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, k0, k1, i0, i1, (int)m, 0, tie_bits, st); });
    hipLaunchKernelGGL(k_qry_prim, dim3(grid_for(m)), dim3(kBlock), 0, st, m, fin, i1, k0);
    HIP_OK(hipGetLastError());
    cub_call(e, [&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, k0, k1, i1, i0, (int)m, 0, 64, st); });
    hipLaunchKernelGGL(k_qry_rows, dim3(grid_for(n_rows + 1)), dim3(kBlock), 0, st, n_rows, m, fin, i0, S, n_ips, n_names, d_by_rank,
                       d_noff, d_rows, d_lens);
    HIP_OK(hipGetLastError());
    cub_call(e, [&](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, d_lens, d_offs, (int)(n_rows + 1), st); });
    HIP_OK(hipEventRecord(E.ev[1], st));
    uint64_t total = 0;
    pin_get(e, &total, d_offs + n_rows, 8);
    pin_sync(e);
    ms += E.ms(0, 1);
    uint8_t *d_bytes = tmp.get<uint8_t>(total + 16);
    if (tmp.nomem) throw BjxError(BJX_ERR_NOMEM, who + ": no device memory for the rows' bytes");
    HIP_OK(hipEventRecord(E.ev[0], st));
    hipLaunchKernelGGL(k_qry_bytes, dim3(grid_for(n_rows)), dim3(kBlock), 0, st, n_rows, m, fin, i0, S, n_ips, used, d_noff, d_nbytes,
                       d_offs, total, d_rows, d_bytes);
    HIP_OK(hipGetLastError());
    HIP_OK(hipEventRecord(E.ev[1], st));
    e->qry_rows.resize(n_rows);
    e->qry_bytes.resize(total + 1);
    HIP_OK(hipMemcpyAsync(e->qry_rows.data(), d_rows, n_rows * sizeof(bjx_state_row), hipMemcpyDeviceToHost, st));
    if (total) HIP_OK(hipMemcpyAsync(e->qry_bytes.data(), d_bytes, total, hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    ms += E.ms(0, 1);
    out->n_rows = n_rows;
    out->rows = e->qry_rows.data();
    out->bytes = e->qry_bytes.data();
    out->n_bytes = total;
    out->device_ms = ms;
    return BJX_OK;
  });
}

extern "C" int bjx_state_query(bjx_engine *e, const bjx_state_filter *f, bjx_state_rows *out) {
  return state_query_impl(e, f, nullptr, 0, false, out, nullptr);
}

extern "C" int bjx_state_query_nets(bjx_engine *e, const bjx_state_filter *f, const bjx_str *nets, size_t n_nets,
                                    bjx_state_rows *out, const uint64_t **net_ips) {
  return state_query_impl(e, f, nets, n_nets, true, out, net_ips);
}

extern "C" size_t bjx_state_dump(bjx_engine *e, char *out, size_t cap) {
  size_t size = 0;  // stays 0 on every failure
  guarded(e, [&]() -> int {
    read_counters(e);
    const uint64_t n_ips = e->host_counters[0], used = e->host_counters[1];
    std::vector<uint64_t> off(n_ips);
    std::vector<uint32_t> len(n_ips);
    std::vector<StSlot> st(e->st_cap);
    std::vector<uint8_t> arena(used);
    HIP_OK(hipMemcpy(off.data(), e->S.ip_off, n_ips * 8, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(len.data(), e->S.ip_len, n_ips * 4, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(arena.data(), e->S.arena, used, hipMemcpyDeviceToHost));
    HIP_OK(hipMemcpy(st.data(), e->S.st, e->st_cap * sizeof(StSlot), hipMemcpyDeviceToHost));
    std::vector<std::vector<std::pair<uint32_t, uint64_t>>> per_ip(n_ips);
    for (uint64_t i = 0; i < e->st_cap; ++i)
      if (st[i].key && st[i].valid) per_ip[(st[i].key >> 24) - 1].push_back({(uint32_t)(st[i].key & 0xFFFFFF), i});
    std::string s;
    char buf[96];
    for (uint64_t id = 0; id < n_ips; ++id) {
      s.append(reinterpret_cast<const char *>(arena.data() + off[id]), len[id]);
      s += ":\n";
      std::sort(per_ip[id].begin(), per_ip[id].end(),
                [&](const std::pair<uint32_t, uint64_t> &a, const std::pair<uint32_t, uint64_t> &b) {
                  return e->names[a.first] < e->names[b.first];
                });
      for (auto &p : per_ip[id]) {
        s += "\t" + e->names[p.first] + ":\n";
        snprintf(buf, sizeof buf, "\t\t{%lld %lld}\n", (long long)st[p.second].hits, (long long)st[p.second].start);
        s += buf;
      }
      s += "\n";
    }
    if (out && cap) memcpy(out, s.data(), std::min(cap, s.size()));
    size = s.size();
    return BJX_OK;
  });
  return size;
}

// ---- trim: bjx_state_trim (the budget's checks, the select's host step, the
// cutoff from the candidates, the node's max and sum: state_trim.h).  The
// cutoff is a k-th largest over interval_start_ns -- of all states, and of the
// newest start per IP -- found by an MSB-first radix select that moves no
// state: each pass counts, by the next digit, the keys that carry the digits
// fixed so far, reading the 32-byte slots in place; the host picks the digit
// the rank falls into (bjx_trim::step).  The key is the start with its sign bit
// flipped (unsigned order = signed order), five digits of 13, 13, 13, 13, 12 bits.
// The first pass over the table also takes each IP's newest start (a 64-bit
// atomicMax into newest[ip id]) and marks the IPs that hold a state (one bit
// each); the select over the IPs then reads that array.  Starts cluster in
// time, so almost every key has the same high digits: a thread counts a run of
// equal digits before it touches LDS, as k_qry_hist does.  The mark pass that
// follows is k_exp_mark with two more counters, the rebuild the expiry's own.
namespace {

__device__ __forceinline__ void trim_count(uint32_t *s_h, uint32_t d, uint32_t &run_d, uint32_t &run_n) {
  if (d != run_d && run_n) {
    atomicAdd(&s_h[run_d], run_n);
    run_n = 0;
  }
  run_d = d;
  ++run_n;
}
__device__ __forceinline__ void trim_flush(uint32_t *s_h, uint32_t run_d, uint32_t run_n, unsigned long long *__restrict__ hist) {
  if (run_n) atomicAdd(&s_h[run_d], run_n);
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < bjx_trim::kBins; k += kBlock)
    if (s_h[k]) atomicAdd(&hist[k], (unsigned long long)s_h[k]);
}
// grid-stride over the state table.  newest != NULL (the first pass of a trim
// with max_ips): newest[id] = max key of IP id's states, bit id of has[] set
// (both zeroed before).  hist != NULL: hist[d] += the live states whose key is
// under prefix and has digit p equal to d (kBins counters, zeroed before).
__global__ __launch_bounds__(kBlock) void k_trim_hist_st(uint64_t st_cap, const StSlot *__restrict__ st, uint64_t n_ips,
                                                         uint64_t prefix, uint32_t p, unsigned long long *__restrict__ newest,
                                                         uint32_t *__restrict__ has, unsigned long long *__restrict__ hist) {
  __shared__ uint32_t s_h[bjx_trim::kBins];
  for (uint32_t k = threadIdx.x; k < bjx_trim::kBins; k += kBlock) s_h[k] = 0;
  __syncthreads();
  uint32_t run_d = 0, run_n = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < st_cap; i += (uint64_t)gridDim.x * kBlock) {
    const StSlot v = st[i];
    if (!st_survives(v, INT64_MIN, n_ips)) continue;  // (its IP id is below n_ips)
    const uint64_t key = bjx_trim::key_of(v.start);
    if (newest) {
      const uint64_t id = (v.key >> 24) - 1;
      // both only grow, so a plain read that already covers this state spares
      // the atomic (an IP has many states; a stale read costs one atomic more)
      if (newest[id] < key) atomicMax(&newest[id], (unsigned long long)key);
      if (!((has[id >> 5] >> (id & 31)) & 1u)) atomicOr(&has[id >> 5], 1u << (id & 31));
    }
    if (hist && bjx_trim::under(key, prefix, p)) trim_count(s_h, bjx_trim::digit(key, p), run_d, run_n);
  }
  if (hist) trim_flush(s_h, run_d, run_n, hist);
}
// the same count over newest[], for the IPs whose bit in has[] is set
__global__ __launch_bounds__(kBlock) void k_trim_hist_ip(uint64_t n_ips, const unsigned long long *__restrict__ newest,
                                                         const uint32_t *__restrict__ has, uint64_t prefix, uint32_t p,
                                                         unsigned long long *__restrict__ hist) {
  __shared__ uint32_t s_h[bjx_trim::kBins];
  for (uint32_t k = threadIdx.x; k < bjx_trim::kBins; k += kBlock) s_h[k] = 0;
  __syncthreads();
  uint32_t run_d = 0, run_n = 0;
  for (uint64_t id = (uint64_t)blockIdx.x * kBlock + threadIdx.x; id < n_ips; id += (uint64_t)gridDim.x * kBlock) {
    if (!((has[id >> 5] >> (id & 31)) & 1u)) continue;
    const uint64_t key = newest[id];
    if (bjx_trim::under(key, prefix, p)) trim_count(s_h, bjx_trim::digit(key, p), run_d, run_n);
  }
  trim_flush(s_h, run_d, run_n, hist);
}
// k_exp_mark, counting also what goes: cnt[0] += states kept, cnt[1] += live
// states dropped (start < cutoff), cnt[2] += those of them with start >=
// live_floor (one atomic each per block)
__global__ __launch_bounds__(kBlock) void k_trim_mark(uint64_t st_cap, const StSlot *__restrict__ st, int64_t cutoff,
                                                      int64_t live_floor, uint64_t n_ips, uint32_t *__restrict__ keep,
                                                      unsigned long long *__restrict__ cnt) {
  uint64_t kept = 0, gone = 0, live = 0, z = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < st_cap; i += (uint64_t)gridDim.x * blockDim.x) {
    const StSlot v = st[i];
    if (!st_survives(v, INT64_MIN, n_ips)) continue;
    if (v.start >= cutoff) {
      keep[(v.key >> 24) - 1] = 1u;  // every writer stores the same value
      ++kept;
    } else {
      ++gone;
      if (v.start >= live_floor) ++live;
    }
  }
  block_sum2(kept, gone);
  __syncthreads();  // block_sum2's shared words are read before they are written again
  block_sum2(live, z);
  if (threadIdx.x == 0 && kept) atomicAdd(&cnt[0], (unsigned long long)kept);
  if (threadIdx.x == 0 && gone) atomicAdd(&cnt[1], (unsigned long long)gone);
  if (threadIdx.x == 0 && live) atomicAdd(&cnt[2], (unsigned long long)live);
}

// blocks of a grid-stride pass over n items (bjx_debug_set_trim_grid lowers the cap)
unsigned trim_grid(const bjx_engine *e, uint64_t n) {
  const uint64_t cap = e->dbg_trim_grid ? e->dbg_trim_grid : 2048;
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(grid_for(n), cap));
}

// The selection (the engine lock held).  A bound the counters already meet
// needs no pass: counters[2] counts the claimed slots, which are never fewer
// than the live states, and counters[0] the IPs.
void trim_select_locked(bjx_engine *e, const bjx_trim_budget *b, bjx_trim::Picked *P) {
  if (const char *why = bjx_trim::check_budget(b)) throw BjxError(BJX_ERR_ARG, std::string("bjx_state_trim: ") + why);
  if (e->batch_open) throw BjxError(BJX_ERR_ARG, "bjx_state_trim between bjx_match_batch and its bjx_finish_batch");
  HIP_OK(hipDeviceSynchronize());  // the tables as the last batch left them
  State &S = e->S;
  hipStream_t st = e->stream;
  read_counters(e);
  const uint64_t n_ips = e->host_counters[0], n_st = e->host_counters[2];
  if (n_ips >= 0x7FFFFFFFull) throw BjxError(BJX_ERR_CAPACITY, "more than 2^31 distinct IPs");
  const bool want_st = b->max_states && n_st > b->max_states, want_ip = b->max_ips && n_ips > b->max_ips;
  bjx_trim::Cut c_st, c_ip;
  double ms = 0;
  if (want_st || want_ip) {
    using namespace bjx_trim;
    SnapEvents E;
    E.create();
    ExpAlloc tmp;
    unsigned long long *newest = want_ip ? tmp.get<unsigned long long>(n_ips + 1) : nullptr;
    uint32_t *has = want_ip ? tmp.get<uint32_t>(n_ips / 32 + 1) : nullptr;
    unsigned long long *hist = tmp.get<unsigned long long>(2 * kBins);
    if (tmp.nomem) throw BjxError(BJX_ERR_NOMEM, "bjx_state_trim: no device memory for the selection");
    std::vector<uint64_t> h(2 * kBins);
    Select sel[2];  // 0: over the states, 1: over the IPs' newest starts
    bool open[2] = {want_st, want_ip};
    const uint64_t bound[2] = {b->max_states, b->max_ips};
    Cut *cut[2] = {&c_st, &c_ip};
    HIP_OK(hipEventRecord(E.ev[0], st));
    if (want_ip) {
      HIP_OK(hipMemsetAsync(newest, 0, (n_ips + 1) * 8, st));
      HIP_OK(hipMemsetAsync(has, 0, (n_ips / 32 + 1) * 4, st));
    }
    for (uint32_t p = 0; p < kDigits && (open[0] || open[1]); ++p) {
      HIP_OK(hipMemsetAsync(hist, 0, 2 * kBins * 8, st));
      if (open[0] || (p == 0 && want_ip)) {
        hipLaunchKernelGGL(k_trim_hist_st, dim3(trim_grid(e, e->st_cap)), dim3(kBlock), 0, st, e->st_cap, S.st, n_ips, sel[0].prefix,
                           p, p == 0 ? newest : nullptr, has, open[0] ? hist : nullptr);
        HIP_OK(hipGetLastError());
      }
      if (open[1]) {
        hipLaunchKernelGGL(k_trim_hist_ip, dim3(trim_grid(e, n_ips)), dim3(kBlock), 0, st, n_ips, newest, has, sel[1].prefix, p,
                           hist + kBins);
        HIP_OK(hipGetLastError());
      }
      HIP_OK(hipMemcpyAsync(h.data(), hist, 2 * kBins * 8, hipMemcpyDeviceToHost, st));
      HIP_OK(hipStreamSynchronize(st));
      for (int w = 0; w < 2; ++w) {
        if (!open[w]) continue;
        const uint64_t *hw = h.data() + w * kBins;
        if (p == 0) {  // the first histogram counts every value: |V|
          uint64_t total = 0;
          for (uint32_t d = 0; d < kBins; ++d) total += hw[d];
          if (unbounded(bound[w], total)) { open[w] = false; continue; }
          sel[w].rank = bound[w] + 1;
        }
        if (!step(&sel[w], hw)) throw BjxError(BJX_ERR_DEVICE, "internal: trim histogram below the rank");
        if (sel[w].done()) {
          *cut[w] = cut_after(value_of(sel[w].prefix));
          open[w] = false;
        }
      }
    }
    HIP_OK(hipEventRecord(E.ev[1], st));
    HIP_OK(hipStreamSynchronize(st));
    ms = E.ms(0, 1);
  }
  *P = bjx_trim::pick(b->floor_cutoff_ns, c_st, c_ip);
  P->select_ms = ms;
}

// The trim at a cutoff (the engine lock held): the expiry with the trim's
// counts, its no-op rule and its dry run.  R's cutoff, bound, budget_met and
// select_ms are the caller's.
void trim_apply_locked(bjx_engine *e, int64_t cutoff, int64_t live_floor, uint32_t flags, bjx_trim_stats *R) {
  if (flags & ~(uint32_t)BJX_TRIM_DRY_RUN) throw BjxError(BJX_ERR_ARG, "bjx_state_trim: budget: unknown flag bits");
  if (e->batch_open) throw BjxError(BJX_ERR_ARG, "bjx_state_trim between bjx_match_batch and its bjx_finish_batch");
  HIP_OK(hipDeviceSynchronize());  // nothing of an earlier batch may land after the rebuild
  State &S = e->S;
  hipStream_t st = e->stream;
  read_counters(e);
  const uint64_t n_ips = e->host_counters[0], used = e->host_counters[1], n_st = e->host_counters[2];
  if (n_ips >= 0x7FFFFFFFull) throw BjxError(BJX_ERR_CAPACITY, "more than 2^31 distinct IPs");
  R->states_before = n_st; R->ips_before = n_ips;
  R->states_dropped = R->states_dropped_live = R->ips_dropped = 0;
  R->arena_bytes_before = R->arena_bytes_after = used;
  R->device_bytes_before = R->device_bytes_after = state_device_bytes(e->ip_cap, e->st_cap, S.arena_cap);
  R->device_ms = 0;
  if (cutoff == INT64_MIN || !n_st) return;  // no start is below it / no state

  SnapEvents E;
  E.create();
  ExpAlloc tmp;
  Kept K(tmp, n_ips);
  if (tmp.nomem) throw BjxError(BJX_ERR_NOMEM, "bjx_state_trim: no device memory for the scan buffers");
  unsigned long long gone = 0, live = 0;
  e->chk.ensure(8);
  HIP_OK(hipEventRecord(E.ev[0], st));
  HIP_OK(hipMemsetAsync(K.keep, 0, (n_ips + 1) * 4, st));
  HIP_OK(hipMemsetAsync(e->chk.p, 0, 32, st));
  hipLaunchKernelGGL(k_trim_mark, dim3((unsigned)std::min<uint64_t>(grid_for(e->st_cap), 8192)), dim3(kBlock), 0, st, e->st_cap,
                     S.st, cutoff, live_floor, n_ips, K.keep, e->chk.p);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(k_exp_len, dim3(grid_for(n_ips + 1)), dim3(kBlock), 0, st, n_ips, K.keep, S.ip_len, K.klen);
  HIP_OK(hipGetLastError());
  pin_get(e, &gone, e->chk.p + 1, 8);  // land with scan_kept's reads
  pin_get(e, &live, e->chk.p + 2, 8);
  scan_kept(e, K, n_ips, used, e->st_cap, E.ev[1], "internal: trim counts exceed the tables");
  R->device_ms = E.ms(0, 1);
  if (!gone) return;  // the tables were only read
  R->states_dropped = gone;
  R->states_dropped_live = live;
  R->ips_dropped = n_ips - K.ips;
  R->arena_bytes_after = K.bytes;
  if (flags & BJX_TRIM_DRY_RUN) return;
  e->counters_fresh = false;
  rebuild_kept(e, K, n_ips, used, E.ev[2], E.ev[3], "bjx_state_trim: no device memory for the new tables (state unchanged)",
               [&](NewTables &nw) {
                 hipLaunchKernelGGL(k_exp_st, dim3(grid_for(e->st_cap)), dim3(kBlock), 0, st, e->st_cap, S.st, cutoff, n_ips, K.nid,
                                    nw.st, nw.st_cap - 1);
               });
  R->device_bytes_after = state_device_bytes(e->ip_cap, e->st_cap, S.arena_cap);
  R->device_ms += E.ms(2, 3);
}

}  // namespace

int bjx_trim_select(bjx_engine *e, const bjx_trim_budget *b, bjx_trim::Picked *out) {
  return guarded(e, [&]() -> int {
    trim_select_locked(e, b, out);
    return BJX_OK;
  });
}

int bjx_trim_apply(bjx_engine *e, int64_t cutoff_ns, int64_t live_floor_ns, uint32_t flags, bjx_trim_stats *out) {
  return guarded(e, [&]() -> int {
    bjx_trim_stats R{};
    trim_apply_locked(e, cutoff_ns, live_floor_ns, flags, &R);
    if (out) *out = R;
    return BJX_OK;
  });
}

// Trim: the selection, then the expiry at the cutoff it found, under one hold
// of the engine lock.
extern "C" int bjx_state_trim(bjx_engine *e, const bjx_trim_budget *b, bjx_trim_stats *out) {
  return guarded(e, [&]() -> int {
    bjx_trim::Picked P;
    trim_select_locked(e, b, &P);
    bjx_trim_stats R{};
    trim_apply_locked(e, P.cutoff, b->floor_cutoff_ns, b->flags, &R);
    R.cutoff_ns = P.cutoff; R.bound = P.bound; R.budget_met = P.budget_met;
    R.select_ms = P.select_ms;
    R.device_ms += P.select_ms;
    if (out) *out = R;
    return BJX_OK;
  });
}

// ---- groups: bjx_state_query_groups (the checks, the key of an address, the
// group record, the rows' order, the node's merge: state_groups.h).  One pass
// over the state table adds every selected state into a 32-byte record per
// held IP (k_grp_scan: a state count, a hits sum, the newest start under the
// trim's biased key; an IP has at most as many states as there are names, so
// these atomics do not pile up).  One lane per held IP with a count then parses the
// address in place, masks it and appends its key (k_grp_key).  The keys are
// sorted through an index by the bits in which keys can differ -- the low
// word, the high word, then the family bit when both families are present --
// and laid out in that order (k_grp_sorted).  k_grp_heads marks the first key
// of every run of equal keys, a scan numbers the runs, and k_grp_runs reduces
// each run to one record: a block owns kGrpTile consecutive keys, a thread
// sums its kGrpItems keys in registers run by run and adds each run to the
// block's LDS record of that group; a group that lies inside the tile is then
// stored plainly, and only the tile's first and last group, when they go on in
// a neighbouring tile, are added to global memory -- so a /0 group of every
// IP costs two global atomics a block, not one a member.  The records come out
// in key order, which is the rows' tie order: min_ips is a stable compaction
// (flags and a scan), the order a stable sort by the primary key alone.
namespace {

constexpr int kGrpItems = 4;                                // k_grp_runs: consecutive keys per thread
constexpr uint32_t kGrpTile = kBlock * kGrpItems;           // keys per block of k_grp_runs
static_assert(sizeof(bjx_group_row) == 56 && sizeof(bjx_group_spec) == 24, "the groups structs of the C ABI");
// what the scan adds up per held IP: one 32-byte record, so that the three
// atomics of a state fall into one cache line and k_grp_runs reads an IP's
// values with one load (the scan itself runs at the rate of its atomics and
// took the same time with three arrays: DESIGN.md §2 "Groups")
struct GrpAcc {
  unsigned long long hsum, newest;  // hits, wrapping; the newest start as bjx_groups::start_key
  uint32_t cnt, _pad[3];            // selected states
};
static_assert(sizeof(GrpAcc) == 32, "GrpAcc is half a cache line");

// grid-stride over the state table (k_rm_mark's shape); sel != NULL: only the
// states of IPs with sel[id] set.  acc[] zeroed before; tot[0] += selected
// states (one atomic per block)
__global__ __launch_bounds__(kBlock) void k_grp_scan(uint64_t st_cap, const StSlot *__restrict__ st, QFilter F, uint64_t n_ips,
                                                     uint32_t n_names, const uint32_t *__restrict__ sel,
                                                     GrpAcc *__restrict__ acc, unsigned long long *__restrict__ tot) {
  uint64_t n = 0, z = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < st_cap; i += (uint64_t)gridDim.x * blockDim.x) {
    const StSlot v = st[i];
    if (!rm_selected(v, F, n_ips, n_names, sel)) continue;  // (its IP id is below n_ips)
    const uint64_t id = (v.key >> 24) - 1;
    atomicAdd(&acc[id].cnt, 1u);
    atomicAdd(&acc[id].hsum, (unsigned long long)v.hits);
    const unsigned long long key = bjx_groups::start_key(v.start);
    if (acc[id].newest < key) atomicMax(&acc[id].newest, key);  // it only grows: a read that covers this state spares the atomic
    ++n;
  }
  block_sum2(n, z);
  if (threadIdx.x == 0 && n) atomicAdd(&tot[0], (unsigned long long)n);
}

// One lane per held IP; every block runs the same number of passes
// (block_alloc).  An IP with a count whose bytes parse gets entry k of the key
// arrays: c_lo / c_hi the masked address, c_id its id with the family bit on
// top, perm[k] = k.  ctr[1] += entries (block_alloc), ctr[2] += IPs with a
// count, ctr[3] / ctr[4] += those that do not parse and their states,
// ctr[5] += IPv6 entries (one atomic each per block)
__global__ __launch_bounds__(kBlock) void k_grp_key(uint64_t n_ips, const GrpAcc *__restrict__ acc,
                                                    const uint64_t *__restrict__ ip_off, const uint32_t *__restrict__ ip_len,
                                                    const uint8_t *__restrict__ arena, uint64_t arena_used, uint32_t v4_bits,
                                                    uint32_t v6_bits, uint64_t room, unsigned long long *__restrict__ ctr,
                                                    uint64_t *__restrict__ c_lo, uint64_t *__restrict__ c_hi,
                                                    uint32_t *__restrict__ c_id, uint32_t *__restrict__ perm) {
  uint64_t has = 0, bad = 0, bad_st = 0, n6 = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < n_ips; base += (uint64_t)gridDim.x * kBlock) {
    const uint64_t id = base + threadIdx.x;
    const uint32_t c = id < n_ips ? acc[id].cnt : 0u;
    bool ok = false;
    uint32_t fam6 = 0;
    uint64_t hi = 0, lo = 0;
    if (c) {
      ++has;
      uint8_t a[16];
      if (net_ip_addr(id, ip_off, ip_len, arena, arena_used, a)) {
        ok = true;
        bjx_groups::pack(a, v4_bits, v6_bits, &fam6, &hi, &lo);
        n6 += fam6;
      } else {
        ++bad;
        bad_st += c;
      }
    }
    const uint64_t k = block_alloc(&ctr[1], ok ? 1 : 0);
    if (ok && k < room) {
      c_lo[k] = lo;
      c_hi[k] = hi;
      c_id[k] = (uint32_t)id | (fam6 << 31);
      perm[k] = (uint32_t)k;
    }
  }
  block_sum2(has, bad);
  __syncthreads();  // block_sum2's shared words are read before they are written again
  block_sum2(bad_st, n6);
  if (threadIdx.x == 0 && has) atomicAdd(&ctr[2], (unsigned long long)has);
  if (threadIdx.x == 0 && bad) atomicAdd(&ctr[3], (unsigned long long)bad);
  if (threadIdx.x == 0 && bad_st) atomicAdd(&ctr[4], (unsigned long long)bad_st);
  if (threadIdx.x == 0 && n6) atomicAdd(&ctr[5], (unsigned long long)n6);
}
// the next sort's key of entry perm[j]: the high word (what == 0) or the family bit
__global__ void k_grp_word(uint64_t n, const uint32_t *__restrict__ perm, const uint64_t *__restrict__ c_hi,
                           const uint32_t *__restrict__ c_id, uint32_t what, uint64_t *__restrict__ out) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t q = perm[j];
  out[j] = q < n ? (what ? (uint64_t)(c_id[q] >> 31) : c_hi[q]) : ~0ull;  // (a permutation of [0, n): always inside)
}
// the entries in sorted order
__global__ void k_grp_sorted(uint64_t n, const uint32_t *__restrict__ perm, const uint64_t *__restrict__ c_lo,
                             const uint64_t *__restrict__ c_hi, const uint32_t *__restrict__ c_id, uint64_t *__restrict__ s_lo,
                             uint64_t *__restrict__ s_hi, uint32_t *__restrict__ s_id) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t q = perm[j];
  const bool in = q < n;  // (a permutation of [0, n): always inside)
  s_lo[j] = in ? c_lo[q] : 0;
  s_hi[j] = in ? c_hi[q] : 0;
  s_id[j] = in ? c_id[q] : 0x7FFFFFFFu;  // (an id k_grp_runs does not follow)
}
// head[j] = 1 where sorted entry j begins a run of equal keys, over [0, n] (the last entry 0: the scan's total lands there)
__global__ void k_grp_heads(uint64_t n, const uint64_t *__restrict__ s_lo, const uint64_t *__restrict__ s_hi,
                            const uint32_t *__restrict__ s_id, uint32_t *__restrict__ head) {
  const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j > n) return;
  if (j == n) { head[j] = 0; return; }
  head[j] = j == 0 || s_lo[j] != s_lo[j - 1] || s_hi[j] != s_hi[j - 1] || ((s_id[j] ^ s_id[j - 1]) >> 31) ? 1u : 0u;
}
// Block b reduces sorted entries [b * kGrpTile, (b + 1) * kGrpTile) (the grid
// is exactly the tiles).  gpos = the exclusive scan of head: entry j lies in
// group gpos[j] + head[j] - 1.  out[] zeroed before; the entry that begins a
// group writes its key.
__global__ __launch_bounds__(kBlock) void k_grp_runs(uint64_t n, const uint64_t *__restrict__ s_lo, const uint64_t *__restrict__ s_hi,
                                                     const uint32_t *__restrict__ s_id, const uint32_t *__restrict__ head,
                                                     const uint32_t *__restrict__ gpos, uint64_t n_ips,
                                                     const GrpAcc *__restrict__ acc, uint64_t n_groups,
                                                     bjx_groups::Rec *__restrict__ out) {
  __shared__ uint32_t l_ips[kGrpTile];
  __shared__ unsigned long long l_st[kGrpTile], l_hits[kGrpTile], l_new[kGrpTile];
  const uint64_t t0 = (uint64_t)blockIdx.x * kGrpTile;
  if (t0 >= n) return;  // (the grid is exactly the tiles)
  const uint64_t t1 = t0 + kGrpTile < n ? t0 + kGrpTile : n;
  for (uint32_t k = threadIdx.x; k < kGrpTile; k += kBlock) {
    l_ips[k] = 0;
    l_st[k] = l_hits[k] = l_new[k] = 0;
  }
  __syncthreads();
  const uint64_t g0 = (uint64_t)gpos[t0] + head[t0] - 1;  // the tile's first group (head[0] is 1)
  uint64_t run = ~0ull;
  uint32_t a_ips = 0;
  unsigned long long a_st = 0, a_hits = 0, a_new = 0;
  auto flush = [&]() {
    const uint64_t l = run - g0;  // the tile holds at most kGrpTile groups
    if (a_ips && l < kGrpTile) {
      atomicAdd(&l_ips[l], a_ips);
      atomicAdd(&l_st[l], a_st);
      atomicAdd(&l_hits[l], a_hits);
      atomicMax(&l_new[l], a_new);
    }
    a_ips = 0;
    a_st = a_hits = a_new = 0;
  };
  const uint64_t j0 = t0 + (uint64_t)threadIdx.x * kGrpItems;
#pragma unroll
  for (int i = 0; i < kGrpItems; ++i) {
    const uint64_t j = j0 + i;
    if (j >= t1) break;
    const uint32_t h = head[j], w = s_id[j], id = w & 0x7FFFFFFFu;
    const uint64_t g = (uint64_t)gpos[j] + h - 1;
    if (g != run) {
      flush();
      run = g;
    }
    if (h && g < n_groups) {
      out[g].hi = s_hi[j];
      out[g].lo = s_lo[j];
      out[g].fam6 = w >> 31;
    }
    if (id < n_ips) {
      const GrpAcc v = acc[id];
      a_ips += 1;
      a_st += v.cnt;
      a_hits += v.hsum;
      a_new = v.newest > a_new ? v.newest : a_new;
    }
  }
  flush();
  __syncthreads();
  const uint64_t g1 = (uint64_t)gpos[t1 - 1] + head[t1 - 1] - 1;  // the tile's last group
  const uint64_t n_local = g1 - g0 + 1;
  const bool open_front = head[t0] == 0;           // the first group began in an earlier tile
  const bool open_back = t1 < n && head[t1] == 0;  // the last group goes on in the next tile
  for (uint64_t l = threadIdx.x; l < n_local && l < kGrpTile; l += kBlock) {
    const uint64_t g = g0 + l;
    if (g >= n_groups) continue;
    if ((l == 0 && open_front) || (l == n_local - 1 && open_back)) {
      atomicAdd((unsigned long long *)&out[g].n_ips, (unsigned long long)l_ips[l]);
      atomicAdd((unsigned long long *)&out[g].n_states, l_st[l]);
      atomicAdd((unsigned long long *)&out[g].hits, l_hits[l]);
      atomicMax((unsigned long long *)&out[g].newest, l_new[l]);
    } else {
      out[g].n_ips = l_ips[l];
      out[g].n_states = l_st[l];
      out[g].hits = l_hits[l];
      out[g].newest = l_new[l];
    }
  }
}
// ok[g] = 1 for the groups with n_ips >= min_ips, over [0, n_groups] (the last entry 0)
__global__ void k_grp_ok(uint64_t n_groups, const bjx_groups::Rec *__restrict__ recs, uint64_t min_ips, uint32_t *__restrict__ ok) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g > n_groups) return;
  ok[g] = g < n_groups && recs[g].n_ips >= min_ips ? 1u : 0u;
}
// the kept groups, still in key order: the primary key turned round (a
// smaller word is an earlier row) and the group's index.  top: an upper bound
// of the unsigned primaries, so that their words stay within its bits
__global__ void k_grp_prim(uint64_t n_groups, const bjx_groups::Rec *__restrict__ recs, const uint32_t *__restrict__ ok,
                           const uint32_t *__restrict__ pos, uint64_t room, uint32_t order, uint64_t top,
                           uint64_t *__restrict__ prim, uint32_t *__restrict__ gi) {
  const uint64_t g = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups || !ok[g]) return;
  const uint64_t k = pos[g];
  if (k >= room) return;  // (a scan of ok[]: always inside)
  const bjx_groups::Rec r = recs[g];
  const uint64_t v = order == BJX_GROUPS_BY_IPS ? r.n_ips : r.n_states;
  prim[k] = order == BJX_GROUPS_BY_HITS ? bjx_query::key_desc((int64_t)r.hits) : (v <= top ? top - v : 0);
  gi[k] = (uint32_t)g;
}
__global__ void k_grp_rows(uint64_t n_rows, const uint32_t *__restrict__ gi, uint64_t n_groups,
                           const bjx_groups::Rec *__restrict__ recs, bjx_groups::Rec *__restrict__ rows) {
  const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n_rows) return;
  const uint32_t g = gi[r];
  rows[r] = g < n_groups ? recs[g] : bjx_groups::Rec{};  // (an index of a group: always inside)
}

// The query (the engine lock held by the caller's guarded()).  list == NULL:
// the rows into e->grp_rows and *out.  list != NULL (the node): every group
// in key order into *list, at most `room` of them, and the counts into *cnt.
int groups_locked(bjx_engine *e, const bjx_state_filter *f, const bjx_group_spec *g, bjx_state_groups *out, uint64_t room,
                  std::vector<bjx_groups::Rec> *list, bjx_groups::Counts *cnt) {
  const std::string who = "bjx_state_query_groups";
  if (out) memset(out, 0, sizeof *out);
  if (list) list->clear();
  if (cnt) *cnt = bjx_groups::Counts{};
  if (const char *why = bjx_groups::check_filter(f)) throw BjxError(BJX_ERR_ARG, who + ": " + why);
  if (const char *why = bjx_groups::check_spec(g)) throw BjxError(BJX_ERR_ARG, who + ": " + why);
  if (e->batch_open) throw BjxError(BJX_ERR_ARG, who + " between bjx_match_batch and its bjx_finish_batch");
  HIP_OK(hipDeviceSynchronize());  // the tables as the last batch left them
  State &S = e->S;
  hipStream_t st = e->stream;
  SnapEvents E;
  E.create();
  read_counters(e);
  const uint64_t n_ips = e->host_counters[0], used = e->host_counters[1], n_st = e->host_counters[2];
  const uint32_t n_names = (uint32_t)e->names.size();
  if (!list) e->grp_rows.clear();
  QFilter F{f->min_hits, f->min_start_ns, f->max_start_ns, kNone, 0u};
  if (f->name.ptr) {
    auto it = e->name_ids.find(std::string(f->name.ptr, f->name.len));
    if (it == e->name_ids.end()) return BJX_OK;  // never interned: no state can carry it
    F.name = it->second;
  }
  if (bjx_query::empty_window(*f) || !n_ips || !n_st || !n_names) return BJX_OK;
  if (n_ips >= 0x7FFFFFFFull) throw BjxError(BJX_ERR_CAPACITY, who + ": 2^31 distinct IPs or more");
  bjx_remove::List L;  // the filter's ip as a list of one (k_rm_ips finds it)
  bjx_remove::pack(*f, nullptr, 0, &L);

  ExpAlloc tmp;
  GrpAcc *d_acc = tmp.get<GrpAcc>(n_ips + 1);
  unsigned long long *d_ctr = tmp.get<unsigned long long>(8);
  uint32_t *sel = L.restrict ? tmp.get<uint32_t>(n_ips + 1) : nullptr;
  const uint64_t off_bytes = ((uint64_t)L.n_entries() + 1) * 4;
  const uint64_t list_bytes = L.restrict ? off_bytes + L.bytes.size() : 0;
  uint8_t *d_list = L.restrict ? tmp.get<uint8_t>(((list_bytes + 3) & ~3ull) + 16) : nullptr;
  if (tmp.nomem) throw BjxError(BJX_ERR_NOMEM, who + ": no device memory for the per-IP sums");
  if (L.restrict) {
    std::vector<uint8_t> img(list_bytes);
    memcpy(img.data(), L.off.data(), off_bytes);
    if (!L.bytes.empty()) memcpy(img.data() + off_bytes, L.bytes.data(), L.bytes.size());
    snap_copy_in(e, d_list, img.data(), list_bytes);  // one upload; waits for the stream
  }
  double ms = 0;

  // 1. the per-IP sums
  HIP_OK(hipEventRecord(E.ev[0], st));
  HIP_OK(hipMemsetAsync(d_ctr, 0, 64, st));
  HIP_OK(hipMemsetAsync(d_acc, 0, (n_ips + 1) * sizeof(GrpAcc), st));
  if (L.restrict) {
    HIP_OK(hipMemsetAsync(sel, 0, (n_ips + 1) * 4, st));
    hipLaunchKernelGGL(k_rm_ips, dim3(grid_for(L.sel_count)), dim3(kBlock), 0, st, L.sel_first, L.sel_count,
                       reinterpret_cast<const uint32_t *>(d_list), d_list + off_bytes, e->dbg_hash_mask, S.ip, S.ip_mask, n_ips, S.ip_off,
                       S.ip_len, S.arena, used, sel);
    HIP_OK(hipGetLastError());
  }
  hipLaunchKernelGGL(k_grp_scan, dim3((unsigned)std::min<uint64_t>(grid_for(e->st_cap), 8192)), dim3(kBlock), 0, st, e->st_cap, S.st, F,
                     n_ips, n_names, sel, d_acc, d_ctr);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(E.ev[1], st));
  unsigned long long matched = 0;
  pin_get(e, &matched, d_ctr, 8);
  pin_sync(e);
  ms += E.ms(0, 1);
  if (matched > n_st) throw BjxError(BJX_ERR_DEVICE, "internal: groups counts disagree with the tables");
  bjx_groups::Counts C;
  C.n_matched = matched;
  auto done = [&]() {
    C.device_ms = ms;
    if (cnt) *cnt = C;
    if (out) {
      out->n_matched = C.n_matched; out->n_ips_matched = C.n_ips_matched;
      out->n_ips_unparsed = C.n_ips_unparsed; out->n_states_unparsed = C.n_states_unparsed;
      out->device_ms = ms;
    }
    return BJX_OK;
  };
  if (!matched) return done();

  // 2. the keys of the IPs with a count
  const uint64_t key_room = std::min<uint64_t>(n_ips, matched);  // an entry is an IP with a selected state
  uint64_t *c_lo = tmp.get<uint64_t>(key_room), *c_hi = tmp.get<uint64_t>(key_room);
  uint64_t *w0 = tmp.get<uint64_t>(key_room), *w1 = tmp.get<uint64_t>(key_room);
  uint32_t *c_id = tmp.get<uint32_t>(key_room), *p0 = tmp.get<uint32_t>(key_room), *p1 = tmp.get<uint32_t>(key_room);
  uint32_t *head = tmp.get<uint32_t>(key_room + 1), *gpos = tmp.get<uint32_t>(key_room + 1);
  if (tmp.nomem) throw BjxError(BJX_ERR_NOMEM, who + ": no device memory for the keys");
  HIP_OK(hipEventRecord(E.ev[0], st));
  hipLaunchKernelGGL(k_grp_key, dim3((unsigned)std::min<uint64_t>(grid_for(n_ips), 8192)), dim3(kBlock), 0, st, n_ips, d_acc, S.ip_off,
                     S.ip_len, S.arena, used, g->v4_bits, g->v6_bits, key_room, d_ctr, c_lo, c_hi, c_id, p0);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(E.ev[1], st));
  unsigned long long got[5] = {};  // entries, IPs with a count, unparsed IPs, their states, IPv6 entries
  pin_get(e, got, d_ctr + 1, sizeof got);
  pin_sync(e);
  ms += E.ms(0, 1);
  const uint64_t n = got[0];
  if (n > key_room || got[1] > n_ips || n + got[2] != got[1] || got[3] > matched || got[4] > n)
    throw BjxError(BJX_ERR_DEVICE, "internal: groups keys disagree with the counts");
  C.n_ips_matched = got[1];
  C.n_ips_unparsed = got[2];
  C.n_states_unparsed = got[3];
  if (!n) return done();

  // 3. sort through the index, the low word first; the runs; one record a run
  const bjx_groups::SortBits B = bjx_groups::sort_bits(g->v4_bits, g->v6_bits);
  uint32_t *perm = p0, *spare = p1;
  HIP_OK(hipEventRecord(E.ev[0], st));
  auto sort_by = [&](const uint64_t *keys, int b0, int b1) {
    cub_call(e, [&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, keys, w1, perm, spare, (int)n, b0, b1, st); });
    std::swap(perm, spare);
  };
  if (B.lo_end > B.lo_begin) sort_by(c_lo, B.lo_begin, B.lo_end);
  if (B.hi_end > B.hi_begin && got[4]) {
    hipLaunchKernelGGL(k_grp_word, dim3(grid_for(n)), dim3(kBlock), 0, st, n, perm, c_hi, c_id, 0u, w0);
    HIP_OK(hipGetLastError());
    sort_by(w0, B.hi_begin, B.hi_end);
  }
  if (got[4] && got[4] < n) {  // both families: the family bit above everything
    hipLaunchKernelGGL(k_grp_word, dim3(grid_for(n)), dim3(kBlock), 0, st, n, perm, c_hi, c_id, 1u, w0);
    HIP_OK(hipGetLastError());
    sort_by(w0, 0, 1);
  }
  uint64_t *s_lo = w0, *s_hi = w1;
  uint32_t *s_id = spare;
  hipLaunchKernelGGL(k_grp_sorted, dim3(grid_for(n)), dim3(kBlock), 0, st, n, perm, c_lo, c_hi, c_id, s_lo, s_hi, s_id);
  HIP_OK(hipGetLastError());
  hipLaunchKernelGGL(k_grp_heads, dim3(grid_for(n + 1)), dim3(kBlock), 0, st, n, s_lo, s_hi, s_id, head);
  HIP_OK(hipGetLastError());
  cub_call(e, [&](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, head, gpos, (int)(n + 1), st); });
  HIP_OK(hipEventRecord(E.ev[1], st));
  uint32_t n_groups32 = 0;
  pin_get(e, &n_groups32, gpos + n, 4);
  pin_sync(e);
  ms += E.ms(0, 1);
  const uint64_t G = n_groups32;
  if (!G || G > n) throw BjxError(BJX_ERR_DEVICE, "internal: groups runs disagree with the keys");
  if (list && G > room) throw BjxError(BJX_ERR_CAPACITY, who + ": more groups than the node merges");
  bjx_groups::Rec *recs = tmp.get<bjx_groups::Rec>(G);
  if (tmp.nomem) throw BjxError(BJX_ERR_NOMEM, who + ": no device memory for the groups");
  HIP_OK(hipEventRecord(E.ev[0], st));
  HIP_OK(hipMemsetAsync(recs, 0, G * sizeof(bjx_groups::Rec), st));
  hipLaunchKernelGGL(k_grp_runs, dim3((unsigned)((n + kGrpTile - 1) / kGrpTile)), dim3(kBlock), 0, st, n, s_lo, s_hi, s_id, head, gpos,
                     n_ips, d_acc, G, recs);
  HIP_OK(hipGetLastError());
  if (list) {
    HIP_OK(hipEventRecord(E.ev[1], st));
    list->resize(G);
    HIP_OK(hipMemcpyAsync(list->data(), recs, G * sizeof(bjx_groups::Rec), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
    ms += E.ms(0, 1);
    return done();
  }

  // 4. min_ips (a stable compaction), the order (a stable sort), the first rows
  bjx_groups::Rec *d_rows = tmp.get<bjx_groups::Rec>(std::min<uint64_t>(g->limit, G));
  uint32_t *ok = tmp.get<uint32_t>(G + 1), *pos = tmp.get<uint32_t>(G + 1);
  if (tmp.nomem) throw BjxError(BJX_ERR_NOMEM, who + ": no device memory for the rows");
  hipLaunchKernelGGL(k_grp_ok, dim3(grid_for(G + 1)), dim3(kBlock), 0, st, G, recs, g->min_ips, ok);
  HIP_OK(hipGetLastError());
  cub_call(e, [&](void *t, size_t &b) { return hipcub::DeviceScan::ExclusiveSum(t, b, ok, pos, (int)(G + 1), st); });
  HIP_OK(hipEventRecord(E.ev[1], st));
  uint32_t n_min32 = 0;
  pin_get(e, &n_min32, pos + G, 4);
  pin_sync(e);
  ms += E.ms(0, 1);
  const uint64_t n_min = n_min32;
  if (n_min > G) throw BjxError(BJX_ERR_DEVICE, "internal: groups compaction disagrees with the runs");
  out->n_groups = G;
  out->n_groups_min = n_min;
  const uint64_t n_rows = std::min<uint64_t>(g->limit, n_min);
  if (!n_rows) return done();
  uint64_t *pr0 = tmp.get<uint64_t>(n_min), *pr1 = tmp.get<uint64_t>(n_min);
  uint32_t *gi0 = tmp.get<uint32_t>(n_min), *gi1 = tmp.get<uint32_t>(n_min);
  if (tmp.nomem) throw BjxError(BJX_ERR_NOMEM, who + ": no device memory for the order");
  const uint64_t top = g->order == BJX_GROUPS_BY_IPS ? n : matched;  // no group has more IPs / states
  const int bits = g->order == BJX_GROUPS_BY_HITS ? 64 : std::max(1, bit_width(top));
  HIP_OK(hipEventRecord(E.ev[0], st));
  hipLaunchKernelGGL(k_grp_prim, dim3(grid_for(G)), dim3(kBlock), 0, st, G, recs, ok, pos, n_min, g->order, top, pr0, gi0);
  HIP_OK(hipGetLastError());
  cub_call(e, [&](void *t, size_t &b) { return hipcub::DeviceRadixSort::SortPairs(t, b, pr0, pr1, gi0, gi1, (int)n_min, 0, bits, st); });
  hipLaunchKernelGGL(k_grp_rows, dim3(grid_for(n_rows)), dim3(kBlock), 0, st, n_rows, gi1, G, recs, d_rows);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(E.ev[1], st));
  std::vector<bjx_groups::Rec> h_rows(n_rows);
  HIP_OK(hipMemcpyAsync(h_rows.data(), d_rows, n_rows * sizeof(bjx_groups::Rec), hipMemcpyDeviceToHost, st));
  HIP_OK(hipStreamSynchronize(st));
  ms += E.ms(0, 1);
  e->grp_rows.reserve(n_rows);
  for (const bjx_groups::Rec &r : h_rows) e->grp_rows.push_back(bjx_groups::row_of(r, *g));
  out->n_rows = n_rows;
  out->rows = e->grp_rows.data();
  return done();
}

}  // namespace

// test hook (include/banjax_gpu_debug.h): the sorted keys one block of k_grp_runs reduces
extern "C" uint32_t bjx_debug_groups_tile(void) { return kGrpTile; }

extern "C" int bjx_state_query_groups(bjx_engine *e, const bjx_state_filter *f, const bjx_group_spec *g, bjx_state_groups *out) {
  if (!e || !f || !g || !out) return BJX_ERR_ARG;
  return guarded(e, [&]() -> int { return groups_locked(e, f, g, out, 0, nullptr, nullptr); });
}

int bjx_groups_list(bjx_engine *e, const bjx_state_filter *f, const bjx_group_spec *g, uint64_t room,
                    std::vector<bjx_groups::Rec> *list, bjx_groups::Counts *counts) {
  if (!e || !f || !g || !list || !counts) return BJX_ERR_ARG;
  return guarded(e, [&]() -> int { return groups_locked(e, f, g, nullptr, room, list, counts); });
}

// ---- names: bjx_state_query_names (the checks, the histogram bucket, the
// record per name, the rows' order, the node's merge: state_names.h).  One
// pass over the state table (k_nam_scan, k_qry_scan's shape: 64-bit indices,
// kNamItems slots per thread and pass, a capped grid) stores keep[ip id] = 1
// for every selected state -- a hipCUB sum of keep[] is n_ips_matched, as in
// the query -- and adds the state into the accumulators of its name: one
// histogram bin by bjx_names::bucket(hits), the hits sum, and three maxima
// (the largest hits, the newest start, the complement of the oldest start, all
// as unsigned keys, so that zeroed memory is the empty accumulator).  The
// count of a name is the sum of its bins and is never added on its own.
// LDS path: while all interned names fit, the accumulators are LDS arrays
// indexed by name id, [field][name] so that neighbouring names fall into
// neighbouring banks: 16 u32 bins and four 64-bit words, 96 bytes a name.
// A maximum is read before it is raised (it only grows: a read that already
// covers the state spares the atomic).  At its end a block adds its non-empty
// bins to the global records, at most one global atomic per field, name and
// block.  Global path: the same adds, straight to the global records.
// k_nam_compact appends the records with a count densely (block_alloc) and
// fills in the count and the name id; the host copies exactly those.
namespace {

constexpr int kNamBlock = 1024;  // threads of k_nam_scan: with 96 B of LDS a name a CU holds one block, which then brings 16 waves
constexpr int kNamItems = 4;     // state slots per thread and pass
constexpr uint32_t kNamLdsBytes = 96;                                // LDS per name: 4 x 8 + 16 x 4
constexpr uint32_t kNamLdsMax = 128 * 1024;                          // dynamic LDS a block may ask for (of gfx950's 160 KiB; rule_stats.h takes the same)
constexpr uint32_t kNamLdsNames = kNamLdsMax / kNamLdsBytes;         // names the LDS path takes: 1,365
constexpr unsigned kNamGridLds = 256;    // blocks at most on the LDS path: one per CU, each flushes its bins once
constexpr unsigned kNamGridGlobal = 2048;  // blocks at most on the global path (nothing to flush)
static_assert(sizeof(bjx_name_row) == 184 && sizeof(bjx_names_spec) == 16 && sizeof(bjx_state_names) == 72,
              "the names structs of the C ABI");

// raise a maximum that only grows.  The plain read may be stale while other
// waves raise the word with atomics, but a stale value is never above the
// current one: the read can only fail to spare an atomicMax, it can never
// skip an update that was needed.
__device__ __forceinline__ void nam_max(unsigned long long *p, unsigned long long v) {
  if (*reinterpret_cast<volatile unsigned long long *>(p) < v) atomicMax(p, v);
}

// grid-stride over the state table; sel != NULL: only the states of IPs with
// sel[id] set.  g[n_names] zeroed before; keep[ip id] = 1 for a selected
// state; tot[0] += selected states (one atomic per block).  LDS: the dynamic
// LDS holds n_names * kNamLdsBytes bytes.
template <bool LDS>
__global__ __launch_bounds__(kNamBlock) void k_nam_scan(uint64_t st_cap, const StSlot *__restrict__ st, QFilter F, uint64_t n_ips,
                                                        uint32_t n_names, const uint32_t *__restrict__ sel,
                                                        uint32_t *__restrict__ keep, bjx_names::Rec *__restrict__ g,
                                                        unsigned long long *__restrict__ tot) {
  extern __shared__ unsigned long long nam_lds[];
  __shared__ unsigned long long s_n;
  unsigned long long *const l64 = nam_lds;                                            // [4][n_names]: hits, max_hits, newest, oldest_inv
  uint32_t *const l32 = reinterpret_cast<uint32_t *>(nam_lds + 4 * (size_t)n_names);  // [16][n_names]: the histogram
  if constexpr (LDS) {
    for (uint32_t i = threadIdx.x; i < 4 * n_names; i += kNamBlock) l64[i] = 0;
    for (uint32_t i = threadIdx.x; i < BJX_NAMES_HIST * n_names; i += kNamBlock) l32[i] = 0;
  }
  if (threadIdx.x == 0) s_n = 0;
  __syncthreads();
  unsigned long long n = 0;
  constexpr uint64_t kTile = (uint64_t)kNamBlock * kNamItems;
  for (uint64_t base = (uint64_t)blockIdx.x * kTile; base < st_cap; base += (uint64_t)gridDim.x * kTile) {
    StSlot v[kNamItems];
#pragma unroll
    for (int j = 0; j < kNamItems; ++j) {
      const uint64_t i = base + (uint64_t)j * kNamBlock + threadIdx.x;
      v[j] = i < st_cap ? st[i] : StSlot{0, 0, 0, 0};  // (an empty slot never passes)
    }
#pragma unroll
    for (int j = 0; j < kNamItems; ++j) {
      if (!rm_selected(v[j], F, n_ips, n_names, sel)) continue;  // (its IP id is below n_ips, its name id below n_names)
      keep[(v[j].key >> 24) - 1] = 1u;                          // every writer stores the same value
      const uint32_t name = (uint32_t)(v[j].key & 0xFFFFFFull);
      const uint32_t b = bjx_names::bucket(v[j].hits);
      const unsigned long long kh = bjx_names::key_of(v[j].hits), ks = bjx_names::key_of(v[j].start);
      if constexpr (LDS) {
        atomicAdd(&l32[b * n_names + name], 1u);
        atomicAdd(&l64[name], (unsigned long long)v[j].hits);
        nam_max(&l64[n_names + name], kh);
        nam_max(&l64[2 * n_names + name], ks);
        nam_max(&l64[3 * n_names + name], ~ks);
      } else {
        bjx_names::Rec *r = &g[name];
        atomicAdd((unsigned long long *)&r->hist[b], 1ull);
        atomicAdd((unsigned long long *)&r->hits, (unsigned long long)v[j].hits);
        nam_max((unsigned long long *)&r->max_hits, kh);
        nam_max((unsigned long long *)&r->newest, ks);
        nam_max((unsigned long long *)&r->oldest_inv, ~ks);
      }
      ++n;
    }
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) n += __shfl_xor(n, d);
  if ((threadIdx.x & 63) == 0 && n) atomicAdd(&s_n, n);
  __syncthreads();
  if (threadIdx.x == 0 && s_n) atomicAdd(&tot[0], s_n);
  if constexpr (LDS) {
    for (uint32_t i = threadIdx.x; i < n_names; i += kNamBlock) {
      bool any = false;
#pragma unroll
      for (int b = 0; b < BJX_NAMES_HIST; ++b) {
        const uint32_t c = l32[b * n_names + i];
        if (c) {
          atomicAdd((unsigned long long *)&g[i].hist[b], (unsigned long long)c);
          any = true;
        }
      }
      if (!any) continue;
      if (l64[i]) atomicAdd((unsigned long long *)&g[i].hits, l64[i]);
      atomicMax((unsigned long long *)&g[i].max_hits, l64[n_names + i]);
      atomicMax((unsigned long long *)&g[i].newest, l64[2 * n_names + i]);
      atomicMax((unsigned long long *)&g[i].oldest_inv, l64[3 * n_names + i]);
    }
  }
}

// One lane per interned name; every block runs the same number of passes
// (block_alloc).  A name with a count gets entry k of out[]: its record with
// n_states = the sum of its bins and its id.  ctr[1] += entries.
__global__ __launch_bounds__(kBlock) void k_nam_compact(uint32_t n_names, const bjx_names::Rec *__restrict__ g, uint64_t room,
                                                        unsigned long long *__restrict__ ctr, bjx_names::Rec *__restrict__ out) {
  for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < n_names; base += (uint64_t)gridDim.x * kBlock) {
    const uint64_t id = base + threadIdx.x;
    uint64_t cnt = 0;
    if (id < n_names) {
#pragma unroll
      for (int b = 0; b < BJX_NAMES_HIST; ++b) cnt += g[id].hist[b];
    }
    const uint64_t k = block_alloc(&ctr[1], cnt ? 1 : 0);
    if (cnt && k < room) {  // the record is copied only for a name in use
      out[k] = g[id];
      out[k].n_states = cnt;
      out[k].id = (uint32_t)id;
      out[k]._pad = 0;
    }
  }
}

// The query (the engine lock held by the caller's guarded()).  list == NULL:
// the rows into e->nam_rows / e->nam_bytes and *out.  list != NULL (the
// node): every name with a selected state into *list, at most `room` of them,
// and the counts into *cnt.
int names_locked(bjx_engine *e, const bjx_state_filter *f, const bjx_names_spec *s, bjx_state_names *out, uint64_t room,
                 std::vector<bjx_names::Item> *list, bjx_names::Counts *cnt) {
  const std::string who = "bjx_state_query_names";
  if (out) memset(out, 0, sizeof *out);
  if (list) list->clear();
  if (cnt) *cnt = bjx_names::Counts{};
  if (const char *why = bjx_names::check_filter(f)) throw BjxError(BJX_ERR_ARG, who + ": " + why);
  if (const char *why = bjx_names::check_spec(s)) throw BjxError(BJX_ERR_ARG, who + ": " + why);
  if (e->batch_open) throw BjxError(BJX_ERR_ARG, who + " between bjx_match_batch and its bjx_finish_batch");
  HIP_OK(hipDeviceSynchronize());  // the tables as the last batch left them
  State &S = e->S;
  hipStream_t st = e->stream;
  SnapEvents E;
  E.create();
  read_counters(e);
  const uint64_t n_ips = e->host_counters[0], used = e->host_counters[1], n_st = e->host_counters[2];
  const uint32_t n_names = (uint32_t)e->names.size();
  e->nam_path = 0;
  if (!list) {
    e->nam_rows.clear();
    e->nam_bytes.clear();
  }
  QFilter F{f->min_hits, f->min_start_ns, f->max_start_ns, kNone, 0u};
  if (f->name.ptr) {
    auto it = e->name_ids.find(std::string(f->name.ptr, f->name.len));
    if (it == e->name_ids.end()) return BJX_OK;  // never interned: no state can carry it
    F.name = it->second;
  }
  if (bjx_query::empty_window(*f) || !n_ips || !n_st || !n_names) return BJX_OK;
  if (n_ips >= 0x7FFFFFFFull) throw BjxError(BJX_ERR_CAPACITY, who + ": 2^31 distinct IPs or more");
  bjx_remove::List L;  // the filter's ip as a list of one (k_rm_ips finds it)
  bjx_remove::pack(*f, nullptr, 0, &L);

  // every buffer, before anything is launched: all sizes are known now
  ExpAlloc tmp;
  bjx_names::Rec *d_acc = tmp.get<bjx_names::Rec>(n_names), *d_out = tmp.get<bjx_names::Rec>(n_names);
  uint32_t *keep = tmp.get<uint32_t>(n_ips + 1);
  uint32_t *d_sum = tmp.get<uint32_t>(4);
  unsigned long long *d_ctr = tmp.get<unsigned long long>(8);  // [0] matched [1] names with a count
  uint32_t *sel = L.restrict ? tmp.get<uint32_t>(n_ips + 1) : nullptr;
  const uint64_t off_bytes = ((uint64_t)L.n_entries() + 1) * 4;
  const uint64_t list_bytes = L.restrict ? off_bytes + L.bytes.size() : 0;
  uint8_t *d_list = L.restrict ? tmp.get<uint8_t>(((list_bytes + 3) & ~3ull) + 16) : nullptr;
  if (tmp.nomem) throw BjxError(BJX_ERR_NOMEM, who + ": no device memory for the per-name records");
  {  // and the sum's scratch, so that cub_call below finds it in place
    size_t b = 0;
    HIP_OK(hipcub::DeviceReduce::Sum((void *)nullptr, b, keep, d_sum, (int)n_ips, st));
    e->cub_tmp.ensure(b + 16);
  }
  if (L.restrict) {
    std::vector<uint8_t> img(list_bytes);
    memcpy(img.data(), L.off.data(), off_bytes);
    if (!L.bytes.empty()) memcpy(img.data() + off_bytes, L.bytes.data(), L.bytes.size());
    snap_copy_in(e, d_list, img.data(), list_bytes);  // one upload; waits for the stream
  }

  // the path and the grid.  The LDS bins are u32: one block must walk fewer
  // than 2^32 slots, so the grid never falls below st_cap / 2^32 + 1 blocks
  // (one block, whatever the cap, up to a table of 2^32 slots = 128 GiB).
  const uint32_t lds_names = e->dbg_nam_lds_names ? std::min(e->dbg_nam_lds_names, kNamLdsNames) : kNamLdsNames;
  const bool lds = n_names <= lds_names;
  const uint64_t tiles = (e->st_cap + (uint64_t)kNamBlock * kNamItems - 1) / ((uint64_t)kNamBlock * kNamItems);
  uint64_t cap = e->dbg_nam_blocks ? e->dbg_nam_blocks : (lds ? kNamGridLds : kNamGridGlobal);
  cap = std::max<uint64_t>(cap, (e->st_cap >> 32) + 1);
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(tiles, cap));
  const uint32_t lds_bytes = lds ? n_names * kNamLdsBytes : 0;
  if (lds && lds_bytes > 64 * 1024 && lds_bytes > e->nam_lds_set) {  // past the 64 KB of dynamic LDS a kernel has by default
    HIP_OK(hipFuncSetAttribute(reinterpret_cast<const void *>(&k_nam_scan<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)kNamLdsMax));
    e->nam_lds_set = kNamLdsMax;
  }

  HIP_OK(hipEventRecord(E.ev[0], st));
  HIP_OK(hipMemsetAsync(d_ctr, 0, 64, st));
  HIP_OK(hipMemsetAsync(d_sum, 0, 16, st));
  HIP_OK(hipMemsetAsync(d_acc, 0, (size_t)n_names * sizeof(bjx_names::Rec), st));
  HIP_OK(hipMemsetAsync(keep, 0, (n_ips + 1) * 4, st));
  if (L.restrict) {
    HIP_OK(hipMemsetAsync(sel, 0, (n_ips + 1) * 4, st));
    hipLaunchKernelGGL(k_rm_ips, dim3(grid_for(L.sel_count)), dim3(kBlock), 0, st, L.sel_first, L.sel_count,
                       reinterpret_cast<const uint32_t *>(d_list), d_list + off_bytes, e->dbg_hash_mask, S.ip, S.ip_mask, n_ips, S.ip_off,
                       S.ip_len, S.arena, used, sel);
    HIP_OK(hipGetLastError());
  }
  if (lds)
    hipLaunchKernelGGL(k_nam_scan<true>, dim3(grid), dim3(kNamBlock), lds_bytes, st, e->st_cap, S.st, F, n_ips, n_names, sel, keep, d_acc,
                       d_ctr);
  else
    hipLaunchKernelGGL(k_nam_scan<false>, dim3(grid), dim3(kNamBlock), 0, st, e->st_cap, S.st, F, n_ips, n_names, sel, keep, d_acc, d_ctr);
  HIP_OK(hipGetLastError());
  e->nam_path = lds ? 1 : 2;
  cub_call(e, [&](void *t, size_t &b) { return hipcub::DeviceReduce::Sum(t, b, keep, d_sum, (int)n_ips, st); });
  hipLaunchKernelGGL(k_nam_compact, dim3((unsigned)std::min<uint64_t>(grid_for(n_names), 1024)), dim3(kBlock), 0, st, n_names, d_acc,
                     (uint64_t)n_names, d_ctr, d_out);
  HIP_OK(hipGetLastError());
  HIP_OK(hipEventRecord(E.ev[1], st));
  unsigned long long got[2] = {0, 0};
  uint32_t ips_matched = 0;
  pin_get(e, got, d_ctr, 16);
  pin_get(e, &ips_matched, d_sum, 4);
  pin_sync(e);
  const double ms = E.ms(0, 1);
  const uint64_t matched = got[0], n_used = got[1];
  if (matched > n_st || n_used > n_names || n_used > matched || ips_matched > matched || (matched != 0) != (n_used != 0))
    throw BjxError(BJX_ERR_DEVICE, "internal: names counts disagree with the tables");
  if (list && n_used > room) throw BjxError(BJX_ERR_CAPACITY, who + ": more names than the node merges");
  std::vector<bjx_names::Rec> recs(n_used);
  if (n_used) {
    HIP_OK(hipMemcpyAsync(recs.data(), d_out, n_used * sizeof(bjx_names::Rec), hipMemcpyDeviceToHost, st));
    HIP_OK(hipStreamSynchronize(st));
  }
  uint64_t sum = 0;
  std::vector<bjx_names::Item> items(n_used);
  for (uint64_t k = 0; k < n_used; ++k) {
    if (recs[k].id >= n_names) throw BjxError(BJX_ERR_DEVICE, "internal: names records disagree with the interned names");
    items[k].name = e->names[recs[k].id];
    items[k].r = recs[k];
    sum += recs[k].n_states;
  }
  if (sum != matched) throw BjxError(BJX_ERR_DEVICE, "internal: names records do not add up to the matched states");
  bjx_names::Counts C;
  C.n_matched = matched;
  C.n_ips_matched = ips_matched;
  C.device_ms = ms;
  if (list) {
    *list = std::move(items);
    *cnt = C;
    return BJX_OK;
  }
  bjx_names::finish(std::move(items), *s, C, out, &e->nam_rows, &e->nam_bytes);
  return BJX_OK;
}

}  // namespace

// test hooks (include/banjax_gpu_debug.h)
extern "C" int bjx_debug_set_names(bjx_engine *e, uint32_t max_lds_names, uint32_t max_blocks) {
  if (!e) return BJX_ERR_ARG;
  std::lock_guard<std::mutex> g(e->mu);
  e->dbg_nam_lds_names = max_lds_names;
  e->dbg_nam_blocks = max_blocks;
  return BJX_OK;
}
extern "C" int bjx_debug_names_info(bjx_engine *e, int *path, uint32_t *lds_names_max) {
  if (!e) return BJX_ERR_ARG;
  std::lock_guard<std::mutex> g(e->mu);
  if (path) *path = e->nam_path;
  if (lds_names_max) *lds_names_max = kNamLdsNames;
  return BJX_OK;
}

extern "C" int bjx_state_query_names(bjx_engine *e, const bjx_state_filter *f, const bjx_names_spec *s, bjx_state_names *out) {
  if (!e || !f || !s || !out) return BJX_ERR_ARG;
  return guarded(e, [&]() -> int { return names_locked(e, f, s, out, 0, nullptr, nullptr); });
}

int bjx_names_list(bjx_engine *e, const bjx_state_filter *f, const bjx_names_spec *s, uint64_t room,
                   std::vector<bjx_names::Item> *list, bjx_names::Counts *counts) {
  if (!e || !f || !s || !list || !counts) return BJX_ERR_ARG;
  return guarded(e, [&]() -> int { return names_locked(e, f, s, nullptr, room, list, counts); });
}
