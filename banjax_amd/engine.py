"""One MI355X engine (bjx_engine): persistent rate-limit state in HBM plus the
batch pipeline of include/banjax_gpu.h."""
from __future__ import annotations

import ctypes as C
from typing import Iterable, List, Optional, Sequence, Tuple

from . import _lib
from .config import Config, Ruleset

INT64_MIN = -(1 << 63)
INT64_MAX = (1 << 63) - 1


class BatchOutput:
    """Host view of one bjx_process_batch.  The arrays live in engine-owned
    pinned memory valid until the next process(); `trips` / `results` are
    materialized as Python records only when read (trips_array() gives the
    zero-copy numpy view the Banner replay iterates)."""

    def __init__(self, res: _lib.BatchResult, copy_results: bool):
        self.n_lines = res.n_lines
        self.consumed_bytes = res.consumed_bytes
        self.n_results = res.n_results
        self.n_events = res.n_events
        self.n_trips = res.n_trips
        self.device_ms = res.device_ms
        self.match_kernel_ms = res.match_kernel_ms
        self._res = res
        self._trips = None
        self._results = None
        self._copy = copy_results
        self.line_flags = (bytes(C.string_at(res.line_flags, res.n_lines)) if res.n_lines else b"") \
            if copy_results else None

    @property
    def trips(self):
        if self._trips is None:
            self._need_full_trips()
            self._trips = [self._res.trips[i] for i in range(self.n_trips)] if self.n_trips else []
        return self._trips

    def _need_full_trips(self):
        if self.n_trips and not self._res.trips:
            raise ValueError("this batch was run with compact_trips=True: its trips are in trips_compact(), "
                             "not in full bjx_trip records")

    def trips_compact(self):
        """BJX_TRIPS_COMPACT: numpy uint64 words, line byte offset << 24 | rule index (zero-copy)."""
        import numpy as np
        if not self.n_trips or not self._res.trips_compact:
            return np.zeros(0, dtype=np.uint64)
        buf = (C.c_uint64 * self.n_trips).from_address(C.addressof(self._res.trips_compact.contents))
        return np.ctypeslib.as_array(buf)

    def trips_array(self):
        import numpy as np
        if not self.n_trips:
            return np.zeros(0, dtype=np.dtype(_lib.Trip))
        self._need_full_trips()
        buf = (_lib.Trip * self.n_trips).from_address(C.addressof(self._res.trips.contents))
        return np.ctypeslib.as_array(buf)

    @property
    def results(self):
        if not self._copy:
            return None
        if self._results is None:
            self._results = [self._res.results[i] for i in range(self.n_results)] if self.n_results else []
        return self._results


class BanBatch:
    """Host view of bjx_batch_bans: per-IP decision updates (trip order of
    their representative trip) and the LogRegexBan lines of the batch."""

    def __init__(self, bb: _lib.BanBatch):
        import numpy as np
        self.n_ips = bb.n_ips
        self.n_trips = bb.n_trips
        if bb.n_ips:
            arr = (_lib.IpDecision * bb.n_ips).from_address(C.addressof(bb.ips.contents))
            self.ips = np.ctypeslib.as_array(arr).copy()
        else:
            self.ips = np.zeros(0, dtype=np.dtype(_lib.IpDecision))
        self.log = C.string_at(bb.log, bb.log_bytes) if bb.log_bytes else b""
        n = bb.n_trips
        self.log_off = np.ctypeslib.as_array(bb.log_off, shape=(n + 1,)).copy() if n else np.zeros(1, np.uint64)
        self.log_kind = np.ctypeslib.as_array(bb.log_kind, shape=(n,)).copy() if n else np.zeros(0, np.uint8)
        m = bb.n_ips
        self.ip_off = np.ctypeslib.as_array(bb.ip_off, shape=(m + 1,)).copy() if m else np.zeros(1, np.uint64)
        self.ip_bytes = C.string_at(bb.ip_bytes, int(self.ip_off[m])) if m and self.ip_off[m] else b""

    def ip(self, r: int) -> bytes:
        """IP bytes of record r (the Update key)."""
        return self.ip_bytes[int(self.ip_off[r]):int(self.ip_off[r + 1])]

    def lines(self):
        """(kind, line without '\\n') per trip that logs (kind 1 Logger, 2 LoggerTemp)."""
        out = []
        for t in range(self.n_trips):
            k = int(self.log_kind[t])
            if k:
                out.append((k, self.log[int(self.log_off[t]):int(self.log_off[t + 1]) - 1]))
        return out


def _decision_entries(entries):
    entries = list(entries)
    arr = (_lib.DecisionEntry * max(1, len(entries)))()
    keep = []
    for i, (site, dec, ip) in enumerate(entries):
        s = _lib.Str(None, 0) if site is None else _lib.mkstr(site)
        ipb = _lib.mkstr(ip)
        keep.append((s, ipb))
        arr[i] = _lib.DecisionEntry(s, dec, ipb)
    return arr, len(entries), keep


def _ban_options(expiring_ttl_s, disable_logging, tz_offset_s, zone):
    hosts = [h for h in disable_logging]
    arr = (_lib.Str * max(1, len(hosts)))()
    strs = [_lib.mkstr(h) for h in hosts]
    for i, x in enumerate(strs):
        arr[i] = x
    ttl = (int(expiring_ttl_s) * 1_000_000_000) & ((1 << 64) - 1)
    if ttl >= 1 << 63:
        ttl -= 1 << 64
    trans = zone.transitions if zone is not None else []
    off = zone.offset_s if zone is not None else tz_offset_s
    tz = (_lib.TzTransition * max(1, len(trans)))(*[_lib.TzTransition(a, o, 0) for a, o in trans])
    return _lib.BanOptions(ttl, off, 0, arr, len(hosts), tz, len(trans)), (arr, tz, strs)


class Engine:
    def __init__(self, device: int = 0, ip_capacity: int = 0, state_capacity: int = 0, ip_arena_bytes: int = 0):
        L = _lib.lib()
        h = C.c_void_p()
        err = C.create_string_buffer(512)
        opts = _lib.EngineOptions(ip_capacity, state_capacity, ip_arena_bytes)
        rc = L.bjx_engine_create(device, C.byref(opts), C.byref(h), err, 512)
        if rc != _lib.OK:
            raise _lib.BanjaxGpuError(rc, "bjx_engine_create: " + err.value.decode(errors="replace"))
        self._h = h
        self.device = device

    def _check(self, rc, what):
        if rc < 0:
            msg = _lib.lib().bjx_engine_last_error(self._h)
            raise _lib.BanjaxGpuError(rc, "%s: %s" % (what, (msg or b"").decode(errors="replace")))
        return rc

    def set_decision_lists(self, entries: Iterable[Tuple[Optional[str], int, str]]):
        """StaticDecisionLists from config (decision.go:278-374)."""
        arr, n, keep = _decision_entries(entries)
        self._check(_lib.lib().bjx_engine_set_decision_lists(self._h, arr, n), "set_decision_lists")

    def set_ban_options(self, expiring_ttl_s: int, disable_logging: Iterable[str] = (), tz_offset_s: int = 0,
                        zone=None):
        """Banner settings of the device decision emission (bjx_engine_set_ban_options);
        zone: a regex_rate_limiter.Zone (local-zone transitions), else the fixed
        offset tz_offset_s."""
        o, keep = _ban_options(expiring_ttl_s, disable_logging, tz_offset_s, zone)
        self._check(_lib.lib().bjx_engine_set_ban_options(self._h, C.byref(o)), "set_ban_options")

    def bans(self) -> BanBatch:
        """Decision updates and ban-log lines of the last batch (run with emit_bans)."""
        bb = _lib.BanBatch()
        self._check(_lib.lib().bjx_batch_bans(self._h, C.byref(bb)), "batch_bans")
        return BanBatch(bb)

    def process(self, rs: Ruleset, data, now_ns: int, copy_results: bool = False, device_ptr: Optional[int] = None,
                nbytes: Optional[int] = None, emit_bans: bool = False, ban_log: bool = True,
                compact_trips: bool = False, rule_stats: bool = False) -> BatchOutput:
        """consumeLine over every complete line of `data` (bytes) or of a device
        buffer (device_ptr, nbytes) already resident in HBM.  emit_bans with
        ban_log=False: the per-IP decision records only (BJX_BAN_RECORDS_ONLY).
        compact_trips: trips as 8-byte words (BatchOutput.trips_compact).
        rule_stats: also count the batch's RuleResults per rule (rule_stats())."""
        res = _lib.BatchResult()
        flags = (_lib.COPY_RESULTS if copy_results else 0) | (_lib.EMIT_BANS if emit_bans else 0) | \
            (_lib.TRIPS_COMPACT if compact_trips else 0) | (_lib.RULE_STATS if rule_stats else 0)
        if emit_bans and not ban_log:
            flags |= _lib.BAN_RECORDS_ONLY
        if device_ptr is not None:
            rc = _lib.lib().bjx_process_batch(self._h, rs.handle, C.c_void_p(device_ptr), nbytes, now_ns,
                                              flags | _lib.INPUT_DEVICE, C.byref(res))
        else:
            buf = _lib.b(data)
            rc = _lib.lib().bjx_process_batch(self._h, rs.handle, C.c_char_p(buf), len(buf), now_ns, flags,
                                              C.byref(res))
        self._check(rc, "process_batch")
        self._batch_rules = len(rs)
        return BatchOutput(res, copy_results)

    # ---- multi-GPU batch (include/banjax_gpu.h); buffers are device pointers
    def match(self, rs: Ruleset, now_ns: int, device_ptr: int, nbytes: int, copy_results: bool = False):
        """consumeLine up to Apply (bjx_match_batch) over a device buffer."""
        res = _lib.BatchResult()
        flags = (_lib.COPY_RESULTS if copy_results else 0) | _lib.INPUT_DEVICE
        self._check(_lib.lib().bjx_match_batch(self._h, rs.handle, C.c_void_p(device_ptr), nbytes, now_ns, flags,
                                               C.byref(res)), "match_batch")
        self._batch_rules = len(rs)
        return res

    def events_partition(self, n_parts: int) -> List[Tuple[int, int, int]]:
        """Per owner: (event lines, events, IP bytes) this engine sends."""
        arr = (C.c_uint64 * (3 * n_parts))()
        self._check(_lib.lib().bjx_events_partition(self._h, n_parts, arr), "events_partition")
        return [(arr[3 * k], arr[3 * k + 1], arr[3 * k + 2]) for k in range(n_parts)]

    def events_pack(self, lines_ptr: int, events_ptr: int, bytes_ptr: int):
        self._check(_lib.lib().bjx_events_pack(self._h, C.c_void_p(lines_ptr), C.c_void_p(events_ptr),
                                               C.c_void_p(bytes_ptr)), "events_pack")

    def apply_events(self, rs: Ruleset, lines_ptr: int, events_ptr: int, bytes_ptr: int,
                     src_counts: List[Tuple[int, int, int]], out_ptr: int):
        arr = (C.c_uint64 * max(1, 3 * len(src_counts)))()
        for k, (a, b, c) in enumerate(src_counts):
            arr[3 * k], arr[3 * k + 1], arr[3 * k + 2] = a, b, c
        self._check(_lib.lib().bjx_apply_events(self._h, rs.handle, C.c_void_p(lines_ptr), C.c_void_p(events_ptr),
                                                C.c_void_p(bytes_ptr), len(src_counts), arr, C.c_void_p(out_ptr)),
                    "apply_events")

    def apply_events_trips(self, rs: Ruleset, lines_ptr: int, events_ptr: int, bytes_ptr: int,
                           src_counts: List[Tuple[int, int, int]], trip_base: List[int], trips_ptr: int) -> List[int]:
        """Trips-only Apply: per source, its tripping events' packed indices
        (trip_base[k] + index in source k's segment) into trips_ptr, source
        order; returns the per-source counts."""
        n = len(src_counts)
        arr = (C.c_uint64 * max(1, 3 * n))()
        for k, (a, b, c) in enumerate(src_counts):
            arr[3 * k], arr[3 * k + 1], arr[3 * k + 2] = a, b, c
        base = (C.c_uint64 * max(1, n))(*trip_base)
        cnt = (C.c_uint64 * max(1, n))()
        self._check(_lib.lib().bjx_apply_events_trips(self._h, rs.handle, C.c_void_p(lines_ptr), C.c_void_p(events_ptr),
                                                      C.c_void_p(bytes_ptr), n, arr, base, C.c_void_p(trips_ptr), cnt),
                    "apply_events_trips")
        return [cnt[k] for k in range(n)]

    def finish_trips(self, trips_ptr: int, n: int, emit_bans: bool = False, rule_stats: bool = False) -> BatchOutput:
        res = _lib.BatchResult()
        flags = (_lib.EMIT_BANS if emit_bans else 0) | (_lib.RULE_STATS if rule_stats else 0)
        self._check(_lib.lib().bjx_finish_batch_trips(self._h, C.c_void_p(trips_ptr), n, flags, C.byref(res)),
                    "finish_batch_trips")
        return BatchOutput(res, False)

    def finish(self, outcomes_ptr: int, copy_results: bool = False, emit_bans: bool = False,
               rule_stats: bool = False) -> BatchOutput:
        res = _lib.BatchResult()
        flags = (_lib.COPY_RESULTS if copy_results else 0) | (_lib.EMIT_BANS if emit_bans else 0) | \
            (_lib.RULE_STATS if rule_stats else 0)
        self._check(_lib.lib().bjx_finish_batch(self._h, C.c_void_p(outcomes_ptr), flags, C.byref(res)),
                    "finish_batch")
        return BatchOutput(res, copy_results)

    PHASES = ("count", "scan", "resolve", "emit", "capacity", "ip_state_claim", "sort_apply", "trips", "exchange")

    def scan_stats(self):
        out = (C.c_uint64 * 13)()
        _lib.lib().bjx_debug_scan_stats(self._h, out, 13)
        return {"pair_filter_hits": out[0], "literal_hits": out[1], "fallback_lines": out[2], "scan_image_bytes": out[3],
                "dfa_jobs": out[4], "ip_table_slots": out[5], "ips": out[6], "state_table_slots": out[7], "states": out[8],
                "gram_table_hits": out[9], "grouping": out[10], "long_runs": out[11], "record_bytes": out[12]}

    def state_stats(self):
        """Occupancy of the HBM rate-limit tables (bjx_state_stats_get)."""
        st = _lib.StateStats()
        self._check(_lib.lib().bjx_state_stats_get(self._h, C.byref(st)), "state_stats")
        return {k: getattr(st, k) for k, _ in _lib.StateStats._fields_}

    def phase_ms(self):
        """Device ms of the last batch's phases; "exchange" (a node batch only)
        is the part of "capacity" spent partitioning, packing, moving and
        unpacking the event records."""
        n = len(self.PHASES)
        out = (C.c_double * n)()
        _lib.lib().bjx_debug_phase_ms(self._h, out, n)
        d = {k: round(out[i], 3) for i, k in enumerate(self.PHASES)}
        if not d["exchange"]:
            del d["exchange"]
        return d

    def kernel_ms(self):
        """Device ms of the last batch's k_scan, per-line kernel and DFA-job resolve (HIP events)."""
        out = (C.c_double * 5)()
        _lib.lib().bjx_debug_kernel_ms(self._h, out, 5)
        return {"k_scan": out[0], "k_lines": out[1], "dfa_jobs": out[2]}

    def line_kernel(self):
        """The last batch's per-line kernel: ("k_lines2", window bytes per line), ("k_lines", staging bytes per
        wave), or ("k_parse_match", 0) when every scope is past 128 rules and the per-line fallback took every line."""
        out = (C.c_double * 5)()
        _lib.lib().bjx_debug_kernel_ms(self._h, out, 5)
        names = {1: "k_lines", 2: "k_lines2", 3: "k_parse_match"}
        return names.get(int(out[3])), int(out[4])

    def state_get(self, ip, name):
        hits, start = C.c_int64(), C.c_int64()
        ipb, nb = _lib.b(ip), _lib.b(name)
        rc = self._check(_lib.lib().bjx_state_get(self._h, ipb, len(ipb), nb, len(nb), C.byref(hits), C.byref(start)),
                         "state_get")
        return (hits.value, start.value) if rc == 1 else None

    def state_len(self) -> int:
        return self._check(_lib.lib().bjx_state_len(self._h), "state_len")

    def debug_set_ip_hash_mask(self, mask: int):
        """Test hook: IP hashes become (hash & mask) | 1 (0 = off)."""
        self._check(_lib.lib().bjx_debug_set_ip_hash_mask(self._h, mask), "debug_set_ip_hash_mask")

    def debug_set_claim_budget(self, max_new: int):
        """Test hook: cap the first claim launch per table and batch (0 = off)."""
        self._check(_lib.lib().bjx_debug_set_claim_budget(self._h, max_new), "debug_set_claim_budget")

    def debug_set_slot_cache(self, on: int):
        """Test hook: state-slot cache on (1), off (0), default (-1), from the next batch."""
        self._check(_lib.lib().bjx_debug_set_slot_cache(self._h, on), "debug_set_slot_cache")

    def debug_set_bucket_bits(self, bits: int):
        """Test hook: the two-level rate-limit grouping uses `bits` high slot
        bits (1..16; 0 = the default 16), from the next batch."""
        self._check(_lib.lib().bjx_debug_set_bucket_bits(self._h, bits), "debug_set_bucket_bits")

    def debug_set_rec8_max_events(self, max_events: int):
        """Test hook: the 8-byte event records only for batches of at most
        max_events events (0 = the default 2^28), from the next batch."""
        self._check(_lib.lib().bjx_debug_set_rec8_max_events(self._h, max_events), "debug_set_rec8_max_events")

    def debug_state_slots(self, ips, names):
        """Test hook: the state-table slot of each (ips[k], names[k]) state, -1
        where there is none, as a numpy int64 array; one launch for the whole
        list (bjx_debug_state_slots).  The engine is unchanged."""
        import numpy as np
        ipb = [_lib.b(x) for x in ips]
        nmb = [_lib.b(x) for x in names]
        assert len(ipb) == len(nmb)
        n = len(ipb)
        out = np.full(n, -1, dtype=np.int64)
        if not n:
            return out
        off = np.zeros(n + 1, dtype=np.uint32)
        total = np.cumsum(np.fromiter((len(x) for x in ipb), dtype=np.uint64, count=n))
        assert int(total[-1]) < 1 << 32
        off[1:] = total
        blob = np.frombuffer(b"".join(ipb) + b"\0", dtype=np.uint8)
        table = sorted(set(nmb))
        where = {x: k for k, x in enumerate(table)}
        idx = np.fromiter((where[x] for x in nmb), dtype=np.uint32, count=n)
        arr = (_lib.Str * len(table))(*[_lib.Str(x, len(x)) for x in table])
        self._check(_lib.lib().bjx_debug_state_slots(self._h, blob.ctypes.data, off.ctypes.data, arr, len(table),
                                                     idx.ctypes.data, n, out.ctypes.data), "debug_state_slots")
        return out

    def debug_job_counts(self):
        """Test hook: the last batch's sorted DFA jobs per rule of its ruleset,
        (windowed, legacy, line_pass_runs): the counts under the job keys r and
        n_rules + r, and how often the per-line pass ran (2 when the job buffers
        grew).  Computed on demand (bjx_debug_job_counts)."""
        n = getattr(self, "_batch_rules", 0)
        w, l = (C.c_uint32 * max(1, n))(), (C.c_uint32 * max(1, n))()
        runs = C.c_uint32()
        self._check(_lib.lib().bjx_debug_job_counts(self._h, w, l, n, C.byref(runs)), "debug_job_counts")
        return list(w[:n]), list(l[:n]), runs.value

    def state_clear(self):
        self._check(_lib.lib().bjx_state_clear(self._h), "state_clear")

    def state_expire(self, cutoff_ns: int) -> dict:
        """Drop every state whose window started before cutoff_ns and every IP
        left without one; the tables are rebuilt and shrink (bjx_state_expire).
        Returns the bjx_expire_stats fields."""
        st = _lib.ExpireStats()
        self._check(_lib.lib().bjx_state_expire(self._h, cutoff_ns, C.byref(st)), "state_expire")
        return {k: getattr(st, k) for k, _ in _lib.ExpireStats._fields_}

    def state_dump(self) -> str:
        n = _lib.lib().bjx_state_dump(self._h, None, 0)
        buf = C.create_string_buffer(n + 1)
        _lib.lib().bjx_state_dump(self._h, buf, n)
        return buf.raw[:n].decode(errors="replace")

    _snap = "bjx_state"

    def state_export_bound(self) -> int:
        """An upper bound on the size of state_export()'s blob (no pass over the tables)."""
        return getattr(_lib.lib(), self._snap + "_export_bound")(self._h)

    def state_export(self, min_start_ns: int = INT64_MIN, cap: Optional[int] = None) -> bytes:
        """The rate-limit state as one snapshot blob (banjax_amd/snapshot.py has
        the format): every state whose window started at or after min_start_ns.
        The engine is unchanged.  cap: the buffer size to offer (default: the
        library's bound); too small raises BJX_ERR_CAPACITY with the size
        needed in the error's `needed`.  The call's bjx_snapshot_stats are left
        in self.snapshot_stats."""
        L = _lib.lib()
        if cap is None:
            cap = self.state_export_bound()
        buf = (C.c_uint8 * max(cap, 1))()
        n, st = C.c_uint64(0), _lib.SnapshotStats()
        rc = getattr(L, self._snap + "_export")(self._h, min_start_ns, C.cast(buf, C.c_void_p), cap, C.byref(n), C.byref(st))
        try:
            self._check(rc, "state_export")
        except _lib.BanjaxGpuError as x:
            x.needed = n.value
            raise
        self.snapshot_stats = {k: getattr(st, k) for k, _ in _lib.SnapshotStats._fields_}
        return bytes(memoryview(buf)[:n.value])

    def state_import(self, blob: bytes, part: int = 0, n_parts: int = 1) -> dict:
        """Restore a snapshot into this (empty) engine; with n_parts > 1 only the
        IPs part `part` owns.  Returns the bjx_snapshot_stats fields."""
        st = _lib.SnapshotStats()
        blob = bytes(blob)
        self._check(_lib.lib().bjx_state_import(self._h, blob, len(blob), part, n_parts, C.byref(st)), "state_import")
        return {k: getattr(st, k) for k, _ in _lib.SnapshotStats._fields_}

    _merge = "bjx_state_merge"

    def state_merge(self, blob: bytes, policy=_lib.MERGE_NEWER, min_start_ns: int = INT64_MIN, part: int = 0,
                    n_parts: int = 1, dry_run: bool = False) -> dict:
        """Fold a snapshot into this engine, which may hold state
        (bjx_state_merge; banjax_amd/state_merge.py is its model).  policy:
        _lib.MERGE_NEWER (the larger (start, hits) wins a key both sides hold),
        _KEEP (the engine's record stays) or _REPLACE (the snapshot's wins), or
        "newer" / "keep" / "replace".  Snapshot records that started before
        min_start_ns, and with n_parts > 1 the IPs `part` does not own, are
        skipped.  The engine's IPs keep their order; new ones follow in
        snapshot order.  Nothing to add or replace: the engine is left exactly
        as it was.  dry_run: the counts as the real call would report them,
        nothing changed.  Returns the bjx_merge_stats fields."""
        policy = {"newer": _lib.MERGE_NEWER, "keep": _lib.MERGE_KEEP, "replace": _lib.MERGE_REPLACE}.get(policy, policy)
        o = _lib.MergeOptions(min_start_ns, part, n_parts, policy, _lib.MERGE_DRY_RUN if dry_run else 0)
        st = _lib.MergeStats()
        blob = bytes(blob)
        self._check(getattr(_lib.lib(), self._merge)(self._h, blob, len(blob), C.byref(o), C.byref(st)), "state_merge")
        return {k: getattr(st, k) for k, _ in _lib.MergeStats._fields_}

    _query = "bjx_state_query"

    def state_query(self, ip=None, name=None, min_hits: int = INT64_MIN, min_start_ns: int = INT64_MIN,
                    max_start_ns: int = INT64_MAX, order: int = _lib.QUERY_BY_HITS, limit: int = 100, nets=None) -> dict:
        """Counts and the first `limit` states that pass the filter
        (bjx_state_query; banjax_amd/state_query.py documents the order and is
        its model).  ip / name None: every IP / rule name; b"" is a value.
        order: _lib.QUERY_BY_HITS or _lib.QUERY_BY_START (or "hits" / "start").
        limit 0: the counts only.  Returns {"n_matched", "n_ips_matched",
        "rows": [(ip, name, hits, start_ns)] (bytes, bytes, int, int),
        "device_ms"}.  The engine is unchanged.
        nets (an iterable of "IP" / "IP/len" entries, str or bytes; not None):
        only states whose IP lies in one of these networks
        (bjx_state_query_nets; banjax_amd/state_nets.py is the model of the
        entries and of membership).  The answer gains "net_ips": per entry, in
        the order given, the distinct IPs inside it with a selected state."""
        order = {"hits": _lib.QUERY_BY_HITS, "start": _lib.QUERY_BY_START}.get(order, order)
        ipb = None if ip is None else _lib.b(ip)
        nb = None if name is None else _lib.b(name)
        f = _lib.StateFilter(_lib.Str(ipb, len(ipb or b"")), _lib.Str(nb, len(nb or b"")), min_hits, min_start_ns,
                             max_start_ns, order, limit)
        out = _lib.StateRows()
        if nets is None:
            self._check(getattr(_lib.lib(), self._query)(self._h, C.byref(f), C.byref(out)), "state_query")
        else:
            lst = [_lib.b(x) for x in nets]
            arr = (_lib.Str * max(len(lst), 1))(*[_lib.Str(x, len(x)) for x in lst])
            counts = C.POINTER(C.c_uint64)()
            self._check(getattr(_lib.lib(), self._query + "_nets")(self._h, C.byref(f), arr, len(lst), C.byref(out),
                                                                   C.byref(counts)), "state_query")
        blob = C.string_at(out.bytes, out.n_bytes) if out.n_bytes else b""
        rows = []
        for k in range(out.n_rows):
            r = out.rows[k]
            rows.append((blob[r.ip_off:r.ip_off + r.ip_len], blob[r.name_off:r.name_off + r.name_len], r.hits, r.start_ns))
        ans = {"n_matched": out.n_matched, "n_ips_matched": out.n_ips_matched, "rows": rows, "device_ms": out.device_ms}
        if nets is not None:
            ans["net_ips"] = [counts[k] for k in range(len(lst))]
        return ans

    _remove = "bjx_state_remove"

    def state_remove(self, ips=None, ip=None, name=None, min_hits: int = INT64_MIN, min_start_ns: int = INT64_MIN,
                     max_start_ns: int = INT64_MAX, nets=None) -> dict:
        """Forget every state that passes the filter (state_query's ip, name,
        min_hits, min_start_ns, max_start_ns) and, with `ips` (an iterable of
        str / bytes; None or empty: no list, as n_ips == 0 in C), whose IP is listed; every IP left without
        a state goes too (bjx_state_remove; banjax_amd/state_remove.py is its
        model).  Nothing selected: the engine is left exactly as it was.
        nets (an iterable of "IP" / "IP/len" entries; not None, and then
        without `ips`): the states whose IP lies in one of these networks
        (bjx_state_remove_nets); an empty or malformed nets is an error, never
        "every IP".  Returns the bjx_remove_stats fields."""
        if nets is not None and ips is not None:
            raise ValueError("state_remove: ips and nets together")
        ipb = None if ip is None else _lib.b(ip)
        nb = None if name is None else _lib.b(name)
        f = _lib.StateFilter(_lib.Str(ipb, len(ipb or b"")), _lib.Str(nb, len(nb or b"")), min_hits, min_start_ns,
                             max_start_ns, _lib.QUERY_BY_HITS, 0)
        lst = [_lib.b(x) for x in (nets if nets is not None else ips or [])]
        arr = (_lib.Str * max(len(lst), 1))(*[_lib.Str(x, len(x)) for x in lst])
        st = _lib.RemoveStats()
        if nets is not None:
            self._check(getattr(_lib.lib(), self._remove + "_nets")(self._h, C.byref(f), arr, len(lst), C.byref(st)),
                        "state_remove")
            return {k: getattr(st, k) for k, _ in _lib.RemoveStats._fields_}
        self._check(getattr(_lib.lib(), self._remove)(self._h, C.byref(f), arr if lst else None, len(lst), C.byref(st)),
                    "state_remove")
        return {k: getattr(st, k) for k, _ in _lib.RemoveStats._fields_}

    _trim = "bjx_state_trim"

    def state_trim(self, max_states: int = 0, max_ips: int = 0, floor_cutoff_ns: int = INT64_MIN,
                   dry_run: bool = False) -> dict:
        """Evict the oldest states until at most max_states states and max_ips
        IPs are left (0: no bound); states that started before floor_cutoff_ns
        always go (bjx_state_trim; banjax_amd/state_trim.py is its model).  The
        cutoff is found on the device and the expiry at that cutoff follows;
        nothing to drop leaves the engine exactly as it was.  dry_run: the
        cutoff and the counts as the real call would report them, nothing
        changed.  Returns the bjx_trim_stats fields."""
        bud = _lib.TrimBudget(max_states, max_ips, floor_cutoff_ns, _lib.TRIM_DRY_RUN if dry_run else 0, 0)
        st = _lib.TrimStats()
        self._check(getattr(_lib.lib(), self._trim)(self._h, C.byref(bud), C.byref(st)), "state_trim")
        return {k: getattr(st, k) for k, _ in _lib.TrimStats._fields_}

    _groups = "bjx_state_query_groups"

    def state_query_groups(self, v4_bits: int = 24, v6_bits: int = 64, order=_lib.GROUPS_BY_IPS, limit: int = 100,
                           min_ips: int = 0, ip=None, name=None, min_hits: int = INT64_MIN,
                           min_start_ns: int = INT64_MIN, max_start_ns: int = INT64_MAX) -> dict:
        """The networks that hold the most counting IPs: the held IPs with a
        state that passes the filter (state_query's ip, name, min_hits,
        min_start_ns, max_start_ns), grouped by their address masked to
        v4_bits / v6_bits (bjx_state_query_groups; banjax_amd/state_groups.py
        documents the grouping and the order and is its model).  order:
        _lib.GROUPS_BY_IPS, _BY_STATES or _BY_HITS (or "ips" / "states" /
        "hits"); rows only for groups of at least min_ips IPs; limit 0: the
        counts only.  Returns {"n_matched", "n_ips_matched", "n_ips_unparsed",
        "n_states_unparsed", "n_groups", "n_groups_min", "rows":
        [state_groups.GroupRow], "device_ms"}.  A row's .net ("170.85.195.0/24",
        "2001:db8:85a3:c55a::/64") is an entry state_query(nets=[...]) and
        state_remove(nets=[...]) take as it is.  The engine is unchanged."""
        from .state_groups import GroupRow, net_text
        order = {"ips": _lib.GROUPS_BY_IPS, "states": _lib.GROUPS_BY_STATES, "hits": _lib.GROUPS_BY_HITS}.get(order, order)
        ipb = None if ip is None else _lib.b(ip)
        nb = None if name is None else _lib.b(name)
        f = _lib.StateFilter(_lib.Str(ipb, len(ipb or b"")), _lib.Str(nb, len(nb or b"")), min_hits, min_start_ns,
                             max_start_ns, _lib.QUERY_BY_HITS, 0)
        g = _lib.GroupSpec(v4_bits, v6_bits, order, limit, min_ips)
        out = _lib.StateGroups()
        self._check(getattr(_lib.lib(), self._groups)(self._h, C.byref(f), C.byref(g), C.byref(out)), "state_query_groups")
        rows = []
        for k in range(out.n_rows):
            r = out.rows[k]
            addr = bytes(r.addr)
            rows.append(GroupRow(net_text(r.family, r.bits, addr), r.family, r.bits, addr, r.n_ips, r.n_states, r.hits_sum,
                                 r.newest_start_ns))
        ans = {k: getattr(out, k) for k in ("n_matched", "n_ips_matched", "n_ips_unparsed", "n_states_unparsed", "n_groups",
                                            "n_groups_min", "device_ms")}
        ans["rows"] = rows
        return ans

    _names = "bjx_state_query_names"

    def state_query_names(self, order=_lib.NAMES_BY_STATES, limit: int = 100, min_states: int = 0, ip=None, name=None,
                          min_hits: int = INT64_MIN, min_start_ns: int = INT64_MIN, max_start_ns: int = INT64_MAX) -> dict:
        """Which rule names hold the state: the states that pass the filter
        (state_query's ip, name, min_hits, min_start_ns, max_start_ns) totalled
        per rule name (bjx_state_query_names; banjax_amd/state_names.py
        documents the totals, the histogram buckets and the order and is its
        model).  order: _lib.NAMES_BY_STATES, _BY_HITS, _BY_MAX_HITS,
        _BY_NEWEST or _BY_NAME (or "states" / "hits" / "max_hits" / "newest" /
        "name"); rows only for names of at least min_states states; limit 0:
        the counts only.  Returns {"n_matched", "n_ips_matched", "n_names",
        "n_names_min", "rows": [state_names.NameRow], "device_ms"}; a row's
        .name is bytes, what state_remove(name=...) takes.  After a reload,
        state_names.orphans(rows, current rule names) are the rows to remove.
        The engine is unchanged."""
        from .state_names import ORDERS, NameRow
        order = ORDERS.get(order, order)
        ipb = None if ip is None else _lib.b(ip)
        nb = None if name is None else _lib.b(name)
        f = _lib.StateFilter(_lib.Str(ipb, len(ipb or b"")), _lib.Str(nb, len(nb or b"")), min_hits, min_start_ns,
                             max_start_ns, _lib.QUERY_BY_HITS, 0)
        s = _lib.NamesSpec(order, limit, min_states)
        out = _lib.StateNames()
        self._check(getattr(_lib.lib(), self._names)(self._h, C.byref(f), C.byref(s), C.byref(out)), "state_query_names")
        blob = C.string_at(out.bytes, out.n_bytes) if out.n_bytes else b""
        rows = []
        for k in range(out.n_rows):
            r = out.rows[k]
            rows.append(NameRow(blob[r.name_off:r.name_off + r.name_len], r.n_states, r.hits_sum, r.max_hits,
                                r.newest_start_ns, r.oldest_start_ns, tuple(r.hist)))
        ans = {k: getattr(out, k) for k in ("n_matched", "n_ips_matched", "n_names", "n_names_min", "device_ms")}
        ans["rows"] = rows
        return ans

    def debug_set_names(self, max_lds_names: int = 0, max_blocks: int = 0):
        """Test hook: state_query_names bins in LDS only up to max_lds_names interned names and
        scans with at most max_blocks blocks (0 = default)."""
        self._check(_lib.lib().bjx_debug_set_names(self._h, max_lds_names, max_blocks), "debug_set_names")

    def debug_names_info(self):
        """-> (where the last state_query_names binned: "none" / "lds" / "global", the most interned names the LDS path takes)"""
        path, top = C.c_int(0), C.c_uint32(0)
        self._check(_lib.lib().bjx_debug_names_info(self._h, C.byref(path), C.byref(top)), "debug_names_info")
        return {0: "none", 1: "lds", 2: "global"}[path.value], top.value

    def debug_set_trim_grid(self, max_blocks: int):
        """Test hook: the block cap of state_trim's counting passes (0 = default)."""
        self._check(_lib.lib().bjx_debug_set_trim_grid(self._h, max_blocks), "debug_set_trim_grid")

    _rule_stats = "bjx_"

    def rule_stats(self, total: bool = False) -> dict:
        """Per-rule counts of the last batch (run with rule_stats=True), or with
        total=True of every such batch since its ruleset came into use
        (bjx_batch_rule_stats / bjx_rule_stats_total; banjax_amd/rule_stats.py
        is the model).  Returns {"n_batches", "n_lines", "device_ms", "rules"}:
        rules is a numpy structured array (matches, skip_host, trips) indexed
        by ruleset rule index, copied out of the library's memory once."""
        import numpy as np
        out = _lib.RuleStats()
        name = self._rule_stats + ("rule_stats_total" if total else "batch_rule_stats")
        self._check(getattr(_lib.lib(), name)(self._h, C.byref(out)), name)
        if out.n_rules:
            view = (_lib.RuleStat * out.n_rules).from_address(C.addressof(out.rules.contents))
            rules = np.ctypeslib.as_array(view).copy()
        else:
            rules = np.zeros(0, dtype=np.dtype(_lib.RuleStat))
        return {"n_batches": out.n_batches, "n_lines": out.n_lines, "device_ms": out.device_ms, "rules": rules}

    def rule_stats_reset(self):
        """Forget the totals (rule_stats(total=True) is empty until the next flagged batch)."""
        name = self._rule_stats + "rule_stats_reset"
        self._check(getattr(_lib.lib(), name)(self._h), name)

    def debug_set_rule_stats_lds(self, max_rules: int):
        """Test hook: LDS bins only for rulesets of at most max_rules rules (0 = default)."""
        self._check(_lib.lib().bjx_debug_set_rule_stats_lds(self._h, max_rules), "debug_set_rule_stats_lds")

    def debug_rule_stats_path(self) -> str:
        """Where the last rule_stats=True batch binned: "lds", "global", or "none" (no results, nothing launched)."""
        return {0: "none", 1: "lds", 2: "global"}[self._check(_lib.lib().bjx_debug_rule_stats_path(self._h),
                                                              "debug_rule_stats_path")]

    def close(self):
        h = getattr(self, "_h", None)
        if h and _lib._lib is not None:
            _lib._lib.bjx_engine_destroy(h)
        self._h = None

    def __del__(self):
        self.close()


class _NodeEngine(Engine):
    """A node's engine: closing it is the node's business."""

    def close(self):
        self._h = None


class Node:
    """The GPUs of one host behind one handle (bjx_node_*): one
    engine per entry of `devices` (repeats allowed), matching sharded by chunk,
    RegexRateLimitStates sharded by IP, the exchange done inside the library.
    Results are in global (reference) order, as one Engine returns them."""

    def __init__(self, devices: Sequence[int], ip_capacity: int = 0, state_capacity: int = 0, ip_arena_bytes: int = 0):
        L = _lib.lib()
        h = C.c_void_p()
        err = C.create_string_buffer(512)
        devs = (C.c_int * len(devices))(*devices)
        opts = _lib.EngineOptions(ip_capacity, state_capacity, ip_arena_bytes)
        rc = L.bjx_node_create(devs, len(devices), C.byref(opts), C.byref(h), err, 512)
        if rc != _lib.OK:
            raise _lib.BanjaxGpuError(rc, "bjx_node_create: " + err.value.decode(errors="replace"))
        self._h = h
        self.devices = list(devices)

    def __len__(self):
        return len(self.devices)

    @property
    def exchange(self) -> str:
        """How the library moves the event records: "rccl" or "copies"."""
        return "rccl" if _lib.lib().bjx_node_exchange_kind(self._h) == 1 else "copies"

    def engine(self, k: int) -> "Engine":
        """Engine k (stats and debug hooks); owned by the node."""
        h = _lib.lib().bjx_node_engine(self._h, k)
        if not h:
            raise IndexError(k)
        e = Engine.__new__(_NodeEngine)
        e._h, e.device, e._node = C.c_void_p(h), self.devices[k], self
        return e

    def _check(self, rc, what):
        if rc < 0:
            msg = _lib.lib().bjx_node_last_error(self._h)
            raise _lib.BanjaxGpuError(rc, "%s: %s" % (what, (msg or b"").decode(errors="replace")))
        return rc

    def set_decision_lists(self, entries: Iterable[Tuple[Optional[str], int, str]]):
        arr, n, keep = _decision_entries(entries)
        self._check(_lib.lib().bjx_node_set_decision_lists(self._h, arr, n), "node_set_decision_lists")

    def set_ban_options(self, expiring_ttl_s: int, disable_logging: Iterable[str] = (), tz_offset_s: int = 0,
                        zone=None):
        o, keep = _ban_options(expiring_ttl_s, disable_logging, tz_offset_s, zone)
        self._check(_lib.lib().bjx_node_set_ban_options(self._h, C.byref(o)), "node_set_ban_options")

    def process(self, rs: Ruleset, data, now_ns: int, copy_results: bool = False, emit_bans: bool = False,
                rule_stats: bool = False) -> BatchOutput:
        """consumeLine over the complete lines of a host buffer, split over the engines."""
        res = _lib.BatchResult()
        flags = (_lib.COPY_RESULTS if copy_results else 0) | (_lib.EMIT_BANS if emit_bans else 0) | \
            (_lib.RULE_STATS if rule_stats else 0)
        buf = _lib.b(data)
        self._check(_lib.lib().bjx_node_process_batch(self._h, rs.handle, C.c_char_p(buf), len(buf), now_ns, flags,
                                                      C.byref(res)), "node_process_batch")
        return BatchOutput(res, copy_results)

    def process_chunks(self, rs: Ruleset, chunks: Sequence[Tuple[int, int]], now_ns: int, copy_results: bool = False,
                       emit_bans: bool = False, compact_trips: bool = False, rule_stats: bool = False) -> BatchOutput:
        """chunks[k] = (device pointer on engine k's GPU, bytes); all but the last end in '\\n'."""
        res = _lib.BatchResult()
        flags = (_lib.COPY_RESULTS if copy_results else 0) | (_lib.EMIT_BANS if emit_bans else 0) | _lib.INPUT_DEVICE | \
            (_lib.TRIPS_COMPACT if compact_trips else 0) | (_lib.RULE_STATS if rule_stats else 0)
        ptrs = (C.c_void_p * len(chunks))(*[p for p, _ in chunks])
        lens = (C.c_size_t * len(chunks))(*[n for _, n in chunks])
        self._check(_lib.lib().bjx_node_process_chunks(self._h, rs.handle, ptrs, lens, now_ns, flags, C.byref(res)),
                    "node_process_chunks")
        return BatchOutput(res, copy_results)

    def bans(self) -> BanBatch:
        bb = _lib.BanBatch()
        self._check(_lib.lib().bjx_node_batch_bans(self._h, C.byref(bb)), "node_batch_bans")
        return BanBatch(bb)

    def state_get(self, ip, name):
        hits, start = C.c_int64(), C.c_int64()
        ipb, nb = _lib.b(ip), _lib.b(name)
        rc = self._check(_lib.lib().bjx_node_state_get(self._h, ipb, len(ipb), nb, len(nb), C.byref(hits),
                                                       C.byref(start)), "node_state_get")
        return (hits.value, start.value) if rc == 1 else None

    def state_len(self) -> int:
        return self._check(_lib.lib().bjx_node_state_len(self._h), "node_state_len")

    def state_stats(self):
        st = _lib.StateStats()
        self._check(_lib.lib().bjx_node_state_stats_get(self._h, C.byref(st)), "node_state_stats")
        return {k: getattr(st, k) for k, _ in _lib.StateStats._fields_}

    def state_clear(self):
        self._check(_lib.lib().bjx_node_state_clear(self._h), "node_state_clear")

    def state_expire(self, cutoff_ns: int) -> dict:
        """Engine.state_expire on every shard: stats summed, device_ms the slowest shard's."""
        st = _lib.ExpireStats()
        self._check(_lib.lib().bjx_node_state_expire(self._h, cutoff_ns, C.byref(st)), "node_state_expire")
        return {k: getattr(st, k) for k, _ in _lib.ExpireStats._fields_}

    def state_dump(self) -> str:
        n = _lib.lib().bjx_node_state_dump(self._h, None, 0)
        buf = C.create_string_buffer(n + 1)
        _lib.lib().bjx_node_state_dump(self._h, buf, n)
        return buf.raw[:n].decode(errors="replace")

    _snap = "bjx_node_state"
    state_export_bound = Engine.state_export_bound
    state_export = Engine.state_export  # the shards merged into one snapshot, IPs engine-major

    _merge = "bjx_node_state_merge"
    state_merge = Engine.state_merge  # engine k merges the IPs it owns (part, n_parts stay 0, 1); stats summed

    _query = "bjx_node_state_query"
    state_query = Engine.state_query  # every shard's answer merged, IPs engine-major; an ip filter asks its owner only

    _remove = "bjx_node_state_remove"
    state_remove = Engine.state_remove  # every shard gets the filter and the whole list; stats summed

    _trim = "bjx_node_state_trim"
    state_trim = Engine.state_trim  # the budget per engine, one cutoff for the node (the engines' largest); stats summed

    _groups = "bjx_node_state_query_groups"
    state_query_groups = Engine.state_query_groups  # the shards' complete group lists merged by key, then min_ips, order, limit

    _names = "bjx_node_state_query_names"
    state_query_names = Engine.state_query_names  # the shards' complete name lists merged by name bytes, then min_states, order, limit

    _rule_stats = "bjx_node_"
    rule_stats = Engine.rule_stats  # the engines' arrays summed; engine(k).rule_stats() has engine k's own
    rule_stats_reset = Engine.rule_stats_reset  # the node's totals; each engine keeps its own

    def state_import(self, blob: bytes) -> dict:
        """Restore a snapshot taken on any number of engines: engine k takes the IPs it owns."""
        st = _lib.SnapshotStats()
        blob = bytes(blob)
        self._check(_lib.lib().bjx_node_state_import(self._h, blob, len(blob), C.byref(st)), "node_state_import")
        return {k: getattr(st, k) for k, _ in _lib.SnapshotStats._fields_}

    def close(self):
        h = getattr(self, "_h", None)
        if h and _lib._lib is not None:
            _lib._lib.bjx_node_destroy(h)
        self._h = None

    def __del__(self):
        self.close()
