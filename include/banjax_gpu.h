/*
 * banjax_gpu.h — C ABI of libbanjax_gpu.so, the MI355X engine behind banjax's
 * regex rate-limiting log tailer.
 *
 * Drop-in boundary: a Go host keeps banjax's surface (YAML schema,
 * consumeLine/RunLogTailer, RegexRateLimitStates, BannerInterface, decision
 * lists) and calls these entry points through cgo (binding: INTEGRATION.md).
 * Plain pointers and sizes only; no GPU or torch types cross the boundary.
 *
 * Reference interfaces replaced (deflect-ca/banjax):
 *   bjx_ruleset_compile     RegexWithRate.UnmarshalYAML        internal/config.go:96-131
 *                           (regexp.Compile per rule, config.go:110; reload: config_holder.go:55-66)
 *   bjx_engine_set_decision_lists  newStaticDecisionListsFromConfig  internal/decision.go:278-374
 *   bjx_process_batch       consumeLine + applyRegexToLog per line
 *                           internal/regex_rate_limiter.go:113-269, fed by RunLogTailer :21-78
 *   bjx_state_get           RegexRateLimitStates.Get           internal/rate_limit.go:81-96
 *   bjx_state_len           RegexRateLimitStates.Len           internal/rate_limit.go:30-35
 *   bjx_state_dump          RegexRateLimitStates.String        internal/rate_limit.go:98-103,204-220
 *   bjx_node_*              the same surface over every GPU of the host (one RegexRateLimitStates,
 *                           banjax.go:80; one consumer goroutine, regex_rate_limiter.go:54-77)
 *   bjx_tailer_*            tail.TailFile(Follow, SeekEnd) + tailer.Lines in RunLogTailer
 *                           internal/regex_rate_limiter.go:21-78 (github.com/hpcloud/tail v1.0.0)
 *
 * Ownership: input buffers are borrowed for the duration of a call.  Result
 * arrays are engine-owned and valid until the next bjx_process_batch on the
 * same engine.  Rulesets are immutable; a reload compiles a new one (state is
 * keyed by rule *name* and survives, as in the reference).
 * Threading: one bjx_process_batch at a time per engine; bjx_state_* may be
 * called from other threads (they serialise on the engine lock, as the
 * reference's mutex does, rate_limit.go:19).
 * Errors: int status (BJX_OK = 0, negative code) + a caller buffer for the
 * message.  Malformed log lines are data (BJX_LINE_ERROR), never API errors.
 */
#ifndef BANJAX_GPU_H
#define BANJAX_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define BJX_ABI_VERSION 5  /* 5: IP slots of the exchange byte pool 4-byte aligned; trips-only node return */

enum bjx_status {
  BJX_OK = 0,
  BJX_ERR_REGEX = -1,       /* a rule's regex does not compile (Go error text in err) */
  BJX_ERR_ARG = -2,
  BJX_ERR_DEVICE = -3,      /* HIP runtime failure / no GPU */
  BJX_ERR_NOMEM = -4,
  BJX_ERR_TOO_COMPLEX = -5, /* rule exceeds the engine's automaton limits */
  BJX_ERR_CAPACITY = -6,    /* state tables full (raise bjx_engine_options) */
  BJX_ERR_DECISION = -7,    /* unknown decision string / value */
  BJX_TAIL_STOPPED = -8,    /* bjx_tailer_next: the followed file was deleted or renamed (tail stops) */
  BJX_ERR_IO = -9           /* bjx_tailer: read/open failure other than "not there yet" */
};

/* Decision, reference internal/decision.go:20-28 */
enum bjx_decision { BJX_ALLOW = 1, BJX_CHALLENGE = 2, BJX_NGINX_BLOCK = 3, BJX_IPTABLES_BLOCK = 4 };
/* RateLimitMatchType, reference internal/rate_limit.go:175-181 */
enum bjx_match_type { BJX_FIRST_TIME = 0, BJX_OUTSIDE_INTERVAL = 1, BJX_INSIDE_INTERVAL = 2 };
/* ConsumeLineResult.{Error,OldLine,Exempted}, reference regex_rate_limiter.go:80-85 */
enum bjx_line_flag { BJX_LINE_ERROR = 1, BJX_LINE_OLD = 2, BJX_LINE_EXEMPTED = 4 };

typedef struct bjx_str {
  const char *ptr;
  size_t len;
} bjx_str;

/* One RegexWithRate (config.go:87-94), already decoded from YAML by the host. */
typedef struct bjx_rule_spec {
  bjx_str name;               /* Rule */
  bjx_str regex;              /* RE2 / Go regexp syntax */
  int64_t interval_ns;        /* time.Duration(interval * 1e9), computed by the host (config.go:116) */
  int64_t hits_per_interval;  /* HitsPerInterval (Go int) */
  int32_t decision;           /* enum bjx_decision (ParseDecision, decision.go:30-43) */
  const bjx_str *hosts_to_skip; /* HostsToSkip keys whose value is true */
  size_t n_hosts_to_skip;
} bjx_rule_spec;

/* per_site_regexes_with_rates[host] (config.go:19) */
typedef struct bjx_site_rules {
  bjx_str host;
  const bjx_rule_spec *rules;
  size_t n_rules;
} bjx_site_rules;

typedef struct bjx_ruleset bjx_ruleset;
typedef struct bjx_engine bjx_engine;

/* Compile every rule (regexp.Compile semantics, syntax.Perl flags).  Rule
   indices: global rules 0..n_global-1, then each site's rules in order.  On a
   compile error returns BJX_ERR_REGEX, *err_rule = failing index and the Go
   error text ("error parsing regexp: ...") in err, and no ruleset. */
int bjx_ruleset_compile(const bjx_rule_spec *global_rules, size_t n_global, const bjx_site_rules *per_site,
                        size_t n_sites, bjx_ruleset **out, int64_t *err_rule, char *err, size_t err_len);
void bjx_ruleset_release(bjx_ruleset *rs);
size_t bjx_ruleset_num_rules(const bjx_ruleset *rs);
/* Per-rule automaton statistics (DFA states, rune classes) for diagnostics. */
int bjx_ruleset_rule_info(const bjx_ruleset *rs, size_t rule_idx, uint32_t *dfa_states, uint32_t *classes,
                          uint32_t *flags);

typedef struct bjx_engine_options {
  uint64_t ip_capacity;       /* distinct IPs kept (the reference never evicts, rate_limit.go:45-67; here eviction is
                                 explicit and opt-in, bjx_state_expire, which also shrinks back to this); 0 = default */
  uint64_t state_capacity;    /* distinct (ip, rule name) states; 0 = default */
  uint64_t ip_arena_bytes;    /* bytes of IP strings; 0 = default */
} bjx_engine_options;

/* One engine per GPU (device index as HIP sees it).  opts may be NULL. */
int bjx_engine_create(int device, const bjx_engine_options *opts, bjx_engine **out, char *err, size_t err_len);
void bjx_engine_destroy(bjx_engine *e);

/* Static decision lists used by CheckIsAllowed (decision.go:185-216): one
   entry per IP/CIDR string of global_decision_lists (site.ptr == NULL) or
   per_site_decision_lists[site], in config order.  Replaces previous lists
   (StaticDecisionLists.UpdateFromConfig on reload, banjax.go:113). */
typedef struct bjx_decision_entry {
  bjx_str site;     /* ptr == NULL: global */
  int32_t decision; /* enum bjx_decision */
  bjx_str ip;       /* IP or CIDR text */
} bjx_decision_entry;
int bjx_engine_set_decision_lists(bjx_engine *e, const bjx_decision_entry *entries, size_t n);

/* RuleResult of one matched (line, rule) pair, reference regex_rate_limiter.go:87-93.
   RegexMatch is implied (only matches are reported, as consumeLine does, :189,208). */
typedef struct bjx_rule_result {
  uint64_t line_idx;
  uint32_t rule_idx;  /* ruleset rule index */
  uint16_t rule_pos;  /* position in the line's evaluation order (per-site rules, then global) */
  uint8_t skip_host;
  uint8_t seen_ip;
  uint8_t match_type; /* enum bjx_match_type */
  uint8_t exceeded;
  uint8_t _pad[2];
} bjx_rule_result;

/* A rate-limit trip (RateLimitResult.Exceeded): the host replays
   Banner.BanOrChallengeIp then Banner.LogRegexBan for it, in the order given
   (regex_rate_limiter.go:254-266).  Offsets are relative to the line start in
   the caller's buffer. */
typedef struct bjx_trip {
  uint64_t line_idx;
  uint64_t line_offset; /* byte offset of the line in the batch */
  uint32_t line_len;    /* without '\n' */
  uint32_t rule_idx;
  int64_t ts_ns;        /* parsed line timestamp (LogRegexBan logTime) */
  uint32_t ip_off, ip_len;
  uint32_t host_off, host_len;
  uint32_t rest_off;    /* timeIpRest[2]: rest runs to line_len */
  int32_t decision;
} bjx_trip;

enum bjx_batch_flags {
  BJX_INPUT_DEVICE = 1,   /* bytes is a device pointer already resident in HBM */
  BJX_COPY_RESULTS = 2,   /* also copy per-line flags and RuleResults to host memory */
  BJX_EMIT_BANS = 4,      /* also build the batch's decision updates and ban-log lines (bjx_batch_bans) */
  BJX_BAN_RECORDS_ONLY = 8, /* with BJX_EMIT_BANS: the per-IP decision records only; no LogRegexBan lines
                              are built or copied (log_bytes 0, every log_kind 0) */
  BJX_TRIPS_COMPACT = 16,   /* trips as 8-byte words in trips_compact (trips NULL): what the host cannot
                              re-derive from its own copy of the bytes -- which line, which rule */
  BJX_RULE_STATS = 32       /* also count the batch's RuleResults per rule (bjx_batch_rule_stats) */
};

/* BJX_TRIPS_COMPACT trip word: the line's byte offset in the batch (40 bits)
   and the rule index (24 bits).  Everything else in bjx_trip follows from the
   line's bytes: line_len = up to its '\n', ts / IP / host / rest = the first
   four space-separated fields (as consumeLine splits them), decision =
   the rule's, line_idx = the newlines before it. */
#define BJX_TRIP_OFFSET(w) ((uint64_t)(w) >> 24)
#define BJX_TRIP_RULE(w) ((uint32_t)((w) & 0xFFFFFFu))

typedef struct bjx_batch_result {
  uint64_t n_lines;        /* complete ('\n'-terminated) lines processed */
  uint64_t consumed_bytes; /* offset after the last '\n' (the caller carries the rest) */
  uint64_t n_results;      /* RuleResults (matched rules) */
  uint64_t n_events;       /* RuleResults that reached RegexRateLimitStates.Apply */
  uint64_t n_trips;
  const uint8_t *line_flags;        /* host, n_lines entries, if BJX_COPY_RESULTS */
  const bjx_rule_result *results;   /* host, n_results entries in reference order, if BJX_COPY_RESULTS */
  const bjx_trip *trips;            /* host, n_trips entries in reference order */
  double device_ms;                 /* device time of the batch (HIP events) */
  double match_kernel_ms;           /* device time of the match kernel alone */
  const uint64_t *trips_compact;    /* host, n_trips trip words in reference order, if BJX_TRIPS_COMPACT (ABI 4) */
} bjx_batch_result;

/* consumeLine for every complete line of bytes[0..n) with injected clock
   now_ns (time.Now(), used for OldLine). */
int bjx_process_batch(bjx_engine *e, const bjx_ruleset *rs, const uint8_t *bytes, size_t n, int64_t now_ns,
                      uint32_t flags, bjx_batch_result *out);

/* ---- Multi-GPU batch.  One engine per GPU; each matches its
   own contiguous chunk of the log, and RegexRateLimitStates shards by IP:
   event lines go to owner (ip_hash >> 32) % n_parts.  Sequence per engine:
     bjx_match_batch                     consumeLine up to Apply (no state touched)
     bjx_events_partition                per-owner sizes of the outgoing records
     bjx_events_pack                     records into caller device buffers, owner-major
     -- caller: all-to-all of the three buffers (RCCL) --
     bjx_apply_events                    Apply for the received records, in source order
     -- caller: all-to-all of the outcome bytes back --
     bjx_finish_batch                    trips / RuleResults of the local lines
   (trips only: bjx_apply_events_trips, the trip lists back, bjx_finish_batch_trips)
   Source order must be stream order (rank r holds the r-th chunk), which makes
   the owner's event order the reference's.  All buffers are device pointers
   allocated by the caller; the engine never retains them. */
typedef struct bjx_event_line {  /* 16 B (ABI 4; the owner hashes the IP bytes itself) */
  int64_t ts_ns;     /* parsed line timestamp */
  uint32_t ip_off;   /* offset of the IP bytes in this owner's part of the byte buffer: each IP
                        starts a 4-byte aligned slot of (ip_len + 3) & ~3 bytes, zero padded (ABI 5) */
  uint16_t ip_len;
  uint16_t n_events; /* events of the line; their rule indices follow in the event buffer */
} bjx_event_line;

int bjx_match_batch(bjx_engine *e, const bjx_ruleset *rs, const uint8_t *bytes, size_t n, int64_t now_ns, uint32_t flags,
                    bjx_batch_result *out);
/* counts[3*p + 0/1/2] = event lines / events / IP slot bytes going to owner p
   (host array); 1 <= n_parts <= 256.  The byte buffers are 4-byte aligned. */
int bjx_events_partition(bjx_engine *e, uint32_t n_parts, uint64_t *counts);
int bjx_events_pack(bjx_engine *e, bjx_event_line *d_lines, uint32_t *d_events, uint8_t *d_bytes);
/* received records of n_src sources, concatenated in source order; src_counts as
   bjx_events_partition's counts, one triple per source.  d_out: one outcome
   byte per received event (bit0 seenIp, bits1-2 MatchType, bit3 Exceeded). */
int bjx_apply_events(bjx_engine *e, const bjx_ruleset *rs, const bjx_event_line *d_lines, const uint32_t *d_events,
                     const uint8_t *d_bytes, uint32_t n_src, const uint64_t *src_counts, uint8_t *d_out);
/* d_outcomes: one byte per packed event, in bjx_events_pack order */
int bjx_finish_batch(bjx_engine *e, const uint8_t *d_outcomes, uint32_t flags, bjx_batch_result *out);
/* Trips-only round trip (a batch without BJX_COPY_RESULTS needs no per-event
   outcome): the owner hands back, per source, the packed indices of that
   source's events that came out Exceeded.  trip_base[k] is added to each index
   inside source k's received segment (the caller passes that segment's offset
   in source k's bjx_events_pack order); d_trips (device, room for every
   received event) gets the sources' lists concatenated in source order, each
   ascending; trip_counts[k] (host) their lengths.  Replaces the outcome bytes
   + bjx_finish_batch when the batch needs trips (and bans) only. */
int bjx_apply_events_trips(bjx_engine *e, const bjx_ruleset *rs, const bjx_event_line *d_lines, const uint32_t *d_events,
                           const uint8_t *d_bytes, uint32_t n_src, const uint64_t *src_counts, const uint64_t *trip_base,
                           uint32_t *d_trips, uint64_t *trip_counts);
/* d_trips: n packed event indices (bjx_events_pack order) that came out Exceeded,
   in any order; flags without BJX_COPY_RESULTS */
int bjx_finish_batch_trips(bjx_engine *e, const uint32_t *d_trips, uint64_t n, uint32_t flags, bjx_batch_result *out);

/* RegexRateLimitStates.Get(ip)[name]: 1 found (num_hits, start_ns set), 0 not found, <0 error. */
int bjx_state_get(bjx_engine *e, const char *ip, size_t ip_len, const char *name, size_t name_len,
                  int64_t *num_hits, int64_t *interval_start_ns);
/* RegexRateLimitStates.Len(): number of distinct IPs with state. */
int64_t bjx_state_len(bjx_engine *e);
/* Occupancy of the persistent rate-limit state in HBM.  The reference never
   evicts state (rate_limit.go:45-67) and the engine never does on its own:
   the tables grow (rehashed on the device, 3/4 load factor) until a batch's
   growth cannot be allocated, which returns BJX_ERR_CAPACITY; device_bytes
   lets the host watch that coming (metrics, alongside Len(): config.go:165).
   Eviction is explicit and opt-in: bjx_state_expire below. */
typedef struct bjx_state_stats {
  uint64_t ips;            /* distinct IP strings (RegexRateLimitStates.Len) */
  uint64_t ip_slots;       /* IP table capacity */
  uint64_t states;         /* (ip, rule name) states */
  uint64_t state_slots;    /* state table capacity */
  uint64_t arena_bytes;    /* IP string bytes stored */
  uint64_t arena_capacity;
  uint64_t device_bytes;   /* HBM held by the state tables and the arena */
  uint64_t rehashes;       /* table growths so far */
} bjx_state_stats;
int bjx_state_stats_get(bjx_engine *e, bjx_state_stats *out);
/* Drop every rate-limit state (a fresh RegexRateLimitStates). */
int bjx_state_clear(bjx_engine *e);

/* ---- Explicit expiry of stale state (no counterpart in the reference, which
   is restarted often enough to get away without one).
   Drops every state whose interval_start_ns < cutoff_ns and every IP left
   with no state, and compacts what survives into new tables sized by the
   growth rule (3/4 load factor) on the survivor counts, never below the
   capacities the engine was created with: the tables shrink.  Surviving IPs
   keep their relative (first-seen) order in bjx_state_dump; rehashes does not
   count an expiry.  Nothing calls it implicitly.

   Contract.  Apply (rate_limit.go:37-78) writes {1, t} both for a state it
   does not know (FirstTime) and for one whose window is over (t - start >
   Interval: OutsideInterval), then runs the same NumHits > HitsPerInterval
   check.  So forgetting a state whose next event would be OutsideInterval
   changes no Exceeded, no stored state and no later event of that key; the
   one RuleResult of that next event reads match_type FIRST_TIME instead of
   OUTSIDE_INTERVAL, and the first RuleResult of an IP all of whose states
   went (whichever rule it is for) reads seen_ip 0 instead of 1.
   Len / Get / String stop listing what was dropped.  Lines older than
   now - 10 s never reach Apply (OldLine, regex_rate_limiter.go:164-167), so
   while the host's now_ns never goes backwards and no reload lengthens an
   interval,
       cutoff = now_ns - 10 s - max(interval_ns over all rules of the config)
   (saturating int64; on underflow INT64_MIN: nothing is dropped) drops only
   such states: the expiry is trip-transparent.  Any other cutoff is allowed
   and simply means "those states are forgotten"; INT64_MAX equals
   bjx_state_clear in everything a caller can observe.
   Preview: a counts-only bjx_state_query with max_start_ns = cutoff_ns - 1
   reports as n_matched the states_dropped an expiry at cutoff_ns would, and
   drops nothing.

   Takes the engine lock like the other bjx_state_* calls.  Not legal between
   bjx_match_batch and the bjx_finish_batch* that closes it (BJX_ERR_ARG; the
   node call waits for the node batch instead).  The new tables are allocated
   before the old ones are freed: BJX_ERR_NOMEM leaves the state untouched and
   usable.  out may be NULL. */
typedef struct bjx_expire_stats {
  uint64_t states_before, states_dropped;
  uint64_t ips_before, ips_dropped;
  uint64_t arena_bytes_before, arena_bytes_after;
  uint64_t device_bytes_before, device_bytes_after;  /* as bjx_state_stats.device_bytes */
  double device_ms;                                  /* device time of the pass (HIP events) */
} bjx_expire_stats;
int bjx_state_expire(bjx_engine *e, int64_t cutoff_ns, bjx_expire_stats *out);

/* ---- Snapshot and restore of the rate-limit state (no counterpart in the
   reference, whose few thousand states live in a Go map and are simply lost on
   restart).  A snapshot carries the state out of the process -- across a
   restart of the host, a library upgrade, a move to another GPU or to another
   number of GPUs -- and back in before the first batch.

   Format, version 1, little-endian (DESIGN.md §2 "Snapshot"):
   a 64-byte header {magic[8] "BJXSTATE", u32 version = 1, u32 header_bytes =
   64, u64 total_bytes, n_names, names_bytes, n_ips, ip_bytes, n_states}, then
   u64 name_off[n_names + 1], the name bytes, u64 ip_off[n_ips + 1], the IP
   bytes and n_states records {u32 ip, u32 name, i64 hits, i64 start}, each
   section padded with zeros to 8 bytes.  The form is canonical: names sorted
   bytewise, distinct, each used by a record; every IP with a record; records
   strictly ascending by (ip, name).  The bytes depend on the logical state and
   the IP order alone (not on slot layout, table sizes, name-id history or the
   debug hash mask), so export(import(x)) == x.  Limits: n_names < 2^24,
   n_ips < 2^31, n_states < 2^31 (past them export is BJX_ERR_CAPACITY).

   bjx_state_export_bound: an upper bound on the snapshot's size from the
   counters and the interned names, without a pass over the tables (0 on
   error); allocate that much and call export once.

   bjx_state_export writes every state with valid != 0 and interval_start_ns >=
   min_start_ns and every IP that keeps at least one, IPs in first-seen order.
   INT64_MIN exports everything; the trip-transparent cutoff of
   bjx_state_expire exports exactly what an expiry would keep, without
   expiring.  The engine is unchanged.  *len receives the exact size; cap too
   small: BJX_ERR_CAPACITY with *len set, out unspecified.  Not legal between
   bjx_match_batch and its bjx_finish_batch* (BJX_ERR_ARG), as expiry.

   bjx_state_import is legal only on an engine that holds no state (ips == 0
   and states == 0) and has no open batch (else BJX_ERR_ARG).  It takes the
   IPs whose owner (hash_bytes(ip) >> 32) % n_parts == part -- the node's owner
   function on the unmasked hash; pass 0, 1 for everything; n_parts 1..256.
   Afterwards everything a caller can observe equals an engine that computed
   that state itself: bjx_state_get / _len / _dump (IPs in snapshot order),
   every later RuleResult (seen_ip, match_type, exceeded), trips and bans.
   Rule names are interned into this engine, so import works before any
   ruleset was bound and whatever ids the names had.  The tables are sized by
   the growth rule on what is imported, never below the creation capacities.
   A snapshot that fails validation: BJX_ERR_ARG, the message names the check;
   a failed allocation: BJX_ERR_NOMEM; both leave the engine empty and usable.
   stats and len may be NULL. */
typedef struct bjx_snapshot_stats {
  uint64_t ips, states, names, bytes;        /* what the snapshot holds / what was imported */
  uint64_t ips_skipped, states_skipped;      /* export: below min_start_ns; import: owned by another part */
  double device_ms;                          /* HIP events, copies excluded */
} bjx_snapshot_stats;
uint64_t bjx_state_export_bound(bjx_engine *e);
int bjx_state_export(bjx_engine *e, int64_t min_start_ns, uint8_t *out, uint64_t cap, uint64_t *len,
                     bjx_snapshot_stats *stats);
int bjx_state_import(bjx_engine *e, const uint8_t *snap, uint64_t len, uint32_t part, uint32_t n_parts,
                     bjx_snapshot_stats *stats);
/* ---- Merge: fold a snapshot into an engine that holds state (no counterpart
   in the reference).  Import needs an empty engine; this call is for the host
   that has already processed batches when a snapshot reaches it: it takes over
   a leaving host's traffic (failover, consolidation), it began tailing before
   the snapshot of its previous life was read back (late restore), or a live
   node is re-sharded onto.

   Snapshot: a version-1 blob, validated exactly as bjx_state_import validates
   it (the same host and device checks, the same messages).

   Which side counts.  On the engine the states with valid != 0 -- exactly
   what bjx_state_export writes; a slot claimed with valid == 0 is absent.  From
   the snapshot the records of the IPs the part owns ((hash_bytes(ip) >> 32) %
   n_parts == part, as import; 0, 1: all) whose interval_start_ns >=
   min_start_ns (INT64_MIN: all).  The others are skipped.

   Conflict.  A key is (IP bytes, rule name bytes); the policy decides a key
   both sides hold.
     BJX_MERGE_NEWER    the record with the larger interval_start_ns wins; on
                        equal starts the larger hits (signed); equal in both:
                        nothing changes.  That is the lexicographic maximum of
                        (start, hits), so merging states is idempotent,
                        commutative and associative.  Why this rule: a later
                        start means that side saw the older window end, and on a
                        shared window the larger count is the closer one to the
                        count over the union of the two streams.  No merge of two
                        fixed-window counters reproduces the union stream
                        exactly (each side has counted only its own lines, and
                        the window a stream opens depends on its own first
                        line); in particular a count that a trip set back to 0
                        loses to the pre-trip count of the same window.
     BJX_MERGE_KEEP     the engine's record stays; the snapshot only fills gaps.
     BJX_MERGE_REPLACE  the snapshot's record wins (counted in states_replaced
                        only when it differs).
   A key only the snapshot holds is added under every policy.

   Order and ids.  The engine's IPs keep their ids and their first-seen order.
   A snapshot IP the engine does not hold that brings at least one record is
   appended after them, in snapshot order, under the next dense ids; one all of
   whose records are skipped is not added.  Names are interned into this
   engine, as import does.

   Equivalence.  Everything a caller can observe afterwards equals an engine
   that imported the snapshot M = merge_model(export(engine before), snap,
   options) (banjax_amd/state_merge.py is that model): bjx_state_get / _len /
   _dump / _query* / _export -- export is canonical, so export(after) == M byte
   for byte -- and every later RuleResult's seen_ip, match_type and exceeded,
   trips and bans.

   Nothing to change (every record skipped, or every conflict keeps the
   engine's record; merging an engine's own export is this case): the engine is
   left exactly as it was.  No rebuild runs, no table changes size, rehashes is
   unchanged and the stats' after values equal their before values.

   BJX_MERGE_DRY_RUN: every count and arena_bytes_after come back as the real
   call would report them (and the errors it would return), nothing changes,
   device_bytes_after = device_bytes_before.

   Tables.  One path: the union is built into new tables -- the engine's
   entries re-put as growth does, the new IPs and records as import does --
   and swapped in; everything a change of tables resets is reset (the hot-name
   slot cache too).  They are sized by the growth rule on the union counts,
   never below the present capacities: a merge never shrinks.  The new tables
   are allocated before the old ones are freed: BJX_ERR_NOMEM leaves the state
   untouched and usable.  rehashes does not count a merge.  The rebuild makes a
   merge cost O(engine state + snapshot), whatever the share that changes.
   Temporary device memory: the snapshot from its ip_off section on, 44 bytes
   per snapshot IP and 1 per record, 4 bytes per held IP, and (dry run
   included) the new tables next to the old.

   Errors.  BJX_ERR_ARG, the engine unchanged in every case: a NULL handle,
   snap or o; an unknown policy or unknown flag bits; part / n_parts out of
   range (n_parts 1..256, part < n_parts); a call between bjx_match_batch and
   its bjx_finish_batch*; a snapshot that fails a check (the message names it);
   an IP that appears twice in the snapshot, whether or not the engine holds it
   (seen among the IPs the part owns that bring a record or that the engine
   holds).  BJX_ERR_CAPACITY: the union would reach 2^31 IPs or 2^24 names.
   out may be NULL.  Takes the engine lock like the other bjx_state_* calls.

   bjx_node_state_merge waits for the node batch; engine k merges with part =
   k, n_parts = size, so the caller's part / n_parts must be 0, 1
   (BJX_ERR_ARG).  Counts and bytes are summed, the snap_* fields reported
   once, device_ms is the slowest shard's; a dry run is dry on every shard.
   Every shard is asked even when one fails: the first failure is returned and
   the shards already done stay done.  Every policy is idempotent, so the
   caller repeats the call, as with bjx_node_state_remove. */
enum bjx_merge_policy { BJX_MERGE_NEWER = 0, BJX_MERGE_KEEP = 1, BJX_MERGE_REPLACE = 2 };
enum bjx_merge_flags { BJX_MERGE_DRY_RUN = 1 };
typedef struct bjx_merge_options { /* 24 B */
  int64_t min_start_ns;   /* snapshot records with interval_start_ns below this are skipped (INT64_MIN: none) */
  uint32_t part, n_parts; /* as bjx_state_import: only IPs with (hash_bytes(ip) >> 32) % n_parts == part; 0, 1: all */
  uint32_t policy;        /* enum bjx_merge_policy */
  uint32_t flags;         /* enum bjx_merge_flags */
} bjx_merge_options;
typedef struct bjx_merge_stats { /* 136 B */
  uint64_t snap_ips, snap_states, snap_names, snap_bytes; /* what the snapshot holds */
  uint64_t ips_before, ips_added;                          /* IPs the engine did not hold and now does */
  uint64_t ips_skipped;     /* snapshot IPs that brought nothing: other part, or every record skipped */
  uint64_t states_before;
  uint64_t states_added;    /* key not held (or held with valid == 0) */
  uint64_t states_replaced; /* key held, the snapshot's record won and differs */
  uint64_t states_kept;     /* key held, the engine's record stays (lost, or equal) */
  uint64_t states_skipped;  /* other part, or below min_start_ns; the four add up to snap_states */
  uint64_t arena_bytes_before, arena_bytes_after;
  uint64_t device_bytes_before, device_bytes_after; /* as bjx_state_stats.device_bytes */
  double device_ms;                                 /* HIP events, copies excluded */
} bjx_merge_stats;
int bjx_state_merge(bjx_engine *e, const uint8_t *snap, uint64_t len, const bjx_merge_options *o, bjx_merge_stats *out);
/* ---- Query: top-K, counts and Get(ip) over the state where it lives.
   bjx_state_dump (RegexRateLimitStates.String, the /rate_limit_states route,
   http_server.go:193-198) is text of every state and bjx_state_get answers one
   (ip, name); this call answers "which IPs are closest to tripping rule X",
   "how many states does rule X hold", "what would an expiry at this cutoff
   drop" and the reference's whole-map Get(ip) (rate_limit.go:81-96) in one
   pass, and a small answer comes back.

   Which states count: those with valid != 0 -- exactly what bjx_state_export
   writes -- that pass all five conditions of the filter.  n_matched counts
   them, n_ips_matched the distinct IPs among them.

   Order: total, and a function of the logical state alone.  Primary key
   descending (hits for BJX_QUERY_BY_HITS, interval_start_ns for
   BJX_QUERY_BY_START), then IP in first-seen order ascending (the order of
   bjx_state_dump), then rule name bytewise ascending.  Slot layout, table
   sizes, name-id history and the debug hash mask do not show.  The rows are
   the first min(limit, n_matched) states in that order; limit 0 asks for the
   counts only.

   Not errors: a name the engine never interned or an IP it does not hold
   (zero rows, zero counts); min_start_ns > max_start_ns (zero rows).
   BJX_ERR_ARG: limit > BJX_QUERY_MAX_ROWS, an unknown order, a NULL f, out or
   handle, a call between bjx_match_batch and its bjx_finish_batch* (the node
   call waits for the node batch instead, as expiry and export do).  A failed
   allocation: BJX_ERR_NOMEM.  The engine is unchanged in every case.  Takes
   the engine lock like the other bjx_state_* calls.  rows and bytes are
   engine-owned (node-owned for the node call) and stay valid until the next
   query on that handle.

   With an ip filter no table is scanned: the IP is found as bjx_state_get
   finds it and one probe per interned name follows, so Get(ip) costs the
   number of names the engine has ever seen -- and returns states kept under a
   name a reload removed, as the reference's Get does.

   Expiry preview: a counts-only query with max_start_ns = cutoff - 1 has
   n_matched equal to the states_dropped bjx_state_expire(cutoff) would report
   (cutoff > INT64_MIN; at INT64_MIN an expiry drops nothing). */
enum bjx_query_order { BJX_QUERY_BY_HITS = 0, BJX_QUERY_BY_START = 1 };
#define BJX_QUERY_MAX_ROWS 65536
typedef struct bjx_state_filter {   /* 64 B */
  bjx_str ip;            /* ptr NULL: every IP; else exactly these bytes (len 0 is a value): Get(ip) */
  bjx_str name;          /* ptr NULL: every rule name; else exactly this name (len 0 is a value) */
  int64_t min_hits;      /* hits >= min_hits        (INT64_MIN: all) */
  int64_t min_start_ns;  /* interval_start_ns >= .. (INT64_MIN: all) */
  int64_t max_start_ns;  /* interval_start_ns <= .. (INT64_MAX: all) */
  uint32_t order;        /* enum bjx_query_order */
  uint32_t limit;        /* rows wanted, 0..BJX_QUERY_MAX_ROWS; 0: counts only */
} bjx_state_filter;
typedef struct bjx_state_row {      /* 40 B */
  uint64_t ip_off, name_off;        /* into bjx_state_rows.bytes */
  uint32_t ip_len, name_len;
  int64_t hits, start_ns;
} bjx_state_row;
typedef struct bjx_state_rows {     /* 56 B */
  uint64_t n_matched;      /* states that pass the filter */
  uint64_t n_ips_matched;  /* distinct IPs among them */
  uint64_t n_rows;         /* min(limit, n_matched) */
  const bjx_state_row *rows;
  const uint8_t *bytes; uint64_t n_bytes;
  double device_ms;        /* HIP events, copies excluded */
} bjx_state_rows;
int bjx_state_query(bjx_engine *e, const bjx_state_filter *f, bjx_state_rows *out);
/* ---- Remove: forget chosen states.  The reference's host owns a Go map and
   can delete from it; here the state lives in HBM, so the host asks.  Uses: an
   unban (the reference's POST /unban, http_server.go:262-312, clears the
   decision and leaves the IP's counters, often exactly at their threshold),
   a rule whose rate or regex changed on reload (state is keyed by rule name
   and survives it), a new allow-list entry (a single IP; for an IP/len entry
   use bjx_state_remove_nets below), a false positive found with
   bjx_state_query.

   Selection: a state is dropped when it has valid != 0 and passes the five
   conditions of *f exactly as bjx_state_query reads them (ip, name, min_hits,
   min_start_ns, max_start_ns; order and limit are not read) and, when
   n_ips > 0, its IP is one of ips[0..n_ips), compared by bytes.  The list and
   the filter mean both: f->ip together with a list selects only when that IP
   is in the list.  Duplicates in the list are allowed, a listed IP the engine
   does not hold is not an error, a length-0 IP is a value.  Every IP left
   without a state goes too.  A counts-only bjx_state_query with the same
   filter previews a removal without a list: its n_matched is states_dropped.

   Not errors (nothing is selected): a name the engine never interned, an
   empty start window.  An all-pass filter without a list drops everything:
   whatever a caller can observe then equals bjx_state_clear.
   BJX_ERR_ARG: a NULL handle or f; n_ips > 0 with NULL ips; an entry (or
   f->ip, f->name) with len > 0 and a NULL ptr; 2^32 list bytes or more in
   total; a call between bjx_match_batch and its bjx_finish_batch* (the node
   call waits for the node batch instead, as expiry does).  The new tables are
   allocated before the old ones are freed: BJX_ERR_NOMEM leaves the state
   untouched and usable.  out may be NULL.  Takes the engine lock like the
   other bjx_state_* calls.

   Afterwards everything observable equals an engine that imported a snapshot
   of the surviving states: bjx_state_get / _len / _dump / _query / _export,
   every later RuleResult (seen_ip, match_type, exceeded), trips and bans.
   Surviving IPs keep their relative first-seen order and ids are dense again;
   a removed IP that returns is a new IP, after them.  The tables are rebuilt
   as bjx_state_expire rebuilds them, with its sizing rule (never below the
   creation capacities, never above the present ones); rehashes does not count
   a removal.  states_dropped is states_before minus the states kept, the
   expiry's convention: a removal with max_start_ns = cutoff - 1 and everything
   else open reports what bjx_state_expire(cutoff) reports and leaves the same
   state.

   When nothing is selected the engine is left exactly as it was: no rebuild
   runs, no table changes size, and the stats' after equals their before
   (unlike the expiry, which always rebuilds: an unban of an IP the engine does
   not hold is the common case and must not move the tables). */
typedef struct bjx_remove_stats {   /* 80 B */
  uint64_t states_before, states_dropped;
  uint64_t ips_before, ips_dropped;          /* IPs left without any state */
  uint64_t ips_found;                        /* distinct listed IPs the engine held (0 without a list) */
  uint64_t arena_bytes_before, arena_bytes_after;
  uint64_t device_bytes_before, device_bytes_after;  /* as bjx_state_stats.device_bytes */
  double device_ms;                          /* HIP events, copies excluded */
} bjx_remove_stats;
int bjx_state_remove(bjx_engine *e, const bjx_state_filter *f, const bjx_str *ips, size_t n_ips, bjx_remove_stats *out);
/* ---- Nets: bjx_state_query and bjx_state_remove with the IPs chosen by
   network.  Uses: a new allow-list entry IP/len (the counters of every address
   in it stay in HBM otherwise), unbanning a range, "what is this /24 doing".

   Entries: nets[k] is text as an Allow entry of a decision list is written,
   an address or address/bits, read by net.ParseIP / net.ParseCIDR rules (no
   zone; bits in decimal, at most the family's length; bits equal to it is the
   single address; host bits set in the address are masked away).
   BJX_ERR_ARG, with the engine unchanged: an entry that does not parse (the
   message names its index), n_nets == 0 (a nets call never means "every IP"),
   n_nets > BJX_NETS_MAX, NULL nets, an entry with len > 0 and a NULL ptr, and
   what bjx_state_query / bjx_state_remove refuse in *f.

   Membership: a held IP is in a network exactly when a global Allow decision
   list made of these entries would exempt a line of that IP
   (CheckIsAllowed).  The IP's stored bytes are parsed as net.ParseIP parses
   them; text that does not parse is in no network.  A v4-mapped address
   compares as IPv4, against IPv4 networks only, and an IPv6 network never
   holds it: ::/0 holds no IPv4 text, 0.0.0.0/0 no IPv6 text, and
   ::ffff:10.0.0.0/104 is 10.0.0.0/8.  Duplicate and nested entries are fine.

   Selection: a state is selected when it has valid != 0, passes the five
   conditions of *f exactly as bjx_state_query reads them and its IP is in at
   least one entry.  f->ip together with nets means both: that IP, and only
   when a network holds it.

   bjx_state_query_nets: order, limit, rows, bytes, ownership, locking and the
   open-batch rule are bjx_state_query's; n_matched and n_ips_matched count the
   selected states and their distinct IPs.  (*net_ips)[k], for each of the
   n_nets entries in the caller's order, is the number of distinct held IPs
   inside entry k with at least one selected state; nested and duplicate
   entries each count, so the sum may exceed n_ips_matched.  net_ips may be
   NULL; the array is engine-owned and valid until the next query on the
   handle.  A counts-only call (limit 0) previews bjx_state_remove_nets with
   the same arguments: its n_matched is the removal's states_dropped.

   bjx_state_remove_nets: everything bjx_state_remove promises, with "the IP
   is in a network" in place of "the IP is in the list": the result equals an
   engine that imported a snapshot of the survivors, first-seen order kept, ids
   dense; nothing selected leaves the engine exactly as it was; the new tables
   are allocated before the old ones are freed.  ips_found is the number of
   distinct held IPs inside any network, whether or not a state of theirs was
   selected.  out may be NULL. */
#define BJX_NETS_MAX 65536
int bjx_state_query_nets(bjx_engine *e, const bjx_state_filter *f, const bjx_str *nets, size_t n_nets,
                         bjx_state_rows *out, const uint64_t **net_ips);
int bjx_state_remove_nets(bjx_engine *e, const bjx_state_filter *f, const bjx_str *nets, size_t n_nets,
                          bjx_remove_stats *out);
/* ---- Trim: evict the oldest state down to a budget.  Under a flood of
   distinct source addresses the states are fresh, so the trip-transparent
   cutoff of bjx_state_expire frees nothing, and the host cannot know which
   cutoff frees enough: the distribution of interval_start_ns lives in HBM.
   This call answers "keep this engine's state under max_states states and
   max_ips IPs, and lose the least recent information possible": it finds the
   cutoff on the device and expires at it.

   Which states count: those with valid != 0 -- exactly what bjx_state_export
   writes and bjx_state_query counts.

   The cutoff.  For a multiset V of int64 and a bound k, cut(V, k) is the
   smallest C with #{v in V : v >= C} <= k: INT64_MIN when k == 0 (no bound)
   or |V| <= k, else v + 1 for the (k + 1)-th largest value v of V, saturating
   at INT64_MAX.  With
       C_states = cut(the starts of all states, max_states)
       C_ips    = cut({the newest start of each held IP}, max_ips)
   the cutoff is C = max(floor_cutoff_ns, C_states, C_ips).

   The trim is bjx_state_expire(C): every state with interval_start_ns < C
   goes and every IP left without a state goes too; the survivors keep their
   first-seen order under dense ids; the tables are rebuilt by the expiry's
   path with its sizing rule; the new tables are allocated before the old ones
   are freed (BJX_ERR_NOMEM leaves the state untouched and usable); rehashes
   does not count a trim.  Afterwards everything observable equals an engine
   that imported a snapshot of the survivors.

   Ties: states that share a start go or stay together, so the result is a
   function of the logical state alone (never of slot layout) and may hold
   fewer states than the budget allows.  Saturated case: when more than k
   values equal INT64_MAX, C = INT64_MAX, those states stay and budget_met is
   0; in every other case budget_met is 1.

   bound says what set C: BJX_TRIM_BY_IPS if C_ips == C and C_ips > INT64_MIN,
   else BJX_TRIM_BY_STATES if C_states == C and C_states > INT64_MIN, else
   BJX_TRIM_BY_FLOOR if floor_cutoff_ns > INT64_MIN, else BJX_TRIM_BY_NONE.

   states_dropped_live counts the dropped states with interval_start_ns >=
   floor_cutoff_ns.  A host that passes the trip-transparent cutoff of
   bjx_state_expire as the floor reads here how many evictions were not
   transparent: forgetting such a state can turn a later InsideInterval event
   into FirstTime, restart its count and so delay or lose a trip (see the
   expiry's contract for what a forgotten state changes).  states_dropped
   counts the valid states that went.

   When no state would be dropped the engine is left exactly as it was: no
   rebuild runs, no table changes size and the stats' after equals their
   before (as bjx_state_remove, unlike the expiry: the trim is meant to be
   called after every batch).  A budget the counters already meet costs no pass
   over the tables.

   BJX_TRIM_DRY_RUN computes cutoff_ns, bound, budget_met, the three dropped
   counts and arena_bytes_after exactly as the real call would report them and
   changes nothing; device_bytes_after = device_bytes_before.

   BJX_ERR_ARG: a NULL handle or b, unknown flag bits, a call between
   bjx_match_batch and its bjx_finish_batch* (the node call waits for the node
   batch instead, as expiry does).  out may be NULL.  Takes the engine lock
   like the other bjx_state_* calls.  Temporary device memory of the
   selection: 8 bytes and one bit per held IP (only with max_ips) and 128 KiB
   of digit counters; no per-state temporary -- the state table is read in
   place, at most five times. */
enum bjx_trim_flags { BJX_TRIM_DRY_RUN = 1 };
enum bjx_trim_bound { BJX_TRIM_BY_NONE = 0, BJX_TRIM_BY_FLOOR = 1, BJX_TRIM_BY_STATES = 2, BJX_TRIM_BY_IPS = 3 };
typedef struct bjx_trim_budget {   /* 32 B */
  uint64_t max_states;      /* keep at most this many states; 0: no bound */
  uint64_t max_ips;         /* keep at most this many IPs;    0: no bound */
  int64_t floor_cutoff_ns;  /* states that started before this always go (INT64_MIN: none) */
  uint32_t flags;           /* bjx_trim_flags */
  uint32_t _pad;
} bjx_trim_budget;
typedef struct bjx_trim_stats {    /* 104 B */
  int64_t cutoff_ns;                 /* the cutoff C that was (or would be) applied */
  uint32_t bound;                    /* enum bjx_trim_bound: what set C */
  uint32_t budget_met;               /* 0 only in the saturated case above */
  uint64_t states_before, states_dropped, states_dropped_live;
  uint64_t ips_before, ips_dropped;
  uint64_t arena_bytes_before, arena_bytes_after;
  uint64_t device_bytes_before, device_bytes_after;  /* as bjx_state_stats.device_bytes */
  double select_ms;                  /* HIP events around finding C */
  double device_ms;                  /* select + mark/scan + rebuild, copies excluded */
} bjx_trim_stats;
int bjx_state_trim(bjx_engine *e, const bjx_trim_budget *b, bjx_trim_stats *out);
/* ---- Groups: the networks that hold the most counting IPs.  The nets calls
   act on a network once somebody names it; this call finds it.  During a flood
   of distinct source addresses "which /24s (or IPv6 /64s) hold the most IPs
   right now" becomes an allow entry, a ban or a bjx_state_remove_nets call,
   and the distribution lives in HBM.

   Selection: a state is selected when it has valid != 0 and passes the five
   conditions of *f exactly as bjx_state_query reads them (ip, name, min_hits,
   min_start_ns, max_start_ns).  f->order and f->limit change nothing in the
   answer (a filter bjx_state_query refuses is still refused); f->ip is
   honoured: the groups of that one IP's selected states.  An IP is selected
   when at least one of its states is.

   Group of an IP: its stored bytes are parsed as net.ParseIP parses them.
   Text that does not parse belongs to no group and is counted in
   n_ips_unparsed / n_states_unparsed.  A v4-mapped address (dotted-quad text
   or ::ffff:a.b.c.d text) is IPv4 and is masked to v4_bits; every other
   address is IPv6 and is masked to v6_bits.  The group is (family, masked
   address).  This is the membership rule of the nets calls: for every row,
   bjx_state_query_nets with the same *f, limit 0 and the single entry
   addr/bits reports n_matched == n_states and net_ips[0] == n_ips.

   Rows: the groups with n_ips >= min_ips, ordered by the primary key
   descending -- n_ips, n_states or hits_sum (as signed int64) -- then family 4
   before family 6, then addr bytewise ascending; the first `limit` of them.
   The order is total and a function of the logical state alone: slot layout,
   table sizes and the debug hash mask do not show.  hits_sum wraps as Go's
   int addition does.  Over all groups, the n_ips add up to n_ips_matched -
   n_ips_unparsed and the n_states to n_matched - n_states_unparsed.

   Not errors (zero rows, zero counts): an engine without state, a name the
   engine never interned, an empty start window.  BJX_ERR_ARG, with the engine
   unchanged: a NULL handle, f, g or out; v4_bits > 32; v6_bits > 128; an
   unknown order; limit > BJX_GROUPS_MAX_ROWS; what bjx_state_query refuses in
   *f, and f->ip or f->name with len > 0 and a NULL ptr; a call between
   bjx_match_batch and its bjx_finish_batch* (the node call waits for the node
   batch instead).  BJX_ERR_NOMEM: a failed allocation.  The engine is
   unchanged in every case: the tables are only read.  rows is engine-owned and
   valid until the next groups query on the handle.  Takes the engine lock
   like the other bjx_state_* calls.

   Temporary device memory: proportional to the held IPs, 32 bytes per held IP
   (a state count, a hits sum and a newest start each) and at most about 170
   per selected IP (sort keys, their permutation, the group records); no
   per-state temporary -- the state table is read in place, once. */
enum bjx_group_order { BJX_GROUPS_BY_IPS = 0, BJX_GROUPS_BY_STATES = 1, BJX_GROUPS_BY_HITS = 2 };
#define BJX_GROUPS_MAX_ROWS 65536
typedef struct bjx_group_spec {     /* 24 B */
  uint32_t v4_bits;   /* 0..32:  prefix length IPv4 addresses are grouped by */
  uint32_t v6_bits;   /* 0..128: the same for IPv6 */
  uint32_t order;     /* enum bjx_group_order */
  uint32_t limit;     /* rows wanted, 0..BJX_GROUPS_MAX_ROWS; 0: counts only */
  uint64_t min_ips;   /* rows only for groups with n_ips >= min_ips (0 and 1: every group) */
} bjx_group_spec;
typedef struct bjx_group_row {      /* 56 B */
  uint8_t addr[16];   /* the masked network; IPv4 in addr[0..4), the rest 0 */
  uint32_t family;    /* 4 or 6 */
  uint32_t bits;      /* v4_bits or v6_bits */
  uint64_t n_ips;     /* distinct held IPs of the group with a selected state */
  uint64_t n_states;  /* selected states of those IPs */
  int64_t hits_sum;   /* sum of their hits, wrapping as Go int addition */
  int64_t newest_start_ns; /* largest interval_start_ns among them */
} bjx_group_row;
typedef struct bjx_state_groups {   /* 72 B */
  uint64_t n_matched, n_ips_matched;          /* exactly bjx_state_query's for the same *f */
  uint64_t n_ips_unparsed, n_states_unparsed; /* selected, but the IP text is no address: in no group */
  uint64_t n_groups;      /* distinct groups */
  uint64_t n_groups_min;  /* those with n_ips >= min_ips */
  uint64_t n_rows;        /* min(limit, n_groups_min) */
  const bjx_group_row *rows;  /* engine-owned (node-owned), valid until the next groups query on the handle */
  double device_ms;       /* HIP events, copies excluded */
} bjx_state_groups;
int bjx_state_query_groups(bjx_engine *e, const bjx_state_filter *f, const bjx_group_spec *g, bjx_state_groups *out);
/* ---- Names: which rule names hold the state.  State is keyed by IP bytes
   and rule name and survives ruleset swaps, so after a reload that renames,
   drops or retunes rules the engine still keeps every state of the old names.
   bjx_state_remove and bjx_state_query act on a name once somebody gives it;
   this call lists the names: one pass over the state table, aggregated per
   name on the device, and a small answer.

   Selection: a state is selected when it has valid != 0 and passes the five
   conditions of *f exactly as bjx_state_query reads them (ip, name, min_hits,
   min_start_ns, max_start_ns).  f->order and f->limit change nothing in the
   answer (a filter bjx_state_query refuses is still refused).  f->ip is
   honoured as the groups call honours it (the names that IP holds; the table
   is still read once, there is no scan-free path); f->name set gives at most
   one row.

   Rows: a name without a selected state has no row, however it came to be
   interned (a bound ruleset whose rule never matched, a claim that was refused
   or undone, a removal since).  The names with n_states >= min_states are
   ordered by the primary key descending -- n_states, hits_sum (as signed
   int64), max_hits or newest_start_ns; BJX_NAMES_BY_NAME has no primary key --
   then by name bytewise ascending, a prefix before the longer name; the first
   `limit` of them.  The order is total and a function of the logical state
   alone: slot layout, table sizes, name ids, the order the names were
   interned in and the debug hash mask do not show.  A row's name is
   bytes[name_off, name_off + name_len).  hits_sum wraps as Go's int addition
   does.  hist counts the row's states by hits: bucket 0 hits <= 0, bucket b
   (1..14) the hits of bit length b, 2^(b-1) <= hits < 2^b, bucket 15 hits >=
   2^14.  Over all names the n_states add up to n_matched; for every row
   sum(hist) == n_states.

   Against the other calls, for every row: bjx_state_query with the same *f
   and name = the row's name reports n_matched == n_ips_matched == n_states
   ((ip, name) is unique), its top row by hits carries max_hits and by start
   newest_start_ns; with min_hits = 2^k added (k = 0..14, f->min_hits <= 2^k)
   it reports hist[k+1] + ... + hist[15]; bjx_state_remove with the same
   filter and that name reports states_dropped == n_states.

   Not errors (zero rows, zero counts): an engine without state, a name the
   engine never interned, an empty start window, an IP not held.
   BJX_ERR_ARG, with the engine unchanged: a NULL handle, f, s or out; an
   unknown order; limit > BJX_NAMES_MAX_ROWS; what bjx_state_query refuses in
   *f, and f->ip or f->name with len > 0 and a NULL ptr; a call between
   bjx_match_batch and its bjx_finish_batch* (the node call waits for the node
   batch instead).  BJX_ERR_NOMEM: a failed allocation (everything is of known
   size and allocated before the first launch).  The engine is unchanged in
   every case: the tables are only read.  rows and bytes are engine-owned and
   valid until the next names query on the handle.  Takes the engine lock like
   the other bjx_state_* calls.

   Temporary device memory: two arrays of 176-byte records sized by the names
   the engine has interned (the accumulators and their compacted copy), 4 bytes
   per held IP for n_ips_matched, and with f->ip another 4 per held IP; no
   per-state temporary -- the state table is read in place, once.  What is
   copied back is proportional to the names in use, not to the names
   interned.  Cost: while the engine has interned at most 1,365 names (what
   bjx_debug_names_info reports as lds_names_max) the per-name sums are kept
   in on-chip memory and the call costs about what a counts-only
   bjx_state_query costs; past that every selected state adds straight to the
   per-name records in device memory and the call changes class -- about 170
   times slower on a state of 55M states under 1,006 names (DESIGN.md §2
   "Names").  Names stay interned for the life of the engine, so a host that
   reloads rulesets with ever new names gets there over time. */
enum bjx_names_order { BJX_NAMES_BY_STATES = 0, BJX_NAMES_BY_HITS = 1, BJX_NAMES_BY_MAX_HITS = 2,
                       BJX_NAMES_BY_NEWEST = 3, BJX_NAMES_BY_NAME = 4 };
#define BJX_NAMES_MAX_ROWS 65536
#define BJX_NAMES_HIST 16
typedef struct bjx_names_spec {   /* 16 B */
  uint32_t order;       /* enum bjx_names_order */
  uint32_t limit;       /* rows wanted, 0..BJX_NAMES_MAX_ROWS; 0: counts only */
  uint64_t min_states;  /* rows only for names with n_states >= min_states (0 and 1: every name) */
} bjx_names_spec;
typedef struct bjx_name_row {     /* 184 B */
  uint64_t name_off; uint32_t name_len, _pad;   /* into bjx_state_names.bytes */
  uint64_t n_states;          /* selected states under the name == distinct IPs holding one ((ip, name) is unique) */
  int64_t hits_sum;           /* wrapping as Go int addition, as bjx_group_row */
  int64_t max_hits;
  int64_t newest_start_ns, oldest_start_ns;
  uint64_t hist[BJX_NAMES_HIST]; /* by hits: bucket 0: hits <= 0; bucket b: bit_length(hits) == b; bucket 15: hits >= 2^14 */
} bjx_name_row;
typedef struct bjx_state_names {  /* 72 B */
  uint64_t n_matched, n_ips_matched;  /* exactly bjx_state_query's for the same *f */
  uint64_t n_names;       /* distinct names with a selected state */
  uint64_t n_names_min;   /* those with n_states >= min_states */
  uint64_t n_rows;        /* min(limit, n_names_min) */
  const bjx_name_row *rows; const uint8_t *bytes; uint64_t n_bytes;  /* engine-owned (node-owned), valid until the next names query on the handle */
  double device_ms;       /* HIP events, copies excluded */
} bjx_state_names;
int bjx_state_query_names(bjx_engine *e, const bjx_state_filter *f, const bjx_names_spec *s, bjx_state_names *out);
/* RegexRateLimitStates.String(): "ip:\n\trule:\n\t\t{hits start}\n" blocks, IPs in
   first-seen order.  Returns the full length (writes at most cap bytes). */
size_t bjx_state_dump(bjx_engine *e, char *out, size_t cap);

/* ---- Log-tail front end.  Replaces github.com/hpcloud/tail
   v1.0.0 as RunLogTailer uses it (regex_rate_limiter.go:30-58: Follow, start
   at EOF) with bulk reads into pinned buffers and batches of complete lines:
     - a line is the bytes before '\n' ('\r' kept), exactly tail.Line.Text;
     - a trailing partial line is held until its '\n' arrives (tail seeks back
       over it and re-reads, same effect);
     - a missing file is waited for, then followed from its end (MustExist false);
     - a file that shrinks below the read offset was truncated: it is re-read
       from offset 0 and the held partial line is dropped (tail's reopen);
     - a file deleted or renamed away stops the tail (ReOpen false):
       bjx_tailer_next returns BJX_TAIL_STOPPED once every batch is handed out.
   A reader thread fills the next pinned slot and issues its host-to-device
   copy on a copy stream while the caller runs bjx_process_batch on the
   previous slot (double buffering with slots = 2).  Batch = one config
   snapshot for all its lines (the reference reads configHolder.Get() per
   line, :58-59; a reload takes effect at the next batch). */
typedef struct bjx_tailer bjx_tailer;

typedef struct bjx_tailer_options {
  int32_t device;        /* GPU that receives each batch (HBM copy); -1 = host framing only */
  int32_t from_start;    /* 0: first open seeks to EOF (Whence io.SeekEnd, :32-36); 1: offset 0 */
  uint32_t slots;        /* pinned (+ device) buffers in flight; 0 = 2 */
  uint32_t poll_ms;      /* wait at EOF before looking again; 0 = 20 */
  uint64_t batch_bytes;  /* largest batch; 0 = 256 MiB (a longer line grows the slot) */
} bjx_tailer_options;

typedef struct bjx_tail_batch {
  uint32_t slot;               /* give back with bjx_tailer_release */
  uint32_t reopened;           /* the file was truncated and re-read from 0 before this batch */
  const uint8_t *host_bytes;   /* pinned host copy: trips' line offsets index it */
  const uint8_t *device_bytes; /* HBM copy, complete: pass to bjx_process_batch with BJX_INPUT_DEVICE (NULL if device = -1) */
  uint64_t n_bytes;            /* ends with '\n' */
  uint64_t file_offset;        /* file offset of host_bytes[0] */
} bjx_tail_batch;

int bjx_tailer_open(const char *path, size_t path_len, const bjx_tailer_options *opts, bjx_tailer **out, char *err,
                    size_t err_len);
/* Next batch, oldest first.  Waits up to timeout_ms (< 0: forever).  Returns
   1 with *out filled, 0 on timeout, BJX_TAIL_STOPPED, or an error code. */
int bjx_tailer_next(bjx_tailer *t, int32_t timeout_ms, bjx_tail_batch *out);
int bjx_tailer_release(bjx_tailer *t, uint32_t slot);
/* bytes read from the file so far / handed out in batches (held partial line = difference) */
int bjx_tailer_stats(bjx_tailer *t, uint64_t *read_bytes, uint64_t *batched_bytes, uint64_t *batches);
void bjx_tailer_close(bjx_tailer *t);

/* Last error message of an engine call. */
const char *bjx_engine_last_error(bjx_engine *e);
/* ---- Trip -> decision emission.  Replaces the per-trip
   host replay of Banner.BanOrChallengeIp -> DynamicDecisionLists.Update
   (internal/iptables.go:273-294, internal/decision.go:404-439) and
   Banner.LogRegexBan (internal/iptables.go:179-228) that consumeLine runs for
   every trip (internal/regex_rate_limiter.go:254-266).
   Options hold for every later batch run with BJX_EMIT_BANS. */
/* One UTC-offset change of the local time zone LogRegexBan formats its
   timestring in (logTime.Format in time.Local, internal/iptables.go:187). */
typedef struct bjx_tz_transition {
  int64_t utc_start_s; /* first Unix second the offset applies to */
  int32_t offset_s;    /* seconds east of UTC from then on */
  int32_t _pad;
} bjx_tz_transition;

typedef struct bjx_ban_options {
  int64_t expiring_ttl_ns;          /* expiring_decision_ttl_seconds * 1e9 (config.go) */
  int32_t tz_offset_s;              /* UTC offset (seconds east) before the first transition, or always when there are none */
  uint32_t _pad;
  const bjx_str *disable_logging;   /* config.DisableLogging hosts set to true (LoggerTemp lines) */
  size_t n_disable_logging;
  const bjx_tz_transition *tz_transitions; /* the zone's offset changes, ascending by utc_start_s (DST rules
                                              expanded; a Go host walks time.Local with Time.ZoneBounds) */
  size_t n_tz_transitions;
} bjx_ban_options;
int bjx_engine_set_ban_options(bjx_engine *e, const bjx_ban_options *opts);

/* One per distinct IP that tripped in the batch.  Applying
   Update(ip, expires_ns, decision, fromBaskerville=false, domain) once per
   record, with ip / domain (host) taken from trips[trip_idx], leaves the
   decision lists exactly as the per-trip replay does: the entry changes only
   when decision beats the one held, and the first trip with the IP's highest
   decision is the last strict escalation.  iptables: some trip decided
   IptablesBlock (banIp, which the reference calls per such trip). */
typedef struct bjx_ip_decision {
  uint64_t trip_idx;
  uint64_t n_trips;     /* trips of this IP in the batch */
  int64_t expires_ns;   /* now_ns + expiring_ttl_ns (Go wrapping add) */
  int32_t decision;     /* highest decision over the IP's trips */
  uint32_t iptables;
} bjx_ip_decision;

typedef struct bjx_ban_batch {
  uint64_t n_ips;
  const bjx_ip_decision *ips;   /* host, ordered by trip_idx */
  uint64_t n_trips;
  const char *log;              /* host: LogRegexBan lines in trip order, each ending in '\n' */
  uint64_t log_bytes;
  const uint64_t *log_off;      /* host, n_trips + 1: trip t's line is log[log_off[t], log_off[t+1]) (empty: < 6 words) */
  const uint8_t *log_kind;      /* host, n_trips: 0 no line, 1 Logger, 2 LoggerTemp (disable_logging host) */
  const uint8_t *ip_bytes;      /* host: record r's IP (the Update key) is ip_bytes[ip_off[r], ip_off[r+1]) */
  const uint64_t *ip_off;       /* host, n_ips + 1 */
} bjx_ban_batch;
/* The last batch's emission (valid until the next batch; needs BJX_EMIT_BANS). */
int bjx_batch_bans(bjx_engine *e, bjx_ban_batch *out);

/* ---- Per-rule statistics of a batch (no counterpart in the reference, whose
   host could count inside its per-line loop; here the RuleResults exist only
   as per-line masks in HBM, so they are counted there and a few counters per
   rule come back).  A batch closed with BJX_RULE_STATS -- bjx_process_batch,
   bjx_finish_batch, bjx_finish_batch_trips and the node batch calls read the
   flag; bjx_match_batch ignores it -- also counts, per ruleset rule index,
   the RuleResults of the closing engine's own lines: every one (matches),
   those that were SkipHost and never reached Apply (skip_host; the rule's
   events are matches - skip_host) and those whose RateLimitResult came out
   Exceeded (trips; an event applied on another owner counts at the engine
   that matched the line, as its trip does).  The counts do not depend on
   BJX_COPY_RESULTS, BJX_EMIT_BANS or BJX_TRIPS_COMPACT.  A batch without any
   RuleResult, or of zero bytes, gives n_rules rows of zeros.

   bjx_batch_rule_stats: the last batch (n_batches 1); BJX_ERR_ARG when it ran
   without the flag.  bjx_rule_stats_total: the sum over every flagged batch
   since the ruleset came into use: the totals start over when a flagged batch
   runs with another ruleset than the flagged batch before it (rule indices
   mean nothing across rulesets); before any flagged batch, and after
   bjx_rule_stats_reset, n_rules 0 and rules NULL.  An unflagged batch changes
   neither the totals nor what they are keyed to.  The library checks on the
   host that the rows add up to the batch's n_results, n_events and n_trips
   (BJX_ERR_DEVICE "internal: ..." otherwise).  The calls take the engine lock;
   the node calls wait for the node batch and return the sum of the engines'
   arrays, device_ms the slowest engine's.  Without the flag a batch launches,
   allocates and copies nothing for this. */
typedef struct bjx_rule_stat {   /* 24 B, one per rule of the batch's ruleset, by ruleset rule index */
  uint64_t matches;    /* RuleResults of the rule (RegexMatch), SkipHost ones included */
  uint64_t skip_host;  /* of those, SkipHost: they never reached Apply; events = matches - skip_host */
  uint64_t trips;      /* of those, RateLimitResult.Exceeded */
} bjx_rule_stat;
typedef struct bjx_rule_stats {
  uint64_t n_rules;             /* bjx_ruleset_num_rules of the ruleset counted */
  const bjx_rule_stat *rules;   /* engine-owned (node-owned), valid until the next batch / next call of the same kind */
  uint64_t n_batches, n_lines;  /* batches and complete lines summed in (1 and the batch's n_lines for the last batch) */
  double device_ms;             /* HIP events around the counting alone; totals: summed */
} bjx_rule_stats;
int bjx_batch_rule_stats(bjx_engine *e, bjx_rule_stats *out);
int bjx_rule_stats_total(bjx_engine *e, bjx_rule_stats *out);
int bjx_rule_stats_reset(bjx_engine *e);

/* ---- Node: the GPUs of one host behind one handle.  The Go
   host keeps ONE RegexRateLimitStates (rate_limit.go:19-28, created once in
   banjax.go:80) fed by ONE consumer goroutine (regex_rate_limiter.go:54-77);
   a node keeps that shape over n_devices engines.  Engine k matches the k-th
   contiguous chunk of the batch, the rate-limit state is sharded by IP (owner
   (ip_hash >> 32) % n_devices), and the library moves the event records to
   their owners and the outcome bytes back itself (an RCCL all-to-all of
   ncclSend / ncclRecv pairs over xGMI when every engine has a GPU of its own,
   device-to-device copies when engines share a GPU; no caller collective).
   Results come back in the reference's global order, exactly as one engine
   over the whole batch returns them.  Env: BJX_NODE_EXCHANGE=peer|rccl forces
   the copies / RCCL (rccl: creation fails when it cannot be had). */
typedef struct bjx_node bjx_node;
/* devices: HIP device index of each engine (repeats allowed: engines sharing a GPU). */
int bjx_node_create(const int *devices, size_t n_devices, const bjx_engine_options *opts, bjx_node **out, char *err,
                    size_t err_len);
void bjx_node_destroy(bjx_node *n);
size_t bjx_node_size(const bjx_node *n);
/* Engine k of the node (its own stats and debug hooks); owned by the node. */
bjx_engine *bjx_node_engine(bjx_node *n, size_t k);
/* How the node moves its records: 1 RCCL, 0 device copies, -1 no node. */
int bjx_node_exchange_kind(const bjx_node *n);
const char *bjx_node_last_error(bjx_node *n);
/* bjx_engine_set_decision_lists / bjx_engine_set_ban_options on every engine. */
int bjx_node_set_decision_lists(bjx_node *n, const bjx_decision_entry *entries, size_t count);
int bjx_node_set_ban_options(bjx_node *n, const bjx_ban_options *opts);
/* consumeLine over the complete lines of a host buffer: split at '\n' into
   n_devices chunks of about equal size.  line_offset / line_idx in the result
   are relative to bytes, as bjx_process_batch's. */
int bjx_node_process_batch(bjx_node *n, const bjx_ruleset *rs, const uint8_t *bytes, size_t len, int64_t now_ns,
                           uint32_t flags, bjx_batch_result *out);
/* Same over chunks already resident in HBM: chunks[k] is a device pointer on
   engine k's GPU (flags must include BJX_INPUT_DEVICE) and every chunk but the
   last ends in '\n'.  Offsets are relative to the chunks' concatenation. */
int bjx_node_process_chunks(bjx_node *n, const bjx_ruleset *rs, const uint8_t *const *chunks, const size_t *lens,
                            int64_t now_ns, uint32_t flags, bjx_batch_result *out);
/* The last node batch's decision emission (BJX_EMIT_BANS), merged over the
   engines: one record per IP (highest decision, its first trip), trip_idx
   into the node batch's trips; log lines in node trip order. */
int bjx_node_batch_bans(bjx_node *n, bjx_ban_batch *out);
/* RegexRateLimitStates.Get / Len / String / occupancy over every shard. */
int bjx_node_state_get(bjx_node *n, const char *ip, size_t ip_len, const char *name, size_t name_len, int64_t *num_hits,
                       int64_t *interval_start_ns);
int64_t bjx_node_state_len(bjx_node *n);
size_t bjx_node_state_dump(bjx_node *n, char *out, size_t cap);
int bjx_node_state_stats_get(bjx_node *n, bjx_state_stats *out);
int bjx_node_state_clear(bjx_node *n);
/* bjx_state_expire on every shard with the same cutoff: counts and bytes
   summed, device_ms the slowest shard's.  out may be NULL. */
int bjx_node_state_expire(bjx_node *n, int64_t cutoff_ns, bjx_expire_stats *out);
/* Snapshot of the whole node: the shards' exports merged into one snapshot,
   IPs engine-major (engine 0's in its first-seen order, then engine 1's, ...:
   the order of bjx_node_state_dump); counts summed, device_ms the slowest
   shard's.  Import: engine k imports with part = k, n_parts = size, so a
   snapshot taken on any number of engines (or on one engine) restores into
   any other number; a failure leaves every engine empty.  Both wait for the
   node batch, as bjx_node_state_expire does.  Each engine uploads the whole
   snapshot and keeps its part. */
uint64_t bjx_node_state_export_bound(bjx_node *n);
int bjx_node_state_export(bjx_node *n, int64_t min_start_ns, uint8_t *out, uint64_t cap, uint64_t *len,
                          bjx_snapshot_stats *stats);
int bjx_node_state_import(bjx_node *n, const uint8_t *snap, uint64_t len, bjx_snapshot_stats *stats);
/* bjx_state_merge over the node (its contract is with bjx_state_merge): engine
   k merges part k of size, so o->part, o->n_parts must be 0, 1.  Counts and
   bytes summed, snap_* once, device_ms the slowest shard's.  Every shard is
   asked even when one fails; the first failure is returned, the shards done
   stay done, and the caller repeats the call (every policy is idempotent).
   Waits for the node batch.  out may be NULL. */
int bjx_node_state_merge(bjx_node *n, const uint8_t *snap, uint64_t len, const bjx_merge_options *o, bjx_merge_stats *out);
/* bjx_state_query over the node.  Every shard answers the same filter and
   limit and the host merges the answers: an IP lives on one engine and the
   global first-seen order is the engine-major order of bjx_node_state_dump, so
   the global first `limit` states are among the shards' first `limit` each.
   Counts are summed, device_ms is the slowest shard's.  With an ip filter only
   the owning engine is asked.  Waits for the node batch, as
   bjx_node_state_expire does; rows and bytes are node-owned until the next
   query on the node. */
int bjx_node_state_query(bjx_node *n, const bjx_state_filter *f, bjx_state_rows *out);
/* bjx_state_remove over the node.  Every engine gets the same filter and the
   whole list; an IP lives on one engine, so the sums are exact: counts and
   bytes summed, device_ms the slowest shard's.  Waits for the node batch, as
   bjx_node_state_expire does.  Every shard is asked even when one fails; the
   first failure is returned, and the shards already done stay done.  Removal
   is idempotent, so the caller repeats the call (the repeat's stats count
   what it still found).  out may be NULL. */
int bjx_node_state_remove(bjx_node *n, const bjx_state_filter *f, const bjx_str *ips, size_t n_ips, bjx_remove_stats *out);
/* bjx_state_query_nets / bjx_state_remove_nets over the node.  Every engine
   gets the same filter and nets (with an ip filter too).  Rows are merged as
   bjx_node_state_query merges them; net_ips and the removal's stats are
   summed, exactly, because an IP lives on one engine; device_ms is the slowest
   shard's.  net_ips is node-owned until the next query on the node.  Both wait
   for the node batch, as bjx_node_state_expire does.  On removal every shard
   is asked and the first failure is returned, as in bjx_node_state_remove. */
int bjx_node_state_query_nets(bjx_node *n, const bjx_state_filter *f, const bjx_str *nets, size_t n_nets,
                              bjx_state_rows *out, const uint64_t **net_ips);
int bjx_node_state_remove_nets(bjx_node *n, const bjx_state_filter *f, const bjx_str *nets, size_t n_nets,
                               bjx_remove_stats *out);
/* bjx_state_trim over the node.  The budget is per engine (each engine's HBM
   is its own); the node keeps one cutoff, so that the node as a whole "forgot
   everything before C".  Waits for the node batch, as bjx_node_state_expire
   does; runs the selection on every engine, takes C = the largest of their
   cutoffs and applies C on every engine (a trim with C as the floor and no
   bounds).  Counts and bytes are summed; cutoff_ns = C; bound is that of the
   engine that gave C (the lowest engine index among several); budget_met is
   the AND over the engines; select_ms and device_ms are the slowest engine's;
   states_dropped_live is counted against the caller's floor, not against C.
   A selection that fails on one engine is still run on the others and nothing
   is applied; when applying, every engine is asked even when one fails.  The
   first failure is returned and the call is idempotent, so the caller repeats
   it, as with bjx_node_state_remove.  out may be NULL. */
int bjx_node_state_trim(bjx_node *n, const bjx_trim_budget *b, bjx_trim_stats *out);
/* bjx_state_query_groups over the node.  A group spans engines (the owner of
   an IP is a hash of its bytes), so the shards' top rows do not determine the
   node's: every engine builds its complete group list in key order, the host
   merges the lists by key (counts and hits summed, the newest start the
   largest) and only then applies min_ips, the order and the limit -- a group
   below min_ips on every shard can still reach it in total.  The answer equals
   one engine over the union of the state.  n_matched, n_ips_matched and the
   unparsed counts are summed, device_ms is the slowest shard's.  When the
   shards' lists together hold more than 2^24 groups the call returns
   BJX_ERR_CAPACITY (use shorter prefixes or a narrower filter).  rows is
   node-owned until the next groups query on the node.  Waits for the node
   batch, as bjx_node_state_expire does. */
int bjx_node_state_query_groups(bjx_node *n, const bjx_state_filter *f, const bjx_group_spec *g, bjx_state_groups *out);
/* bjx_state_query_names over the node.  A name's states are spread over the
   engines (the owner of an IP is a hash of its bytes), so every engine gives
   the complete list of its names, the host merges the lists by name bytes
   (counts, hits_sum -- wrapping -- and hist added, max_hits and
   newest_start_ns the largest, oldest_start_ns the smallest) and only then
   applies min_states, the order and the limit: no per-shard limit cuts before
   the merge.  The answer equals one engine over the union of the state.
   n_matched and n_ips_matched are summed, device_ms is the slowest shard's.
   When the shards' lists together hold more than 2^20 names the call returns
   BJX_ERR_CAPACITY.  rows and bytes are node-owned until the next names query
   on the node.  Waits for the node batch, as bjx_node_state_expire does. */
int bjx_node_state_query_names(bjx_node *n, const bjx_state_filter *f, const bjx_names_spec *s, bjx_state_names *out);
/* bjx_batch_rule_stats / bjx_rule_stats_total / bjx_rule_stats_reset over the
   node: the engines' arrays summed (engine k counted chunk k's lines),
   n_lines summed, device_ms the slowest engine's (totals: those summed). */
int bjx_node_batch_rule_stats(bjx_node *n, bjx_rule_stats *out);
int bjx_node_rule_stats_total(bjx_node *n, bjx_rule_stats *out);
int bjx_node_rule_stats_reset(bjx_node *n);

int bjx_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* BANJAX_GPU_H */
