/*
 * banjax_gpu_debug.h — self-test hooks of libbanjax_gpu.so (not part of the
 * drop-in boundary; never used by bjx_process_batch).
 *
 * bjx_debug_rule_match_host evaluates one compiled rule's DFA or bit-parallel
 * NFA tables on the host, so the rule compiler can be checked against the oracle on machines
 * without a GPU.  The product matches on the GPU only.
 */
#ifndef BANJAX_GPU_DEBUG_H
#define BANJAX_GPU_DEBUG_H
#include <stddef.h>
#include <stdint.h>
#include "banjax_gpu.h"
#ifdef __cplusplus
extern "C" {
#endif
/* 1 match, 0 no match, <0 error */
int bjx_debug_rule_match_host(const bjx_ruleset *rs, size_t rule_idx, const uint8_t *text, size_t n);
/* required literal the prefilter uses for a rule (bytes written, full length returned) */
size_t bjx_debug_rule_literal(const bjx_ruleset *rs, size_t rule_idx, char *out, size_t cap);
/* Test hook (host only): how many literals a bind of this ruleset interns
   (prefilter literals, the host-free pieces of host-split ones, anchored
   prefixes).  At most 8: the scan keeps each literal's first candidate per
   line (Bind::cfirst); at most 32: a bit of the overflow summary names one
   literal (Bind::lits_small); ids are given in rule order. */
size_t bjx_debug_ruleset_literals(const bjx_ruleset *rs);
/* a prefilter rule whose every match begins within a bounded distance of its
   literals (its DFA jobs start near the first hit): that distance in bytes;
   -1 for every other rule */
int bjx_debug_rule_lead(const bjx_ruleset *rs, size_t rule_idx);
/* Test hook: regexp/syntax's parse of one pattern alone (accept / refuse and
   Go's error text, e.g. the "expression too large" limits), no automaton. */
int bjx_debug_regex_parse(const char *pattern, size_t len, char *err, size_t err_len);
/* device ms of the last batch's phases: framing count, scan, per-line resolve,
   emit, capacity check, IP/state slot claim, sort + automaton, trips; then the
   node exchange as this engine saw it (bjx_events_partition to the start of
   its owner's rate-limit stage: partition, pack, the wait for the copies,
   unpack; 0 for a batch without one), which the capacity phase of a node
   batch contains (returns 9) */
size_t bjx_debug_phase_ms(bjx_engine *e, double *out, size_t cap);
/* device ms of the last batch's dominant kernels, from HIP events on the
   engine stream: k_scan, the per-line kernel, DFA-job sort + k_dfa / k_nfa;
   then which per-line kernel ran (2 = k_lines2, 1 = k_lines, 3 = the wide
   per-line kernel k_parse_match on every line: rulesets of more than 128
   global rules) and its window bytes per line (k_lines2) or staging bytes per
   wave (k_lines), 0 for k_parse_match (returns 5) */
size_t bjx_debug_kernel_ms(bjx_engine *e, double *out, size_t cap);
/* last batch: gram bitset hits, recorded literal hits, lines sent to the per-line
   fallback, bytes of the scan's LDS image, DFA jobs; then the state
   tables: IP slots, IPs, state slots, states; then gram table hits, the
   rate-limit grouping (0: full sort by state slot; else two-level, 1 + the
   events of its oversized buckets), rate-limit runs that crossed a k_apply
   chunk (k_long_runs), the bytes of the event records the rate-limit stage
   sorted (8, 12 or 16) (returns the count, 13) */
size_t bjx_debug_scan_stats(bjx_engine *e, uint64_t *out, size_t cap);
/* Test hook: IP hashes become (hash & mask) | 1 (0 = off), so distinct IPs
   share 64-bit hashes and the exact collision path of the IP table runs. */
int bjx_debug_set_ip_hash_mask(bjx_engine *e, uint64_t mask);
/* Test hook: the first claim launch of each table in a batch may add at most
   max_new entries (0 = off), forcing the roll-back / re-claim path. */
int bjx_debug_set_claim_budget(bjx_engine *e, uint64_t max_new);
/* Test hook: the per-IP state-slot cache of k_st_claim on (1), off (0) or as
   BJX_SLOT_CACHE / the default says (-1), from the next batch on. */
int bjx_debug_set_slot_cache(bjx_engine *e, int on);
/* Test hook (host side): the two-level grouping of the rate-limit stage uses
   `bits` high state-slot bits, from the next batch on: 2^bits buckets of
   2^L slots, L = log2(state slots) - bits.  0 = the default 16; 1..16 are
   accepted, anything else is BJX_ERR_ARG.  The grouping still needs
   0 < L <= 15 (otherwise the full sort runs and scan_stats' grouping is 0), so
   with the default 2^22-slot table bits 16..7 give L = 6..15: every L
   k_bucket_apply can run at without a table of 2^(16 + L) slots.  Unused, the
   same kernels run with the same arguments as without the hook. */
int bjx_debug_set_bucket_bits(bjx_engine *e, uint32_t bits);
/* Test hook: the 8-byte event records are tried only for batches of at most
   max_events rate-limit events (0 = the default, the 2^28 of the record's
   event index field; more is BJX_ERR_ARG), from the next batch on. */
int bjx_debug_set_rec8_max_events(bjx_engine *e, uint64_t max_events);
/* Test hook (host only, no device): one event record of `form` bytes (8, 12 or
   16) made from (ts, rule, first, ev) against `base` (ms for the 8-byte form, ns
   for the 12-byte one, unused at 16) by the functions the kernels use.
   out[0..4]: fits(ts, base), time(base), rule_id(), seen(), and the event index
   read as the kernels after the sort read it (its word of the record and a
   mask).  A record made of values that do not fit holds garbage, as on the
   device, where the batch is claimed again.  bjx_debug_event_record_bits:
   out[0..2] = the form's timestamp, rule and event index field widths. */
int bjx_debug_event_record(uint32_t form, int64_t ts, uint32_t rule, int first, uint32_t ev, int64_t base, int64_t *out);
int bjx_debug_event_record_bits(uint32_t form, uint32_t *out);
/* Test hook: the counting passes of bjx_state_trim (over the state table and
   over the per-IP newest starts) launch at most max_blocks blocks (0 = the
   default cap), so that their grid-stride loops wrap on small inputs. */
int bjx_debug_set_trim_grid(bjx_engine *e, uint32_t max_blocks);
/* The number of sorted keys one block of bjx_state_query_groups' run reduction
   (k_grp_runs) handles: the tests place group sizes and boundaries around it. */
uint32_t bjx_debug_groups_tile(void);
/* Test hook: bjx_state_query_names keeps its per-name bins in LDS only while
   the engine has interned at most max_lds_names names (0 = default, what the
   LDS a block may have holds; a larger value changes nothing), and its pass
   over the state table launches at most max_blocks blocks (0 = the default
   cap), so that small inputs reach both paths, the exact boundary and one
   block that walks the whole table. */
int bjx_debug_set_names(bjx_engine *e, uint32_t max_lds_names, uint32_t max_blocks);
/* *path: where the engine's last bjx_state_query_names binned: 1 LDS, 2 the
   global records, 0 nothing was launched.  *lds_names_max: the most interned
   names the LDS path takes without the hook.  Either may be NULL. */
int bjx_debug_names_info(bjx_engine *e, int *path, uint32_t *lds_names_max);
/* Test hook: the state-table slot index each of n (IP, rule name) states
   occupies, found as bjx_state_get finds it (hash, probe chain, IP bytes,
   then the state's key), in one launch for the whole list; -1 where there is
   no such state.  IP k is ip_bytes[ip_off[k], ip_off[k + 1]) (ip_off has
   n + 1 entries and starts at 0; the packed list of bjx_state_remove), its
   name is names[name_idx[k]].  Writes nothing in the engine.  A state keeps
   its slot until the tables are rebuilt (growth, expire, remove, import,
   clear): bjx_state_stats' state_slots and rehashes tell. */
int bjx_debug_state_slots(bjx_engine *e, const uint8_t *ip_bytes, const uint32_t *ip_off, const bjx_str *names,
                          size_t n_names, const uint32_t *name_idx, size_t n, int64_t *slots);
/* Test hook: rules compiled afterwards use the bit-parallel NFA once their DFA
   passes `cap` states (0 = default 4096; 1 = every rule that fits the NFA),
   process-wide; clears the compiled-pattern cache. */
int bjx_debug_set_dfa_state_cap(uint32_t cap);
/* Test hook: rules compiled afterwards (on != 0) go straight to the wide
   block-cooperative NFA (kRuleNfaWide), process-wide; clears the
   compiled-pattern cache. */
int bjx_debug_force_wide_nfa(int on);
/* Test hook: BJX_RULE_STATS bins in LDS only for rulesets of at most max_rules
   rules (0 = default, the LDS a block may have); past it the counting kernels
   add straight to the global counters. */
int bjx_debug_set_rule_stats_lds(bjx_engine *e, uint32_t max_rules);
/* where the engine's last BJX_RULE_STATS batch binned: 1 LDS, 2 the global
   counters, 0 nothing was launched (no results) */
int bjx_debug_rule_stats_path(bjx_engine *e);
/* Test hook: what the DFA job stage of the engine's last batch (the last one
   that held a complete line) saw.  For each of the n_rules rules of that
   batch's ruleset (any other n_rules is BJX_ERR_ARG): its sorted jobs under the windowed key r (k_dfa's) and under
   the legacy key n_rules + r (k_dfa_legacy's, k_nfa's, k_nfa_wide's); their
   sum over the rules is bjx_debug_scan_stats' DFA jobs.  line_pass_runs (may be
   null): how often the per-line pass ran, 1, or 2 when the job buffers grew.
   Computed on demand from the sorted keys the batch left on the device (one
   k_rule_bounds launch); a batch that does not call it runs the same kernels
   with the same arguments as without the hook. */
int bjx_debug_job_counts(bjx_engine *e, uint32_t *windowed, uint32_t *legacy, size_t n_rules, uint32_t *line_pass_runs);
#ifdef __cplusplus
}
#endif
#endif
