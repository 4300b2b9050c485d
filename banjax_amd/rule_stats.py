"""The per-rule statistics (bjx_batch_rule_stats / bjx_rule_stats_total) in
pure Python: executable documentation of what is counted, and what the tests
compute their expected answers with.

A RuleResult is one matched (line, rule) pair, as consumeLine reports it
(regex_rate_limiter.go:87-93, RegexMatch true).  Per ruleset rule index a batch
counts

    matches    every RuleResult of the rule, SkipHost ones included
    skip_host  of those, the ones whose host is in the rule's hosts_to_skip:
               they never reached RegexRateLimitStates.Apply, so the rule's
               events are matches - skip_host
    trips      of those, the ones whose RateLimitResult came out Exceeded

so sum(matches) is the batch's n_results, sum(matches - skip_host) its n_events
and sum(trips) its n_trips.  The totals are the element-wise sums over the
batches counted under one ruleset.

State is keyed by rule name, not by rule index: a global rule and a per-site
rule of one name feed the same (ip, name) state.  by_name folds the rows that
way, which is what a metrics line would print.
"""
from __future__ import annotations

import numpy as np

DTYPE = np.dtype([("matches", np.uint64), ("skip_host", np.uint64), ("trips", np.uint64)])


def _get(r, *names):
    for n in names:
        if isinstance(r, dict):
            if n in r:
                return r[n]
        elif hasattr(r, n):
            return getattr(r, n)
    raise AttributeError("a RuleResult needs one of %s" % (names,))


def count(results, n_rules: int):
    """results: RuleResults in any order, each anything (object or dict) with
    rule_idx or rule_id, skip_host and exceeded.  -> (matches, skip_host,
    trips), three uint64 arrays of n_rules entries."""
    m = np.zeros(n_rules, np.uint64)
    s = np.zeros(n_rules, np.uint64)
    t = np.zeros(n_rules, np.uint64)
    one = np.uint64(1)
    for r in results:
        i = int(_get(r, "rule_idx", "rule_id"))
        if not 0 <= i < n_rules:
            raise IndexError("rule index %d outside a ruleset of %d rules" % (i, n_rules))
        m[i] += one
        if _get(r, "skip_host"):
            s[i] += one
        if _get(r, "exceeded"):
            t[i] += one
    return m, s, t


def as_rows(matches, skip_host, trips):
    """The three arrays as the structured array Engine.rule_stats returns in "rules"."""
    rows = np.zeros(len(matches), DTYPE)
    rows["matches"], rows["skip_host"], rows["trips"] = matches, skip_host, trips
    return rows


def by_name(cfg, stats):
    """cfg: a Config; stats: what Engine.rule_stats returns, its "rules" array,
    or a (matches, skip_host, trips) triple, indexed like cfg.all_rules().
    -> {rule name: {"matches", "skip_host", "events", "trips"}} in first-seen
    rule order, rule indices of one name summed."""
    rows = stats["rules"] if isinstance(stats, dict) else stats
    if isinstance(rows, tuple):
        rows = as_rows(*rows)
    rules = cfg.all_rules()
    if len(rows) != len(rules):
        raise ValueError("%d rows for a config of %d rules" % (len(rows), len(rules)))
    out = {}
    for r, row in zip(rules, rows):
        d = out.setdefault(r.rule, {"matches": 0, "skip_host": 0, "events": 0, "trips": 0})
        d["matches"] += int(row["matches"])
        d["skip_host"] += int(row["skip_host"])
        d["events"] += int(row["matches"]) - int(row["skip_host"])
        d["trips"] += int(row["trips"])
    return out
