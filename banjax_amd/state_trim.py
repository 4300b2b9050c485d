"""The budgeted trim (bjx_state_trim / bjx_node_state_trim) in pure Python:
executable documentation of which cutoff a budget gives and what then goes, and
what the tests compute their expected state and stats with.

A state is (ip, rule name, hits, interval_start_ns).  For a multiset V of int64
and a bound k, cut(V, k) is the smallest C with #{v in V : v >= C} <= k:

    INT64_MIN                     when k == 0 (no bound) or |V| <= k
    v + 1, saturating at INT64_MAX  for the (k + 1)-th largest value v of V

The trim's cutoff is C = max(floor_cutoff_ns, C_states, C_ips) with

    C_states = cut(the starts of all states, max_states)
    C_ips    = cut({the newest start of each IP}, max_ips)

and the trim is the expiry at C: every state with start < C goes, every IP
left without a state goes too, the others keep their relative order
(state_remove.remove with max_start_ns = C - 1).  States that share a start go
or stay together, so fewer than the budget may stay.  When more than k values
equal INT64_MAX the cut saturates: C = INT64_MAX, those states stay and
budget_met is 0.

bound names what set C: BY_IPS if C_ips == C and C_ips > INT64_MIN, else
BY_STATES if C_states == C and C_states > INT64_MIN, else BY_FLOOR if the floor
is above INT64_MIN, else BY_NONE.  states_dropped_live counts the dropped states
with start >= floor_cutoff_ns: with the expiry's trip-transparent cutoff as the
floor, the evictions that can change a later result.

A node trims every engine at one cutoff, the largest of the engines' own
(node_trim): the budget is per engine, the cutoff the node's.
"""
from __future__ import annotations

from .state_query import INT64_MAX, INT64_MIN, _b
from .state_remove import remove

BY_NONE, BY_FLOOR, BY_STATES, BY_IPS = 0, 1, 2, 3
DRY_RUN = 1


def cut(values, k):
    """-> (C, saturated)"""
    if k == 0 or len(values) <= k:
        return INT64_MIN, False
    v = sorted(values, reverse=True)[k]
    return (INT64_MAX, True) if v == INT64_MAX else (v + 1, False)


def pick(ips_in_order, states, max_states=0, max_ips=0, floor_cutoff_ns=INT64_MIN):
    """The selection alone -> (C, bound, budget_met)."""
    held = [d for d in states.values() if d]
    c_st, sat_st = cut([s[1] for d in held for s in d.values()], max_states)
    c_ip, sat_ip = cut([max(s[1] for s in d.values()) for d in held], max_ips)
    c = max(floor_cutoff_ns, c_st, c_ip)
    if c_ip == c and c_ip > INT64_MIN:
        bound = BY_IPS
    elif c_st == c and c_st > INT64_MIN:
        bound = BY_STATES
    else:
        bound = BY_FLOOR if floor_cutoff_ns > INT64_MIN else BY_NONE
    return c, bound, int(not (sat_st or sat_ip))


def apply(ips_in_order, states, cutoff_ns, live_floor_ns):
    """The expiry at cutoff_ns -> (surviving ips_in_order, surviving states,
    counts): the bjx_trim_stats fields that follow from the logical state,
    states_dropped_live counted against live_floor_ns."""
    if cutoff_ns > INT64_MIN:
        kept_ips, kept, c = remove(ips_in_order, states, max_start_ns=cutoff_ns - 1)
    else:
        kept_ips, kept, c = remove(ips_in_order, states, min_start_ns=1, max_start_ns=0)  # an empty window: nothing goes
    live = sum(1 for d in states.values() for s in d.values() if live_floor_ns <= s[1] < cutoff_ns)
    counts = {k: c[k] for k in ("states_before", "states_dropped", "ips_before", "ips_dropped", "arena_bytes_before",
                                "arena_bytes_after")}
    counts["states_dropped_live"] = live
    return kept_ips, kept, counts


def trim(ips_in_order, states, max_states=0, max_ips=0, floor_cutoff_ns=INT64_MIN):
    """ips_in_order, states: what snapshot.parse returns (or the arguments of
    snapshot.build): the IPs in first-seen order and {ip: {rule name: (hits,
    start_ns)}}.  -> (surviving ips_in_order, surviving states, stats), IPs and
    names as bytes; stats has the bjx_trim_stats fields that follow from the
    logical state: cutoff_ns, bound, budget_met, states_before, states_dropped,
    states_dropped_live, ips_before, ips_dropped, arena_bytes_before,
    arena_bytes_after."""
    c, bound, met = pick(ips_in_order, states, max_states, max_ips, floor_cutoff_ns)
    kept_ips, kept, stats = apply(ips_in_order, states, c, floor_cutoff_ns)
    stats.update(cutoff_ns=c, bound=bound, budget_met=met)
    return kept_ips, kept, stats


def node_trim(parts, max_states=0, max_ips=0, floor_cutoff_ns=INT64_MIN):
    """parts: [(ips_in_order, states)] per engine.  -> ([(surviving ips,
    surviving states)] per engine, the node's stats): one cutoff, the largest
    of the engines'; bound from the first engine that gave it; budget_met the
    AND; counts summed."""
    picked = [pick(i, s, max_states, max_ips, floor_cutoff_ns) for i, s in parts]
    c = max(p[0] for p in picked)
    bound = next(p[1] for p in picked if p[0] == c)
    total, out = {}, []
    for i, s in parts:
        kept_ips, kept, counts = apply(i, s, c, floor_cutoff_ns)
        out.append((kept_ips, kept))
        for k, v in counts.items():
            total[k] = total.get(k, 0) + v
    total.update(cutoff_ns=c, bound=bound, budget_met=int(all(p[2] for p in picked)))
    return out, total


__all__ = ["cut", "pick", "apply", "trim", "node_trim", "BY_NONE", "BY_FLOOR", "BY_STATES", "BY_IPS", "DRY_RUN", "_b"]
