"""Per-rule-name totals over the state (bjx_state_query_names /
bjx_node_state_query_names) in pure Python: executable documentation of the
selection, of the totals and the histogram buckets, of the wrap and of the
order of the rows, and what the tests compute their expected answers with.

Which states are selected is state_query.select's rule (ip, name, min_hits and
the start window; its order and limit play no part).  A name with no selected
state has no row.

A row carries, over the selected states under its name: n_states (which is
also the number of distinct IPs holding one: (ip, name) is unique), hits_sum
(wrapping as Go's int does), max_hits, newest_start_ns, oldest_start_ns and
hist, the states counted by their hits:

    bucket 0        hits <= 0
    bucket b, 1..14 hits of bit length b: 2^(b-1) <= hits < 2^b
    bucket 15       hits >= 2^14

The rows are the names with n_states >= min_states, ordered by

    1. the primary key, descending: n_states, hits_sum, max_hits or
       newest_start_ns; BY_NAME has none
    2. the name, bytewise ascending (a prefix before the longer name)

which is total and depends on the logical state alone; the first `limit` of
them are returned.  A node answers as one engine over the union of its
engines' state would.
"""
from __future__ import annotations

from collections import namedtuple

from . import state_query

BY_STATES, BY_HITS, BY_MAX_HITS, BY_NEWEST, BY_NAME = 0, 1, 2, 3, 4
ORDERS = {"states": BY_STATES, "hits": BY_HITS, "max_hits": BY_MAX_HITS, "newest": BY_NEWEST, "name": BY_NAME}
MAX_ROWS = 65536
HIST = 16
NODE_MAX_NAMES = 1 << 20
INT64_MIN, INT64_MAX = state_query.INT64_MIN, state_query.INT64_MAX

# name: bytes; hist: a tuple of HIST counts
NameRow = namedtuple("NameRow", "name n_states hits_sum max_hits newest_start_ns oldest_start_ns hist")


def bucket(hits: int) -> int:
    """the histogram bucket of a hit count"""
    return 0 if hits <= 0 else min(hits.bit_length(), HIST - 1)


def wrap64(v: int) -> int:
    """v as a Go int after wrapping addition"""
    return ((v + (1 << 63)) & ((1 << 64) - 1)) - (1 << 63)


def names(ips_in_order, states, order=BY_STATES, limit: int = 100, min_states: int = 0, ip=None, name=None,
          min_hits=INT64_MIN, min_start_ns=INT64_MIN, max_start_ns=INT64_MAX) -> dict:
    """ips_in_order, states: as state_query.select takes them; order: BY_STATES,
    BY_HITS, BY_MAX_HITS, BY_NEWEST, BY_NAME (or a key of ORDERS).  ->
    {"n_matched", "n_ips_matched", "n_names", "n_names_min", "rows": [NameRow]}."""
    order = ORDERS.get(order, order)
    if order not in ORDERS.values():
        raise ValueError("order")
    if not 0 <= limit <= MAX_ROWS:
        raise ValueError("limit")
    out = {"n_matched": 0, "n_ips_matched": 0}
    acc, seen = {}, set()
    for i in ips_in_order:
        if i in seen:
            continue
        seen.add(i)
        # one IP at a time: select's rows are then all of its passing states
        n, _, rows = state_query.select([i], {i: states.get(i, {})}, ip=ip, name=name, min_hits=min_hits,
                                        min_start_ns=min_start_ns, max_start_ns=max_start_ns, limit=state_query.MAX_ROWS)
        if not n:
            continue
        assert n == len(rows)
        out["n_matched"] += n
        out["n_ips_matched"] += 1
        for _, nm, hits, start in rows:
            a = acc.setdefault(nm, [0, 0, INT64_MIN, INT64_MIN, INT64_MAX, [0] * HIST])
            a[0] += 1
            a[1] += hits
            a[2] = max(a[2], hits)
            a[3] = max(a[3], start)
            a[4] = min(a[4], start)
            a[5][bucket(hits)] += 1
    rows = [NameRow(nm, a[0], wrap64(a[1]), a[2], a[3], a[4], tuple(a[5])) for nm, a in acc.items()]
    out["n_names"] = len(rows)
    rows = [r for r in rows if r.n_states >= min_states]
    out["n_names_min"] = len(rows)
    primary = {BY_STATES: lambda r: r.n_states, BY_HITS: lambda r: r.hits_sum, BY_MAX_HITS: lambda r: r.max_hits,
               BY_NEWEST: lambda r: r.newest_start_ns, BY_NAME: lambda r: 0}[order]
    rows.sort(key=lambda r: (-primary(r), r.name))
    out["rows"] = rows[:limit]
    return out


def orphans(rows, current_rule_names):
    """The rows whose name no current rule has: what a host removes after a
    reload (state_remove(name=row.name) for each).  current_rule_names: str or
    bytes."""
    have = {state_query._b(n) for n in current_rule_names}
    return [r for r in rows if r.name not in have]
