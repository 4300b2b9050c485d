"""The state query (bjx_state_query / bjx_node_state_query) in pure Python:
executable documentation of the filter and the order, and what the tests
compute their expected answers with.

A state is (ip, rule name, hits, interval_start_ns).  It passes the filter when

    ip   is None or equals the state's IP bytes        (b"" is a value)
    name is None or equals the state's rule name bytes (b"" is a value)
    hits >= min_hits and min_start_ns <= interval_start_ns <= max_start_ns

The passing states are ordered by

    1. the primary key, descending: hits (BY_HITS) or interval_start_ns (BY_START)
    2. the IP's position in first-seen order, ascending (the order of
       bjx_state_dump and of a snapshot's IPs; for a node, engine-major)
    3. the rule name, bytewise ascending (a prefix before the longer name)

which is total -- (IP, name) is unique -- and depends on the logical state
alone: not on slot layout, table sizes, the ids names were interned under or
the debug hash mask.  The answer is the number of passing states, the number
of distinct IPs among them and the first min(limit, n_matched) of them.

With nets (bjx_state_query_nets; entries and membership: state_nets.py) a state
passes only when its IP lies in one of the networks, and the answer gains
net_ips: per entry, in the order given, the distinct IPs inside it that have a
passing state.
"""
from __future__ import annotations

BY_HITS, BY_START = 0, 1
MAX_ROWS = 65536
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def _b(x) -> bytes:
    return x if isinstance(x, bytes) else str(x).encode()


def select(ips_in_order, states, ip=None, name=None, min_hits=INT64_MIN, min_start_ns=INT64_MIN,
           max_start_ns=INT64_MAX, order=BY_HITS, limit=0, nets=None):
    """ips_in_order, states: what snapshot.parse returns (or the arguments of
    snapshot.build): the IPs in first-seen order and {ip: {rule name: (hits,
    start_ns)}}.  -> (n_matched, n_ips_matched, [(ip, name, hits, start_ns)])
    with ip and name as bytes; with nets (not None: a list of entries) a
    fourth element, net_ips."""
    from .state_nets import Nets
    table = None if nets is None else Nets(nets)
    if order not in (BY_HITS, BY_START):
        raise ValueError("order")
    if not 0 <= limit <= MAX_ROWS:
        raise ValueError("limit")
    want_ip = None if ip is None else _b(ip)
    want_name = None if name is None else _b(name)
    states = {_b(i): {_b(n): v for n, v in d.items()} for i, d in states.items()}
    passing, seen = [], set()
    for pos, i in enumerate(_b(x) for x in ips_in_order):
        if i in seen:
            continue
        seen.add(i)
        if want_ip is not None and i != want_ip:
            continue
        if table is not None and not table.holds(i):
            continue
        for n, (hits, start) in states.get(i, {}).items():
            if want_name is not None and n != want_name:
                continue
            if hits >= min_hits and min_start_ns <= start <= max_start_ns:
                passing.append((-(start if order == BY_START else hits), pos, n, i, hits, start))
    passing.sort(key=lambda t: t[:3])
    rows = [(i, n, hits, start) for _, _, n, i, hits, start in passing[:limit]]
    if table is None:
        return len(passing), len({t[1] for t in passing}), rows
    net_ips = [0] * len(table.entries)
    for i in {t[3] for t in passing}:
        for k in table.which(i):
            net_ips[k] += 1
    return len(passing), len({t[1] for t in passing}), rows, net_ips
