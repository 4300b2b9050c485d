"""The state removal (bjx_state_remove / bjx_node_state_remove) in pure Python:
executable documentation of which states go, and what the tests compute their
expected state and counts with.

A state is (ip, rule name, hits, interval_start_ns).  It is dropped when it
passes the filter as state_query.select reads it

    ip   is None or equals the state's IP bytes        (b"" is a value)
    name is None or equals the state's rule name bytes (b"" is a value)
    hits >= min_hits and min_start_ns <= interval_start_ns <= max_start_ns

and, when a list is given (ips is not None and not empty), its IP is one of the
listed ones, compared by bytes.  The list and the filter mean both, so ip
together with a list selects only when that IP is listed.  Duplicates in the
list and listed IPs that are not held change nothing.  Every IP left without a
state goes too; the others keep their relative order.

With nets (bjx_state_remove_nets; entries and membership: state_nets.py) "its
IP lies in one of the networks" takes the list's place, and ips_found counts
the held IPs inside any network.
"""
from __future__ import annotations

from .state_query import INT64_MAX, INT64_MIN, _b


def remove(ips_in_order, states, ips=None, ip=None, name=None, min_hits=INT64_MIN, min_start_ns=INT64_MIN,
           max_start_ns=INT64_MAX, nets=None):
    """ips_in_order, states: what snapshot.parse returns (or the arguments of
    snapshot.build): the IPs in first-seen order and {ip: {rule name: (hits,
    start_ns)}}.  -> (surviving ips_in_order, surviving states, counts), IPs
    and names as bytes; counts has the bjx_remove_stats fields that follow from
    the logical state: states_before, states_dropped, ips_before, ips_dropped,
    ips_found, arena_bytes_before, arena_bytes_after.  nets (not None: a list
    of entries) and ips exclude each other."""
    from .state_nets import Nets
    if nets is not None and ips is not None:
        raise ValueError("ips and nets together")
    table = None if nets is None else Nets(nets)
    want_ip = None if ip is None else _b(ip)
    want_name = None if name is None else _b(name)
    listed = None if not ips else {_b(x) for x in ips}
    states = {_b(i): {_b(n): tuple(v) for n, v in d.items()} for i, d in states.items()}
    order, seen = [], set()
    for i in (_b(x) for x in ips_in_order):
        if i not in seen and states.get(i):
            seen.add(i)
            order.append(i)
    kept_ips, kept = [], {}
    n_before = n_kept = 0
    in_net = set() if table is None else {i for i in order if table.holds(i)}
    for i in order:
        ip_ok = (want_ip is None or i == want_ip) and (listed is None or i in listed) and (table is None or i in in_net)
        d = {}
        for n, (hits, start) in states[i].items():
            n_before += 1
            if ip_ok and (want_name is None or n == want_name) and hits >= min_hits and min_start_ns <= start <= max_start_ns:
                continue
            d[n] = (hits, start)
        if d:
            kept_ips.append(i)
            kept[i] = d
            n_kept += len(d)
    counts = {
        "states_before": n_before, "states_dropped": n_before - n_kept,
        "ips_before": len(order), "ips_dropped": len(order) - len(kept_ips),
        "ips_found": len(in_net) if table is not None else 0 if listed is None else sum(1 for i in order if i in listed),
        "arena_bytes_before": sum(len(i) for i in order), "arena_bytes_after": sum(len(i) for i in kept_ips),
    }
    return kept_ips, kept, counts
