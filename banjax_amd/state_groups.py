"""Top networks by prefix (bjx_state_query_groups / bjx_node_state_query_groups)
in pure Python: executable documentation of the selection, of the group an IP
belongs to and of the order of the rows, and what the tests compute their
expected answers with.

Which states are selected is state_query.select's rule (ip, name, min_hits and
the start window; its order and limit play no part).  An IP is selected when
at least one of its states is.

The group of a selected IP: its bytes are parsed by state_nets.parse_ip
(net.ParseIP).  Text that does not parse is in no group and is counted as
unparsed.  A v4-mapped address -- dotted-quad text or ::ffff:a.b.c.d text -- is
IPv4 and is masked to v4_bits; every other address is IPv6 and is masked to
v6_bits.  The group is (family, masked address), the membership rule of the
nets calls: state_nets.Nets([row.net]) holds exactly the row's IPs.

A group carries n_ips (its selected IPs), n_states (their selected states),
hits_sum (the sum of those states' hits, wrapping as Go's int does) and
newest_start_ns (the largest interval_start_ns among them).  The rows are the
groups with n_ips >= min_ips, ordered by

    1. the primary key, descending: n_ips, n_states or hits_sum
    2. family 4 before family 6
    3. the masked address, bytewise ascending

which is total and depends on the logical state alone; the first `limit` of
them are returned.  A node answers as one engine over the union of its
engines' state would.
"""
from __future__ import annotations

import ipaddress
from collections import namedtuple

from . import state_query
from .state_nets import _V4_PREFIX, parse_ip

BY_IPS, BY_STATES, BY_HITS = 0, 1, 2
MAX_ROWS = 65536
NODE_MAX_GROUPS = 1 << 24
INT64_MIN, INT64_MAX = state_query.INT64_MIN, state_query.INT64_MAX

# addr: 16 bytes, IPv4 in addr[0:4] and the rest 0; net: text a nets call reads back to the same network
GroupRow = namedtuple("GroupRow", "net family bits addr n_ips n_states hits_sum newest_start_ns")


def group_of(ip, v4_bits: int, v6_bits: int):
    """-> (family 4 or 6, the masked address as 16 bytes laid out as GroupRow.addr), or None for text that is no address."""
    p = parse_ip(ip)
    if p is None:
        return None
    a16 = p[0]
    if a16[:12] == _V4_PREFIX:
        v = int.from_bytes(a16[12:], "big") & (((1 << v4_bits) - 1) << (32 - v4_bits))
        return 4, v.to_bytes(4, "big") + b"\0" * 12
    v = int.from_bytes(a16, "big") & (((1 << v6_bits) - 1) << (128 - v6_bits))
    return 6, v.to_bytes(16, "big")


def net_text(family: int, bits: int, addr: bytes) -> str:
    """"a.b.c.d/bits", or the compressed IPv6 form and "/bits": an entry of a nets call."""
    if family == 4:
        return "%d.%d.%d.%d/%d" % (addr[0], addr[1], addr[2], addr[3], bits)
    return "%s/%d" % (ipaddress.IPv6Address(bytes(addr)).compressed, bits)


def wrap64(v: int) -> int:
    """v as a Go int after wrapping addition"""
    return ((v + (1 << 63)) & ((1 << 64) - 1)) - (1 << 63)


def groups(ips_in_order, states, v4_bits: int = 24, v6_bits: int = 64, order: int = BY_IPS, limit: int = 100, min_ips: int = 0,
           ip=None, name=None, min_hits=INT64_MIN, min_start_ns=INT64_MIN, max_start_ns=INT64_MAX) -> dict:
    """ips_in_order, states: as state_query.select takes them; order: BY_IPS,
    BY_STATES, BY_HITS (or "ips" / "states" / "hits").  -> {"n_matched",
    "n_ips_matched", "n_ips_unparsed", "n_states_unparsed", "n_groups",
    "n_groups_min", "rows": [GroupRow]}."""
    order = {"ips": BY_IPS, "states": BY_STATES, "hits": BY_HITS}.get(order, order)
    if not 0 <= v4_bits <= 32 or not 0 <= v6_bits <= 128:
        raise ValueError("bits")
    if order not in (BY_IPS, BY_STATES, BY_HITS):
        raise ValueError("order")
    if not 0 <= limit <= MAX_ROWS:
        raise ValueError("limit")
    out = {"n_matched": 0, "n_ips_matched": 0, "n_ips_unparsed": 0, "n_states_unparsed": 0}
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
        key = group_of(i, v4_bits, v6_bits)
        if key is None:
            out["n_ips_unparsed"] += 1
            out["n_states_unparsed"] += n
            continue
        a = acc.setdefault(key, [0, 0, 0, INT64_MIN])
        a[0] += 1
        a[1] += n
        a[2] += sum(r[2] for r in rows)
        a[3] = max(a[3], max(r[3] for r in rows))
    rows = [GroupRow(net_text(fam, v4_bits if fam == 4 else v6_bits, addr), fam, v4_bits if fam == 4 else v6_bits, addr,
                     a[0], a[1], wrap64(a[2]), a[3]) for (fam, addr), a in acc.items()]
    out["n_groups"] = len(rows)
    rows = [r for r in rows if r.n_ips >= min_ips]
    out["n_groups_min"] = len(rows)
    primary = {BY_IPS: lambda r: r.n_ips, BY_STATES: lambda r: r.n_states, BY_HITS: lambda r: r.hits_sum}[order]
    rows.sort(key=lambda r: (-primary(r), r.family, r.addr))
    out["rows"] = rows[:limit]
    return out
