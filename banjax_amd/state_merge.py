"""bjx_state_merge in pure Python: executable documentation, and what the
tests compute their expected snapshots and counts with.

merge(engine_blob, snap_blob, ...) takes the engine's state as its export and
returns the snapshot an engine would have to import to equal the merged one
(include/banjax_gpu.h: "Equivalence"), with the counts of bjx_merge_stats that
follow from the two states alone.

A key is (IP bytes, rule name bytes).  From the snapshot count the records of
the IPs the part owns ((hash_bytes(ip) >> 32) % n_parts == part) whose start is
at or after min_start_ns.  A key both sides hold goes by the policy:
    NEWER    the larger (start, hits) wins, compared as a pair of signed ints
    KEEP     the engine's record stays
    REPLACE  the snapshot's record wins
The engine's IPs keep their order; a snapshot IP the engine does not hold that
brings a record follows them, in snapshot order.
"""
from __future__ import annotations

from . import snapshot

NEWER, KEEP, REPLACE = 0, 1, 2
INT64_MIN = -(1 << 63)
_M32 = 0xFFFFFFFF


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & _M32


def hash_bytes(p: bytes) -> int:
    """bjx::hash_bytes (banjax_amd/csrc/bjx_common.h), restated: the owner of an IP is (hash >> 32) % n_parts."""
    n = len(p)
    a, b = 0x9E3779B9 ^ n, (0x7F4A7C15 + n * 0x85EBCA6B) & _M32
    i = 0
    while i + 4 <= n:
        w = int.from_bytes(p[i:i + 4], "little")
        a = (_rotl(a ^ w, 7) * 0x27D4EB2D) & _M32
        b = (_rotl((b + w) & _M32, 13) * 0x165667B1) & _M32
        i += 4
    t = int.from_bytes(p[i:], "little")
    a = (_rotl(a ^ t ^ 0xA5A5A5A5, 7) * 0x27D4EB2D) & _M32
    b = (_rotl((b + t) & _M32, 13) * 0x165667B1) & _M32
    a ^= b >> 16; a = (a * 0x85EBCA6B) & _M32; a ^= a >> 13; a = (a * 0xC2B2AE35) & _M32; a ^= a >> 16
    b ^= a >> 15; b = (b * 0x2C1B3C6D) & _M32; b ^= b >> 12; b = (b * 0x297A2D39) & _M32; b ^= b >> 15
    h = (a << 32) | b
    return 0x1234567 if h in (0, (1 << 64) - 1) else h


def owner(ip: bytes, n_parts: int) -> int:
    return (hash_bytes(ip) >> 32) % n_parts


def wins(policy: int, mine, theirs) -> bool:
    """Does the snapshot's (hits, start) replace the engine's?  Equal records never do."""
    if policy == KEEP or mine == theirs:
        return False
    if policy == REPLACE:
        return True
    if policy != NEWER:
        raise ValueError("unknown policy")
    return (theirs[1], theirs[0]) > (mine[1], mine[0])


def merge_states(ips, states, snap_ips, snap_states, policy=NEWER, min_start_ns=INT64_MIN, part=0, n_parts=1):
    """The same on parsed states (snapshot.parse's pair): -> (ips, states, stats)."""
    if not (1 <= n_parts <= 256 and 0 <= part < n_parts):
        raise ValueError("part / n_parts out of range")
    out_ips = list(ips)
    out = {ip: dict(d) for ip, d in states.items()}
    s = dict(snap_ips=len(snap_ips), snap_states=sum(len(d) for d in snap_states.values()),
             snap_names=len({n for d in snap_states.values() for n in d}),
             ips_before=len(ips), ips_added=0, ips_skipped=0, states_before=sum(len(d) for d in states.values()),
             states_added=0, states_replaced=0, states_kept=0, states_skipped=0,
             arena_bytes_before=sum(len(ip) for ip in ips))
    for ip in snap_ips:
        recs = snap_states[ip]
        if owner(ip, n_parts) != part:
            s["ips_skipped"] += 1
            s["states_skipped"] += len(recs)
            continue
        brought = 0
        for name in sorted(recs):
            rec = recs[name]
            if rec[1] < min_start_ns:
                s["states_skipped"] += 1
                continue
            brought += 1
            held = out.get(ip)
            if held is None:
                out[ip] = held = {}
                out_ips.append(ip)
                s["ips_added"] += 1
            if name not in held:
                held[name] = rec
                s["states_added"] += 1
            elif wins(policy, held[name], rec):
                held[name] = rec
                s["states_replaced"] += 1
            else:
                s["states_kept"] += 1
        if not brought:
            s["ips_skipped"] += 1
    s["arena_bytes_after"] = sum(len(ip) for ip in out_ips)
    return out_ips, out, s


def merge(engine_blob: bytes, snap_blob: bytes, policy=NEWER, min_start_ns=INT64_MIN, part=0, n_parts=1):
    """-> (merged_blob, stats): the snapshot of the merged engine and the
    bjx_merge_stats fields that do not depend on table sizes or timing."""
    ips, states = snapshot.parse(engine_blob)
    snap_ips, snap_states = snapshot.parse(snap_blob)
    out_ips, out, s = merge_states(ips, states, snap_ips, snap_states, policy, min_start_ns, part, n_parts)
    s["snap_bytes"] = len(snap_blob)
    return snapshot.build(out_ips, out), s
