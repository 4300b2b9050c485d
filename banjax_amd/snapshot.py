"""The state snapshot format (bjx_state_export / bjx_state_import), version 1,
in pure Python: executable documentation, and what the tests compute their
expected bytes with.

Little-endian.  Header, 64 bytes:
    magic[8] = b"BJXSTATE", u32 version = 1, u32 header_bytes = 64,
    u64 total_bytes, n_names, names_bytes, n_ips, ip_bytes, n_states
then five sections, each padded with zeros to 8 bytes:
    u64 name_off[n_names + 1] | name bytes | u64 ip_off[n_ips + 1] | IP bytes |
    n_states records {u32 ip, u32 name, i64 hits, i64 start}
Canonical form: names sorted bytewise, distinct, each used by a record; every
IP has a record; records strictly ascending by (ip, name).  The bytes follow
from the logical state and the order of the IPs alone.
"""
from __future__ import annotations

import struct

MAGIC = b"BJXSTATE"
VERSION, HEADER_BYTES, REC_BYTES = 1, 64, 24
_HDR = struct.Struct("<8sII6Q")
_REC = struct.Struct("<IIqq")


def _b(x) -> bytes:
    return x if isinstance(x, bytes) else str(x).encode()


def _pad8(b: bytes) -> bytes:
    return b + b"\0" * (-len(b) % 8)


def layout(n_names, names_bytes, n_ips, ip_bytes, n_states):
    """Section offsets: (name_off, names, ip_off, ips, records, total)."""
    o_name_off = HEADER_BYTES
    o_names = o_name_off + 8 * (n_names + 1)
    o_ip_off = o_names + (names_bytes + 7) // 8 * 8
    o_ips = o_ip_off + 8 * (n_ips + 1)
    o_recs = o_ips + (ip_bytes + 7) // 8 * 8
    return o_name_off, o_names, o_ip_off, o_ips, o_recs, o_recs + REC_BYTES * n_states


def build(ips_in_order, states) -> bytes:
    """ips_in_order: the IPs (str or bytes) in snapshot order; states: {ip:
    {rule name: (hits, start_ns)}}.  IPs without a state are left out."""
    states = {_b(ip): {_b(n): v for n, v in d.items()} for ip, d in states.items()}
    ips = [_b(ip) for ip in ips_in_order if states.get(_b(ip))]
    names = sorted({n for ip in ips for n in states[ip]})
    idx = {n: k for k, n in enumerate(names)}
    recs = []
    for i, ip in enumerate(ips):
        for n in sorted(states[ip]):
            hits, start = states[ip][n]
            recs.append(_REC.pack(i, idx[n], hits, start))

    def offs(items):
        out, t = [0], 0
        for x in items:
            t += len(x)
            out.append(t)
        return struct.pack("<%dQ" % len(out), *out)

    nb, ib = b"".join(names), b"".join(ips)
    total = layout(len(names), len(nb), len(ips), len(ib), len(recs))[-1]
    blob = _HDR.pack(MAGIC, VERSION, HEADER_BYTES, total, len(names), len(nb), len(ips), len(ib), len(recs)) + \
        offs(names) + _pad8(nb) + offs(ips) + _pad8(ib) + b"".join(recs)
    assert len(blob) == total
    return blob


def parse(blob: bytes):
    """-> (ips in snapshot order (bytes), {ip: {name: (hits, start_ns)}}); raises
    ValueError on a blob that is not a canonical version 1 snapshot."""
    blob = bytes(blob)
    if len(blob) < HEADER_BYTES:
        raise ValueError("header: shorter than 64 bytes")
    magic, ver, hb, total, n_names, names_bytes, n_ips, ip_bytes, n_states = _HDR.unpack_from(blob)
    if magic != MAGIC or ver != VERSION or hb != HEADER_BYTES:
        raise ValueError("magic / version / header_bytes")
    if total != len(blob):
        raise ValueError("total_bytes")
    o_name_off, o_names, o_ip_off, o_ips, o_recs, end = layout(n_names, names_bytes, n_ips, ip_bytes, n_states)
    if end != total:
        raise ValueError("section sizes")

    def strings(o_off, o_bytes, n, nbytes):
        off = struct.unpack_from("<%dQ" % (n + 1), blob, o_off)
        if off[0] != 0 or off[-1] != nbytes or any(a > b for a, b in zip(off, off[1:])):
            raise ValueError("offsets")
        return [blob[o_bytes + a:o_bytes + b] for a, b in zip(off, off[1:])]

    names = strings(o_name_off, o_names, n_names, names_bytes)
    ips = strings(o_ip_off, o_ips, n_ips, ip_bytes)
    if any(a >= b for a, b in zip(names, names[1:])):
        raise ValueError("names: not sorted and distinct")
    states, prev = {}, None
    per_ip = [dict() for _ in ips]
    used = set()
    for j in range(n_states):
        i, n, hits, start = _REC.unpack_from(blob, o_recs + REC_BYTES * j)
        if i >= n_ips or n >= n_names:
            raise ValueError("records: index out of range")
        if prev is not None and (i, n) <= prev:
            raise ValueError("records: not strictly ascending")
        prev = (i, n)
        used.add(n)
        per_ip[i][names[n]] = (hits, start)
    if any(not d for d in per_ip) or len(used) != n_names:
        raise ValueError("an IP without a record / a name without one")
    for ip, d in zip(ips, per_ip):
        if ip in states:
            raise ValueError("ips: an IP appears twice")
        states[ip] = d
    return ips, states
