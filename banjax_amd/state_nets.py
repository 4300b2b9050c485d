"""Selection of rate-limit state by network (bjx_state_query_nets /
bjx_state_remove_nets and their node forms) in pure Python: executable
documentation of how an entry is read and of when a held IP lies in it, and
what the tests compute their expected values with.

An entry is text as an Allow entry of a decision list is written: an address,
or address/bits.  It is read as Go's net.ParseIP / net.ParseCIDR read it: no
zone, IPv4 fields without leading zeros, bits in decimal and at most the
family's length (32 for dotted-quad text, 128 for text with a colon).  The
address is masked to `bits`; bits equal to the family's length is the single
address.  An entry that cannot be read is an error, never an empty selection.

Membership is CheckIsAllowed's rule for a global Allow list made of the
entries.  The IP's bytes are parsed with net.ParseIP; text that does not parse
is in no network.  An address whose 16-byte form is v4-mapped (dotted-quad
text, or ::ffff:a.b.c.d text) compares as IPv4 and against IPv4 networks only;
every other address against IPv6 networks only.  An IPv6-text entry whose
masked network is v4-mapped -- ::ffff:a.b.c.d/(96 + n) -- is the IPv4 network
a.b.c.d/n, so ::ffff:0:0/96 is 0.0.0.0/0 and ::/0 holds no dotted quad.
"""
from __future__ import annotations

NETS_MAX = 65536
_V4_PREFIX = b"\0" * 10 + b"\xff\xff"
_DIGITS = frozenset("0123456789")
_HEX = frozenset("0123456789abcdefABCDEF")


def _text(x) -> str:
    return x.decode("latin-1") if isinstance(x, (bytes, bytearray)) else str(x)


def _parse_v4(s: str):
    """Four decimal fields 0..255 without leading zeros -> 4 bytes, or None."""
    parts = s.split(".")
    if len(parts) != 4:
        return None
    out = bytearray()
    for p in parts:
        if not 1 <= len(p) <= 3 or not set(p) <= _DIGITS or (len(p) > 1 and p[0] == "0") or int(p) > 255:
            return None
        out.append(int(p))
    return bytes(out)


def _parse_v6(s: str):
    """RFC 4291 text, one "::" at most, an embedded dotted quad as the last 32 bits -> 16 bytes, or None."""
    if "%" in s:
        return None
    head, sep, tail = s.partition("::")
    if sep and "::" in tail:
        return None

    def groups(t, last):
        """-> bytes of the 16-bit groups of t (a dotted quad allowed at the end when last)"""
        if t == "":
            return b""
        out = bytearray()
        fields = t.split(":")
        for k, f in enumerate(fields):
            if "." in f:
                q = _parse_v4(f) if last and k == len(fields) - 1 else None
                if q is None:
                    return None
                out += q
            elif 1 <= len(f) <= 4 and set(f) <= _HEX:
                out += int(f, 16).to_bytes(2, "big")
            else:
                return None
        return bytes(out)

    if not sep:
        b = groups(head, True)
        return b if b is not None and len(b) == 16 else None
    hb, tb = groups(head, tail == ""), groups(tail, True)
    if hb is None or tb is None or len(hb) + len(tb) > 14:
        return None
    if "." in head:        # a dotted quad ends the address: nothing may follow it
        return None
    return hb + b"\0" * (16 - len(hb) - len(tb)) + tb


def parse_ip(text):
    """net.ParseIP -> (the 16-byte form, True for dotted-quad text) or None.
    The first of '.', ':' decides the family, as in Go."""
    s = _text(text)
    for c in s:
        if c == ".":
            q = _parse_v4(s)
            return (_V4_PREFIX + q, True) if q is not None else None
        if c == ":":
            b = _parse_v6(s)
            return (b, False) if b is not None else None
        if c == "%":
            return None
    return None


def parse_entry(text):
    """-> (family 4 or 6, bits, the masked network as an int of that family's
    width), or None when the entry cannot be read."""
    s = _text(text)
    addr, slash, bits_text = s.partition("/")
    p = parse_ip(addr)
    if p is None:
        return None
    a16, is4 = p
    width = 32 if is4 else 128
    if slash:
        if not bits_text or not set(bits_text) <= _DIGITS:
            return None
        bits = 0
        for c in bits_text:            # leading zeros are fine; Go's dtoi gives up at 0xFFFFFF
            bits = bits * 10 + int(c)
            if bits >= 0xFFFFFF:
                return None
        if bits > width:
            return None
    else:
        bits = width
    v = int.from_bytes(a16[12:] if is4 else a16, "big")
    v &= ((1 << bits) - 1) << (width - bits)
    if not is4 and v.to_bytes(16, "big")[:12] == _V4_PREFIX:   # (bits >= 96)
        return 4, bits - 96, v & 0xFFFFFFFF
    return (4 if is4 else 6), bits, v


class Nets:
    """The entries of one call.  ValueError, naming the index, for one that cannot be read;
    for none at all and for more than NETS_MAX."""

    def __init__(self, entries):
        entries = list(entries)
        if not entries:
            raise ValueError("nets: an empty list")
        if len(entries) > NETS_MAX:
            raise ValueError("nets: more than NETS_MAX entries")
        self.entries = []
        for k, e in enumerate(entries):
            n = parse_entry(e)
            if n is None:
                raise ValueError("nets: entry %d is not an address or address/bits" % k)
            self.entries.append(n)
        self._by_len, self._where = {}, {}
        for k, (fam, bits, v) in enumerate(self.entries):
            self._by_len.setdefault((fam, bits), set()).add(v)
            self._where.setdefault((fam, bits, v), []).append(k)

    def _keys(self, ip):
        """the (family, bits, network) triples that hold the IP text"""
        p = parse_ip(ip)
        if p is None:
            return
        a16 = p[0]
        fam, width = (4, 32) if a16[:12] == _V4_PREFIX else (6, 128)
        v = int.from_bytes(a16[12:] if fam == 4 else a16, "big")
        for (f, bits), nets in self._by_len.items():
            if f == fam:
                key = v & (((1 << bits) - 1) << (width - bits))
                if key in nets:
                    yield (f, bits, key)

    def holds(self, ip) -> bool:
        return next(self._keys(ip), None) is not None

    def which(self, ip):
        """indices of the entries, in the caller's order, that hold the IP (duplicates each count)"""
        return sorted(k for key in self._keys(ip) for k in self._where[key])
