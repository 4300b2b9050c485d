"""The event records of the rate-limit sort (engine_types.h EvRec, EvRec12,
EvRec8) on the host, through bjx_debug_event_record: the make / fits / time /
rule_id / seen the kernels use, and the event index read as the kernels after
the sort read it.  Round trips at every field's edges, and for the 8-byte form
the identity it rests on: the oracle's timestamp of a text S.mmm is a function
of the millisecond count alone, and fits() says no for every other timestamp.
"""
import ctypes as C
import random

import pytest

from banjax_amd import _lib
from oracle import oracle as O

MS = 1_000_000
Y2000, Y2100 = 946_684_800, 4_102_444_800


def bits(form):
    out = (C.c_uint32 * 3)()
    assert _lib.lib().bjx_debug_event_record_bits(form, out) == 0
    return tuple(out)


def rec(form, ts, rule=0, first=False, ev=0, base=0):
    """-> (fits, time, rule_id, seen, event index)"""
    out = (C.c_int64 * 5)()
    assert _lib.lib().bjx_debug_event_record(form, ts, rule, int(first), ev, base, out) == 0
    return bool(out[0]), out[1], out[2], bool(out[3]), out[4]


def ns_of_ms(m):
    """The reference's int64(ParseFloat("S.mmm") * 1e9) from the ms count: the
    nearest double of m / 1000 (what a correct parse of the text gives), one
    multiply, truncation."""
    return int((m / 1000.0) * 1e9)


def oracle_ts(text):
    rc, f = O.parse_float(text)
    assert rc == 0, text
    return int(f * 1e9)


def test_field_widths():
    tb, rb, eb = bits(8)
    assert tb + rb + 1 + eb == 64
    assert (1 << rb) >= 1006 and (1 << eb) >= 192_000_000       # the default bench's rules and events per batch
    assert (1 << (tb - 1)) >= 1_250_000                          # its timestamps: 1,250 s past the clock
    assert bits(12) == (44, 19, 32) and bits(16) == (64, 31, 32)
    assert _lib.lib().bjx_debug_event_record_bits(10, (C.c_uint32 * 3)()) != 0
    assert _lib.lib().bjx_debug_event_record(10, 1, 0, 0, 0, 0, (C.c_int64 * 5)()) != 0


@pytest.mark.parametrize("base_ms", [1_700_000_000_000, 1_700_000_000_000 - (1 << 23), Y2000 * 1000, 7])
def test_rec8_offset_edges(base_ms):
    tb, rb, eb = bits(8)
    span = 1 << tb
    for off, ok in ((0, True), (1, True), (span - 1, True), (span, False), (-1, False), (span + 5, False), (-span, False)):
        m = base_ms + off
        if m <= 0:
            continue
        ts = ns_of_ms(m)
        f, t, r, s, e = rec(8, ts, 5, False, 9, base_ms)
        assert f == ok, (off, ts)
        if ok:
            assert (t, r, s, e) == (ts, 5, True, 9), off


def test_rec8_off_grid_and_nonpositive():
    base_ms = 1_700_000_000_000 - (1 << 23)
    m = next(x for x in range(1_700_000_123_456, 1_700_000_123_556) if ns_of_ms(x) != x * MS)
    ts = ns_of_ms(m)
    assert ts % 256 == 0 and abs(ts - m * MS) < 256      # today's epoch: a 256-ns grid, not whole ms
    assert rec(8, ts, 0, False, 0, base_ms)[:2] == (True, ts)
    for d in (-256, 256, -1, 1, 499_999, -499_999, 500_000):
        assert not rec(8, ts + d, 0, False, 0, base_ms)[0], d
    assert not rec(8, m * MS, 0, False, 0, base_ms)[0] or m * MS == ts
    for ts0 in (0, -1, -MS, -(1 << 62), -(1 << 63)):
        for b in (0, -(1 << 23), base_ms):
            assert not rec(8, ts0, 0, False, 0, b)[0], (ts0, b)
    assert not rec(8, (1 << 63) - 1, 0, False, 0, base_ms)[0]


def test_rule_index_event_and_first_bit_edges():
    base8 = 1_700_000_000_000 - (1 << 23)
    ts = ns_of_ms(1_700_000_000_123)
    base12 = ts - (1 << 43)
    for form, base in ((8, base8), (12, base12), (16, 0)):
        _, rb, eb = bits(form)
        rmax, emax = (1 << rb) - 1, (1 << eb) - 1
        for rule in (0, 1, rmax - 1, rmax):
            for ev in (0, 1, emax - 1, emax):
                for first in (False, True):
                    got = rec(form, ts, rule, first, ev, base)
                    assert got == (True, ts, rule, not first, ev), (form, rule, ev, first, got)


def test_rec12_and_rec16_time_edges():
    base = 1_700_000_000_000_000_000
    for d, ok in ((0, True), ((1 << 44) - 1, True), (1 << 44, False), (-1, False)):
        f, t, _, _, _ = rec(12, base + d, 3, True, 4, base)
        assert f == ok and (not ok or t == base + d)
    for ts in (-(1 << 63), -1, 0, 1, (1 << 63) - 1):
        assert rec(16, ts, 3, True, 4, 123)[:2] == (True, ts)


def test_msec_sweep():
    """100,000 random (S, mmm) over 2000-2100: the record fits and gives back
    exactly the oracle's timestamp of the text S.mmm; the same text with more
    fractional digits that is not a whole ms does not fit."""
    rnd = random.Random(20261021)
    half = 1 << (bits(8)[0] - 1)
    for k in range(100_000):
        s, mmm = rnd.randrange(Y2000, Y2100), rnd.randrange(1000)
        ts = oracle_ts("%d.%03d" % (s, mmm))
        m = 1000 * s + mmm
        assert ts == ns_of_ms(m)
        base = m - rnd.randrange(half) - (half if k & 1 else 0)
        f, t, r, seen, ev = rec(8, ts, k & 1023, bool(k & 4), k, base)
        assert f and t == ts and r == (k & 1023) and seen == (not (k & 4)) and ev == k, (s, mmm, base)
        if k % 10 == 0:
            extra = "%d" % rnd.randrange(1, 10 ** rnd.randrange(1, 4))     # a non-zero tail: 4 to 6 fractional digits
            text = "%d.%03d%s" % (s, mmm, extra)
            t2 = oracle_ts(text)
            assert t2 != ts
            assert not rec(8, t2, 0, False, 0, base)[0], text
