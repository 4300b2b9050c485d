"""References and corpora for the two header fields the device parses with its
own code: the timestamp (strconv.ParseFloat, then int64(f * 1e9) and the
OldLine test) and the client IP (net.ParseIP, then CheckIsAllowed).  Plain
Python, no engine: tests/test_header_fields_cpu.py holds the host build of
bjx_common.h and the oracle against these, tests/test_gpu_header_fields.py
the values the kernels compute.

The references are written from Go's documented behaviour, not from the C code:

  * ParseFloat's syntax is the grammar of Go's floating-point literals as two
    regular expressions plus the underscore rule ("only between two digits or
    between the base prefix and a digit"); its value is float() /
    float.fromhex(), which are correctly rounded (round half to even), as Go's
    result is.  A finite token that rounds to +-Inf is Go's range error.
  * int64(f * 1e9) is one IEEE multiply and a truncation; on amd64 a NaN or a
    product outside [-2^63, 2^63) converts to MinInt64.
  * net.ParseIP is ipaddress.ip_address() with every text that holds a '%'
    refused (Go has no zones there); IPv4 is carried as ::ffff:a.b.c.d.
  * CheckIsAllowed is a model of internal/decision.go:185-216 and 278-374 with
    ipfilter's ToggleIP / NetAllowed and net.IPNet.Contains: per scope an
    exact-text map (last writer wins) and an Allow filter that holds every
    allow entry, a CIDR whose mask covers every bit filed as one address,
    Contains mapping a v4-mapped network and its mask to 4 bytes (so a 4-byte
    client never matches a 16-byte network), the site's scope before the
    global one.

Left out on purpose: one unparsable text listed under two decisions of one
scope.  The reference fills its exact map while ranging over a Go map of
decisions, so which decision wins there depends on Go's map iteration order.
"""
from __future__ import annotations

import functools
import ipaddress
import json
import math
import random
import re
import struct
from fractions import Fraction

INT64_MIN, INT64_MAX = -2 ** 63, 2 ** 63 - 1
LINE_ERROR, LINE_OLD, LINE_EXEMPTED = 1, 2, 4
S = 10 ** 9
OLD_NS = 10 * S
NAN_BITS = 0x7FF8000000000001  # math.NaN() in Go, what ParseFloat("nan") returns

# ------------------------------------------------------------------ timestamp reference

_A = re.ASCII
_DEC = re.compile(r"[+-]?(?:[0-9]+(?:\.[0-9]*)?|\.[0-9]+)(?:[eE][+-]?[0-9]+)?", _A)
_HEX = re.compile(r"[+-]?0[xX](?:[0-9a-fA-F]+(?:\.[0-9a-fA-F]*)?|\.[0-9a-fA-F]+)[pP][+-]?[0-9]+", _A)
_SPECIAL = re.compile(r"[+-]?(?:inf|infinity)|nan", _A | re.I)
_HEXPFX = re.compile(r"[+-]?0[xX]", _A)


def _underscores_ok(t: str) -> bool:
    """An underscore stands between two digits, or between the 0x prefix and a digit."""
    m = _HEXPFX.match(t)
    start = m.end() if m else 0
    digits = "0123456789abcdefABCDEF" if m else "0123456789"
    for i, c in enumerate(t):
        if c != "_":
            continue
        after_digit = (i > start and t[i - 1] in digits) or (m is not None and i == start)
        if not after_digit or i + 1 >= len(t) or t[i + 1] not in digits:
            return False
    return True


def ref_parse_float(tok: bytes):
    """strconv.ParseFloat(tok, 64) -> (rc, float): rc 0, -1 syntax error, -2 range error."""
    t = tok.decode("latin-1")
    if "_" in t:
        if not _underscores_ok(t):
            return -1, 0.0
        t = t.replace("_", "")
    if _SPECIAL.fullmatch(t):
        return 0, float(t)
    if _HEX.fullmatch(t):
        try:
            f = float.fromhex(t)
        except OverflowError:
            f = -math.inf if t[0] == "-" else math.inf
    elif _DEC.fullmatch(t):
        f = float(t)
    else:
        return -1, 0.0
    return (-2 if math.isinf(f) else 0), f


def f64_bits(f: float) -> int:
    if f != f:
        return NAN_BITS
    return struct.unpack("<Q", struct.pack("<d", f))[0]


def ref_ns(f: float) -> int:
    """int64(f * 1e9) on amd64 (CVTTSD2SQ: NaN and out of range give MinInt64)."""
    x = f * 1e9
    if x != x or not (-9223372036854775808.0 <= x < 9223372036854775808.0):
        return INT64_MIN
    return int(x)


def ref_ns_exact(f: float) -> int:
    """The same with the multiply done exactly and rounded once (Fraction's
    conversion rounds to nearest even): the cross-check of the float multiply."""
    if f != f or math.isinf(f):
        return INT64_MIN
    try:
        x = float(Fraction(f) * S)
    except OverflowError:
        return INT64_MIN
    if not (-9223372036854775808.0 <= x < 9223372036854775808.0):
        return INT64_MIN
    return int(x)


def go_sub(t: int, u: int) -> int:
    """time.Time.Sub: the difference saturated to the int64 range."""
    return max(INT64_MIN, min(INT64_MAX, t - u))


def ref_line(tok: bytes, now_ns: int, exempt: bool = False):
    """-> (flag, ns or None): what consumeLine makes of a line with this timestamp token."""
    rc, f = ref_parse_float(tok)
    if rc != 0:
        return LINE_ERROR, None
    ns = ref_ns(f)
    if go_sub(now_ns, ns) > OLD_NS:
        return LINE_OLD, ns
    return (LINE_EXEMPTED if exempt else 0), ns


ACCEPT = [b"1_23.50_0_0e+1_2", b"0x_1_2.3_4_5p+1_2", b"0_1"]
REJECT = [b"_123.5", b"1__23.5", b"123_.5", b"123._5", b"123.5_e+12", b"123.5e_+12", b"123.5e+_12", b"123.5e+12_", b"1e",
          b"1e-", b".", b".e1", b"0x", b"0x.p1", b"0x1", b"+nan", b"infin", b"nanx", b""]


def check_known_answers():
    """Answers that do not depend on Python's conversions."""
    for t in ACCEPT:
        assert ref_parse_float(t)[0] == 0, t
    for t in REJECT:
        assert ref_parse_float(t)[0] == -1, t
    assert ref_parse_float(b"1_23.50_0_0e+1_2")[1] == 1.235e14
    assert ref_parse_float(b"0x_1_2.3_4_5p+1_2")[1] == 74565.0  # 0x12.345 * 2^12 = 0x12345
    assert ref_parse_float(b"1.7976931348623157e308") == (0, float.fromhex("0x1.fffffffffffffp1023"))
    assert ref_parse_float(b"1.7976931348623159e308")[0] == -2 and ref_parse_float(b"1e309")[0] == -2
    assert ref_parse_float(b"-0x1p1024") == (-2, -math.inf)
    assert f64_bits(ref_parse_float(b"4.9e-324")[1]) == 1 and f64_bits(ref_parse_float(b"3e-324")[1]) == 1
    assert ref_parse_float(b"2e-324") == (0, 0.0)
    assert f64_bits(ref_parse_float(b"-0")[1]) == 1 << 63
    # doubles near 2^63 are multiples of 1024: 9223372036.854775 s is the last second count whose product stays below
    assert ref_ns(9223372036.854776) == INT64_MIN and ref_ns(9223372036.854775) == 2 ** 63 - 1024
    assert ref_ns(-9223372036.854775) == -(2 ** 63 - 1024) and ref_ns(-9223372037.0) == INT64_MIN
    assert ref_ns(math.nan) == INT64_MIN and ref_ns(math.inf) == INT64_MIN and ref_ns(-0.0) == 0
    assert ref_line(b"5", 15 * S)[0] == 0 and ref_line(b"5", 15 * S + 1)[0] == LINE_OLD
    assert ref_line(b"-inf", 0)[0] == LINE_OLD and ref_line(b"1e10", INT64_MAX)[0] == LINE_OLD


# ------------------------------------------------------------------ timestamp corpus

T0 = 1_700_000_000  # the base time, seconds; the corpus batches run at NOW_BASE and at NOW_EPOCH
NOW_BASE = (T0 + 9) * S + 500_000_000
NOW_EPOCH = 5 * S


def exact_decimal(num: int, k: int) -> str:
    """num / 10^k, every digit."""
    s = str(num)
    if k == 0:
        return s
    if len(s) <= k:
        s = "0" * (k - len(s) + 1) + s
    return s[:-k] + "." + s[-k:]


def halfway(d: float) -> str:
    """The exact decimal of the point halfway between d (> 0) and the next double up."""
    mid = Fraction(d) + Fraction(math.ulp(d)) / 2
    k = mid.denominator.bit_length() - 1
    return exact_decimal(mid.numerator * 5 ** k, k)


def _perturbed(h: str):
    """h (ends in 5), and its last digit one down and one up."""
    assert h[-1] == "5"
    return [h, h[:-1] + "4", h[:-1] + "6"]


def _near_base(rnd) -> float:
    return T0 + rnd.randrange(0, 16 * 2 ** 22) / 2 ** 22  # a double in [T0, T0 + 16), spacing 2^-22 s


@functools.lru_cache(maxsize=None)
def ts_corpus():
    """[(class, token)]: 2,000 to 4,000 tokens, fixed seed."""
    rnd = random.Random(0x7157)
    out = []

    def add(cls, tok):
        out.append((cls, tok if isinstance(tok, bytes) else tok.encode()))

    def digs(n, first_nonzero=False, last_nonzero=False):
        s = "".join(rnd.choice("0123456789") for _ in range(n))
        if n and first_nonzero and s[0] == "0":
            s = "7" + s[1:]
        if n and last_nonzero and s[-1] == "0":
            s = s[:-1] + "3"
        return s

    # --- the limits of parse_float_fast: significant digits, mantissa, fraction digits, bytes, leading zeros
    for _ in range(40):
        sec = str(T0 + rnd.randrange(16))
        for nd in (15, 16, 17):
            add("limits", sec + "." + digs(nd - 10, last_nonzero=True))
        add("limits", sec)                                     # no fraction, no point
        add("limits", sec + ".")                               # 0 fraction digits
        add("limits", sec + "." + digs(1))
    for m in (2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, 2 ** 53 + 2):
        for k in (6, 7, 9):                                    # 9007199254.740991: a time past the base
            add("limits", exact_decimal(m, k))
        add("limits", "0" * 5 + exact_decimal(m, 6))
    for tok in ("1844674407.3709551621", "1844674407.3709551616", "184467440.73709551621"):
        add("limits", tok)                                     # 2^64 + 5 and 2^64: a 64-bit mantissa that wrapped would pass for 5 or 0
    for fd in (21, 22, 23):                                    # at most 16 digits after the zeros: tiny values
        for _ in range(12):
            nz = rnd.randrange(1, 17)
            add("limits", "0." + "0" * (fd - nz) + digs(nz, first_nonzero=True, last_nonzero=True))
        add("limits", "0." + "0" * (fd - 16) + str(2 ** 53 - 1))
        add("limits", "0." + "0" * (fd - 16) + str(2 ** 53))
        add("limits", "%d." % (T0 + 3) + "5" + "0" * (fd - 1))  # the same count of fraction digits, 10 + fd digits
    for nbytes in (39, 40, 41):
        for _ in range(8):
            body = "%d.%s" % (T0 + rnd.randrange(16), digs(rnd.randrange(0, 7)))
            add("limits", "0" * (nbytes - len(body)) + body)
        body = "%d." % (T0 + 1)
        add("limits", body + "0" * (nbytes - len(body)))        # trailing zeros: 10 + 28 digits
    for z in (1, 2, 4):
        add("limits", "0" * z + "%d.%s" % (T0 + 2, digs(3)))

    # --- the 14-byte $msec shape and its neighbours
    for _ in range(300):
        add("msec", "%d.%s" % (T0 + rnd.randrange(16), digs(3)))
    for tok in ("9223372036.854", "0000000000.000", "0000000004.999", "0000000000.001", "4294967296.000", "4294967295.999",
                "2147483648.001", "1000000000.000"):
        add("msec", tok)
    for _ in range(10):
        sec, ms = T0 + rnd.randrange(16), digs(3)
        add("msec", "%d.%s" % (sec // 10, ms))                 # 13 bytes
        add("msec", "0%d.%s" % (sec, ms))                      # 15 bytes
        add("msec", "%d.%s" % (sec, ms[:2]))                   # 13 bytes, 2 fraction digits
        add("msec", "%d.%s" % (sec, ms + "7"))                 # 15 bytes, 4 fraction digits
    proto = "%d.%s" % (T0 + 5, "246")
    for pos in range(14):
        for c in "/:._e+-":                                    # '/' and ':' are the bytes next to '0' and '9'
            if not (pos == 10 and c == "."):
                add("msec", proto[:pos] + c + proto[pos + 1:])
    for pos in (0, 5, 9, 11, 13):                              # '.' elsewhere, the 11th byte a digit
        t = proto.replace(".", "0")
        add("msec", t[:pos] + "." + t[pos + 1:])

    # --- one value in every spelling
    for _ in range(24):
        sec, ms = T0 + rnd.randrange(16), digs(3)
        v = float("%d.%s" % (sec, ms))
        m = "%d%s" % (sec, ms)
        hx = v.hex()
        for tok in ("%d.%s" % (sec, ms), "%d.%s000" % (sec, ms), "%d.%s" % (sec, ms) + "0" * 30, "%s.%se9" % (m[0], m[1:]),
                    "%se-3" % m, "%sE-03" % m, "0.%sE+10" % m, ".%se10" % m, "%s000e-6" % m, "%d.%se0" % (sec, ms),
                    "%d.%se+0" % (sec, ms), hx, hx.upper(), hx.replace("0x1.", "0x_1."), "+" + hx,
                    "0x%xp-22" % int(Fraction(v) * 2 ** 22), "0X%X.0P-22" % int(Fraction(v) * 2 ** 22),
                    "%s_%s_%s_%s.%s" % (str(sec)[0], str(sec)[1:4], str(sec)[4:7], str(sec)[7:], ms),
                    "+%d.%s" % (sec, ms), "+%d.%s_%se0" % (sec, ms[0], ms[1:]), "0%d.%s" % (sec, ms)):
            add("spellings", tok)

    # --- exact halfway decimals near the base time: the rounding decides the nanosecond
    for _ in range(160):
        for tok in _perturbed(halfway(_near_base(rnd))):
            add("halfway", tok)
    for _ in range(20):
        h = halfway(_near_base(rnd))
        add("halfway", h + "0" * 7)
        add("halfway", h + "0" * 7 + "1")
        add("halfway", h.replace(".", "") + "e-23")
        add("halfway", "+" + h[:1] + "_" + h[1:])

    # --- long tokens whose tail decides the rounding (Decimal keeps 800 digits, then a sticky flag)
    for n in (100, 799, 800, 801, 1200):
        for _ in range(5):
            h = halfway(_near_base(rnd))                       # 10 + 23 digits
            z = "0" * (n - 34)
            for tail in ("0", "1"):
                add("long", h + z + tail)                      # n digits in all
                add("long", "0" * 9 + h + z + tail)            # leading zeros do not count
            add("long", h[:-1] + "4" + "9" * (n - 33))
        add("long", "%d." % (T0 + 4) + "9" * (n - 10))
    for n in (100, 1200):                                      # digits, then an exponent that brings them back
        add("long", "1" + "0" * n + "e-%d" % (n - 9))
        add("long", "0." + "0" * n + "17e%d" % (n + 10))

    # --- subnormal and tiny values: 0 ns
    for tok in ("4.9e-324", "3e-324", "2e-324", "2.4703282292062327e-324", "2.4703282292062328e-324", "1e-400", "1e-320",
                "2.2250738585072011e-308", "2.2250738585072014e-308", "2.2250738585072012e-308", "0." + "0" * 400 + "1",
                "1e-10", "1e-9", "9.99999999e-10", "0.000000001", "0.0000000019999", "0x1p-1074", "0x1p-1075", "0x1.8p-1075",
                "0x0.8p-1073", "0x1.0000000000001p-1075", "0x1p-1100", "0", "0.0", "0e0", "0x0p0", "00", "000.000",
                halfway(5e-324), halfway(5e-324)[:-1] + "4", halfway(2.2250738585072014e-308),
                halfway(2.225073858507201e-308)):
        add("tiny", tok)

    # --- the int64 edge: values from 9223372036.854775 upward give MinInt64
    for tok in ("9223372036.854774", "9223372036.854775", "9223372036.854776", "9223372036.8547758", "9223372036.854775807",
                "9223372036.854775808", "9223372036.85477", "9223372036.8547", "9223372037", "9223372036", "1e10", "1e19",
                "1e300", "1.7976931348623157e308", "9.223372036854775e9", "0x1.12e0be826d694p+33", "0x1.12e0be826d695p+33",
                "0x1p33", "0x1p63", "-9223372036.854775", "-9223372036.854776", "-9223372036.854775808", "-9223372036.854777",
                "-9223372037", "-1e10", "-1e300", "1e309", "-1e309", "1.7976931348623159e308", "0x1p1024", "0x1.fffffffffffffp1023",
                "0x1.fffffffffffff8p1023", "0x1.fffffffffffff7p1023"):
        add("edge", tok)

    # --- inf, nan, negative values, -0: the flag is the check
    for tok in ("inf", "+inf", "-inf", "Inf", "INF", "infinity", "Infinity", "-INFINITY", "+iNfInItY", "nan", "NaN", "NAN",
                "-0", "-0.0", "-0e5", "-0x0p0", "-5", "-4.999", "-5.000", "-5.000000001", "-4.999999999", "-5.001", "-1",
                "-0.000000001", "-1e-400", "-%d.5" % T0, "+0", "+5"):
        add("special", tok)
    for tok in ACCEPT + REJECT + [b"-nan", b"+infin", b"infinit", b"infinityy", b"in", b"i", b"n", b"na", b"+", b"-", b"+-1",
                                  b"1-", b"1.2.3", b"1..2", b"1e5e5", b"1e5.5", b"0x1p", b"0x1p+", b"0x1.8", b"0xp1", b"0x1p1.5",
                                  b"0X1P1", b"0x1P-1", b"1x", b"0x1g.p1", b"1,5", b"1e+5_", b"_", b"1_", b"_1", b"0_x1p1", b"0x1_p1",
                                  b"0x1p_1", b"0x1p1_0", b"0x_1p1", b"0x__1p1", b"1_e5", b"1e1_0", b"1_0e1", b"1_.0", b"1._0",
                                  b"1.0_", b"+_1", b"+1_0", b"0b1", b"0o7", b"1f", b"1d", b"1.5f", b"\xff1", b"1\xb2",
                                  b"\xd9\xa1", b"1\t", b"\t1", b"1e\x001", b"i_nf", b"in_f", b"1_7e2", b"0x1_7.8_8p0_1"]:
        add("syntax", tok)
    assert 2000 <= len(out) <= 4000, len(out)
    return out


def line_ip(k: int) -> str:
    """The client IP of line k of a timestamp batch: one state per line."""
    return "11.%d.%d.%d" % (k >> 16 & 255, k >> 8 & 255, k & 255)


def ts_line(tok: bytes, k: int, host: str = "h.test", pad: int = 0) -> bytes:
    return tok + b" " + line_ip(k).encode() + b" GET " + host.encode() + b" GET /x HTTP/1.1 ua" + b"p" * pad + b"\n"


def ts_batch(tokens, host: str = "h.test", k0: int = 0) -> bytes:
    """One line per token; line k's client IP is line_ip(k0 + k)."""
    return b"".join(ts_line(t, k0 + k, host) for k, t in enumerate(tokens))


_FAST = re.compile(rb"[0-9]+(?:\.[0-9]*)?")


def fast_accepts(tok: bytes) -> bool:
    """The tokens the line kernels parse themselves (parse_ts_msec, parse_float_fast): digits with
    at most one point, at most 40 bytes, 16 significant digits, a mantissa below 2^53 and 22
    fraction digits.  Every other token sends its line to the per-line fallback.  (What the
    value is does not depend on this: tests/test_header_fields_cpu.py holds it against the host
    build's parse_float_fast.)"""
    if not 0 < len(tok) <= 40 or not _FAST.fullmatch(tok):
        return False
    ip, _, fr = tok.partition(b".")
    return len((ip + fr).lstrip(b"0")) <= 16 and int(ip + fr) < 2 ** 53 and len(fr) <= 22


def fallback_lines(data: bytes, kernel: str, window: int = 112) -> int:
    """Lines of the batch the line kernel hands to the per-line fallback: every line without a
    line pass; else the lines whose timestamp token the kernel does not parse and, for k_lines2,
    the lines whose fourth space lies past the window that starts at the line's 16-byte
    alignment skip."""
    n, pos = 0, 0
    for ln in data.split(b"\n")[:-1]:
        f = ln.split(b" ", 4)
        past = kernel == "k_lines2" and len(f) == 5 and (pos & 15) + len(ln) - len(f[4]) - 1 >= window
        if kernel == "k_parse_match" or (len(f) == 5 and (past or not fast_accepts(f[0]))):
            n += 1
        elif kernel == "k_lines2" and len(f) < 5 and (pos & 15) + len(ln) > window:
            n += 1
        pos += len(ln) + 1
    return n


def narrow_tokens():
    """The corpus tokens within a minute of the base time: a batch of them sorts 12-byte records."""
    out = []
    for _, t in ts_corpus():
        fl, ns = ref_line(t, NOW_BASE)
        if fl == 0 and abs(ns - T0 * S) < 60 * S:
            out.append(t)
    return out


def sweep_floats(n: int, seed: int):
    """n tokens, a third each: exact halfway decimals of random doubles and
    subnormals with the last digit perturbed; random decimals with exponents
    -345..330; random hex floats with exponents -1150..1100."""
    rnd = random.Random(seed)
    out = []
    while len(out) < n:
        k = len(out) % 3
        if k == 0:
            if rnd.random() < 0.3:
                d = struct.unpack("<d", struct.pack("<Q", rnd.randrange(1, 1 << 52)))[0]      # subnormal
            else:
                d = struct.unpack("<d", struct.pack("<Q", rnd.randrange(1, 0x7FE) << 52 | rnd.getrandbits(52)))[0]
            h = halfway(d)
            if "." not in h:
                h += "."
            if h[-1] == ".":
                h += "0"
            c = rnd.randrange(3)
            t = h if c == 0 else h[:-1] + (str(int(h[-1]) - 1) if c == 1 and h[-1] != "0" else "6")
            if rnd.random() < 0.2:
                t = "-" + t
        elif k == 1:
            nd = rnd.choice((1, 5, 15, 16, 17, 18, 19, 20, 21, 30, 40))
            s = "".join(rnd.choice("0123456789") for _ in range(nd))
            p = rnd.randrange(nd + 1)
            t = rnd.choice(("", "", "-", "+")) + (s[:p] + "." + s[p:] if rnd.random() < 0.8 else s)
            if t.lstrip("+-") == ".":
                t += "5"
            if rnd.random() < 0.8:
                t += rnd.choice("eE") + "%+d" % rnd.randrange(-345, 331)
        else:
            nd = rnd.randrange(1, 22)
            s = "".join(rnd.choice("0123456789abcdefABCDEF") for _ in range(nd))
            p = rnd.randrange(nd + 1)
            t = rnd.choice(("", "", "-", "+")) + rnd.choice(("0x", "0X")) + (s[:p] + "." + s[p:] if rnd.random() < 0.8 else s)
            t += rnd.choice("pP") + "%+d" % rnd.randrange(-1150, 1101)
        if rnd.random() < 0.05:      # one byte replaced: mostly syntax errors
            p = rnd.randrange(len(t))
            t = t[:p] + rnd.choice("_.eEpPxX+-09a") + t[p + 1:]
        out.append(t.encode())
    return out


# ------------------------------------------------------------------ IP reference

V4_PREFIX = b"\0" * 10 + b"\xff\xff"


def ref_parse_ip(text):
    """net.ParseIP -> (16 bytes, is4) or None."""
    if isinstance(text, bytes):
        text = text.decode("latin-1")
    if "%" in text:
        return None
    try:
        a = ipaddress.ip_address(text)
    except ValueError:
        return None
    if a.version == 4:
        return V4_PREFIX + a.packed, True
    return a.packed, False


def model_entry(text: str):
    """ToggleIP(text, true): ("addr", 16 bytes), ("sub", netlen, net, mask) or None (not filed)."""
    if "/" in text:
        addr, _, mask = text.partition("/")
        p = ref_parse_ip(addr)
        if p is None or not re.fullmatch(r"[0-9]+", mask, _A):
            return None
        n = int(mask)
        bitlen = 32 if p[1] else 128
        if n >= 0xFFFFFF or n > bitlen:      # dtoi gives up at 0xFFFFFF
            return None
        if n == bitlen:
            return ("addr", p[0])
        nb = bitlen // 8
        m = ((1 << n) - 1) << (bitlen - n)
        net = (int.from_bytes(p[0][16 - nb:], "big") & m).to_bytes(nb, "big")
        mb = m.to_bytes(nb, "big")
        if nb == 16 and net[:12] == V4_PREFIX:   # IPNet.Contains: To4 of the network, the mask's last 4 bytes
            return ("sub", 4, net[12:], mb[12:])
        return ("sub", nb, net, mb)
    p = ref_parse_ip(text)
    return ("addr", p[0]) if p else None


class AllowModel:
    """StaticDecisionLists of entries [(site or None, decision name, text)] in config order."""

    def __init__(self, entries):
        self.exact, self.addrs, self.subs = {}, {}, {}
        for site, dec, text in entries:
            if "/" not in text:
                self.exact.setdefault(site, {})[text] = dec
            if dec != "allow":
                continue
            e = model_entry(text)
            if e and e[0] == "addr":
                self.addrs.setdefault(site, set()).add(e[1])
            elif e:
                self.subs.setdefault(site, []).append(e[1:])

    def _scope(self, sc, text, p):
        if self.exact.get(sc, {}).get(text) == "allow":
            return True
        if p is None:
            return False
        if p[0] in self.addrs.get(sc, ()):
            return True
        ip = p[0][12:] if p[0][:12] == V4_PREFIX else p[0]
        for netlen, net, mask in self.subs.get(sc, ()):
            if netlen == len(ip) and all(a & m == b for a, m, b in zip(ip, mask, net)):
                return True
        return False

    def allowed(self, site, ip) -> bool:
        text = ip.decode("latin-1") if isinstance(ip, bytes) else ip
        p = ref_parse_ip(text)
        return self._scope(site, text, p) or self._scope(None, text, p)


# ------------------------------------------------------------------ IP spellings and sweep

def _compress(groups):
    best_s, best_l, i = -1, 1, 0
    while i < 8:
        j = i
        while j < 8 and groups[j] == 0:
            j += 1
        if j - i > best_l:
            best_s, best_l = i, j - i
        i = max(j, i + 1)
    h = ["%x" % g for g in groups]
    if best_s < 0:
        return ":".join(h)
    return ":".join(h[:best_s]) + "::" + ":".join(h[best_s + best_l:])


def spellings(b16: bytes):
    """Texts of one address: compressed, full 39-byte, upper-case, embedded dotted quad; for a
    v4-mapped one the plain dotted quad and the ::ffff: text as well."""
    g = struct.unpack(">8H", b16)
    quad = "%d.%d.%d.%d" % tuple(b16[12:])
    out = [_compress(g), ":".join("%04x" % x for x in g), _compress(g).upper(), ":".join("%04X" % x for x in g),
           ":".join("%x" % x for x in g[:6]) + ":" + quad]
    if not any(g[:6]):
        out.append("::" + quad)
    if b16[:12] == V4_PREFIX:
        out += [quad, "::ffff:" + quad, "::FFFF:" + quad, "0:0:0:0:0:ffff:" + quad]
    return list(dict.fromkeys(out))


def sweep_ips(n: int, seed: int):
    """n IP-like texts: valid IPv4 / IPv6 in several spellings, and the same with one or two
    bytes inserted, deleted or replaced."""
    rnd = random.Random(seed)
    alpha = "0123456789abcdefABCDEF:.%/g -"
    out = []
    while len(out) < n:
        r = rnd.random()
        if r < 0.3:
            parts = [str(rnd.choice((0, 1, 9, 10, 99, 100, 199, 200, 249, 250, 255, 256, 260, 300, rnd.randrange(256))))
                     for _ in range(rnd.choice((4, 4, 4, 4, 3, 5)))]
            if rnd.random() < 0.15:
                k = rnd.randrange(len(parts))
                parts[k] = rnd.choice(("0", "00", "")) + parts[k]
            t = ".".join(parts)
            if rnd.random() < 0.2:
                t = rnd.choice(("::ffff:", "::", "1:2:3:4:5:6:", "1::", "::FFFF:", "64:ff9b::", "1:2:3:4:5:6:7:")) + t
        else:
            g = [rnd.choice((0, 0, 0, 1, 0xffff, 0xff, 0x1000, rnd.getrandbits(16))) for _ in range(8)]
            c = rnd.randrange(6)
            if c == 0:
                t = _compress(g)
            elif c == 1:
                t = ":".join("%04x" % x for x in g)
            elif c == 2:
                t = ":".join("%X" % x for x in g)
            elif c == 3:
                k = rnd.randrange(0, 9)
                m = rnd.randrange(0, 9 - k)
                t = ":".join("%x" % x for x in g[:k]) + "::" + ":".join("%x" % x for x in g[8 - m:] if m)
            elif c == 4:
                t = rnd.choice(spellings(bytes(rnd.getrandbits(8) for _ in range(16))))
            else:
                t = ":".join("%x" % x for x in g[:rnd.randrange(1, 10)])
        for _ in range(rnd.choice((0, 0, 0, 1, 1, 2))):
            k = rnd.randrange(len(t) + 1)
            op = rnd.randrange(3)
            if op == 0:
                t = t[:k] + rnd.choice(alpha) + t[k:]
            elif op == 1:
                t = t[:k] + t[k + 1:]
            else:
                t = t[:k] + rnd.choice(alpha) + t[k + 1:]
        out.append(t)
    return out


# ------------------------------------------------------------------ allow-list corpus

RULES_YAML = """regexes_with_rates:
  - rule: "all"
    regex: '.*'
    interval: 100000
    hits_per_interval: 1000000000
    decision: challenge
"""
LONG_HOST = "l" * 96 + ".com"   # a 100-byte host field: the header leaves k_lines2's window


def _flip(b: bytes, bit: int) -> bytes:
    x = bytearray(b)
    x[bit // 8] ^= 0x80 >> (bit % 8)
    return bytes(x)


def _last_inside(b: bytes, n: int) -> bytes:
    v = int.from_bytes(b, "big") | ((1 << (len(b) * 8 - n)) - 1)
    return v.to_bytes(len(b), "big")


class AllowCase:
    """One configuration: entries [(site or None, decision, text)], and clients
    [(site the line names, IP text)]."""

    def __init__(self, name):
        self.name, self.entries, self.clients, self.site_rules = name, [], [], []
        self.prefix_sites = []

    def yaml(self) -> str:
        out = [RULES_YAML]
        if self.site_rules:
            out.append("per_site_regexes_with_rates:")
            for h in self.site_rules:
                out.append("  %s:\n    - rule: \"site\"\n      regex: 'GET'\n      interval: 100000\n"
                           "      hits_per_interval: 1000000000\n      decision: nginx_block" % json.dumps(h))
        glob = [e for e in self.entries if e[0] is None]
        if glob:
            out.append("global_decision_lists:")
            for dec in dict.fromkeys(e[1] for e in glob):
                out.append("  %s:" % dec)
                out += ["    - %s" % json.dumps(e[2]) for e in glob if e[1] == dec]
        sites = list(dict.fromkeys(e[0] for e in self.entries if e[0] is not None))
        if sites:
            out.append("per_site_decision_lists:")
            for s in sites:
                out.append("  %s:" % json.dumps(s))
                mine = [e for e in self.entries if e[0] == s]
                for dec in dict.fromkeys(e[1] for e in mine):
                    out.append("    %s:" % dec)
                    out += ["      - %s" % json.dumps(e[2]) for e in mine if e[1] == dec]
        return "\n".join(out) + "\n"

    def config_entries(self):
        """The entries in the order the YAML lists them (grouped by decision per scope)."""
        out = []
        for sc in dict.fromkeys(e[0] for e in self.entries):
            mine = [e for e in self.entries if e[0] == sc]
            for dec in dict.fromkeys(e[1] for e in mine):
                out += [e for e in mine if e[1] == dec]
        return out

    def model(self) -> AllowModel:
        return AllowModel(self.config_entries())

    def lines(self, rotate: int = 0, now_ns: int = NOW_BASE):
        """-> (batch bytes, [(site, ip text)] per line).  rotate: each client meets the site
        `rotate` places on in the list of sites."""
        sites = list(dict.fromkeys(s for s, _ in self.clients))
        idx = {s: k for k, s in enumerate(sites)}
        rows, out = [], []
        for k, (site, ip) in enumerate(self.clients):
            site = sites[(idx[site] + rotate) % len(sites)]
            rows.append((site, ip))
            out.append("%d.%03d %s GET %s GET /x HTTP/1.1 ua\n" % (now_ns // S - 3, k % 1000, ip, site))
        return "".join(out).encode("latin-1"), rows


def _prefix_case(name, base: bytes, lo: int, hi: int, v4_text: bool, other_family: str) -> AllowCase:
    c = AllowCase(name)
    nbits = 32 if v4_text else 128
    for n in range(lo, hi + 1):
        site = "%s-%d.test" % (name, n)
        raw = base[12:] if v4_text else base
        text = "%d.%d.%d.%d" % tuple(raw) if v4_text else ("::ffff:%d.%d.%d.%d" % tuple(base[12:])
                                                              if base[:12] == V4_PREFIX else _compress(struct.unpack(">8H", base)))
        c.entries.append((site, "allow", "%s/%d" % (text, n)))
        c.prefix_sites.append(site)
        cl = [raw, _last_inside(raw, n)]
        if n > 0:
            cl.append(_flip(raw, n - 1))        # differs in the last masked bit: outside
        if n < nbits:
            cl.append(_flip(raw, n))            # differs in the first unmasked bit: inside
        for x in cl:
            for t in spellings(V4_PREFIX + x if v4_text else x):
                c.clients.append((site, t))
        c.clients.append((site, other_family))   # 4-byte against 16-byte: never
    return c


@functools.lru_cache(maxsize=None)
def allow_cases():
    rnd = random.Random(0xA110)
    v4 = V4_PREFIX + bytes([0xA5, 0x5A, 0xC3, 0x3C])
    v6 = bytes([0xA5]) + bytes(rnd.getrandbits(8) | 1 for _ in range(15))   # first byte >= 0x80, no zero group
    mp = V4_PREFIX + bytes([0x9A, 0x65, 0x3C, 0xC3])
    cases = [_prefix_case("v4", v4, 0, 32, True, "a55a:c33c::1"),
             _prefix_case("v6a", v6, 0, 64, False, "165.90.195.60"),
             _prefix_case("v6b", v6, 65, 128, False, "165.90.195.60"),
             _prefix_case("map", mp, 88, 128, False, "a55a:c33c::1")]

    # --- one scope of 1,000 exact addresses over first bytes 00, 7f, 80, ff; every 10th probed with its neighbours
    c = AllowCase("exact")
    addrs = []
    for k in range(1000):
        first = (0x00, 0x7F, 0x80, 0xFF)[k % 4]
        if k % 8 < 4:
            a = bytes([first]) + bytes(rnd.getrandbits(8) for _ in range(7)) + \
                (bytes(8) if k % 16 < 8 else bytes([rnd.choice((0, 0x7F, 0x80, 0xFF))]) + bytes(rnd.getrandbits(8) for _ in range(7)))
            addrs.append(a)
            c.entries.append(("big.test", "allow", rnd.choice(spellings(a)[:3])))
        else:
            a = V4_PREFIX + bytes([first]) + bytes(rnd.getrandbits(8) for _ in range(3))
            addrs.append(a)
            c.entries.append(("big.test", "allow", "%d.%d.%d.%d" % tuple(a[12:])))
    for a in addrs[::10]:
        v = int.from_bytes(a, "big")
        for d in (0, -1, 1, 1 << 64, -(1 << 64), 1 << 63):
            x = ((v + d) % (1 << 128)).to_bytes(16, "big")
            c.clients.append(("big.test", spellings(x)[-1 if x[:12] == V4_PREFIX and rnd.random() < 0.5 else 0]))

    # --- one scope of 300 unparsable strings: probe each, each less its last byte, each plus a byte
    strs = ["", "x" * 16, "y" * 200, "not-an-ip", "1.2.3", "1.2.3.4.5", "01.2.3.4", "1.2.3.04", "::g", "1:2:3:4:5:6:7:8:9",
            "fe80::1%eth0", "1.2.3.4%eth0", "256.1.1.1", ":::", "12345::"]
    while len(strs) < 300:
        stem = "".join(rnd.choice("abcxyz0189:.-") for _ in range(rnd.choice((1, 3, 4, 7, 8, 15, 16, 17, 31, 40))))
        for t in (stem + "!", stem + "!a", stem + "!ab"):      # pairs that share a prefix
            if t not in strs and ref_parse_ip(t) is None:
                strs.append(t)
    strs = strs[:300]
    for t in strs:
        c.entries.append(("str.test", "allow", t))
    for t in strs:
        for p in (t, t[:-1], t + "a", t + "!"):
            if " " not in p:
                c.clients.append(("str.test", p))
    c.clients.append(("big.test", "not-an-ip"))
    c.clients.append(("str.test", "0.0.0.1"))

    # --- lists and rules: an allow list and no rules, rules and no allow list; the global list; odd entries
    c.site_rules = ["rules-only.test", "both.test"]
    c.entries += [("list-only.test", "allow", "10.1.0.0/16"), ("both.test", "allow", "10.2.0.0/16"),
                  (None, "allow", "10.200.0.0/13"), (None, "allow", "2001:db8:8000::/33"), (None, "allow", "global-text"),
                  (None, "challenge", "10.200.0.9"), (None, "challenge", "8.8.8.8"),
                  ("odd.test", "allow", "1.2.3.4/32"), ("odd.test", "allow", "1.2.3.5/032"), ("odd.test", "allow", "1.2.3.6/33"),
                  ("odd.test", "allow", "1.2.4.0/024"), ("odd.test", "allow", "1.2.3.4%eth0"), ("odd.test", "allow", "fe80::1%eth0/64"),
                  ("odd.test", "allow", "10.01.2.3"), ("odd.test", "allow", "10.01.0.0/16"), ("odd.test", "allow", "7.7.7.7/"),
                  ("odd.test", "allow", "7.7.7.8/+8"), ("odd.test", "allow", "7.7.7.9/16777215"), ("odd.test", "allow", "::ffff:7.8.0.0/112"),
                  ("odd.test", "allow", "::ffff:7.9.0.0/16"), ("odd.test", "allow", "::7.10.0.0/112"), ("odd.test", "challenge", "9.9.9.9"),
                  ("odd.test", "allow", "9.9.9.9/32"), ("odd.test", "challenge", "6.6.6.6/32"), ("odd.test", "allow", "::ffff:5.6.7.8"),
                  (LONG_HOST, "allow", "10.77.0.0/17"), (LONG_HOST, "allow", "long-text"), (LONG_HOST, "allow", "2001:db8::77")]
    for site in ("list-only.test", "both.test", "rules-only.test", "odd.test", "nowhere.test", LONG_HOST):
        for ip in ("10.1.2.3", "10.2.2.3", "10.200.0.1", "10.207.255.255", "10.208.0.0", "10.200.0.9", "8.8.8.8", "2001:db8:8000::1",
                   "2001:db8:7fff::1", "2001:DB8:ffff:ffff::", "global-text", "global-tex", "1.2.3.4", "1.2.3.5", "1.2.3.6", "1.2.4.77",
                   "1.2.5.0", "1.2.3.4%eth0", "fe80::1", "fe80::1%eth0", "10.01.2.3", "10.1.2.3", "7.7.7.7", "7.7.7.8", "7.7.7.9",
                   "7.8.1.2", "::ffff:7.8.3.4", "::ffff:708:304", "7.9.1.1", "0.0.0.1", "::1", "::7.10.3.4", "7.10.3.4", "9.9.9.9",
                   "6.6.6.6", "5.6.7.8", "::ffff:5.6.7.8", "::ffff:506:708", "10.77.127.255", "10.77.128.0", "::ffff:10.77.0.1",
                   "long-text", "long-text!", "2001:db8::77", "2001:0db8:0000:0000:0000:0000:0000:0077", "2001:db8::78", "", "-"):
            c.clients.append((site, ip))
    cases.append(c)
    return tuple(cases)


def check_allow_guard():
    """With the references alone: every prefix site has allowed and refused clients, the
    special scopes have both, the long host has both."""
    for c in allow_cases():
        m = c.model()
        by_site = {}
        for site, ip in c.clients:
            by_site.setdefault(site, set()).add(m.allowed(site, ip))
        for site in c.prefix_sites:
            assert by_site[site] == {True, False}, (c.name, site, by_site[site])
        if c.name == "exact":
            for site in ("big.test", "str.test", "list-only.test", "both.test", "rules-only.test", "odd.test", "nowhere.test", LONG_HOST):
                assert by_site[site] == {True, False}, (site, by_site[site])
            _, rows = c.lines(rotate=1)
            assert {m.allowed(s, ip) for s, ip in rows} == {True, False}


def check_ts_guard():
    """With the reference alone: every class holds accepted and refused tokens where both
    exist, old and fresh ones at both clocks, and the float multiply equals the exact one."""
    by = {}
    for cls, tok in ts_corpus():
        rc, f = ref_parse_float(tok)
        by.setdefault(cls, []).append(rc)
        if rc == 0:
            assert ref_ns(f) == ref_ns_exact(f), tok
    assert set(by) == {"limits", "msec", "spellings", "halfway", "long", "tiny", "edge", "special", "syntax"}
    assert set(by["msec"]) == {0, -1} and set(by["syntax"]) == {0, -1} and set(by["edge"]) == {0, -2}
    for cls in ("limits", "spellings", "halfway", "long", "tiny", "special"):
        assert set(by[cls]) == {0}, (cls, set(by[cls]))
    for now in (NOW_BASE, NOW_EPOCH):
        fl = [ref_line(t, now)[0] for _, t in ts_corpus()]
        assert min(fl.count(0), fl.count(LINE_OLD), fl.count(LINE_ERROR)) >= 40, now
    for cls in ("limits", "msec", "spellings", "halfway", "long"):
        # near the base time or later: fresh at the base clock (the tiny values of "limits" at the epoch clock)
        toks = [t for k, t in ts_corpus() if k == cls and ref_parse_float(t)[0] == 0 and t[:1] != b"-"]
        fresh = sum(1 for t in toks if ref_line(t, NOW_BASE)[0] == 0 or ref_line(t, NOW_EPOCH)[0] == 0)
        # (the $msec neighbours that still parse with an underscore, an exponent or the point moved are
        # past the int64 range: old at any clock)
        assert fresh >= len(toks) - (8 if cls == "msec" else 0), (cls, fresh, len(toks))


check_known_answers()
