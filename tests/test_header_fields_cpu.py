"""The timestamp and client-IP parsers three ways on the host: the host build of
the code the kernels share (go_parse_float, parse_float_fast, ns_from_seconds,
go_parse_addr in bjx_common.h; parse_allow_entry in allow_entry.h, through
tests/cpu/header_fields.cpp), the Python references of tests/header_fields.py
(float() / float.fromhex(), ipaddress, a model of CheckIsAllowed written from
the reference's Go), and the oracle (strtod; its own C restatement of the
allow lists).  Return code, value bits, nanoseconds, the 16 address bytes and
the IPv4 flag, the subnet tables and the per-line flags all take part; there
is no exception list.

One difference of representation, not of value: Go's ParseFloat("nan") returns
math.NaN(), bits 0x7FF8000000000001; Python's and C's NaN have other payloads,
so for a NaN the references say "a NaN" and the host build's bits are held
against Go's constant (header_fields.NAN_BITS).

tests/test_gpu_header_fields.py runs the same corpora through the kernels."""
import ctypes
import math
import os
import struct
import subprocess
import tempfile

import pytest

from banjax_amd import Config
from oracle import oracle as O
from tests import header_fields as H
from tests.parity import oracle_config

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="bjx_hf_")
    so = os.path.join(d, "libhf.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", so,
                    os.path.join(HERE, "cpu", "header_fields.cpp")], check=True)
    L = ctypes.CDLL(so)
    p = ctypes.c_void_p
    L.bjx_test_parse_floats.argtypes = [ctypes.c_char_p, p, ctypes.c_uint64, ctypes.c_int, p, p, p]
    L.bjx_test_parse_floats.restype = None
    L.bjx_test_ns_from_seconds.argtypes = [p, ctypes.c_uint64, p]
    L.bjx_test_ns_from_seconds.restype = None
    L.bjx_test_parse_addrs.argtypes = [ctypes.c_char_p, p, ctypes.c_uint64, p, p, p]
    L.bjx_test_parse_addrs.restype = None
    L.bjx_test_allow_entry.argtypes = [ctypes.c_char_p, ctypes.c_uint32, p, p, p]
    L.bjx_test_allow_entry.restype = ctypes.c_int
    return L


def _pack(tokens):
    off = [0]
    for t in tokens:
        off.append(off[-1] + len(t))
    return b"".join(tokens), (ctypes.c_uint64 * len(off))(*off)


def host_floats(lib, tokens, fast=False):
    """-> [(rc, bits, ns)] of go_parse_float (fast: parse_float_fast) on the host build."""
    buf, off = _pack(tokens)
    n = len(tokens)
    rc, bits, ns = (ctypes.c_int32 * n)(), (ctypes.c_uint64 * n)(), (ctypes.c_int64 * n)()
    lib.bjx_test_parse_floats(buf, off, n, 1 if fast else 0, rc, bits, ns)
    return list(zip(rc, bits, ns))


def host_addrs(lib, texts):
    buf, off = _pack(texts)
    n = len(texts)
    ok, out, is4 = (ctypes.c_uint8 * n)(), (ctypes.c_uint8 * (16 * n))(), (ctypes.c_uint8 * n)()
    lib.bjx_test_parse_addrs(buf, off, n, ok, out, is4)
    raw = bytes(out)
    return [(raw[16 * k:16 * k + 16], bool(is4[k])) if ok[k] else None for k in range(n)]


def check_floats(lib, tokens):
    """Host build == Python reference == oracle for every token; where the fast parser
    accepts, the general algorithm (reached with an "e0" suffix, which the fast parser
    declines by spelling alone) gives the same bits.  Returns the count per return code."""
    got = host_floats(lib, tokens)
    fast = host_floats(lib, tokens, fast=True)
    counts = {0: 0, -1: 0, -2: 0}
    again = []
    for tok, (rc, bits, ns), (frc, fbits, fns) in zip(tokens, got, fast):
        wrc, wf = H.ref_parse_float(tok)
        orc, of = O.parse_float(tok)
        assert rc == wrc == orc, (tok, rc, wrc, orc)
        counts[rc] += 1
        if rc == -1:
            assert frc == 1, tok
            continue
        assert bits == H.f64_bits(wf), (tok, hex(bits), wf.hex())
        assert (of != of and wf != wf) or H.f64_bits(of) == bits, (tok, of.hex(), hex(bits))
        if rc == 0:
            assert ns == H.ref_ns(wf) == H.ref_ns_exact(wf), (tok, ns, H.ref_ns(wf), H.ref_ns_exact(wf))
        assert (frc == 0) == H.fast_accepts(tok), tok
        if frc == 0:
            assert rc == 0 and (fbits, fns) == (bits, ns), (tok, hex(fbits), hex(bits))
            again.append(tok)
    general = [t + b"e0" for t in again]
    assert all(r[0] == 1 for r in host_floats(lib, general, fast=True))
    for tok, (rc, bits, ns), t0 in zip(general, host_floats(lib, general), again):
        assert (rc, bits) == (0, H.f64_bits(H.ref_parse_float(t0)[1])), (tok, rc, hex(bits))
    counts["fast"] = len(again)
    return counts


def test_module_guards():
    """The corpora, with the references alone: accepted and refused tokens in every class
    that has both, fresh and old lines at both clocks, allowed and refused clients at every
    prefix site, and the float multiply equal to the exact one."""
    H.check_known_answers()
    H.check_ts_guard()
    H.check_allow_guard()
    assert 2000 <= len(H.ts_corpus()) <= 4000
    assert len(H.narrow_tokens()) > 1000


def test_timestamp_corpus(lib):
    c = check_floats(lib, [t for _, t in H.ts_corpus()])
    assert c[0] > 1800 and c[-1] > 80 and c[-2] >= 5 and c["fast"] > 500, c


def test_known_answers_host(lib):
    """The answers that depend on no library, on the host build."""
    def one(tok):
        return host_floats(lib, [tok])[0]
    assert one(b"1.7976931348623157e308")[:2] == (0, 0x7FEFFFFFFFFFFFFF)
    assert one(b"1.7976931348623159e308")[:2] == (-2, 0x7FF0000000000000) and one(b"-1e309")[:2] == (-2, 0xFFF0000000000000)
    assert one(b"4.9e-324")[:2] == (0, 1) and one(b"3e-324")[:2] == (0, 1) and one(b"2e-324")[:2] == (0, 0)
    assert one(b"nan")[:2] == (0, H.NAN_BITS) and one(b"-0") == (0, 1 << 63, 0)
    assert one(b"0x_1_2.3_4_5p+1_2")[:2] == (0, struct.unpack("<Q", struct.pack("<d", 74565.0))[0])
    assert one(b"9223372036.854775")[2] == 2 ** 63 - 1024 and one(b"9223372036.854776")[2] == H.INT64_MIN
    assert one(b"-9223372036.854776")[2] == H.INT64_MIN and one(b"-9223372036.854775")[2] == -(2 ** 63 - 1024)
    for t in H.ACCEPT:
        assert one(t)[0] == 0, t
    for t in H.REJECT:
        assert one(t)[0] == -1, t


def test_ns_from_seconds_edges(lib):
    """int64(f * 1e9) around both ends of the int64 range, doubles taken bit by bit."""
    fs = []
    for base in (9223372036.854775, -9223372036.854775, 1.7e9, 4.0, 0.0, 5e-324, 1e-9, 1.7976931348623157e308):
        b = struct.unpack("<Q", struct.pack("<d", base))[0]
        fs += [struct.unpack("<d", struct.pack("<Q", (b + d) % (1 << 64)))[0] for d in range(-40, 41)]
    fs += [math.inf, -math.inf, math.nan, -0.0, 9223372036.854776, 2.0 ** 63, -(2.0 ** 63), 2.0 ** 63 / 1e9]
    n = len(fs)
    bits = (ctypes.c_uint64 * n)(*[struct.unpack("<Q", struct.pack("<d", f))[0] for f in fs])
    ns = (ctypes.c_int64 * n)()
    lib.bjx_test_ns_from_seconds(bits, n, ns)
    for f, g in zip(fs, ns):
        assert g == H.ref_ns(f) == H.ref_ns_exact(f), (f.hex(), g)
    assert H.INT64_MIN in list(ns) and max(ns) == 2 ** 63 - 1024


@pytest.mark.parametrize("seed", [1, 2])
def test_float_sweep(lib, seed):
    """51,000 tokens per seed, a third each: exact halfway decimals of random doubles and
    subnormals (last digit perturbed), random decimals with exponents -345..330, random hex
    floats with exponents -1150..1100; one in twenty with a byte replaced."""
    c = check_floats(lib, H.sweep_floats(51_000, seed))
    assert c[0] > 40_000 and c[-1] > 500 and c[-2] > 500, c


def test_ip_corpus_and_sweep(lib):
    """go_parse_addr == ipaddress (any '%' refused) == the oracle: the 16 bytes and, against
    the reference, the IPv4-text flag; over every client and entry text of the allow-list
    corpus and 100,000 generated texts."""
    texts = list(dict.fromkeys([ip for c in H.allow_cases() for _, ip in c.clients] +
                               [e[2] for c in H.allow_cases() for e in c.entries] + H.sweep_ips(100_000, 3)))
    raw = [t.encode("latin-1") for t in texts]
    got = host_addrs(lib, raw)
    n_ok = 0
    for t, b, g in zip(texts, raw, got):
        want = H.ref_parse_ip(t)
        assert g == want, (t, g, want)
        assert O.parse_ip(b) == (want[0] if want else None), t
        n_ok += want is not None
    assert len(texts) > 100_000 and 20_000 < n_ok < len(texts) - 20_000, (len(texts), n_ok)


def host_entry(lib, text):
    net, mask, nl = (ctypes.c_uint8 * 16)(), (ctypes.c_uint8 * 16)(), ctypes.c_uint32()
    b = text.encode("latin-1")
    k = lib.bjx_test_allow_entry(b, len(b), net, mask, ctypes.byref(nl))
    assert k >= 0, text
    if k == 0:
        return None
    if k == 1:
        return ("addr", bytes(net))
    return ("sub", nl.value, bytes(net)[:nl.value], bytes(mask)[:nl.value])


def test_allow_entry_tables(lib):
    """parse_allow_entry's tables (a single address, or netlen / net / mask) equal the model's
    for every entry of the corpus, every prefix length on IPv4, IPv6 and v4-mapped bases with
    host bits set, and the odd mask texts."""
    texts = [e[2] for c in H.allow_cases() for e in c.entries]
    for n in range(0, 130):
        texts += ["165.90.195.61/%d" % n, "a55a:c33c:8001:ff7f:1234:5678:9abc:def1/%d" % n, "::ffff:154.101.60.195/%d" % n,
                  "::ffff:255.255.255.255/%d" % n, "ffff:ffff:ffff:ffff:ffff:ffff:ffff:ffff/%d" % n, "::/%d" % n, "0.0.0.0/%d" % n]
    texts += ["1.2.3.4/", "1.2.3.4/ 8", "1.2.3.4/8 ", "1.2.3.4/-1", "1.2.3.4/0x8", "1.2.3.4/8/8", "/8", "1.2.3.4/00000000000000000008",
              "1.2.3.4/16777214", "1.2.3.4/16777215", "::1/0128", "::1%lo/128", "1.2.3/8", "01.2.3.4/8", "::ffff:1.2.3.4/96",
              "::ffff:1.2.3.4/95", "::fffe:1.2.3.4/96", "0:0:0:0:0:ffff:102:304/120", "::1.2.3.4/120"]
    kinds = {None: 0, "addr": 0, "sub": 0}
    for t in texts:
        got, want = host_entry(lib, t), H.model_entry(t)
        assert got == want, (t, got, want)
        kinds[want[0] if want else None] += 1
    assert min(kinds.values()) > 100, kinds
    # the To4 switch: a v4-mapped network is a 4-byte one from /96 on, a 16-byte one below
    assert host_entry(lib, "::ffff:1.2.3.4/96") == ("sub", 4, bytes(4), bytes(4))
    assert host_entry(lib, "::ffff:1.2.3.4/95")[1] == 16
    assert host_entry(lib, "::ffff:1.2.3.4/121") == ("sub", 4, bytes([1, 2, 3, 0]), bytes([255, 255, 255, 128]))


def _oracle_flags(yaml_text, data, now_ns):
    cfg = Config.from_yaml(yaml_text)
    oc, st = oracle_config(cfg), O.State()
    flags, _, consumed = st.consume(oc, data, now_ns, cap=2 * (data.count(b"\n") + 1))
    assert consumed == len(data)
    return flags, st


@pytest.mark.parametrize("now_ns", [H.NOW_BASE, H.NOW_EPOCH, H.INT64_MAX])
def test_oracle_lines_equal_reference(now_ns):
    """The oracle's per-line flags and each line's state (start = the line's nanoseconds)
    equal the reference's over the corpus."""
    toks = [t for _, t in H.ts_corpus()]
    flags, st = _oracle_flags(H.RULES_YAML, H.ts_batch(toks), now_ns)
    want = [H.ref_line(t, now_ns) for t in toks]
    assert flags == [w[0] for w in want]
    for k, (fl, ns) in enumerate(want):
        assert st.get(H.line_ip(k), "all") == ((1, ns) if fl == 0 else None), (toks[k], k)
    assert len(st) == sum(1 for w in want if w[0] == 0)


def test_oracle_allow_lists_equal_model():
    """The oracle's Exempted flags equal the Python model's, line by line, for every allow-list
    case and with the sites rotated."""
    for c in H.allow_cases():
        m = c.model()
        for rot in (0, 1):
            data, rows = c.lines(rot)
            flags, _ = _oracle_flags(c.yaml(), data, H.NOW_BASE)
            want = [H.LINE_EXEMPTED if m.allowed(s, ip) else 0 for s, ip in rows]
            bad = [(rows[k], flags[k], want[k]) for k in range(len(rows)) if flags[k] != want[k]]
            assert not bad, (c.name, rot, bad[:5])
