"""The two header fields out of the engine, bit for bit (corpora and references:
tests/header_fields.py; the same values on the host build and the oracle:
tests/test_header_fields_cpu.py).

Timestamps: one ALWAYS rule whose window never ends and whose limit never
trips, one client IP per line, so after a batch the exported state holds each
fresh line's (ip, start) and start is the nanoseconds the device computed
from the token: its f64 divide and multiply, parse_ts_msec's word loads, the
Decimal scratch of the general ParseFloat.  start must equal the reference's
int64(float(token) * 1e9) exactly, the line flags its Error / OldLine, and the
lines without a state must be exactly those.  Through each per-line path:
k_lines2, k_lines (BJX_NO_LINES2), and k_parse_match on every line (more than
128 global rules); the tokens the line kernels do not parse are counted on the
fallback list.  Client IPs: the allow-list corpus through the oracle pair,
the Exempted flags also equal to the Python model of CheckIsAllowed.

Each batch is a few thousand short lines."""
import pytest

from banjax_amd import Engine, snapshot
from tests import header_fields as H
from tests.parity import Pair

pytestmark = pytest.mark.gpu

# more than 128 global rules: no line pass, k_parse_match parses and decides every line
WIDE_YAML = H.RULES_YAML + "".join(
    "  - rule: \"n%03d\"\n    regex: 'qq%03dzz'\n    interval: 5\n    hits_per_interval: 5\n    decision: challenge\n" % (k, k)
    for k in range(130))
ONE_ALLOW = "global_decision_lists:\n  allow:\n    - 203.0.113.77\n"
PATHS = ["k_lines2", "k_lines", "k_parse_match"]


@pytest.fixture(scope="module")
def engine():
    e = Engine()
    yield e
    e.close()


def make_pair(engine, path, monkeypatch, extra=""):
    if path == "k_lines":
        monkeypatch.setenv("BJX_NO_LINES2", "1")  # read when the ruleset is bound
    return Pair((WIDE_YAML if path == "k_parse_match" else H.RULES_YAML) + extra, engine)


def run_ts(pair, engine, path, lines, now_ns, tail=b""):
    """lines: [(token, line bytes)], line k's IP H.line_ip(k0 + k) for the k0 its builder used.
    Oracle parity through the pair, then flags and every state against the reference."""
    data = b"".join(ln for _, ln in lines) + tail
    before = {ip for ip in snapshot.parse(engine.state_export())[1]}
    out = pair.feed(data, now_ns)
    assert engine.line_kernel()[0] == path
    assert out.consumed_bytes == len(data) - len(tail) and out.n_lines == len(lines)
    want = [H.ref_line(tok, now_ns) for tok, _ in lines]
    flags = list(out.line_flags)
    bad = [(lines[k][0], flags[k], want[k]) for k in range(len(lines)) if flags[k] != want[k][0]]
    assert not bad, bad[:8]
    states = snapshot.parse(engine.state_export())[1]
    n_fresh = 0
    for (tok, ln), (fl, ns) in zip(lines, want):
        ip = ln.split(b" ", 2)[1]
        if fl == 0:
            n_fresh += 1
            assert states.get(ip) == {b"all": (1, ns)}, (tok, ip, states.get(ip), ns)
        else:
            assert ip not in states, (tok, ip, fl, states[ip])
    assert len(states) - len(before) == n_fresh
    assert engine.scan_stats()["fallback_lines"] == H.fallback_lines(data, path)
    return out, want


def corpus_lines(tokens, k0, host="h.test"):
    return [(t, H.ts_line(t, k0 + k, host)) for k, t in enumerate(tokens)]


@pytest.mark.parametrize("path", PATHS)
def test_timestamp_values(engine, path, monkeypatch):
    """The corpus: a batch within a minute of the base time (the rate-limit stage sorts 12-byte
    records), the whole corpus at a clock of 5 s, where the tiny values are fresh and every
    other fresh line lies decades ahead (16-byte records), and the whole corpus at the base
    clock with one allow entry bound, so check_is_allowed is part of the path."""
    toks = [t for _, t in H.ts_corpus()]
    pair = make_pair(engine, path, monkeypatch)
    narrow = H.narrow_tokens()
    run_ts(pair, engine, path, corpus_lines(narrow, 0), H.NOW_BASE)
    _, want = run_ts(pair, engine, path, corpus_lines(toks, 100_000), H.NOW_EPOCH)
    assert sum(1 for fl, ns in want if fl == 0 and ns < 10 ** 6) > 60  # the tiny values have states here
    if path != "k_parse_match":
        # the general-ParseFloat lines went through k_parse_match<true>: most of the corpus
        assert engine.scan_stats()["fallback_lines"] > 1200
    pair = make_pair(engine, path, monkeypatch, ONE_ALLOW)
    run_ts(pair, engine, path, corpus_lines(toks, 0), H.NOW_BASE)


def placement_lines():
    """$msec, fast-path and general tokens on lines that start at each of the 16 alignments (the
    line before padded), a 100-byte host after an ordinary timestamp, and a $msec line last."""
    toks = [b"%d.%03d" % (H.T0 + 6, 137), b"%d.1234567" % (H.T0 + 7), b"%d.5" % (H.T0 + 2), b"%d" % (H.T0 + 8),
            b"0%d.25" % (H.T0 + 3), b"%d.123456789" % (H.T0 + 4), b"%d.250e0" % (H.T0 + 5)]
    lines, pos, k, seen = [], 0, 0, set()
    for tok in toks:
        for a in range(16):
            for host in ("h.test", H.LONG_HOST) if tok is toks[0] or tok is toks[1] else ("h.test",):
                fill = H.ts_line(b"%d.000" % (H.T0 + 1), k)
                fill = H.ts_line(b"%d.000" % (H.T0 + 1), k, pad=(a - pos - len(fill)) % 16)
                lines.append((fill.split(b" ", 1)[0], fill))
                pos += len(fill)
                assert pos % 16 == a
                ln = H.ts_line(tok, k + 1, host)
                lines.append((tok, ln))
                seen.add((tok, a, host))
                pos += len(ln)
                k += 2
    assert len(seen) == 16 * (len(toks) + 2)
    lines.append((toks[0], H.ts_line(toks[0], k)))
    return lines, k + 1


@pytest.mark.parametrize("path", PATHS)
def test_placement(engine, path, monkeypatch):
    """Every alignment of the line start; the $msec line as the batch's last line with nothing
    after its newline, then again as an unterminated tail, which is not consumed; a batch of
    three lines, whose windows run past the end of the batch (the last wave reads its windows
    byte by byte)."""
    pair = make_pair(engine, path, monkeypatch, ONE_ALLOW)
    lines, k = placement_lines()
    out, _ = run_ts(pair, engine, path, lines, H.NOW_BASE)
    assert set(out.line_flags) == {0}
    msec = b"%d.%03d" % (H.T0 + 6, 999)
    tail = H.ts_line(msec, k + 50)[:-1]
    more = corpus_lines([b"%d.5" % H.T0, b"%d.25e0" % H.T0, msec], k)
    run_ts(pair, engine, path, more, H.NOW_BASE, tail=tail)
    run_ts(pair, engine, path, corpus_lines([msec], k + 10), H.NOW_BASE, tail=tail[:20])
    run_ts(pair, engine, path, corpus_lines([msec], k + 20), H.NOW_BASE)


@pytest.mark.parametrize("path", PATHS)
def test_old_line_boundary(engine, path, monkeypatch):
    """One value in spellings that reach all three parsers, at clocks one nanosecond either
    side of now - ts = 10 s and at the largest clock: OldLine is "more than 10 s"."""
    v = H.T0 + 5.246
    ns = H.ref_ns(v)
    toks = [b"1700000005.246", b"1700000005.2460", b"01700000005.246", b"1700000005.246000000000", b"1700000005.246e0",
            b"1700000005246e-3", b"1.700000005246E9", b"+1700000005.246", b"1_700_000_005.246", v.hex().encode(),
            b"1700000005.246" + b"0" * 30, b"0x%xp-22" % int(v * 2 ** 22), b"1700000005.24600000000000000000001"]
    assert all(H.ref_parse_float(t) == (0, v) for t in toks)
    assert sum(map(H.fast_accepts, toks)) == 3 and len(toks[0]) == 14
    pair = make_pair(engine, path, monkeypatch)
    for b, (now, old) in enumerate([(ns + H.OLD_NS - 1, False), (ns + H.OLD_NS, False), (ns + H.OLD_NS + 1, True),
                                    (H.INT64_MAX, True)]):
        out, want = run_ts(pair, engine, path, corpus_lines(toks, 100 * b), now)
        assert [fl for fl, _ in want] == [H.LINE_OLD if old else 0] * len(toks)


@pytest.mark.parametrize("path", ["k_lines2", "k_lines"])
@pytest.mark.parametrize("case", [c.name for c in H.allow_cases()])
def test_allow_lists(engine, case, path, monkeypatch):
    """The allow-list corpus against the oracle (every flag, result and state) and the Exempted
    flags against the Python model, line by line; then the sites rotated over the same clients.
    The 100-byte host's lines leave k_lines2's window: their IPs meet the allow list in
    k_parse_match<true>."""
    c = next(x for x in H.allow_cases() if x.name == case)
    m = c.model()
    if path == "k_lines":
        monkeypatch.setenv("BJX_NO_LINES2", "1")
    pair = Pair(c.yaml(), engine)
    for rot in (0, 1):
        data, rows = c.lines(rot)
        out = pair.feed(data, H.NOW_BASE)
        assert engine.line_kernel()[0] == path
        want = [H.LINE_EXEMPTED if m.allowed(s, ip) else 0 for s, ip in rows]
        flags = list(out.line_flags)
        bad = [(rows[k], flags[k], want[k]) for k in range(len(rows)) if flags[k] != want[k]]
        assert not bad, bad[:8]
        assert min(want.count(0), want.count(H.LINE_EXEMPTED)) > 50
        if case == "exact" and path == "k_lines2":
            n_long = sum(1 for s, _ in rows if s == H.LONG_HOST)
            assert n_long > 40 and engine.scan_stats()["fallback_lines"] >= n_long
