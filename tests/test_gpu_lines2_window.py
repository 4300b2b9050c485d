"""k_lines2's 112-byte line window: what is read from it, what is not.

k_lines2 (csrc/lines2.h) copies the 16 B-aligned 112 bytes that hold a line's
first bytes into LDS and takes the header (timestamp, IP, method, host: through
the fourth space), the allow-list lookup and the IP key from there.  A line
whose header does not end inside its window goes to the exact per-line
fallback; literal hits, template checks and inline automata past the window
read HBM or become DFA jobs.  The cases here put the fourth space, the spaces
themselves, the batch end and the rule hits on every boundary of that window
(the 4-byte words and 16-byte pieces of the space masks, byte 64 where the
second mask starts, the window end at 112 minus the line's alignment), and
compare everything with the oracle (tests/parity.py).

A line starting at buffer offset s has alignment sk = s % 16, and its bytes
[0, 112 - sk) are in the window: with sk <= 15 a header whose fourth space is
at line offset <= 96 is always inside.  `fallback_lines` of the scan statistics
therefore may not exceed the number of lines built here with the fourth space
past offset 96, which proves the others ran on k_lines2; and every line with
the fourth space at offset >= 112 must be among them.
"""
import pytest

from banjax_amd import Config, Engine
from oracle import oracle as O
from tests.parity import Pair, oracle_config

S = 1_000_000_000
T0 = 1700000000
WIN = 112  # csrc/lines2.h kL2Win

V4 = ["10.0.0.%d" % i for i in range(1, 5)] + ["100.100.100.100"]
V6 = ["2001:0db8:0000:0000:0000:ff00:0042:832%d" % i for i in range(4)]  # 39 bytes each
METHODS = ["GET", "POST"] + ["M" * n for n in range(5, 25)]  # the method token is not interpreted: any length


def host_of_len(n):
    """A host name of exactly n bytes (4 <= n <= 40), one per length."""
    assert 4 <= n <= 40
    return ("s%02d" % n + "a" * 40)[:n - 4] + ".com"


HOSTS = [host_of_len(n) for n in range(4, 41)]


def _cfg():
    out = ["""
regexes_with_rates:
  - rule: "env"
    regex: '\\/\\.env'
    interval: 5
    hits_per_interval: 2
    decision: nginx_block
  - rule: "all"
    regex: '.*'
    interval: 5
    hits_per_interval: 1000000
    decision: challenge
  - rule: "mac firefox"
    regex: 'Macintosh.*Firefox/\\d+'
    interval: 60
    hits_per_interval: 2
    decision: challenge
  - rule: "any firefox"
    regex: '.*Firefox/\\d+'
    interval: 30
    hits_per_interval: 3
    decision: challenge
per_site_regexes_with_rates:"""]
    for h in HOSTS:
        hr = h.replace(".", r"\.")
        out.append("  %s:" % h)
        out.append("    - rule: '%s wp'\n      regex: 'GET %s GET \\/wp-login\\.php HTTP\\/[0-2.]+ .*'\n"
                   "      interval: 60\n      hits_per_interval: 1\n      decision: challenge" % (h, hr))
        out.append("    - rule: '%s xmlrpc'\n      regex: 'POST %s POST \\/xmlrpc\\.php'\n"
                   "      interval: 60\n      hits_per_interval: 1\n      decision: nginx_block" % (h, hr))
    return "\n".join(out) + "\n"


CFG = _cfg()


def header(ip, method, host, ts=b"%d" % T0):
    return b"%s %s %s %s " % (ts, ip.encode(), method.encode(), host.encode())


def header_with_sp3(p, ip):
    """A header whose fourth space is at line offset p, or None if the fields
    cannot make it: timestamp of 10 or 14 bytes, method of 3..24, host of 4..40."""
    for ts in (b"%d" % T0, b"%d.000" % T0):
        for m in METHODS:
            hl = p - (len(ts) + 1 + len(ip) + 1 + len(m) + 1)
            if 4 <= hl <= 40:
                h = header(ip, m, host_of_len(hl), ts)
                assert len(h) - 1 == p and h.count(b" ") == 4
                return h, m, host_of_len(hl)
    return None


def alignment_batch(filler):
    """A first line of `filler` bytes ('\\n' included: no header, an Error
    line), then lines whose fourth space sits at each of line offsets 58..70 and
    104..118, each with an IPv4 address where the fields can reach the offset
    and with a 39-byte IPv6 address.  Returns (data, fourth-space offsets)."""
    data = bytearray(b"x" * (filler - 1) + b"\n")
    sp3s = []
    k = 0
    for p in list(range(58, 71)) + list(range(104, 119)):
        for ip in (V4[k % len(V4)], V6[k % len(V6)]):
            got = header_with_sp3(p, ip)
            if got is None:  # IPv4 headers end before offset 97, IPv6 ones after 58
                assert (":" in ip) == (p < 60)
                continue
            h, m, host = got
            # the line's own rules: the host's template rule, an '/.env' hit, or nothing
            tail = (b"%s /wp-login.php HTTP/1.1 x" % m.encode(), b"%s /a/.env HTTP/1.1 x" % m.encode(),
                    b"%s /index.html HTTP/1.1 x" % m.encode())[k % 3]
            data += h + tail + b"\n"
            sp3s.append(p)
            k += 1
    return bytes(data), sp3s


def spaces_batch():
    """Lines with two adjacent spaces (an empty host field: the third and the
    fourth space) at every pair of window offsets (q, q + 1) around each word
    boundary of the window, the bytes on both sides of the pair taken from
    0x1F, 0x21, 0xA0, 0x00 (one bit, or the top bit, away from a space)."""
    odd = [b"\x1f", b"\x21", b"\xa0", b"\x00"]
    data = bytearray()
    sp3s = []
    k = 0
    for b in range(16, WIN + 8, 4):
        for q in (b - 2, b - 1, b):
            for w in range(4):
                sk = len(data) % 16
                p = q - sk  # line offset of the third space
                ipl = p - 15  # timestamp (10) sp ip sp <odd byte> G <odd byte> sp sp
                if ipl < 1:
                    continue
                ip = (V4[k % 4] + "0" * 200)[:ipl] if ipl >= 8 else "1" * ipl
                line = b"%d %s %sG%s  %sGET /.env x" % (T0, ip.encode(), odd[w], odd[(w + 1) % 4], odd[(w + 2) % 4])
                assert line[p:p + 2] == b"  " and line.count(b" ", 0, p + 2) == 4
                data += line + b"\n"
                sp3s.append(p + 1)
                k += 1
    return bytes(data), sp3s


def fallback_bounds(sp3s):
    return sum(1 for p in sp3s if p >= WIN), sum(1 for p in sp3s if p > 96)


def test_oracle_accepts_window_inputs():
    """CPU: the oracle parses every built header line (no Error flag but the
    filler's), so the GPU cases compare real decisions, not parse errors."""
    cfg = Config.from_yaml(CFG)
    ocfg = oracle_config(cfg)
    n_rules = len(cfg.all_rules())
    for filler in (1, 7, 16):
        data, sp3s = alignment_batch(filler)
        flags, res, consumed = O.State().consume(ocfg, data, T0 * S, cap=(len(sp3s) + 2) * (n_rules + 1))
        assert consumed == len(data)
        assert flags[0] == O.LINE_ERROR and all(f == 0 for f in flags[1:]), flags
        assert len(res) >= len(sp3s)  # the '.*' rule matches every line
        assert min(sp3s) == 58 and max(sp3s) == 118 and fallback_bounds(sp3s)[1] > 0
    data, sp3s = spaces_batch()
    flags, res, consumed = O.State().consume(ocfg, data, T0 * S, cap=(len(sp3s) + 2) * (n_rules + 1))
    assert consumed == len(data) and all(f == 0 for f in flags)


@pytest.fixture(scope="module")
def engine():
    e = Engine()
    yield e
    e.close()


@pytest.fixture(params=[False, True], ids=["default", "lines"])
def pair(request, engine, monkeypatch):
    if request.param:
        monkeypatch.setenv("BJX_LINES", "1")
    return Pair(CFG, engine)


@pytest.mark.gpu
def test_alignment_and_header_length(engine):
    pair = Pair(CFG, engine)
    for filler in range(1, 17):
        data, sp3s = alignment_batch(filler)
        pair.feed(data, T0 * S)
        lo, hi = fallback_bounds(sp3s)
        fb = engine.scan_stats()["fallback_lines"]
        print("filler %d: %d lines, fallback_lines %d, bounds %d..%d" % (filler, len(sp3s), fb, lo, hi))
        assert lo <= fb <= hi, (filler, fb, lo, hi)
    pair.compare_state(V4 + V6)


@pytest.mark.gpu
def test_space_positions(pair):
    data, sp3s = spaces_batch()
    assert len(sp3s) > 200
    pair.feed(data, T0 * S)
    if pair.engine.scan_stats()["fallback_lines"]:
        assert pair.engine.scan_stats()["fallback_lines"] <= fallback_bounds(sp3s)[1]
    pair.compare_state(V4)


def short_line(k, tail=b"GET /.env"):
    return header(V4[k % 4], "GET", HOSTS[k % 7]) + tail + b"\n"


@pytest.mark.gpu
def test_batch_end(pair):
    long_tail = b"GET /" + b"p" * 120 + b"/.env HTTP/1.1 x"
    for n_short in (1, 2, 3):
        data = b"".join(short_line(k, long_tail) for k in range(5)) + b"".join(short_line(k) for k in range(n_short))
        assert all(len(l) < WIN for l in data.split(b"\n")[-1 - n_short:-1])
        pair.feed(data, T0 * S)
    # a batch of fewer than 128 bytes in all, and one shorter than a window
    for data in (short_line(0) + short_line(1) + short_line(2, b"GET /"), short_line(3)):
        assert len(data) < 128
        pair.feed(data, T0 * S)
    assert len(short_line(3)) < WIN
    # the last wave full, and with a single line
    for n in (64, 65):
        data = b"".join(short_line(k, (b"GET /.env", long_tail, b"GET /wp-login.php HTTP/1.1 x")[k % 3]) for k in range(n))
        assert data.count(b"\n") == n
        pair.feed(data, T0 * S)
    pair.compare_state(V4)


ALLOW_CFG = """
global_decision_lists:
  allow:
    - 20.20.20.20
    - 2001:db8::7
    - ::ffff:5.6.7.8
    - 30.30.30.0/24
    - not-an-ip
per_site_decision_lists:
  "h.com":
    allow:
      - 21.21.21.21
      - 2001:db8::9
      - ::ffff:9.9.9.9
      - 171.171.171.0/24
      - also-no-ip
regexes_with_rates:
  - rule: "all"
    regex: '.*'
    interval: 5
    hits_per_interval: 3
    decision: nginx_block
"""
ALLOW_IPS = ["20.20.20.20", "20.20.20.21", "2001:db8::7", "2001:0db8:0000:0000:0000:0000:0000:0007", "2001:db8::8",
             "5.6.7.8", "::ffff:5.6.7.8", "::ffff:0506:0708", "30.30.30.77", "30.30.31.77", "not-an-ip", "not-an-ip2",
             "21.21.21.21", "2001:db8::9", "9.9.9.9", "::ffff:9.9.9.9", "171.171.171.5", "171.171.172.5", "also-no-ip",
             "also-no-i", "0020.20.20.20", ""]


@pytest.mark.gpu
@pytest.mark.parametrize("lines_env", [False, True], ids=["default", "lines"])
def test_allow_lists_from_window(engine, monkeypatch, lines_env):
    if lines_env:
        monkeypatch.setenv("BJX_LINES", "1")
    pair = Pair(ALLOW_CFG, engine)
    data = bytearray()
    for rep in range(3):
        for ip in ALLOW_IPS:
            for host in ("h.com", "other.org"):
                data += b"x" * ((rep * 5 + len(data)) % 7) + b"\n"  # shifts the next line's alignment
                data += b"%d %s GET %s GET /a HTTP/1.1\n" % (T0, ip.encode(), host.encode())
    out = pair.feed(bytes(data), T0 * S)
    n_ex = sum(1 for f in out.line_flags if f == O.LINE_EXEMPTED)
    # at least the four globally listed forms spelled as listed, on both hosts; and not every line
    assert 3 * 2 * 4 <= n_ex < 3 * 2 * len(ALLOW_IPS)
    assert pair.engine.scan_stats()["fallback_lines"] == 0
    pair.compare_state([ip for ip in ALLOW_IPS if ip])


@pytest.mark.gpu
def test_hits_past_window(pair):
    host = HOSTS[20]
    far = b"/" + b"q" * 150
    ua = b"Mozilla/5.0 (Macintosh; Intel Mac OS X 10.15; rv:109.0) Gecko/20100101 Firefox/115.0"
    lines = []
    for k in range(4):
        ip = V4[k]
        pad = b"z" * k  # moves the hits over the word alignments
        # the host's template rule (cfg3's wp-login shape) and its host-split
        # literal rule, each spelled past the window by a long path before it
        lines.append(header(ip, "GET", host) + b"GET " + far + pad + b"?u=GET %s GET /wp-login.php HTTP/1.1 x" % host.encode())
        lines.append(header(ip, "GET", host) + b"GET " + far + pad + b"?u=POST %s POST /xmlrpc.php" % host.encode())
        # ... and with another host's name in it: the literal hits, the check fails
        lines.append(header(ip, "GET", host) + b"GET " + far + pad + b"?u=GET %s GET /wp-login.php HTTP/1.1 x" % HOSTS[21].encode())
        lines.append(header(ip, "POST", HOSTS[21]) + b"POST " + far + pad + b"?u=POST %s POST /xmlrpc.php" % host.encode())
        # the same two inside the window
        lines.append(header(ip, "GET", host) + b"GET /wp-login.php HTTP/1.1 x" + pad)
        lines.append(header(ip, "POST", host) + b"POST /xmlrpc.php" + pad)
        # a line of more than 4.6 KB with hits at its start, in the middle and at its end
        lines.append(header(ip, "GET", host) + b"GET /.env" + b"a" * (2400 + k) + b"/.env" + b"b" * 2300 + b"/.env")
        lines.append(header(ip, "GET", host) + b"GET /" + b"a" * 4700 + pad + b"/.env HTTP/1.1 " + ua)
        # more hits than a line has slots
        lines.append(header(ip, "GET", host) + b"GET " + b"/.env" * (5 + k) + far + b"/.env Firefox/1")
        # lead rules ('.*' before the literal): their jobs start at the literal's
        # first hit, far into the line, and are stepped from HBM
        lines.append(header(ip, "GET", host) + b"GET " + far + pad + b" HTTP/1.1 " + ua)
        lines.append(header(ip, "GET", host) + b"GET " + far + pad + b" HTTP/1.1 Macintosh Firefox/x Firefox/")
        lines.append(header(ip, "GET", host) + b"GET " + far + pad + b" HTTP/1.1 Firefox/" + b"\xc3\xa9" + b"7")
    data = b"\n".join(lines) + b"\n"
    pair.feed(data, T0 * S)
    pair.feed(data, T0 * S + S)
    pair.compare_state(V4)
