"""Shared by tests/test_state_names_cpu.py and tests/test_gpu_state_names.py
(not collected): the worlds and the expected values of bjx_state_query_names.

The nets world (tests/state_nets.build_world through tests/state_remove.Run:
three rule names over a few hundred IPs, states made by real batches) and the
worlds built here as snapshots and imported: the shape world (name shapes,
ties on every primary key, every histogram bucket), the extreme world (hits
and starts at both ends of int64, sums that wrap), the skewed world (one name
holds more than 99% of the states), and count_world(n): n names over a handful
of IPs, for the boundary between the LDS path and the global path.

Expected answers come from banjax_amd.state_names.names, the pure-Python
model; brute() is a second, independent aggregation (one dictionary over the
states) that tests/test_state_names_cpu.py holds the model against."""
from banjax_amd import state_names
from tests import state_nets as N

ORDERS = (state_names.BY_STATES, state_names.BY_HITS, state_names.BY_MAX_HITS, state_names.BY_NEWEST, state_names.BY_NAME)
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
T0 = N.NOW
COUNTS = ("n_matched", "n_ips_matched", "n_names", "n_names_min")

LONG = b"L" * 300
HIGH = b"\xc3\xa9gle\xff\x80"
EMPTY = b""


def _b(x):
    return x if isinstance(x, bytes) else str(x).encode()


def brute(ips_in_order, states, passes=lambda ip, name, hits, start: True):
    """{name bytes: [n_states, hits sum (unwrapped), max hits, newest, oldest, [hits of every state]]}"""
    out = {}
    for ip in dict.fromkeys(ips_in_order):
        for n, (h, s) in states.get(ip, {}).items():
            if not passes(ip, n, h, s):
                continue
            a = out.setdefault(_b(n), [0, 0, INT64_MIN, INT64_MIN, INT64_MAX, []])
            a[0] += 1
            a[1] += h
            a[2] = max(a[2], h)
            a[3] = max(a[3], s)
            a[4] = min(a[4], s)
            a[5].append(h)
    return out


def brute_hist(hits):
    """the histogram by the buckets' bounds, not by bit_length"""
    hist = [0] * 16
    for h in hits:
        if h <= 0:
            hist[0] += 1
        elif h >= 1 << 14:
            hist[15] += 1
        else:
            hist[next(b for b in range(1, 15) if (1 << (b - 1)) <= h < (1 << b))] += 1
    return tuple(hist)


def check_invariants(ans):
    assert ans["n_names_min"] <= ans["n_names"] <= ans["n_matched"] and ans["n_ips_matched"] <= ans["n_matched"]
    for r in ans["rows"]:
        assert sum(r.hist) == r.n_states > 0 and r.oldest_start_ns <= r.newest_start_ns, r
    if len(ans["rows"]) == ans["n_names"]:
        assert sum(r.n_states for r in ans["rows"]) == ans["n_matched"]


def check_names(target, ips, states, **kw):
    """the target's answer equals the model's: every count, every field of every row -> the answer"""
    want = state_names.names(ips, states, **kw)
    got = target.state_query_names(**kw)
    assert {k: got[k] for k in COUNTS} == {k: want[k] for k in COUNTS}, (kw, {k: got[k] for k in COUNTS}, {k: want[k] for k in COUNTS})
    assert got["rows"] == want["rows"], (kw, [r for r, w in zip(got["rows"], want["rows"]) if r != w][:2],
                                         [w for r, w in zip(got["rows"], want["rows"]) if r != w][:2])
    check_invariants(got)
    return got


def check_rows_against_query(target, rows, **filt):
    """the contract's cross-checks against bjx_state_query, for every row (filt: the names
    query's filter, without a name)"""
    floor = filt.get("min_hits", INT64_MIN)
    rest = {k: v for k, v in filt.items() if k != "min_hits"}
    for r in rows:
        a = target.state_query(name=r.name, order="hits", limit=1, **filt)
        assert a["n_matched"] == a["n_ips_matched"] == r.n_states and a["rows"][0][2] == r.max_hits, (r, a)
        a = target.state_query(name=r.name, order="start", limit=1, **filt)
        assert a["rows"][0][3] == r.newest_start_ns and a["rows"][0][1] == r.name, (r, a)
        for k in range(15):
            if floor <= 1 << k:
                a = target.state_query(name=r.name, min_hits=1 << k, limit=0, **rest)
                assert a["n_matched"] == sum(r.hist[k + 1:]), (r, k, a)


# ---- the worlds built as snapshots

N_SHAPE_IPS = 48


def shape_world():
    """-> (ips in snapshot order, states), names as bytes.  48 IPs.
    "all": on every IP (so on every shard of a node), hits 1 + k.
    "solo": one state (so on exactly one shard).
    "hist": hits 1, 2, 4, .. 2^14, 2^20 and their neighbours: every bucket 1..15 and both edges of each.
    "zero": hits 0 and below only: everything in bucket 0.
    "tie1" / "tie2": the same four (hits, start) pairs on different IPs: tied on every primary key.
    "a" / "ab": a prefix of another name; b"": the empty name; HIGH: bytes from 0x80 up; LONG: 300 bytes."""
    ips = ["10.7.%d.%d" % (k // 8, k % 8) for k in range(N_SHAPE_IPS)]
    st = {ip: {} for ip in ips}
    for k, ip in enumerate(ips):
        st[ip][b"all"] = (1 + k, T0 + 1000 * k)
    st[ips[17]][b"solo"] = (3, T0 + 5)
    edges = sorted({v for b in range(15) for v in ((1 << b) - 1, 1 << b, (1 << b) + 1)} | {1 << 20, 0, -1})
    assert len(edges) <= N_SHAPE_IPS
    for k, v in enumerate(edges):
        st[ips[k]][b"hist"] = (v, T0 - k)
    for k in range(6):
        st[ips[30 + k]][b"zero"] = (-k, T0 + 77 + k)
    for k in range(4):
        st[ips[k]][b"tie1"] = (5 + k, T0 + 100 + k)
        st[ips[20 + k]][b"tie2"] = (5 + k, T0 + 100 + k)
    for k in range(5):
        st[ips[2 * k]][b"a"] = (2, T0 + 9000 - k)
    for k in range(3):
        st[ips[3 * k + 1]][b"ab"] = (40, T0 + 3 + k)
    for k in range(7):
        st[ips[5 * k]][EMPTY] = (9, T0 + 50_000 + k)
    for k in range(2):
        st[ips[k + 8]][HIGH] = (300 + k, T0 + 2)
    st[ips[39]][LONG] = (1 << 13, T0 + 60_000)
    return ips, st


def extreme_world():
    """hits and starts at both ends of int64, sums that wrap in both directions"""
    ips = ["192.0.2.%d" % k for k in range(1, 7)]
    st = {
        ips[0]: {"up": (INT64_MAX, INT64_MIN), "down": (INT64_MIN, INT64_MAX), "ends": (INT64_MAX, INT64_MIN)},
        ips[1]: {"up": (INT64_MAX, INT64_MIN + 1), "down": (INT64_MIN, 0), "ends": (INT64_MIN, INT64_MAX)},   # up wraps to -2, down to 0
        ips[2]: {"up": (12, -1), "down": (-1, INT64_MIN)},
        ips[3]: {"neg": (-5, 7), "zero": (0, 0)},
        ips[4]: {"neg": (INT64_MIN, 8), "zero": (0, -1)},
        ips[5]: {"neg": (-1, 9)},
    }
    return ips, st


N_SKEW = 3000


def skewed_world():
    """3000 IPs that all hold "big" (hits 1..64: every lane of a wave on the same name), 20 of
    them "small", 5 "tiny": "big" is more than 99% of the states"""
    ips = ["10.%d.%d.%d" % (20 + (k >> 16), (k >> 8) & 255, k & 255) for k in range(N_SKEW)]
    st = {}
    for k, ip in enumerate(ips):
        st[ip] = {"big": (1 + k % 64, T0 + k)}
        if k % 150 == 0:
            st[ip]["small"] = (k, T0 - k)
        if k % 600 == 7:
            st[ip]["tiny"] = (-3, T0)
    return ips, st


def count_world(n):
    """n names over 5 IPs: name k on IP k % 5, every third also on IP (k + 2) % 5; hits and starts differ"""
    ips = ["10.9.0.%d" % k for k in range(5)]
    st = {ip: {} for ip in ips}
    for k in range(n):
        nm = b"n%05d" % k
        st[ips[k % 5]][nm] = (1 + k % 40, T0 + k)
        if k % 3 == 0:
            st[ips[(k + 2) % 5]][nm] = (k, T0 - k)
    return ips, st
