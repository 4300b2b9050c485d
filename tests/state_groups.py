"""Shared by tests/test_state_groups_cpu.py and tests/test_gpu_state_groups.py
(not collected): the worlds and the expected values of bjx_state_query_groups.

Two worlds.  The nets world (tests/state_nets.world_ips through
tests/state_remove.Run): addresses at the edges of every prefix length in
LEN4 x LEN6, several spellings of one address, v4-mapped text, texts that are
no addresses.  The shape world (a snapshot built here and imported): a few
thousand IPs whose /16 groups have the sizes at which the run reduction takes
another path -- B is the number of sorted keys one block of k_grp_runs reduces
(kGrpTile in banjax_amd/csrc/state_ops.h).

Expected answers come from banjax_amd.state_groups.groups, the pure-Python
model; brute() is a second, independent grouping (the ipaddress module and a
dictionary) that tests/test_state_groups_cpu.py holds the model against."""
import ipaddress
import random

from banjax_amd import state_groups, state_nets
from tests import state_nets as N

B = 1024                       # kGrpTile: kBlock (256) threads of kGrpItems (4) keys; the tests hold it against bjx_debug_groups_tile()
LEN4, LEN6 = N.LEN4, N.LEN6
ORDERS = (state_groups.BY_IPS, state_groups.BY_STATES, state_groups.BY_HITS)
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
T0 = N.NOW
COUNTS = ("n_matched", "n_ips_matched", "n_ips_unparsed", "n_states_unparsed", "n_groups", "n_groups_min")


def brute(ips_in_order, states, v4_bits, v6_bits, passes=lambda name, hits, start: True):
    """{(family, network text): [n_ips, n_states, hits sum (unwrapped), newest start]}, and
    (unparsed IPs, their states): every IP text through state_nets.parse_ip, then the
    ipaddress module masks."""
    out, bad_ips, bad_states = {}, 0, 0
    for ip in ips_in_order:
        sel = [(h, s) for n, (h, s) in states.get(ip, {}).items() if passes(n, h, s)]
        if not sel:
            continue
        p = state_nets.parse_ip(ip)
        if p is None:
            bad_ips += 1
            bad_states += len(sel)
            continue
        a = ipaddress.IPv6Address(p[0])
        if a.ipv4_mapped is not None:
            key = (4, str(ipaddress.IPv4Network((int(a.ipv4_mapped), v4_bits), strict=False)))
        else:
            key = (6, str(ipaddress.IPv6Network((int(a), v6_bits), strict=False)))
        g = out.setdefault(key, [0, 0, 0, INT64_MIN])
        g[0] += 1
        g[1] += len(sel)
        g[2] += sum(h for h, _ in sel)
        g[3] = max(g[3], max(s for _, s in sel))
    return out, (bad_ips, bad_states)


def check_invariants(ans):
    """the two sums every answer with all its rows must satisfy; always: the counts' own bounds"""
    assert ans["n_groups_min"] <= ans["n_groups"] <= ans["n_ips_matched"] - ans["n_ips_unparsed"]
    assert ans["n_ips_unparsed"] <= ans["n_ips_matched"] <= ans["n_matched"]
    assert ans["n_states_unparsed"] <= ans["n_matched"]
    if len(ans["rows"]) == ans["n_groups"]:
        assert sum(r.n_ips for r in ans["rows"]) + ans["n_ips_unparsed"] == ans["n_ips_matched"]
        assert sum(r.n_states for r in ans["rows"]) + ans["n_states_unparsed"] == ans["n_matched"]


def check_groups(target, ips, states, **kw):
    """the target's answer equals the model's: every count, every row -> the answer"""
    want = state_groups.groups(ips, states, **kw)
    got = target.state_query_groups(**kw)
    assert {k: got[k] for k in COUNTS} == {k: want[k] for k in COUNTS}, (kw, {k: got[k] for k in COUNTS}, {k: want[k] for k in COUNTS})
    assert got["rows"] == want["rows"], (kw, got["rows"][:3], want["rows"][:3])
    check_invariants(got)
    return got


# ---- the shape world

def shape_sizes():
    """the /16 groups of 10.k.0.0 in key order: 1, B - 1 (so the next group begins exactly at a
    block boundary), B (exactly one block), B + 1, and one over more than two blocks"""
    return [1, B - 1, B, B + 1, 2 * B + 500]


N_V6_SINGLES = 2000


def shape_world(seed=7):
    """-> (ips in snapshot order, states).  IPv4: 10.k.x.y, shape_sizes()[k] addresses in
    10.k.0.0/16; IPv6: N_V6_SINGLES addresses, each alone in its /64.  Every IP has "r", every
    fifth "s" as well; hits and starts differ from IP to IP.  The order is shuffled, so ids say
    nothing about keys."""
    ips = []
    for k, n in enumerate(shape_sizes()):
        ips += ["10.%d.%d.%d" % (k, j >> 8, j & 255) for j in range(n)]
    ips += ["2001:db8:%x:%x::%x" % (j >> 8, j & 255, j + 1) for j in range(N_V6_SINGLES)]
    random.Random(seed).shuffle(ips)
    states = {}
    for j, ip in enumerate(ips):
        d = {"r": (1 + j % 7, T0 + j)}
        if j % 5 == 0:
            d["s"] = (j % 3, T0 - j)
        states[ip] = d
    return ips, states


def extreme_world():
    """hits sums that wrap and starts at both ends of int64, in two /24s and one /64"""
    ips = ["192.0.2.1", "192.0.2.2", "192.0.2.3", "198.51.100.1", "198.51.100.2", "2001:db8::1", "2001:db8::2", "not an ip"]
    states = {
        "192.0.2.1": {"r": (INT64_MAX, INT64_MIN)},
        "192.0.2.2": {"r": (INT64_MAX, INT64_MIN), "s": (5, INT64_MIN)},     # the /24's sum wraps round to 10; newest INT64_MIN
        "192.0.2.3": {"r": (7, INT64_MIN)},
        "198.51.100.1": {"r": (INT64_MIN, INT64_MAX)},
        "198.51.100.2": {"r": (-1, 0), "s": (INT64_MIN, -1)},                # wraps upwards; newest INT64_MAX
        "2001:db8::1": {"r": (INT64_MIN, INT64_MIN)},                       # hits_sum INT64_MIN: the last place by hits
        "2001:db8::2": {"s": (0, INT64_MIN)},
        "not an ip": {"r": (INT64_MAX, INT64_MAX)},
    }
    return ips, states
