"""bjx_state_query_groups without a GPU: the symbols, struct sizes and argument
checks of the library, the pure-Python model (banjax_amd/state_groups.py)
against a brute-force grouping over the worlds the GPU tests use -- which
shows those worlds are telling -- and the host header
(banjax_amd/csrc/state_groups.h: spec and filter checks, key packing and
masking, the sort's bit ranges, the row comparator, the node merge with its
cap) built for the host from tests/cpu/groups_host.cpp, a program with its own
main."""
import ctypes
import os
import random
import subprocess
import tempfile

from banjax_amd import _lib, state_groups, state_nets
from tests import header_fields as HF
from tests import state_groups as G
from tests import state_nets as N

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu", "groups_host.cpp")
INT64_MIN, INT64_MAX = G.INT64_MIN, G.INT64_MAX


def test_symbols_structs_and_bad_arguments():
    L = _lib.lib()
    for name in ("bjx_state_query_groups", "bjx_node_state_query_groups"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert ctypes.sizeof(_lib.GroupSpec) == 24 and ctypes.sizeof(_lib.GroupRow) == 56 and ctypes.sizeof(_lib.StateGroups) == 72
    assert [k for k, _ in _lib.GroupSpec._fields_] == ["v4_bits", "v6_bits", "order", "limit", "min_ips"]
    assert [k for k, _ in _lib.GroupRow._fields_] == ["addr", "family", "bits", "n_ips", "n_states", "hits_sum", "newest_start_ns"]
    assert [k for k, _ in _lib.StateGroups._fields_] == ["n_matched", "n_ips_matched", "n_ips_unparsed", "n_states_unparsed",
                                                          "n_groups", "n_groups_min", "n_rows", "rows", "device_ms"]
    assert (_lib.GROUPS_BY_IPS, _lib.GROUPS_BY_STATES, _lib.GROUPS_BY_HITS, _lib.GROUPS_MAX_ROWS) == (0, 1, 2, 65536)
    f = _lib.StateFilter(_lib.Str(None, 0), _lib.Str(None, 0), INT64_MIN, INT64_MIN, INT64_MAX, 0, 0)
    g = _lib.GroupSpec(24, 64, 0, 10, 0)
    out = _lib.StateGroups()
    for fn in (L.bjx_state_query_groups, L.bjx_node_state_query_groups):
        assert fn(None, ctypes.byref(f), ctypes.byref(g), ctypes.byref(out)) == _lib.ERR_ARG
        assert fn(None, None, None, None) == _lib.ERR_ARG
    # (each bad spec and bad filter: check_spec / check_filter through tests/cpu/groups_host.cpp below, and on an
    # engine in tests/test_gpu_state_groups.py; with a NULL handle the answer would say nothing about them)
    assert G.B == L.bjx_debug_groups_tile()          # the tile the shape world is built around


def test_model_against_brute_force_on_the_nets_world():
    """Every pair of LEN4 x LEN6: the model's groups are the dictionary's; and the world is telling:
    several groups, unparsed IPs, ties on every primary key, v4-mapped text grouped with the dotted
    quad, ::170.85.195.60 on the IPv6 side."""
    run = N.build_world(None)
    ips, states = run.model.snapshot_args()
    assert ips == N.world_ips()
    ties = set()
    for v4_bits in G.LEN4:
        for v6_bits in G.LEN6:
            a = state_groups.groups(ips, states, v4_bits=v4_bits, v6_bits=v6_bits, limit=65536)
            want, bad = G.brute(ips, states, v4_bits, v6_bits)
            assert a["n_groups"] == a["n_groups_min"] == len(want) == len(a["rows"]) >= 2
            for r in a["rows"]:
                w = want[(r.family, r.net)]
                assert (r.n_ips, r.n_states, r.hits_sum, r.newest_start_ns) == (w[0], w[1], state_groups.wrap64(w[2]), w[3]), (r, w)
                assert state_nets.parse_entry(r.net) == (r.family, r.bits, int.from_bytes(r.addr[:4] if r.family == 4 else r.addr, "big"))
                table = state_nets.Nets([r.net])
                assert sum(1 for ip in ips if table.holds(ip)) == r.n_ips
            assert (a["n_ips_unparsed"], a["n_states_unparsed"]) == bad and bad[0] == len(N.NOT_ADDRESSES)
            G.check_invariants(a)
            for order, field in ((state_groups.BY_IPS, "n_ips"), (state_groups.BY_STATES, "n_states"), (state_groups.BY_HITS, "hits_sum")):
                rows = state_groups.groups(ips, states, v4_bits=v4_bits, v6_bits=v6_bits, order=order, limit=65536)["rows"]
                keys = [getattr(r, field) for r in rows]
                assert keys == sorted(keys, reverse=True) and sorted(rows) == sorted(a["rows"])
                if len(set(keys)) < len(keys):                         # ties, broken by family and address
                    ties.add((v4_bits, v6_bits, order))
                for x, y in zip(rows, rows[1:]):
                    assert getattr(x, field) > getattr(y, field) or (x.family, x.addr) < (y.family, y.addr)
    assert all((v4_bits, v6_bits, order) in ties for v4_bits, v6_bits in ((8, 64), (32, 128), (31, 1)) for order in G.ORDERS)
    a = state_groups.groups(ips, states, v4_bits=32, v6_bits=128, limit=65536)
    by_net = {r.net: r for r in a["rows"]}
    assert by_net["170.85.195.60/32"].n_ips >= 2 and "::ffff:170.85.195.60" in ips           # the mapped text and the dotted quad
    assert by_net["::aa55:c33c/128"].family == 6 and by_net["::aa55:c33c/128"].n_ips == len(HF.spellings(b"\0" * 12 + N.BASE4))
    # filters that take parts of IPs, and limits and floors
    part = state_groups.groups(ips, states, name="slow", limit=65536)
    assert 0 < part["n_ips_matched"] < a["n_ips_matched"] and part["n_matched"] == part["n_ips_matched"]
    assert state_groups.groups(ips, states, limit=0)["rows"] == [] and state_groups.groups(ips, states, limit=0)["n_groups"] > 2
    top = state_groups.groups(ips, states, limit=1)["rows"][0]
    assert state_groups.groups(ips, states, min_ips=top.n_ips + 1)["n_groups_min"] == 0
    assert state_groups.groups(ips, states, min_ips=top.n_ips)["rows"][0] == top


def test_shape_and_extreme_worlds_are_what_the_gpu_tests_say():
    ips, states = G.shape_world()
    sizes = G.shape_sizes()
    assert 4000 < len(ips) < 9000 and len(set(ips)) == len(ips)
    a = state_groups.groups(ips, states, v4_bits=16, v6_bits=64, limit=65536)
    by_net = {r.net: r.n_ips for r in a["rows"]}
    assert [by_net["10.%d.0.0/16" % k] for k in range(len(sizes))] == sizes == [1, G.B - 1, G.B, G.B + 1, 2 * G.B + 500]
    assert sum(1 for r in a["rows"] if r.family == 6 and r.n_ips == 1) == G.N_V6_SINGLES == a["n_groups"] - len(sizes)
    # in key order the B-sized group is exactly the second block, and the long group covers a whole block and more on both sides
    starts = [sum(sizes[:k]) for k in range(len(sizes) + 1)]
    assert starts[2] == G.B and starts[3] == 2 * G.B and starts[4] // G.B + 2 <= (starts[5] - 1) // G.B
    want, bad = G.brute(ips, states, 16, 64)
    assert bad == (0, 0) and {(r.family, r.net): [r.n_ips, r.n_states, r.hits_sum, r.newest_start_ns] for r in a["rows"]} == want
    z = state_groups.groups(ips, states, v4_bits=0, v6_bits=64, limit=3)
    assert (z["rows"][0].net, z["rows"][0].n_ips) == ("0.0.0.0/0", sum(sizes)) and z["n_groups"] == 1 + G.N_V6_SINGLES
    ips, states = G.extreme_world()
    rows = {r.net: r for r in state_groups.groups(ips, states, order=state_groups.BY_HITS)["rows"]}
    assert [rows[k].hits_sum for k in ("192.0.2.0/24", "198.51.100.0/24", "2001:db8::/64")] == [10, -1, INT64_MIN]
    assert [rows[k].newest_start_ns for k in ("192.0.2.0/24", "198.51.100.0/24", "2001:db8::/64")] == [INT64_MIN, INT64_MAX, INT64_MIN]
    want, _ = G.brute(ips, states, 24, 64)
    assert any(not INT64_MIN <= w[2] <= INT64_MAX for w in want.values())       # sums that do wrap


# ---- the host header, through tests/cpu/groups_host.cpp

def _rec(fam6, v, n_ips, n_states, hits, newest):
    """a group record as the script writes it; v: the masked address as an int (IPv4: 32 bits)"""
    hi, lo = (v >> 64, v & ((1 << 64) - 1)) if fam6 else (0, v)
    return "%d %x %x %d %d %d %d" % (fam6, hi, lo, n_ips, n_states, hits, newest)


def _row_line(tag, fam6, v, bits, n_ips, n_states, hits, newest):
    addr = v.to_bytes(16, "big") if fam6 else v.to_bytes(4, "big") + b"\0" * 12
    return "%s %s %d %d %d %d %d %d" % (tag, addr.hex(), 6 if fam6 else 4, bits, n_ips, n_states, state_groups.wrap64(hits), newest)


def _script():
    """-> (command lines, the expected output lines)"""
    rng = random.Random(20250117)
    cmds, want = [], []

    def say(c, w):
        cmds.append(c)
        want.append(w)

    # the checks
    for spec, msg in (((24, 64, 0, 10), "ok"), ((0, 0, 2, 0), "ok"), ((32, 128, 1, 65536), "ok"), ((33, 64, 0, 10), "v4_bits"),
                      ((24, 129, 0, 10), "v6_bits"), ((24, 64, 3, 10), "order"), ((24, 64, 0, 65537), "limit")):
        say("spec %d %d %d %d" % spec, msg)
    for filt, msg in (((0, 0, "-", "-"), "ok"), ((1, 65536, "1.2.3.4", "mid"), "ok"), ((2, 0, "-", "-"), "order"),
                      ((0, 65537, "-", "-"), "limit"), ((0, 0, "N", "-"), "ip with a length"), ((0, 0, "-", "N"), "name with a length")):
        say("filter %d %d %s %s" % filt, msg)
    # masking at the edge lengths, over spellings, mapped text, an IPv6 text that only looks like IPv4, and no addresses
    texts = [N.t4(N.BASE4), "::ffff:" + N.t4(N.BASE4), N.t6(N.BASE6), "::170.85.195.60", "255.255.255.255", "::",
             "ffff:ffff:ffff:ffff:ffff:ffff:ffff:ffff", "0.0.0.0", "::ffff:0:0"] + HF.spellings(N.BASE6)[:4] + \
        [t for t in N.NOT_ADDRESSES if t and " " not in t]
    for t in texts:
        for b4 in (0, 1, 31, 32):
            for b6 in (0, 1, 63, 64, 65, 127, 128):
                k = state_groups.group_of(t, b4, b6)
                if k is None:
                    say("pack %s %d %d" % (t, b4, b6), "pack none")
                    continue
                fam, addr = k
                v = int.from_bytes(addr[:4] if fam == 4 else addr, "big")
                hi, lo = (0, v) if fam == 4 else (v >> 64, v & ((1 << 64) - 1))
                say("pack %s %d %d" % (t, b4, b6), "pack %d %x %x" % (fam, hi, lo))
    # the sort looks at every bit in which two keys can differ, and at no bit past the word
    for b4 in range(33):
        for b6 in (0, 1, 63, 64, 65, 127, 128):
            lo_bits = ([32 - b4] if b4 else []) + ([128 - b6] if b6 > 64 else [])
            lo = (min(lo_bits), 64 if b6 > 64 else 32) if lo_bits else (0, 0)
            hi = (64 - min(b6, 64), 64) if b6 else (0, 0)
            say("bits %d %d" % (b4, b6), "bits %d %d %d %d" % (lo + hi))
    # rows
    for fam6, v, bits in ((0, 0xAA55C300, 24), (1, int.from_bytes(N.BASE6, "big") >> 64 << 64, 64), (0, 0, 0), (1, (1 << 128) - 1, 128)):
        for hits, newest in ((5, 7), (INT64_MIN, INT64_MIN), (INT64_MAX, INT64_MAX), (-1, 0)):
            say("row %s %d %d" % (_rec(fam6, v, 3, 9, hits, newest), bits if not fam6 else 11, bits if fam6 else 77),
                _row_line("row", fam6, v, bits, 3, 9, hits, newest))
    # the comparator: the primary key descending, then family 4 first, then the address
    pool = [(fam6, v, n, s, h) for fam6 in (0, 1) for v in (0, 1, 1 << 31, (1 << 32) - 1) + ((1 << 64, (1 << 127) + 5) if fam6 else ())
            for n, s, h in ((1, 1, 0), (2, 2, -3), (2, 5, INT64_MIN), (7, 7, INT64_MAX))]
    for _ in range(300):
        a, b = rng.choice(pool), rng.choice(pool)
        for order in (0, 1, 2):
            ka = (-(a[2], a[3], a[4])[order], a[0], a[1])
            kb = (-(b[2], b[3], b[4])[order], b[0], b[1])
            say("before %d %s %s" % (order, _rec(a[0], a[1], a[2], a[3], a[4], 0), _rec(b[0], b[1], b[2], b[3], b[4], 0)),
                "before %d" % (ka < kb))
    # the merge: 1, 2 and 5 lists, keys shared between all, some and none of them; then the cap
    keys = [(0, v) for v in (0, 0x0A000000, 0x0A000100, 0xFFFFFF00)] + [(1, v) for v in (0, 5 << 64, (1 << 127) + (9 << 64), 1 << 64)]
    for n_lists in (1, 2, 5):
        for trial in range(6):
            lists, total = [], {}
            for _ in range(n_lists):
                mine = sorted(rng.sample(keys, rng.randint(0, len(keys))))
                recs = []
                for fam6, v in mine:
                    n = rng.randint(1, 4)
                    r = (n, n + rng.randint(0, 3), rng.choice((1, 50, INT64_MAX, INT64_MIN, -7)), rng.choice((INT64_MIN, -5, 0, 99, INT64_MAX)))
                    recs.append((fam6, v) + r)
                    t = total.setdefault((fam6, v), [0, 0, 0, INT64_MIN])
                    t[0] += r[0]; t[1] += r[1]; t[2] += r[2]; t[3] = max(t[3], r[3])
                lists.append(recs)
            for order in (0, 1, 2):
                for limit, min_ips in ((65536, 0), (2, 0), (65536, 3), (1, 5), (0, 0)):
                    n_all = sum(len(l) for l in lists)
                    for cap in (1 << 24, n_all, n_all - 1):
                        if cap < 0:
                            continue
                        cmds.append("merge %d 24 64 %d %d %d %d" % (cap, order, limit, min_ips, n_lists))
                        for l in lists:
                            cmds.append("l %d" % len(l))
                            cmds += ["g " + _rec(*r) for r in l]
                        if n_all > cap:
                            want.append("merge capacity")
                            continue
                        rows = [(k, t) for k, t in total.items() if t[0] >= min_ips]
                        rows.sort(key=lambda kt: (-(kt[1][0], kt[1][1], state_groups.wrap64(kt[1][2]))[order], kt[0]))
                        want.append("merge %d %d %d" % (len(total), len(rows), min(limit, len(rows))))
                        want += [_row_line("r", k[0], k[1], 64 if k[0] else 24, *t) for k, t in rows[:limit]]
    return cmds, want


def _run_and_check(exe):
    cmds, want = _script()
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write("\n".join(cmds) + "\n")
    try:
        r = subprocess.run([exe, f.name], capture_output=True, text=True, timeout=120)
    finally:
        os.unlink(f.name)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = r.stdout.splitlines()
    assert len(got) == len(want), (len(got), len(want))
    for g, w in zip(got, want):
        # the checks' messages are matched by their telling word
        assert g == w or (w.split()[0] not in ("pack", "bits", "row", "before", "merge", "r") and
                          g.startswith(("spec ", "filter ")) and (w == "ok") == g.endswith(" ok") and w in g), (g, w)
    assert sum(1 for w in want if w == "merge capacity") > 10 and sum(1 for w in want if w.startswith("r ")) > 300
    return len(want)


def test_host_header_checks_masking_order_and_merge():
    d = tempfile.mkdtemp(prefix="bjx_groups_")
    exe = os.path.join(d, "groups_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, SRC], check=True)
    assert _run_and_check(exe) > 2000


def test_standalone_program_under_sanitizers():
    """The same program built with ASan + UBSan and run once as a child process
    over the same script (nothing loaded into Python runs under a sanitizer)."""
    d = tempfile.mkdtemp(prefix="bjx_groups_san_")
    exe = os.path.join(d, "groups_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, SRC], check=True)
    _run_and_check(exe)
