"""bjx_state_query_names without a GPU: the symbols, struct sizes and argument
checks of the library, the pure-Python model (banjax_amd/state_names.py)
against a brute-force aggregation over the worlds the GPU tests use -- which
shows those worlds are telling -- and the host header
(banjax_amd/csrc/state_names.h: spec and filter checks, the histogram bucket,
the record and its accumulation, the row comparator per order, the node merge
with its cap) built for the host from tests/cpu/names_host.cpp, a program with
its own main."""
import ctypes
import itertools
import os
import random
import subprocess
import tempfile

from banjax_amd import _lib, state_merge, state_names
from tests import state_names as M
from tests import state_nets as N

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "cpu", "names_host.cpp")
INT64_MIN, INT64_MAX = M.INT64_MIN, M.INT64_MAX


def test_symbols_structs_and_bad_arguments():
    L = _lib.lib()
    for name in ("bjx_state_query_names", "bjx_node_state_query_names"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    for name in ("bjx_debug_set_names", "bjx_debug_names_info"):
        assert hasattr(L, name), name
    public = open(os.path.join(ROOT, "include", "banjax_gpu.h")).read()
    debug = open(os.path.join(ROOT, "include", "banjax_gpu_debug.h")).read()
    for word in ("int bjx_state_query_names(bjx_engine *e, const bjx_state_filter *f, const bjx_names_spec *s, bjx_state_names *out);",
                 "int bjx_node_state_query_names(bjx_node *n, const bjx_state_filter *f, const bjx_names_spec *s, bjx_state_names *out);",
                 "#define BJX_NAMES_MAX_ROWS 65536", "#define BJX_NAMES_HIST 16", "BJX_NAMES_BY_STATES = 0", "BJX_NAMES_BY_HITS = 1",
                 "BJX_NAMES_BY_MAX_HITS = 2", "BJX_NAMES_BY_NEWEST = 3", "BJX_NAMES_BY_NAME = 4"):
        assert word in public, word
    assert "bjx_debug_set_names(" in debug and "bjx_debug_names_info(" in debug
    assert L.bjx_abi_version() == 5
    assert ctypes.sizeof(_lib.NamesSpec) == 16 and ctypes.sizeof(_lib.NameRow) == 184 and ctypes.sizeof(_lib.StateNames) == 72
    assert [k for k, _ in _lib.NamesSpec._fields_] == ["order", "limit", "min_states"]
    assert [k for k, _ in _lib.NameRow._fields_] == ["name_off", "name_len", "_pad", "n_states", "hits_sum", "max_hits",
                                                     "newest_start_ns", "oldest_start_ns", "hist"]
    assert [k for k, _ in _lib.StateNames._fields_] == ["n_matched", "n_ips_matched", "n_names", "n_names_min", "n_rows", "rows",
                                                        "bytes", "n_bytes", "device_ms"]
    assert (_lib.NAMES_BY_STATES, _lib.NAMES_BY_HITS, _lib.NAMES_BY_MAX_HITS, _lib.NAMES_BY_NEWEST, _lib.NAMES_BY_NAME,
            _lib.NAMES_MAX_ROWS, _lib.NAMES_HIST) == (0, 1, 2, 3, 4, 65536, 16)
    assert M.ORDERS == (0, 1, 2, 3, 4) and state_names.MAX_ROWS == 65536 and state_names.HIST == 16
    f = _lib.StateFilter(_lib.Str(None, 0), _lib.Str(None, 0), INT64_MIN, INT64_MIN, INT64_MAX, 0, 0)
    s = _lib.NamesSpec(0, 10, 0)
    out = _lib.StateNames()
    for fn in (L.bjx_state_query_names, L.bjx_node_state_query_names):
        assert fn(None, ctypes.byref(f), ctypes.byref(s), ctypes.byref(out)) == _lib.ERR_ARG
        assert fn(None, None, None, None) == _lib.ERR_ARG
    assert L.bjx_debug_set_names(None, 0, 0) == _lib.ERR_ARG and L.bjx_debug_names_info(None, None, None) == _lib.ERR_ARG
    # (each bad spec and bad filter: check_spec / check_filter through tests/cpu/names_host.cpp below, and on an
    # engine in tests/test_gpu_state_names.py; with a NULL handle the answer would say nothing about them)


def test_bucket_edges_and_wrap():
    want = {-1: 0, 0: 0, 1: 1, 2: 2, 3: 2, 4: 3, (1 << 14) - 1: 14, 1 << 14: 15, INT64_MAX: 15, INT64_MIN: 0}
    assert {h: state_names.bucket(h) for h in want} == want
    for b in range(1, 15):
        assert state_names.bucket((1 << (b - 1))) == b == state_names.bucket((1 << b) - 1)
    assert state_names.wrap64(INT64_MAX + 1) == INT64_MIN and state_names.wrap64(INT64_MIN - 1) == INT64_MAX
    ips, states = M.extreme_world()
    rows = {r.name: r for r in state_names.names(ips, states)["rows"]}
    assert rows[b"up"].hits_sum == state_names.wrap64(2 * INT64_MAX + 12) == 10
    assert rows[b"down"].hits_sum == state_names.wrap64(2 * INT64_MIN - 1) == -1
    assert rows[b"ends"].hits_sum == -1 and (rows[b"ends"].max_hits, rows[b"ends"].newest_start_ns, rows[b"ends"].oldest_start_ns) == \
        (INT64_MAX, INT64_MAX, INT64_MIN)
    assert rows[b"neg"].max_hits == -1 and rows[b"neg"].hist[0] == 3 and rows[b"zero"].hist == (2,) + (0,) * 15
    assert rows[b"up"].hist[15] == 2 and rows[b"up"].hist[4] == 1 and rows[b"down"].hist[0] == 3
    raw = M.brute(ips, states)
    assert sum(1 for a in raw.values() if not INT64_MIN <= a[1] <= INT64_MAX) >= 2          # sums that do wrap


def _hold(ips, states, **filt):
    """the model against the dictionary, for one filter; every order sorted as the contract says"""
    def passes(ip, n, h, s):
        return (filt.get("ip") is None or M._b(filt["ip"]) == M._b(ip)) and (filt.get("name") is None or M._b(filt["name"]) == M._b(n)) and \
            h >= filt.get("min_hits", INT64_MIN) and filt.get("min_start_ns", INT64_MIN) <= s <= filt.get("max_start_ns", INT64_MAX)
    want = M.brute(ips, states, passes)
    a = state_names.names(ips, states, limit=65536, **filt)
    assert a["n_names"] == a["n_names_min"] == len(want) == len(a["rows"])
    assert a["n_matched"] == sum(w[0] for w in want.values())
    assert a["n_ips_matched"] == len({ip for ip in ips for n, (h, s) in states.get(ip, {}).items() if passes(ip, n, h, s)})
    for r in a["rows"]:
        w = want[r.name]
        assert (r.n_states, r.hits_sum, r.max_hits, r.newest_start_ns, r.oldest_start_ns, r.hist) == \
            (w[0], state_names.wrap64(w[1]), w[2], w[3], w[4], M.brute_hist(w[5])), (r, w)
    M.check_invariants(a)
    by_order = {}
    for order, field in zip(M.ORDERS, ("n_states", "hits_sum", "max_hits", "newest_start_ns", None)):
        rows = state_names.names(ips, states, order=order, limit=65536, **filt)["rows"]
        assert sorted(rows) == sorted(a["rows"])
        for x, y in zip(rows, rows[1:]):
            px, py = (getattr(x, field), getattr(y, field)) if field else (0, 0)
            assert px > py or (px == py and x.name < y.name), (order, x, y)
        by_order[order] = rows
    return a, by_order


def test_model_against_brute_force_on_the_nets_world():
    run = N.build_world(None)
    ips, states = run.model.snapshot_args()
    assert ips == N.world_ips()
    a, _ = _hold(ips, states)
    assert [r.name for r in a["rows"]] and {r.name for r in a["rows"]} == {b"fast", b"mid", b"slow"}
    for filt in ({"name": "slow"}, {"min_hits": 2}, {"min_hits": 3, "name": "mid"}, {"min_start_ns": N.NOW + 50_000_000},
                 {"ip": "170.85.195.60"}, {"ip": "01.2.3.4"}, {"ip": "170.85.195.77"}, {"name": "never"},
                 {"min_start_ns": 5, "max_start_ns": 4}):
        _hold(ips, states, **filt)
    assert state_names.names(ips, states, name="slow")["n_names"] == 1
    assert state_names.names(ips, states, ip="170.85.195.77")["rows"] == [] == state_names.names(ips, states, limit=0)["rows"]
    top = state_names.names(ips, states, limit=1)["rows"][0]
    assert state_names.names(ips, states, min_states=top.n_states + 1)["n_names_min"] == 0
    assert state_names.names(ips, states, min_states=top.n_states)["rows"][0] == top
    for bad in ({"order": 5}, {"limit": 65537}, {"limit": -1}):
        try:
            state_names.names(ips, states, **bad)
        except ValueError:
            continue
        raise AssertionError(bad)


def test_the_worlds_are_what_the_gpu_tests_say():
    ips, states = M.shape_world()
    a, by_order = _hold(ips, states)
    rows = {r.name: r for r in a["rows"]}
    # two names tied on each primary key, broken by name
    for field in ("n_states", "hits_sum", "max_hits", "newest_start_ns"):
        assert getattr(rows[b"tie1"], field) == getattr(rows[b"tie2"], field), field
    for order in M.ORDERS:
        names = [r.name for r in by_order[order]]
        assert names.index(b"tie1") + 1 == names.index(b"tie2"), order
    # the five orders pairwise different
    for x, y in itertools.combinations(M.ORDERS, 2):
        assert by_order[x] != by_order[y], (x, y)
    # every bucket non-empty under some name; a name with everything in bucket 0
    assert all(c > 0 for c in rows[b"hist"].hist) and rows[b"hist"].hist[15] >= 2
    assert rows[b"zero"].hist == (rows[b"zero"].n_states,) + (0,) * 15 and rows[b"zero"].n_states == 6
    # the name shapes
    assert {b"a", b"ab", M.EMPTY, M.HIGH, M.LONG} <= set(rows) and len(M.LONG) == 300 and max(M.HIGH) >= 0x80
    names = [r.name for r in by_order[state_names.BY_NAME]]
    assert names[0] == M.EMPTY and names.index(b"a") + 1 == names.index(b"ab") and names[-1] == M.HIGH and names == sorted(names)
    for filt in ({"min_hits": 1}, {"min_hits": 1 << 14}, {"name": M.EMPTY}, {"name": M.LONG}, {"name": b"a"}, {"ip": ips[0]},
                 {"max_start_ns": M.T0}):
        _hold(ips, states, **filt)
    # one shard and all shards of a node of 2 and of 3, under the owner function
    for n_parts in (2, 3):
        on = {nm: {state_merge.owner(M._b(ip), n_parts) for ip in ips if nm in states[ip]} for nm in rows}
        assert len(on[b"solo"]) == 1 and len(on[b"all"]) == n_parts and len(on[b"hist"]) == n_parts
    # the skewed world: one name holds 99% of the states
    ips, states = M.skewed_world()
    a, _ = _hold(ips, states)
    rows = {r.name: r for r in a["rows"]}
    assert rows[b"big"].n_states == M.N_SKEW and rows[b"big"].n_states * 100 >= 99 * a["n_matched"] and len(rows) == 3
    _hold(*M.extreme_world())
    for n in (7, 8, 9):
        ips, states = M.count_world(n)
        a, _ = _hold(ips, states)
        assert a["n_names"] == n and 2 <= len(ips) <= 8


def test_orphans():
    ips, states = M.shape_world()
    rows = state_names.names(ips, states, limit=65536)["rows"]
    gone = state_names.orphans(rows, ["all", b"hist", "solo", "a", ""])
    assert {r.name for r in gone} == {r.name for r in rows} - {b"all", b"hist", b"solo", b"a", b""} and b"ab" in {r.name for r in gone}
    assert [r.name for r in gone] == [r.name for r in rows if r in gone]                    # the rows' order is kept
    assert state_names.orphans(rows, [r.name for r in rows]) == [] and state_names.orphans(rows, []) == rows


# ---- the host header, through tests/cpu/names_host.cpp

def _hx(name: bytes) -> str:
    return name.hex() or "-"


def _item(name, n_states, hits, max_hits, newest, oldest, hist=None):
    s = "%s %d %d %d %d %d" % (_hx(name), n_states, state_names.wrap64(hits), max_hits, newest, oldest)
    return s if hist is None else s + " " + " ".join(str(c) for c in hist)


def _script():
    """-> (command lines, the expected output lines)"""
    rng = random.Random(20250612)
    cmds, want = [], []

    def say(c, w):
        cmds.append(c)
        want.append(w)

    for spec, msg in (((0, 10), "ok"), ((4, 65536), "ok"), ((3, 0), "ok"), ((5, 10), "order"), ((0xFFFFFFFF, 10), "order"),
                      ((0, 65537), "limit")):
        say("spec %d %d" % spec, msg)
    for filt, msg in (((0, 0, "-", "-"), "ok"), ((1, 65536, "1.2.3.4", "mid"), "ok"), ((2, 0, "-", "-"), "order"),
                      ((0, 65537, "-", "-"), "limit"), ((0, 0, "N", "-"), "ip with a length"), ((0, 0, "-", "N"), "name with a length")):
        say("filter %d %d %s %s" % filt, msg)
    for h in [-1, 0, 1, 2, 3, 4, (1 << 14) - 1, 1 << 14, INT64_MAX, INT64_MIN] + [v for b in range(1, 63) for v in ((1 << b) - 1, 1 << b)]:
        say("bucket %d" % h, "bucket %d" % state_names.bucket(h))
    # accumulation: wrapping sums, extrema at both ends
    for _ in range(30):
        sts = [(rng.choice((0, 1, -1, 5, 1 << 14, INT64_MAX, INT64_MIN, rng.randrange(1, 40000))),
                rng.choice((0, -1, INT64_MAX, INT64_MIN, rng.randrange(-10**18, 10**18)))) for _ in range(rng.randint(1, 9))]
        cmds.append("acc %d" % len(sts))
        cmds += ["s %d %d" % s for s in sts]
        hits = [h for h, _ in sts]
        want.append("acc " + _item(b"", len(sts), sum(hits), max(hits), max(s for _, s in sts), min(s for _, s in sts),
                                   M.brute_hist(hits)))
    # the comparator: the primary key descending, then the name bytewise, a prefix first
    names = [b"", b"a", b"ab", b"b", b"\x7f", b"\x80", b"\xff", b"a\x00", b"L" * 300, b"L" * 299]
    pool = [(nm, n, h, m, t) for nm in names for n, h, m, t in ((1, 0, 0, 0), (2, -3, -3, 5), (2, INT64_MIN, INT64_MIN, INT64_MIN),
                                                                (7, INT64_MAX, INT64_MAX, INT64_MAX), (7, 6, 1 << 40, -9))]
    for _ in range(400):
        a, b = rng.choice(pool), rng.choice(pool)
        for order in M.ORDERS:
            ka = (-((a[1], a[2], a[3], a[4], 0)[order]), a[0])
            kb = (-((b[1], b[2], b[3], b[4], 0)[order]), b[0])
            say("before %d %s %s" % (order, _item(a[0], a[1], a[2], a[3], a[4], 0), _item(b[0], b[1], b[2], b[3], b[4], 0)),
                "before %d" % (ka < kb))
    # the merge: 1, 2 and 5 lists, names shared between all, some and none of them; then the cap
    keys = [b"", b"a", b"ab", b"zz", b"\xc3\xa9", b"\xff\xfe", b"L" * 300, b"mid"]
    for n_lists in (1, 2, 5):
        for trial in range(5):
            lists, total = [], {}
            for _ in range(n_lists):
                mine = rng.sample(keys, rng.randint(0, len(keys)))          # any order
                items = []
                for nm in mine:
                    hist = [rng.randint(0, 3) for _ in range(16)]
                    hist[rng.randrange(16)] += 1
                    it = (sum(hist), rng.choice((1, 50, INT64_MAX, INT64_MIN, -7)), rng.choice((INT64_MIN, -5, 0, 99, INT64_MAX)),
                          rng.choice((INT64_MIN, -5, 0, 99, INT64_MAX)), rng.choice((INT64_MIN, -5, 0, 99, INT64_MAX)), hist)
                    items.append((nm,) + it)
                    t = total.setdefault(nm, [0, 0, INT64_MIN, INT64_MIN, INT64_MAX, [0] * 16])
                    t[0] += it[0]; t[1] += it[1]; t[2] = max(t[2], it[2]); t[3] = max(t[3], it[3]); t[4] = min(t[4], it[4])
                    t[5] = [x + y for x, y in zip(t[5], hist)]
                lists.append(items)
            for order in M.ORDERS:
                for limit, min_states in ((65536, 0), (2, 0), (65536, 20), (1, 30), (0, 0)):
                    n_all = sum(len(l) for l in lists)
                    for cap in (1 << 20, n_all, n_all - 1):
                        if cap < 0:
                            continue
                        cmds.append("merge %d %d %d %d %d" % (cap, order, limit, min_states, n_lists))
                        for l in lists:
                            cmds.append("l %d" % len(l))
                            cmds += ["i " + _item(*it) for it in l]
                        if n_all > cap:
                            want.append("merge capacity")
                            continue
                        rows = [(nm, t) for nm, t in total.items() if t[0] >= min_states]
                        rows.sort(key=lambda kt: (-((kt[1][0], state_names.wrap64(kt[1][1]), kt[1][2], kt[1][3], 0)[order]), kt[0]))
                        want.append("merge %d %d %d" % (len(total), len(rows), min(limit, len(rows))))
                        want += ["r " + _item(nm, *t) for nm, t in rows[:limit]]
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
        assert g == w or (w.split()[0] not in ("bucket", "acc", "before", "merge", "r") and
                          g.startswith(("spec ", "filter ")) and (w == "ok") == g.endswith(" ok") and w in g), (g, w)
    assert sum(1 for w in want if w == "merge capacity") > 10 and sum(1 for w in want if w.startswith("r ")) > 300
    return len(want)


def test_host_header_checks_buckets_order_and_merge():
    d = tempfile.mkdtemp(prefix="bjx_names_")
    exe = os.path.join(d, "names_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, SRC], check=True)
    assert _run_and_check(exe) > 2000


def test_standalone_program_under_sanitizers():
    """The same program built with ASan + UBSan and run once as a child process
    over the same script (nothing loaded into Python runs under a sanitizer)."""
    d = tempfile.mkdtemp(prefix="bjx_names_san_")
    exe = os.path.join(d, "names_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, SRC], check=True)
    _run_and_check(exe)
