"""State queries without a GPU: the C symbols, their NULL handling and struct
sizes; the pure-Python model (banjax_amd/state_query.py) against a brute-force
sort; and the host parts of the call -- filter checks, sort key, name ranks and
the node's merge of shard answers (banjax_amd/csrc/state_query.h) -- built for
the host from tests/cpu/query_host.cpp, a program with its own main."""
import ctypes
import functools
import os
import random
import subprocess
import tempfile

import pytest

from banjax_amd import _lib, state_query

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu", "query_host.cpp")
T0 = 1_700_000_000_000_000_000
NAMES = ("mid", "fast", "slow", "a", "ab", "")


def test_symbols_structs_and_null_arguments():
    L = _lib.lib()
    for name in ("bjx_state_query", "bjx_node_state_query"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert ctypes.sizeof(_lib.StateFilter) == 64
    assert ctypes.sizeof(_lib.StateRow) == 40
    assert ctypes.sizeof(_lib.StateRows) == 56
    f, out = _lib.StateFilter(), _lib.StateRows()
    fake = ctypes.c_void_p(8)  # never followed: the NULL checks come first
    for fn in (L.bjx_state_query, L.bjx_node_state_query):
        assert fn(None, ctypes.byref(f), ctypes.byref(out)) == _lib.ERR_ARG
        assert fn(fake, None, ctypes.byref(out)) == _lib.ERR_ARG
        assert fn(fake, ctypes.byref(f), None) == _lib.ERR_ARG


def _sample(seed, n_ips=40, names=NAMES, hits=4):
    """small states with heavy ties: few distinct hits, starts from a handful of values"""
    rng = random.Random(seed)
    ips = ["10.%d.%d.%d" % (seed, k >> 8, k & 255) if k % 3 else "2001:db8::%x:%x" % (seed, k) for k in range(n_ips)]
    rng.shuffle(ips)
    states = {}
    for ip in ips:
        use = rng.sample(list(names), rng.randrange(1, len(names) + 1))
        states[ip] = {n: (rng.randrange(0, hits), T0 + rng.randrange(-2, 3)) for n in use}
    return ips, states


def _brute(ips, states, ip, name, min_hits, lo, hi, order, limit):
    """every state, filtered one condition at a time, ordered with an explicit comparison"""
    flat = []
    for pos, i in enumerate(ips):
        for n, (h, s) in states[i].items():
            flat.append((pos, i.encode(), n.encode(), h, s))
    if ip is not None:
        flat = [t for t in flat if t[1] == ip]
    if name is not None:
        flat = [t for t in flat if t[2] == name]
    flat = [t for t in flat if t[3] >= min_hits]
    flat = [t for t in flat if lo <= t[4] <= hi]

    def cmp(a, b):
        ka, kb = (a[4], b[4]) if order == state_query.BY_START else (a[3], b[3])
        if ka != kb:
            return -1 if ka > kb else 1
        if a[0] != b[0]:
            return -1 if a[0] < b[0] else 1
        return -1 if a[2] < b[2] else (1 if a[2] > b[2] else 0)

    flat.sort(key=functools.cmp_to_key(cmp))
    return len(flat), len({t[0] for t in flat}), [(t[1], t[2], t[3], t[4]) for t in flat[:limit]]


def test_model_against_brute_force():
    rng = random.Random(5)
    for seed in range(1, 5):
        ips, states = _sample(seed)
        total = sum(len(d) for d in states.values())
        for _ in range(120):
            ip = rng.choice([None, None, None, ips[rng.randrange(len(ips))].encode(), b"9.9.9.9", b""])
            name = rng.choice([None, None, b"", b"a", b"ab", b"mid", b"nope"])
            min_hits = rng.choice([state_query.INT64_MIN, 0, 1, 2, 3, 4])
            lo = rng.choice([state_query.INT64_MIN, T0 - 1, T0, T0 + 2])
            hi = rng.choice([state_query.INT64_MAX, T0 + 1, T0, T0 - 2])
            order = rng.choice([state_query.BY_HITS, state_query.BY_START])
            limit = rng.choice([0, 1, 2, 7, total - 1, total, total + 1, 65536])
            got = state_query.select(ips, states, ip=ip, name=name, min_hits=min_hits, min_start_ns=lo, max_start_ns=hi,
                                     order=order, limit=limit)
            assert got == _brute(ips, states, ip, name, min_hits, lo, hi, order, limit)
    # the model takes what snapshot.parse returns as well: bytes keys
    ips, states = _sample(9)
    bstates = {i.encode(): {n.encode(): v for n, v in d.items()} for i, d in states.items()}
    assert state_query.select([i.encode() for i in ips], bstates, limit=50) == state_query.select(ips, states, limit=50)
    with pytest.raises(ValueError):
        state_query.select(ips, states, limit=65537)
    with pytest.raises(ValueError):
        state_query.select(ips, states, order=2)


# ---- the host header, through tests/cpu/query_host.cpp

def _hex(b):
    return b.hex() if b else "-"


def _unhex(h):
    return b"" if h == "-" else bytes.fromhex(h)


def _merge_case(shards, order, limit):
    """shards: [(ips, states)] engine-major.  -> (command lines, expected answer):
    each shard's answer is the model over the shard alone, the expected merge
    the model over all of it with the IPs shard-major."""
    lines = ["merge %d %d %d" % (order, limit, len(shards))]
    all_ips, all_states = [], {}
    for k, (ips, states) in enumerate(shards):
        n, ni, rows = state_query.select(ips, states, order=order, limit=limit)
        lines.append("shard %d %d %d %g" % (n, ni, len(rows), 0.25 * (k + 1)))
        lines += ["row %s %s %d %d" % (_hex(i), _hex(nm), h, s) for i, nm, h, s in rows]
        all_ips += ips
        all_states.update(states)
    return lines, state_query.select(all_ips, all_states, order=order, limit=limit)


def _script():
    """(command lines, [expected output lines per command])"""
    cmds, want = [], []

    def add(lines, out):
        cmds.extend(lines)
        want.append(out)

    for order, limit, ok in ((0, 0, True), (1, 65536, True), (0, 65537, False), (2, 1, False), (7, 1, False)):
        add(["filter %d %d" % (order, limit)], ok)
    vals = [-(1 << 63), -(1 << 63) + 1, -5, -1, 0, 1, 5, (1 << 63) - 2, (1 << 63) - 1]
    add(["key " + " ".join(map(str, vals))], ("key", vals))
    names = [b"mid", b"fast", b"", b"ab", b"a", b"\xff", b"a\x00", b"slow"]
    add(["ranks " + " ".join(_hex(n) for n in names)], ("ranks", names))
    rng = random.Random(21)
    for n_shards in (1, 2, 5):
        for trial in range(6):
            shards = []
            for k in range(n_shards):
                size = rng.choice([0, 0, 3, 11, 25])  # empty shards and shards shorter than the limit
                shards.append(_sample(100 + 10 * trial + k, size, hits=2) if size else ([], {}))
            for order in (0, 1):
                for limit in (0, 1, 5, 20, 65536):
                    lines, exp = _merge_case(shards, order, limit)
                    add(lines, ("merged", exp, max([0.25 * (k + 1) for k in range(n_shards)])))
    return cmds, want


def _run_and_check(exe):
    cmds, want = _script()
    path = os.path.join(os.path.dirname(exe), "script.txt")
    with open(path, "w") as f:
        f.write("\n".join(cmds) + "\n")
    r = subprocess.run([exe, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    out = r.stdout.splitlines()
    at = 0
    for w in want:
        head = out[at].split()
        at += 1
        if isinstance(w, bool):
            assert head[0] == "filter" and (head[1] == "ok") == w, (head, w)
        elif w[0] == "key":
            keys = [int(x) for x in head[1:]]
            assert head[0] == "key" and len(keys) == len(w[1])
            # ascending keys <=> descending values, within u64
            assert all(0 <= k < 1 << 64 for k in keys)
            assert sorted(range(len(keys)), key=lambda k: keys[k]) == sorted(range(len(keys)), key=lambda k: -w[1][k])
        elif w[0] == "ranks":
            assert head[0] == "ranks"
            assert [int(x) for x in head[1:]] == [sorted(w[1]).index(n) for n in w[1]]
        else:
            (n, ni, rows), ms = w[1], w[2]
            assert head[0] == "merged" and [int(head[1]), int(head[2]), int(head[3])] == [n, ni, len(rows)], (head, n, ni)
            assert float(head[4]) == ms
            got = []
            for _ in rows:
                t = out[at].split()
                at += 1
                assert t[0] == "row"
                got.append((_unhex(t[1]), _unhex(t[2]), int(t[3]), int(t[4])))
            assert got == rows
    assert at == len(out)
    return len(want)


def test_host_header_filter_key_ranks_and_node_merge():
    d = tempfile.mkdtemp(prefix="bjx_qry_")
    exe = os.path.join(d, "query_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, SRC], check=True)
    assert _run_and_check(exe) > 180


def test_standalone_program_under_sanitizers():
    """The same program built with ASan + UBSan and run once as a subprocess
    over the same script (never loaded into Python)."""
    d = tempfile.mkdtemp(prefix="bjx_qry_san_")
    exe = os.path.join(d, "query_host")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-o", exe, SRC]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the compiler cannot build with -fsanitize=address,undefined here: " + r.stderr.strip()[-300:])
    _run_and_check(exe)
