"""State removal without a GPU: the C symbols, their NULL handling and the
struct size; the pure-Python model (banjax_amd/state_remove.py) against the
snapshot format and the query's model; that the inputs of the GPU tests are
telling (computed with the oracle and the model alone); and the host parts of
the call -- argument checks, list packing, the filter's ip with a list, the
node's sum (banjax_amd/csrc/state_remove.h) -- built for the host from
tests/cpu/remove_host.cpp, a program with its own main."""
import ctypes
import os
import random
import subprocess
import tempfile

import pytest

from banjax_amd import _lib, snapshot, state_query, state_remove
from tests import state_remove as H

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu", "remove_host.cpp")
T0 = 1_700_000_000_000_000_000
NAMES = ("mid", "fast", "slow", "a", "")


def test_symbols_struct_and_null_arguments():
    L = _lib.lib()
    for name in ("bjx_state_remove", "bjx_node_state_remove"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert ctypes.sizeof(_lib.RemoveStats) == 80
    assert [k for k, _ in _lib.RemoveStats._fields_] == [
        "states_before", "states_dropped", "ips_before", "ips_dropped", "ips_found", "arena_bytes_before",
        "arena_bytes_after", "device_bytes_before", "device_bytes_after", "device_ms"]
    f, out = _lib.StateFilter(), _lib.RemoveStats()
    one = (_lib.Str * 1)(_lib.Str(b"1.2.3.4", 7))
    for fn in (L.bjx_state_remove, L.bjx_node_state_remove):
        # a NULL handle is refused whatever else is passed; nothing is followed
        assert fn(None, ctypes.byref(f), None, 0, ctypes.byref(out)) == _lib.ERR_ARG
        assert fn(None, None, None, 0, None) == _lib.ERR_ARG
        assert fn(None, ctypes.byref(f), one, 1, None) == _lib.ERR_ARG
        assert fn(None, ctypes.byref(f), None, 3, ctypes.byref(out)) == _lib.ERR_ARG


def _sample(seed, n_ips=40):
    rng = random.Random(seed)
    ips = ["10.%d.%d.%d" % (seed, k >> 8, k & 255) if k % 3 else "2001:db8::%x:%x" % (seed, k) for k in range(n_ips)]
    ips.append("")
    rng.shuffle(ips)
    states = {}
    for ip in ips:
        states[ip] = {n: (rng.randrange(0, 4), T0 + rng.randrange(0, 6) * 1_000_000_000)
                      for n in rng.sample(NAMES, rng.randrange(1, len(NAMES) + 1))}
    return ips, states


def _selections(rng, ips):
    yield {}
    yield {"name": "never-interned"}
    yield {"min_start_ns": T0 + 5, "max_start_ns": T0}
    yield {"ips": ["10.250.0.1", "nobody"]}
    yield {"ip": ips[0], "ips": ips[1:5]}           # the filter's IP is not listed: nothing
    yield {"ip": ips[2], "ips": ips[1:5] + ips[2:3]}
    yield {"ip": ""}
    yield {"ips": [""] + ips[:3]}
    for _ in range(40):
        sel = {}
        if rng.random() < 0.6:
            sel["ips"] = rng.sample(ips, rng.randrange(1, 25)) + ["10.250.0.%d" % rng.randrange(9)] * rng.randrange(0, 3)
        if rng.random() < 0.4:
            sel["name"] = rng.choice(NAMES)
        if rng.random() < 0.4:
            sel["min_hits"] = rng.randrange(0, 4)
        if rng.random() < 0.4:
            sel["min_start_ns"] = T0 + rng.randrange(0, 4) * 1_000_000_000
        if rng.random() < 0.4:
            sel["max_start_ns"] = T0 + rng.randrange(2, 6) * 1_000_000_000
        if rng.random() < 0.15:
            sel["ip"] = rng.choice(ips)
        yield sel


def test_model_against_snapshot_and_query():
    """The survivors are a canonical snapshot; what the query's model selects
    with the removal's filter, among the listed IPs, is what went and is gone
    afterwards; the rest is untouched and in its old order; the counts add up."""
    dropped_some = kept_all = 0
    for seed in range(6):
        rng = random.Random(100 + seed)
        ips, states = _sample(seed)
        ips_b = [state_query._b(i) for i in ips]
        for sel in _selections(rng, ips):
            kept_ips, kept, c = state_remove.remove(ips, states, **sel)
            blob = snapshot.build(kept_ips, kept)
            assert snapshot.parse(blob) == (kept_ips, kept)
            filt = {k: v for k, v in sel.items() if k != "ips"}
            listed = None if not sel.get("ips") else {state_query._b(x) for x in sel["ips"]}
            n0, _, rows0 = state_query.select(ips, states, limit=65536, **filt)
            assert n0 == len(rows0)
            gone = [(i, n) for i, n, _, _ in rows0 if listed is None or i in listed]
            # the same filter over the result finds nothing among the listed IPs
            _, _, rows1 = state_query.select(kept_ips, kept, limit=65536, **filt)
            assert not [r for r in rows1 if listed is None or r[0] in listed]
            # exactly the selected states went, nothing else changed
            want = {state_query._b(i): {state_query._b(n): tuple(v) for n, v in d.items()} for i, d in states.items()}
            for i, n in gone:
                del want[i][n]
            want = {i: d for i, d in want.items() if d}
            assert kept == want
            assert kept_ips == [i for i in ips_b if i in want]
            assert c["states_before"] == sum(len(d) for d in states.values())
            assert c["states_dropped"] == len(gone) == c["states_before"] - sum(len(d) for d in kept.values())
            assert c["ips_before"] == len(ips) and c["ips_dropped"] == len(ips) - len(kept_ips)
            assert c["ips_found"] == (0 if listed is None else len(listed & set(ips_b)))
            assert c["arena_bytes_before"] == sum(len(i) for i in ips_b)
            assert c["arena_bytes_after"] == sum(len(i) for i in kept_ips)
            dropped_some += bool(gone)
            kept_all += not gone
    assert dropped_some > 100 and kept_all > 20


def test_model_special_cases():
    ips, states = _sample(7)
    every = sum(len(d) for d in states.values())
    k_ips, kept, c = state_remove.remove(ips, states)  # all-pass, no list: everything
    assert (k_ips, kept, c["states_dropped"], c["ips_dropped"], c["arena_bytes_after"]) == ([], {}, every, len(ips), 0)
    # the expiry as a special case: max_start_ns = cutoff - 1
    cutoff = T0 + 3_000_000_000
    k_ips, kept, c = state_remove.remove(ips, states, max_start_ns=cutoff - 1)
    assert all(s[1] >= cutoff for d in kept.values() for s in d.values())
    assert c["states_dropped"] == sum(1 for d in states.values() for s in d.values() if s[1] < cutoff)
    assert c["states_dropped"] == state_query.select(ips, states, max_start_ns=cutoff - 1)[0]
    # an empty list is no list
    assert state_remove.remove(ips, states, ips=[])[2]["states_dropped"] == every


def test_gpu_test_inputs_are_telling():
    """Conditions on the inputs of tests/test_gpu_state_remove.py, from the
    oracle and the model alone: every selection of the parity run drops some
    states and not all; some IPs lose everything and some keep a part; later
    events show both (FirstTime with seen_ip 1, and seen_ip 0)."""
    run, done = H.parity_run(None, H.stream())
    assert len(done) == 3
    for b, (c, partial) in enumerate(done):
        assert 0 < c["states_dropped"] < c["states_before"], (b, c)
    # the list takes whole IPs, the name and the window a part of many
    assert done[0][0]["ips_dropped"] == 35 and done[1][1] > 0 and done[2][1] > 0
    assert done[0][0]["ips_found"] == 35 and done[1][0]["ips_found"] == 0 and done[2][0]["ips_found"] > 0
    assert run.diff_first > 0 and run.diff_seen > 0
    # the selection with a window and min_hits is narrower than its list alone
    assert done[2][0]["states_dropped"] < done[2][0]["states_before"] // 2


# ---- the host header, through tests/cpu/remove_host.cpp

def _hex(b):
    b = state_query._b(b)
    return b.hex() if b else "-"


def _script():
    """-> (command lines, the expected output lines)"""
    cmds, want = [], []

    def check(line, answer):
        cmds.append(line)
        want.append("check " + answer)

    check("check NOFILTER", "no filter")
    check("check N N 0", "ok")
    check("check - - 0 - - %s" % _hex("1.2.3.4"), "ok")
    check("check N N 1 %s" % _hex("1.2.3.4"), "ips: a count and no list")
    check("check N N 0 %s N3" % _hex("1.2.3.4"), "ips: an entry with a length and no bytes")
    check("check N N 0 N %s" % _hex("1.2.3.4"), "ok")  # a NULL pointer of length 0 is the empty IP
    check("check N5 N 0", "filter: ip with a length and no bytes")
    check("check N N2 0", "filter: name with a length and no bytes")
    check("big %d 2" % (1 << 31), "ips: 2^32 bytes or more in total")
    check("big %d 4096" % (1 << 20), "ips: 2^32 bytes or more in total")
    check("big %d 4095" % (1 << 20), "ok")
    check("big %d 1" % ((1 << 32) - 1), "ok")

    def pack(fip, entries):
        cmds.append("pack %s %s" % ("N" if fip is None else _hex(fip), " ".join(_hex(x) for x in entries)))
        items = [state_query._b(x) for x in entries] + ([] if fip is None else [state_query._b(fip)])
        off = [0]
        for x in items:
            off.append(off[-1] + len(x))
        has_ip = fip is not None
        listed = has_ip and state_query._b(fip) in [state_query._b(x) for x in entries]
        want.append("pack n_list=%d has_ip=%d restrict=%d nothing=%d sel=%d+%d off=%s bytes=%s" % (
            len(entries), has_ip, has_ip or bool(entries), has_ip and bool(entries) and not listed,
            len(entries) if has_ip else 0, 1 if has_ip else len(entries), ",".join(map(str, off)), _hex(b"".join(items))))

    pack(None, [])
    pack("1.2.3.4", [])
    pack("", [])
    pack(None, ["1.2.3.4", "", "2001:db8::1", "1.2.3.4", ""])
    pack("2001:db8::1", ["1.2.3.4", "2001:db8::1"])
    pack("2001:db8::1", ["1.2.3.4", "2001:db8::10", "2001:db8::"])  # a prefix and an extension are other IPs
    pack("", ["1.2.3.4", ""])
    pack("", ["1.2.3.4"])
    rng = random.Random(3)
    for _ in range(30):
        entries = [rng.choice(H.POOL + H.NOT_HELD) for _ in range(rng.randrange(0, 12))]
        pack(rng.choice([None, rng.choice(H.POOL), rng.choice(entries or [""])]), entries)

    shards = [[rng.randrange(1 << 40) for _ in range(9)] + [rng.randrange(1, 100) / 4] for _ in range(5)]
    for n in (0, 1, 5):
        cmds.append("sum %d" % n)
        cmds += ["s " + " ".join("%d" % v for v in s[:9]) + " %g" % s[9] for s in shards[:n]]
        want.append("sum " + " ".join("%d" % sum(s[k] for s in shards[:n]) for k in range(9)) +
                    " %g" % max([s[9] for s in shards[:n]] + [0]))
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
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    return len(want)


def test_host_header_checks_packing_and_node_sum():
    d = tempfile.mkdtemp(prefix="bjx_rm_")
    exe = os.path.join(d, "remove_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, SRC], check=True)
    assert _run_and_check(exe) > 50


def test_standalone_program_under_sanitizers():
    """The same program built with ASan + UBSan and run once as a child process
    over the same script (nothing loaded into Python runs under a sanitizer)."""
    d = tempfile.mkdtemp(prefix="bjx_rm_san_")
    exe = os.path.join(d, "remove_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, SRC], check=True)
    _run_and_check(exe)
