"""Selection of state by network without a GPU: the C symbols and their NULL
handling; the pure-Python model of entries and membership
(banjax_amd/state_nets.py) against the allow-list model of the header tests
and against the oracle's Exempted flag; that the net lists of the GPU tests are
telling (computed with the models alone); and the host parts of the calls --
argument checks, the canonical net table, the entry map, membership of one IP
text, the node's sum (banjax_amd/csrc/state_nets.h) -- built for the host from
tests/cpu/nets_host.cpp, a program with its own main."""
import ctypes
import json
import os
import random
import subprocess
import tempfile

import pytest

from oracle import oracle as O

from banjax_amd import Config, _lib, state_nets, state_query, state_remove
from tests import header_fields as HF
from tests import state_nets as N
from tests import state_remove as H
from tests.parity import oracle_config

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu", "nets_host.cpp")

# entries of every kind: both families, v4-mapped text, host bits set, every edge length
ENTRIES = ["170.85.195.60", "170.85.195.60/32", "10.1.2.3/8", "0.0.0.0/0", "128.0.0.0/1", "170.85.195.60/31", "170.84.0.0/15",
           "::/0", "8000::/1", "2001:db8:85a3:c55a::/64", "2001:db8:85a3:c55a:8000::/65", "2001:db8:85a3:c55a::/63",
           "2001:db8:85a3:c55a:aa55:c33c:ff1:ce5a/127", "2001:db8:85a3:c55a:aa55:c33c:ff1:ce5a/128", "2001:db8::1",
           "::ffff:10.0.0.0/104", "::ffff:0:0/96", "::ffff:1.2.3.4", "::ffff:1.2.3.4/128", "::ffff:1.2.3.4/95", "::1.2.3.4/120",
           "0:0:0:0:0:ffff:102:304/120", "1:2:3:4:5:6:7:8/000000000000000064", "255.255.255.255/32", "ffff::/16"]
BAD_ENTRIES = ["", "1.2.3", "01.2.3.4", "1.2.3.4/33", "1.2.3.4/", "1.2.3.4/-1", "1.2.3.4/8 ", " 1.2.3.4", "1.2.3.4%eth0", "fe80::1%eth0/64",
               "::1/129", "1.2.3.4/16777215", "/8", "1.2.3.4/8/8", "x", "1::2::3", "1.2.3.4/0x8", "::ffff:1.2.3.4/129", "1.2.3.4/٣"]


def test_symbols_and_null_arguments():
    L = _lib.lib()
    for name in ("bjx_state_query_nets", "bjx_node_state_query_nets", "bjx_state_remove_nets", "bjx_node_state_remove_nets"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert _lib.NETS_MAX == state_nets.NETS_MAX == N.NETS_MAX == 65536
    f, rows, st = _lib.StateFilter(), _lib.StateRows(), _lib.RemoveStats()
    one = (_lib.Str * 1)(_lib.Str(b"1.2.3.4", 7))
    p = ctypes.POINTER(ctypes.c_uint64)()
    for fn in (L.bjx_state_query_nets, L.bjx_node_state_query_nets):
        assert fn(None, ctypes.byref(f), one, 1, ctypes.byref(rows), ctypes.byref(p)) == _lib.ERR_ARG
        assert fn(None, None, None, 0, None, None) == _lib.ERR_ARG
    for fn in (L.bjx_state_remove_nets, L.bjx_node_state_remove_nets):
        assert fn(None, ctypes.byref(f), one, 1, ctypes.byref(st)) == _lib.ERR_ARG
        assert fn(None, None, None, 0, None) == _lib.ERR_ARG


# ---- the model of entries and membership

def _allow_model(entries):
    return HF.AllowModel([(None, "allow", e) for e in entries])


def _ip_texts():
    out = HF.sweep_ips(3000, 77)
    for b in (N.BASE6, HF.V4_PREFIX + N.BASE4, HF.V4_PREFIX + bytes([10, 200, 3, 4]), bytes(12) + bytes([1, 2, 3, 4]),
              bytes.fromhex("20010db8000000000000000000000001")):
        out += HF.spellings(b)
    return list(dict.fromkeys(out + N.world_ips()))


def test_entries_equal_the_allow_entry_model():
    """An entry is filed exactly when ToggleIP files it, under the network IPNet.Contains compares."""
    for e in ENTRIES + BAD_ENTRIES + N.all_lengths() + ["::ffff:154.101.60.195/%d" % n for n in range(130)]:
        got, want = state_nets.parse_entry(e), HF.model_entry(e)
        assert (got is None) == (want is None), (e, got, want)
        if want is None:
            continue
        fam, bits, v = got
        if want[0] == "addr":
            mapped = want[1][:12] == HF.V4_PREFIX
            assert got == ((4, 32, int.from_bytes(want[1][12:], "big")) if mapped else (6, 128, int.from_bytes(want[1], "big"))), e
        else:
            _, netlen, net, mask = want
            assert (fam, bits, v) == (4 if netlen == 4 else 6, bin(int.from_bytes(mask, "big")).count("1"),
                                      int.from_bytes(net, "big")), e
    assert all(state_nets.parse_entry(e) is not None for e in ENTRIES)
    assert all(state_nets.parse_entry(e) is None for e in BAD_ENTRIES)
    with pytest.raises(ValueError, match="entry 2 "):
        state_nets.Nets(["1.2.3.4", "::/0", "1.2.3", "bad"])
    with pytest.raises(ValueError):
        state_nets.Nets([])
    with pytest.raises(ValueError):
        state_nets.Nets(["1.2.3.4"] * (N.NETS_MAX + 1))
    state_nets.Nets(["1.2.3.4"] * N.NETS_MAX)


def test_membership_equals_the_allow_list_model():
    """Nets.holds equals CheckIsAllowed with a global Allow list of the same
    entries, for every entry alone, for random groups of them and for the net
    lists of the GPU tests, over swept IP texts and every spelling."""
    texts = _ip_texts()
    rng = random.Random(5)
    groups = [[e] for e in ENTRIES] + [rng.sample(ENTRIES, rng.randrange(2, 9)) for _ in range(40)]
    groups += [nets for name, (_, nets) in N.lists().items() if name != "max"]
    inside = outside = 0
    for g in groups:
        table, model = state_nets.Nets(g), _allow_model(g)
        for t in texts:
            got, want = table.holds(t), model.allowed(None, t)
            assert got == want, (g, t, got, want)
            assert bool(table.which(t)) == got
            inside += got
            outside += not got
    assert inside > 5000 and outside > 5000
    # the decided cases
    assert not state_nets.Nets(["::/0"]).holds("1.2.3.4") and not state_nets.Nets(["::/0"]).holds("::ffff:1.2.3.4")
    assert not state_nets.Nets(["0.0.0.0/0"]).holds("::1") and state_nets.Nets(["0.0.0.0/0"]).holds("::ffff:1.2.3.4")
    assert state_nets.Nets(["::ffff:10.0.0.0/104"]).holds("10.255.0.1") and not state_nets.Nets(["::ffff:10.0.0.0/104"]).holds("11.0.0.0")
    assert state_nets.Nets(["10.1.2.3/8", "10.0.0.0/8", "10.1.0.0/16"]).which("10.1.9.9") == [0, 1, 2]
    for t in N.NOT_ADDRESSES:
        assert not state_nets.Nets(["0.0.0.0/0", "::/0"]).holds(t), t


def test_membership_equals_the_oracles_exempted_flag():
    """The same IP texts as lines through the oracle with the entries as its global allow list."""
    texts = [t for t in _ip_texts() if t and not set(t) & set(" \n\t\r")]
    data = "".join("%d.%03d %s GET h.test GET /x HTTP/1.1 ua\n" % (HF.NOW_BASE // HF.S - 3, k % 1000, t)
                   for k, t in enumerate(texts)).encode("latin-1")
    rng = random.Random(6)
    for g in ([ENTRIES[:7], ENTRIES[7:15], ENTRIES[15:], N.lists()["nested_dup"][1], N.all_lengths()[::7]] +
              [rng.sample(ENTRIES, 5) for _ in range(4)]):
        yaml_text = HF.RULES_YAML + "global_decision_lists:\n  allow:\n" + "".join("    - %s\n" % json.dumps(e) for e in g)
        cfg = Config.from_yaml(yaml_text)
        flags, _, consumed = O.State().consume(oracle_config(cfg), data, HF.NOW_BASE, cap=2 * (len(texts) + 1))
        assert consumed == len(data) and len(flags) == len(texts)
        table = state_nets.Nets(g)
        bad = [(t, f) for t, f in zip(texts, flags) if (f == O.LINE_EXEMPTED) != table.holds(t)]
        assert not bad, (g, bad[:5])
        assert 0 < sum(1 for f in flags if f == O.LINE_EXEMPTED) < len(flags)


# ---- the query's and the removal's models with nets

def test_models_with_nets():
    ips = ["10.0.0.1", "10.0.1.1", "::ffff:10.0.0.2", "2001:db8::1", "bogus", "11.0.0.1"]
    states = {ip: {"a": (k + 1, 100 + k), "b": (1, 200)} for k, ip in enumerate(ips)}
    nets = ["10.0.0.0/24", "10.0.0.0/16", "2001:db8::/32", "10.0.0.0/24", "192.0.2.1"]
    n, n_ips, rows, net_ips = state_query.select(ips, states, nets=nets, limit=3)
    assert (n, n_ips, net_ips) == (8, 4, [2, 3, 1, 2, 0])
    assert rows == [(b"2001:db8::1", b"a", 4, 103), (b"::ffff:10.0.0.2", b"a", 3, 102), (b"10.0.1.1", b"a", 2, 101)]
    n, n_ips, rows, net_ips = state_query.select(ips, states, nets=nets, name="a", min_hits=3, limit=0)
    assert (n, n_ips, rows, net_ips) == (2, 2, [], [1, 1, 1, 1, 0])
    assert state_query.select(ips, states, nets=nets, ip="11.0.0.1", limit=9) == (0, 0, [], [0] * 5)
    assert state_query.select(ips, states, nets=nets, ip="10.0.1.1", limit=0) == (2, 1, [], [0, 1, 0, 0, 0])
    assert state_query.select(ips, states, limit=0) == (12, 6, [])   # without nets: the old answer, three fields
    kept_ips, kept, c = state_remove.remove(ips, states, nets=nets, name="a")
    assert c["ips_found"] == 4 and c["states_dropped"] == 4 and c["ips_dropped"] == 0
    assert c["states_dropped"] == state_query.select(ips, states, nets=nets, name="a")[0]
    kept_ips, kept, c = state_remove.remove(ips, states, nets=nets)
    assert kept_ips == [b"bogus", b"11.0.0.1"] and c["ips_found"] == c["ips_dropped"] == 4
    _, _, c = state_remove.remove(ips, states, nets=nets, ip="11.0.0.1")
    assert (c["ips_found"], c["states_dropped"]) == (4, 0)
    with pytest.raises(ValueError):
        state_remove.remove(ips, states, nets=[])
    with pytest.raises(ValueError):
        state_remove.remove(ips, states, nets=nets, ips=["10.0.0.1"])


def test_gpu_test_inputs_are_telling():
    """Every net list of tests/test_gpu_state_nets.py, on the held IPs it is
    used with: it holds some held IPs and not all; alone it takes whole IPs;
    under a name filter it takes a part of IPs that keep their other states."""
    worlds = {}
    for w in ("world", "count"):
        run = N.build_world(None, N.world_of(w))
        assert list(run.model.st) == N.world_of(w)
        worlds[w] = run.model.snapshot_args()
    run = H.Run(H.CFG, None)
    for data, now in H.stream()[:1]:
        run.feed(data, now)
    worlds["pool"] = run.model.snapshot_args()
    seen = set()
    for name, (w, nets) in N.lists().items():
        ips, states = worlds[w]
        _, _, c = state_remove.remove(ips, states, nets=nets)
        assert 0 < c["ips_found"] < c["ips_before"], (name, c)
        assert c["ips_dropped"] == c["ips_found"] and 0 < c["states_dropped"] < c["states_before"], (name, c)
        kept_ips, kept, c = state_remove.remove(ips, states, nets=nets, name="mid")
        partial = sum(1 for i in kept_ips if len(kept[i]) < len(states[i.decode()]))
        assert c["states_dropped"] > 0 and partial > 0, (name, c)
        n, n_ips, _, net_ips = state_query.select(ips, states, nets=nets, name="mid")
        assert n == c["states_dropped"] and n_ips == partial + c["ips_dropped"] and max(net_ips) > 0, name
        seen.add(w)
    assert seen == {"world", "count", "pool"}
    # the parity run's removals drop some states and not all, whole IPs and parts
    run, done = N.parity_run(None, H.stream())
    for b, (c, partial) in enumerate(done):
        assert 0 < c["states_dropped"] < c["states_before"] and c["ips_found"] > 0, (b, c)
    assert done[0][0]["ips_dropped"] == done[0][0]["ips_found"] > 30 and done[1][1] > 0 and done[2][1] > 0
    assert run.diff_first > 0 and run.diff_seen > 0
    # the spellings of one address are different held IPs that one entry holds alike
    ips, states = worlds["world"]
    for name, base in (("spell4", HF.V4_PREFIX + N.BASE4), ("spell6", N.BASE6)):
        table = state_nets.Nets(N.lists()[name][1])
        texts = HF.spellings(base)
        assert len(texts) >= 5 and all(t in ips and table.holds(t) for t in texts)
    # the sizes: held IPs below the first network, between neighbours and above the last
    for n in N.SIZE_N:
        table = state_nets.Nets(N.lists()["size_%d" % n][1])
        got = [table.holds(ip) for ip in N.size_ips()]
        assert got[0] is False and got[2::2] == [False] * len(N.SIZE_AT)
        assert got[1::2] == [i < n for i in N.SIZE_AT]


# ---- the host header, through tests/cpu/nets_host.cpp

def _hex(b):
    b = state_query._b(b)
    return b.hex() if b else "-"


def _canonical(entries):
    """-> (sorted distinct (family, bits, network), caller entry -> index)"""
    keys = [state_nets.parse_entry(e) for e in entries]
    canon = sorted(set(keys))
    return canon, [canon.index(k) for k in keys]


def _build_line(entries):
    canon, entry = _canonical(entries)
    dirs, k4, k6 = [], [], []
    for fam, bits, v in canon:
        arr = k4 if fam == 4 else k6
        if not dirs or dirs[-1][:2] != [fam, bits]:
            dirs.append([fam, bits, len(arr), 0])
        dirs[-1][3] += 1
        arr.append("%08x" % v if fam == 4 else "%032x" % v)
    return "build dir=%s k4=%s k6=%s entry=%s" % (",".join("%d/%d:%d+%d" % tuple(d) for d in dirs), ",".join(k4) or "-",
                                                   ",".join(k6) or "-", ",".join(map(str, entry)))


def _script():
    """-> (command lines, the expected output lines)"""
    cmds, want = [], []

    def check(line, answer):
        cmds.append(line)
        want.append("check " + answer)

    ip = _hex("1.2.3.4")
    check("check NOFILTER", "no filter")
    check("check N N 1 %s" % ip, "ok")
    check("check - - 1 %s %s" % (ip, _hex("::/0")), "ok")
    check("check N N 0 %s" % ip, "nets: no list")
    check("check N N 0", "nets: no list")
    check("check N N 1", "nets: an empty list (a nets call never means every IP)")
    check("check N N 1 %s N3" % ip, "nets: an entry with a length and no bytes")
    check("check N N 1 N %s" % ip, "ok")   # a NULL pointer of length 0 passes the checks; it does not file
    check("check N5 N 1 %s" % ip, "filter: ip with a length and no bytes")
    check("check N N2 1 %s" % ip, "filter: name with a length and no bytes")
    check("many %d" % (N.NETS_MAX + 1), "nets: more than BJX_NETS_MAX entries")
    check("many %d" % (1 << 40), "nets: more than BJX_NETS_MAX entries")

    def build(entries):
        cmds.append("build " + " ".join(_hex(e) for e in entries))
        bad = next((k for k, e in enumerate(entries) if state_nets.parse_entry(e) is None), None)
        want.append("build bad=%d (nets: entry %d is not an address or address/bits)" % (bad, bad) if bad is not None
                    else _build_line(entries))

    build(["10.1.2.3/8"])
    build(["10.1.2.3/8", "10.0.0.0/8", "10.255.255.255/8", "::ffff:10.0.0.0/104"])      # one network, four times
    build(["0.0.0.0/0", "::/0", "::ffff:0:0/96", "255.1.2.3/0"])
    build(["1.2.3.4", "1.2.3.4/32", "::ffff:1.2.3.4", "::ffff:102:304/128", "::1.2.3.4", "::1.2.3.4/128"])
    build(["10.0.0.0/8", "10.1.0.0/16", "10.1.2.0/24", "10.1.2.3", "10.1.0.0/16"])      # nested, one twice
    build(ENTRIES)
    build(list(reversed(ENTRIES)) + ENTRIES)
    build(N.all_lengths())
    build(["1.2.3.4", "bad", "1.2.3"])
    build(["1.2.3.4/33"])
    build([""])
    for k, e in enumerate(BAD_ENTRIES):
        build(ENTRIES[:k] + [e])
    rng = random.Random(11)
    for _ in range(20):
        build([rng.choice(ENTRIES + ["10.%d.0.0/%d" % (rng.randrange(4), rng.randrange(8, 18)),
                                     "2001:db8:%x::/%d" % (rng.randrange(4), rng.randrange(40, 70))]) for _ in range(rng.randrange(1, 30))])
    build(N.lists()["size_257"][1])

    def holds(text, entries):
        cmds.append("holds %s %s" % (_hex(text), " ".join(_hex(e) for e in entries)))
        canon, entry = _canonical(entries)
        idx = sorted({entry[k] for k in state_nets.Nets(entries).which(text)})
        want.append("holds %d canon=%s" % (bool(idx), ",".join(map(str, idx)) or "-"))

    texts = N.world_ips()[::5] + HF.spellings(N.BASE6) + HF.spellings(HF.V4_PREFIX + N.BASE4) + N.NOT_ADDRESSES + HF.sweep_ips(150, 3)
    for t in texts:
        holds(t, ENTRIES)
        holds(t, N.all_lengths())
    holds("170.85.195.60", ["170.85.195.60", "170.85.195.61/31", "170.85.195.60/32", "0.0.0.0/0", "::/0"])

    shards = [[rng.randrange(1 << 40) for _ in range(6)] for _ in range(5)]
    for n_shards in (0, 1, 5):
        cmds.append("sum 6 %d" % n_shards)
        cmds += ["s " + " ".join(map(str, s)) for s in shards[:n_shards]]
        want.append("sum" + "".join(" %d" % sum(s[k] for s in shards[:n_shards]) for k in range(6 if n_shards else 0)))
    cmds += ["sum 3 3", "s 1 2 3", "s N", "s 10 20 30"]     # a shard without an array adds nothing
    want.append("sum 11 22 33")
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
    for c, g, w in zip(cmds_of(cmds), got, want):
        assert g == w, c
    return len(want)


def cmds_of(cmds):
    """the commands that print an answer (the "s" lines belong to their "sum")"""
    return [c for c in cmds if not c.startswith("s ")]


def test_host_header_checks_tables_and_node_sum():
    d = tempfile.mkdtemp(prefix="bjx_nets_")
    exe = os.path.join(d, "nets_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, SRC], check=True)
    assert _run_and_check(exe) > 300


def test_standalone_program_under_sanitizers():
    """The same program built with ASan + UBSan and run once as a child process
    over the same script (nothing loaded into Python runs under a sanitizer)."""
    d = tempfile.mkdtemp(prefix="bjx_nets_san_")
    exe = os.path.join(d, "nets_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, SRC], check=True)
    _run_and_check(exe)
