"""State chosen by network on the device (bjx_state_query_nets /
bjx_state_remove_nets and their node forms, include/banjax_gpu.h).

Expected values (tests/state_nets.py): the held IPs come from lines fed through
tests/state_remove.Run, the answers from the pure-Python models
(banjax_amd/state_query.py and state_remove.py with nets=, over
banjax_amd/state_nets.py).  tests/test_state_nets_cpu.py pins that model to the
allow-list model and to the oracle's Exempted flag, and shows that every net
list used here selects some held IPs and not all, whole IPs and parts of IPs."""
import json

import pytest

from banjax_amd import Config, Engine, Node, Ruleset, snapshot, state_nets, state_query
from banjax_amd._lib import BanjaxGpuError
from tests import header_fields as HF
from tests import state_nets as N
from tests import state_remove as H
from tests.state_remove import COUNTS, INT64_MAX, INT64_MIN, Run

pytestmark = pytest.mark.gpu
LISTS = N.lists()


@pytest.fixture(scope="module")
def engine():
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def engine_b():
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def wengine():
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def world(wengine):
    """an engine of its own holding every IP of the world, and its model; the tests that use it only query"""
    run = N.build_world(wengine)
    assert H.dump_ips(wengine.state_dump()) == N.world_ips()
    return run


def check_query(target, run, nets, ips_in_order=None, **filt):
    """the answer of the target equals the model's: counts, rows, net_ips"""
    ips, states = run.model.snapshot_args()
    n, n_ips, rows, net_ips = state_query.select(ips if ips_in_order is None else ips_in_order, states, nets=nets, **filt)
    got = target.state_query(nets=nets, **filt)
    assert (got["n_matched"], got["n_ips_matched"]) == (n, n_ips), (nets[:4], filt, got["n_matched"], n)
    assert got["rows"] == rows, (nets[:4], filt)
    assert got["net_ips"] == net_ips, (nets[:4], filt, got["net_ips"][:8], net_ips[:8])
    return got


def selected_ips(target, nets):
    """the held IPs query_nets selects, every state open"""
    return {r[0].decode() for r in target.state_query(nets=nets, limit=65536)["rows"]}


@pytest.mark.parametrize("name", [k for k in LISTS if LISTS[k][0] == "world" and k != "max"])
def test_prefix_lengths_table_sizes_and_spellings(wengine, world, name):
    """Every edge length of both families, the v4-mapped forms, all 162 lengths
    at once, one length with 1 .. 257 networks, nested and duplicate entries:
    the held IPs lie at the edges of each network, in several spellings, and
    among them are texts that are no addresses."""
    nets = LISTS[name][1]
    got = check_query(wengine, world, nets, limit=65536)
    table = state_nets.Nets(nets)
    want = {ip for ip in N.world_ips() if table.holds(ip)}
    assert {r[0].decode() for r in got["rows"]} == want and 0 < len(want) < len(N.world_ips())
    assert not want & set(N.NOT_ADDRESSES)
    check_query(wengine, world, nets, limit=0)


def test_spellings_select_alike_and_non_addresses_never(wengine, world):
    for name, base in (("spell4", HF.V4_PREFIX + N.BASE4), ("spell6", N.BASE6)):
        sel = selected_ips(wengine, LISTS[name][1])
        assert set(HF.spellings(base)) <= sel
    assert "::170.85.195.60" not in selected_ips(wengine, LISTS["spell4"][1])     # IPv6 text that is not v4-mapped
    everything = selected_ips(wengine, ["0.0.0.0/0", "::/0"])
    assert not everything & set(N.NOT_ADDRESSES)
    assert everything == {ip for ip in N.world_ips() if state_nets.parse_ip(ip)}
    v4 = selected_ips(wengine, ["0.0.0.0/0"])
    v6 = selected_ips(wengine, ["::/0"])
    assert not v4 & v6 and v4 | v6 == everything and "::ffff:170.85.195.60" in v4 and "::170.85.195.60" in v6


def test_query_orders_filters_and_limits(wengine, world):
    nets = LISTS["nested_dup"][1]
    n_all = check_query(wengine, world, nets, limit=0)["n_matched"]
    assert n_all > 20
    for order in (state_query.BY_HITS, state_query.BY_START):
        for filt in ({}, {"name": "mid"}, {"min_hits": 2}, {"name": "slow", "min_hits": 1, "min_start_ns": N.NOW + 50_000_000},
                     {"name": "never-interned"}, {"min_start_ns": 5, "max_start_ns": 4}):
            for limit in (0, 1, 7, n_all + 5):
                check_query(wengine, world, nets, order=order, limit=limit, **filt)
    # nested and duplicate entries count separately
    got = wengine.state_query(nets=nets, limit=0)
    assert got["net_ips"][0] == got["net_ips"][3] >= got["net_ips"][1] == got["net_ips"][6] > got["net_ips"][2] > 0
    assert got["net_ips"][5] == 0 and sum(got["net_ips"]) > got["n_ips_matched"]


def test_ip_filter_with_nets(wengine, world):
    nets = LISTS["nested_dup"][1]
    for ip in ("170.85.195.60", "::ffff:170.85.195.60", "2001:db8:85a3:c55a:aa55:c33c:ff1:ce5a",   # inside
               "9.9.9.9", "2001:db8::1", "01.2.3.4", "",                                             # held, outside every net
               "170.85.195.77", "2001:db8:85a3::77", "not-an-ip"):                                   # not held
        for filt in ({}, {"name": "mid"}, {"min_hits": 3}):
            for limit in (0, 5):
                check_query(wengine, world, nets, ip=ip, limit=limit, **filt)
    got = wengine.state_query(nets=nets, ip="170.85.195.60", limit=5)
    assert got["n_ips_matched"] == 1 and got["net_ips"] == [1, 1, 1, 1, 0, 0, 1, 0]
    assert wengine.state_query(nets=nets, ip="9.9.9.9", limit=5)["n_matched"] == 0
    assert wengine.state_query(ip="9.9.9.9", limit=5)["n_matched"] > 0


def test_the_cap_and_bad_arguments(wengine, world):
    """BJX_NETS_MAX entries once; one more, no entry, a typo: BJX_ERR_ARG and nothing changed."""
    check_query(wengine, world, LISTS["max"][1], limit=10)
    before = wengine.state_dump()
    for nets, word in ((LISTS["max"][1] + ["1.2.3.4"], "BJX_NETS_MAX"), ([], "empty"), (["10.0.0.0/8", "10.0.0.0/33"], "entry 1 "),
                       (["10.0.0.0/8", "::/0", "1.2.3"], "entry 2 "), ([""], "entry 0 "), (["1.2.3.4%eth0"], "entry 0 ")):
        for call in (wengine.state_query, wengine.state_remove):
            with pytest.raises(BanjaxGpuError) as ei:
                call(nets=nets)
            assert ei.value.code == -2 and word in str(ei.value), (nets[-2:], str(ei.value))
    import ctypes as C
    from banjax_amd import _lib
    L = _lib.lib()
    f = _lib.StateFilter(_lib.Str(None, 0), _lib.Str(None, 0), INT64_MIN, INT64_MIN, INT64_MAX, 0, 0)
    rows = _lib.StateRows()
    bad = (_lib.Str * 2)(_lib.Str(b"1.2.3.4", 7), _lib.Str(None, 5))
    assert L.bjx_state_query_nets(wengine._h, C.byref(f), None, 1, C.byref(rows), None) == _lib.ERR_ARG
    assert L.bjx_state_remove_nets(wengine._h, C.byref(f), None, 1, None) == _lib.ERR_ARG
    assert L.bjx_state_remove_nets(wengine._h, C.byref(f), bad, 2, None) == _lib.ERR_ARG
    assert L.bjx_state_remove_nets(wengine._h, None, bad, 1, None) == _lib.ERR_ARG
    assert L.bjx_state_query_nets(wengine._h, C.byref(f), bad, 1, C.byref(rows), None) == _lib.OK  # net_ips may be NULL
    assert wengine.state_dump() == before


def test_same_rule_as_the_match_path(wengine, engine_b, world):
    """The held IP texts as lines to an engine whose global decision list
    allows the entries: a line is Exempted exactly when query_nets selects its IP."""
    ips = [ip for ip in N.world_ips() if ip]
    data = "".join("%d.%03d %s GET h.test GET /x HTTP/1.1 ua\n" % (HF.NOW_BASE // HF.S - 3, k % 1000, ip)
                   for k, ip in enumerate(ips)).encode()
    try:
        for name in ("nested_dup", "all_lengths", "mapped/104", "v6/65", "size_257"):
            nets = LISTS[name][1]
            cfg = Config.from_yaml(HF.RULES_YAML + "global_decision_lists:\n  allow:\n" +
                                   "".join("    - %s\n" % json.dumps(e) for e in nets))
            engine_b.state_clear()
            engine_b.set_decision_lists(cfg.decision_entries)
            out = engine_b.process(Ruleset(cfg), data, HF.NOW_BASE, copy_results=True)
            flags = list(out.line_flags)
            assert len(flags) == len(ips)
            sel = selected_ips(wengine, nets)
            bad = [(ip, f) for ip, f in zip(ips, flags) if (f == HF.LINE_EXEMPTED) != (ip in sel)]
            assert not bad, (name, bad[:5])
            assert 0 < flags.count(HF.LINE_EXEMPTED) < len(flags)
    finally:
        engine_b.set_decision_lists([])
        engine_b.state_clear()


def test_unchanged_paths_and_preview(wengine, world):
    """state_query and state_remove without nets answer the same before and after nets calls."""
    plain = [wengine.state_query(limit=20), wengine.state_query(name="mid", order="start", limit=9), wengine.state_query(ip="9.9.9.9")]
    dump = wengine.state_dump()
    nothing = wengine.state_remove(ips=["198.51.100.1"])
    wengine.state_query(nets=LISTS["all_lengths"][1], limit=50)
    wengine.state_remove(nets=["198.51.100.0/24"])
    again = [wengine.state_query(limit=20), wengine.state_query(name="mid", order="start", limit=9), wengine.state_query(ip="9.9.9.9")]
    for a, b in zip(plain, again):
        assert {k: v for k, v in a.items() if k != "device_ms"} == {k: v for k, v in b.items() if k != "device_ms"}
        assert "net_ips" not in b
    s = wengine.state_remove(ips=["198.51.100.1"])
    assert {k: s[k] for k in COUNTS} == {k: nothing[k] for k in COUNTS} and wengine.state_dump() == dump


@pytest.mark.parametrize("n", N.COUNTS_HELD)
def test_held_ip_counts(engine_b, n):
    """1, 255, 257 and 3001 held IPs: one lane, under and over a block, a grid-stride tail."""
    run = N.build_world(engine_b, N.count_ips(n))
    got = check_query(engine_b, run, N.COUNT_NETS, limit=40)
    table = state_nets.Nets(N.COUNT_NETS)
    assert got["n_ips_matched"] == sum(1 for ip in N.count_ips(n) if table.holds(ip)) > 0
    preview = engine_b.state_query(nets=N.COUNT_NETS, name="mid", limit=0)
    s, partial = run.remove(nets=N.COUNT_NETS, name="mid")
    assert s["states_dropped"] == preview["n_matched"] > 0 and s["ips_found"] == got["n_ips_matched"]
    s, _ = run.remove(nets=N.COUNT_NETS)
    assert s["ips_dropped"] == s["ips_found"] == got["n_ips_matched"]
    run.compare_states(ips=N.count_ips(n)[::97], dump=n < 300)
    assert H.dump_ips(engine_b.state_dump()) == list(run.model.st)


def test_more_networks_than_the_counting_table_holds(engine_b):
    """3001 held IPs, walked by one block of k_net_count: 2047, 2048, 2049 and
    2600 of them listed as single addresses next to one /8 that holds most, so
    the block's LDS table of 2048 networks is short of, exactly and over full."""
    run = N.build_world(engine_b, N.count_ips(N.COUNTS_HELD[-1]))
    for n in N.SINGLES_N:
        nets = LISTS["singles_%d" % n][1]
        got = check_query(engine_b, run, nets, limit=0)
        assert got["net_ips"][:n] == [1] * n and got["net_ips"][n] > 2000
        check_query(engine_b, run, nets, name="slow", limit=3)


@pytest.mark.parametrize("mask", [0, 0x2])
def test_remove_parity_across_batches(engine, engine_b, monkeypatch, mask):
    """Three batches with removals by nets in between, under BJX_CHECK=1 (and
    once with every IP on one of two hash values): stats, every later
    RuleResult, trips, state_get, the dump and, byte for byte, the export equal
    the model; a second engine that imports the model's snapshot goes on identically."""
    monkeypatch.setenv("BJX_CHECK", "1")
    engine.debug_set_ip_hash_mask(mask)
    try:
        stream = H.stream()
        run = Run(H.CFG, engine)
        done = []
        for b, (data, now) in enumerate(stream[:3]):
            run.feed(data, now)
            sel = N.pool_selection(b, now)
            preview = engine.state_query(limit=0, **sel)
            s, partial = run.remove(**sel)
            assert preview["n_matched"] == s["states_dropped"]
            done.append((s, partial))
            run.compare_states(dump=not mask)
            if not mask:
                assert engine.state_export() == snapshot.build(*run.model.snapshot_args())
        assert all(0 < s["states_dropped"] < s["states_before"] and s["ips_found"] > 0 for s, _ in done)
        assert done[0][0]["ips_dropped"] == done[0][0]["ips_found"] and done[1][1] > 0 and done[2][1] > 0
        assert run.diff_first > 0 and run.diff_seen > 0
        if not mask:
            engine_b.state_clear()
            engine_b.state_import(snapshot.build(*run.model.snapshot_args()))
            data, now = stream[3]
            run.feed(data, now, targets=[engine, engine_b])
            assert engine.state_export() == engine_b.state_export() == snapshot.build(*run.model.snapshot_args())
    finally:
        engine.debug_set_ip_hash_mask(0)


def test_nothing_selected_leaves_the_engine_as_it_was():
    """Networks that hold nobody, a never-interned name, an empty window, a
    filter IP outside the nets: no rebuild, on an engine whose arena has grown
    past its floor (a rebuild would shrink it)."""
    eng = Engine(ip_arena_bytes=1 << 16)
    try:
        n = 30_000
        ips = ["172.%d.%d.%d" % (16 + (k >> 16), (k >> 8) & 255, k & 255) for k in range(n)]
        run = Run(H.one_rule(60, 100), eng)
        run.feed(H.lines([(k // 10, ip) for k, ip in enumerate(ips)]), H.T0_MS * 1_000_000)
        stats0, dump0 = eng.state_stats(), eng.state_dump()
        assert stats0["arena_capacity"] > 1 << 16
        for sel, found in (({"nets": ["9.9.9.0/24", "2001:db8::/32", "172.15.0.0/16", "::/0"]}, 0),
                           ({"name": "never-interned", "nets": ["172.16.0.0/24"]}, 256),
                           ({"min_start_ns": 5, "max_start_ns": 4, "nets": ["172.16.1.0/25", "172.16.1.128/25", "172.16.1.7"]}, 256),
                           ({"ip": ips[0], "nets": ["172.16.1.0/24"]}, 256),
                           ({"ip": "9.9.9.9", "nets": ["0.0.0.0/0"]}, n),
                           ({"min_hits": 2, "nets": ["0.0.0.0/0"]}, n)):
            s = eng.state_remove(**sel)
            assert (s["states_dropped"], s["ips_dropped"], s["ips_found"]) == (0, 0, found), (sel, s)
            assert s["arena_bytes_after"] == s["arena_bytes_before"] == stats0["arena_bytes"]
            assert s["device_bytes_after"] == s["device_bytes_before"] == stats0["device_bytes"]
            assert eng.state_stats() == stats0, sel
        assert eng.state_dump() == dump0
        s, _ = run.remove(nets=["172.16.0.0/18"])    # and one that selects: the arena shrinks
        assert s["ips_dropped"] == s["ips_found"] == 64 * 256 and s["device_bytes_after"] < s["device_bytes_before"]
        run.compare_states(ips=ips[::997], dump=False)
    finally:
        eng.close()


def test_refused_inside_an_open_batch(engine):
    import torch
    stream = H.stream()
    run = Run(H.CFG, engine)
    data, now = stream[0]
    run.feed(data, now)
    before = engine.state_dump()
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    engine.match(run.rs, now, buf.data_ptr(), len(data))
    for call in (engine.state_remove, engine.state_query):
        with pytest.raises(BanjaxGpuError) as ei:
            call(nets=["10.1.0.0/24"])
        assert ei.value.code == -2
    assert engine.state_dump() == before
    data, now = stream[1]
    run.feed(data, now)
    run.remove(**N.pool_selection(0, now))
    run.compare_states()


def test_node_equals_single_engine(engine):
    """Two engines on device 0: query rows, net_ips and the removal's stats
    through the node equal one engine over the same stream."""
    stream = H.stream()
    nets = LISTS["pool_node"][1] + N.pool_selection(0, 0)["nets"]
    single = Run(H.CFG, engine)
    single.feed(*stream[0])
    node = Node([0, 0])
    try:
        sharded = Run(H.CFG, node)
        sharded.feed(*stream[0])
        order = H.dump_ips(node.state_dump())       # engine-major first-seen order
        assert sorted(order) == sorted(single.model.st)
        for filt in ({"limit": 0}, {"limit": 25}, {"limit": 25, "order": state_query.BY_START, "name": "mid"},
                     {"limit": 500, "min_hits": 2}, {"limit": 5, "ip": "10.1.0.70"}, {"limit": 5, "ip": "10.1.0.1", "name": "fast"}):
            a = check_query(engine, single, nets, **filt)
            b = check_query(node, sharded, nets, ips_in_order=order, **filt)
            assert (a["n_matched"], a["n_ips_matched"], a["net_ips"]) == (b["n_matched"], b["n_ips_matched"], b["net_ips"])
            assert sorted(a["rows"]) == sorted(b["rows"]) or filt["limit"] < a["n_matched"]
        with pytest.raises(BanjaxGpuError) as ei:
            node.state_query(nets=["10.0.0.0/8", "nope"])
        assert ei.value.code == -2 and "entry 1 " in str(ei.value)
        for sel in (N.pool_selection(1, 0), {"nets": LISTS["pool_node"][1]}, {"nets": ["192.0.2.0/24"]}):
            a, _ = single.remove(**sel)
            b, _ = sharded.remove(**sel)
            assert {k: a[k] for k in COUNTS} == {k: b[k] for k in COUNTS}
        sharded.compare_states(dump=False)
        sharded.feed(*stream[1])
        sharded.compare_states(dump=False)
    finally:
        node.close()
