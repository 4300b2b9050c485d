"""Forgetting chosen states on the device (bjx_state_remove, include/banjax_gpu.h).

Expected values (tests/state_remove.py): the oracle says which (line, rule)
pairs are events, a Python restatement of RegexRateLimitStates.Apply replays
them, and banjax_amd.state_remove.remove -- the removal's pure-Python model --
takes the selected states out at the same batch boundaries as the engine.  The
engine must equal that model on the stats, on every later RuleResult, on the
trips, on state_get, on the dump (IPs in first-seen order) and, byte for byte,
on the snapshot.  tests/test_state_remove_cpu.py shows that the selections used
here drop some states and not all, whole IPs and parts of IPs."""
import random

import pytest

from oracle import oracle as O

from banjax_amd import Engine, Node, snapshot
from banjax_amd._lib import BanjaxGpuError
from tests import state_remove as H
from tests.parity import compare_batch
from tests.state_remove import COUNTS, INT64_MAX, INT64_MIN, POOL, S, T0_MS, Run

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def stream():
    return H.stream()


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


def test_model_parity_across_batches(engine, stream, monkeypatch):
    """A list (short and long IPs, some not held, some twice), a rule name, and
    min_hits with a start window and a list, one after each of the first three
    batches, the batches under BJX_CHECK=1."""
    monkeypatch.setenv("BJX_CHECK", "1")
    run, done = H.parity_run(engine, stream)
    assert [s["ips_found"] for s, _ in done][:2] == [35, 0]
    assert all(0 < s["states_dropped"] < s["states_before"] for s, _ in done)
    assert run.diff_first > 0 and run.diff_seen > 0


def test_snapshot_exactness(engine, engine_b, stream):
    """After a removal the export is the snapshot of the model's state byte for
    byte, and an engine that imports it goes on exactly as the one that removed."""
    run = Run(H.CFG, engine)
    for data, now in stream[:2]:
        run.feed(data, now)
    run.remove(**H.selection(0, stream[1][1]))
    run.remove(**H.selection(2, stream[1][1]))
    blob = engine.state_export()
    assert blob == snapshot.build(*run.model.snapshot_args())
    engine_b.state_clear()
    engine_b.state_import(blob)
    assert engine_b.state_dump() == engine.state_dump() == run.model.dump()
    data, now = stream[2]
    run.feed(data, now, targets=[engine, engine_b])
    assert engine.state_export() == engine_b.state_export() == snapshot.build(*run.model.snapshot_args())
    assert engine.state_query(limit=50)["rows"] == engine_b.state_query(limit=50)["rows"]


def test_expiry_is_a_special_case(engine, engine_b, stream):
    """state_expire(cutoff) and state_remove(max_start_ns=cutoff - 1) leave the
    same state and report the same counts; the counts-only query previews them."""
    run = Run(H.CFG, engine)
    engine_b.state_clear()
    for data, now in stream[:2]:
        run.feed(data, now, targets=[engine, engine_b])
    cutoff = stream[1][1] + 45 * S
    preview = engine_b.state_query(max_start_ns=cutoff - 1, limit=0)
    a = engine.state_expire(cutoff)
    b = engine_b.state_remove(max_start_ns=cutoff - 1)
    counts, _ = run.model.remove(max_start_ns=cutoff - 1)
    for k in ("states_before", "states_dropped", "ips_before", "ips_dropped", "arena_bytes_before", "arena_bytes_after"):
        assert a[k] == b[k] == counts[k], (k, a, b, counts)
    assert b["ips_found"] == 0
    assert preview["n_matched"] == b["states_dropped"] > 0 and b["ips_dropped"] > 0
    assert engine.state_export() == engine_b.state_export() == snapshot.build(*run.model.snapshot_args())
    sa, sb = engine.state_stats(), engine_b.state_stats()
    for k in sa:  # the expiry's sizing rule (rehashes is each engine's own history)
        assert k == "rehashes" or sa[k] == sb[k], (k, sa, sb)


def test_nothing_selected_leaves_the_engine_as_it_was():
    """Unknown IPs, a never-interned name, an empty window, a filter IP the
    list does not hold: no rebuild, on an engine whose arena has grown past its
    floor (a rebuild would shrink it, as the expiry does)."""
    eng = Engine(ip_arena_bytes=1 << 16)
    try:
        n = 30_000
        ips = ["172.%d.%d.%d" % (16 + (k >> 16), (k >> 8) & 255, k & 255) for k in range(n)]
        run = Run(H.one_rule(60, 100), eng)
        run.feed(H.lines([(k // 10, ip) for k, ip in enumerate(ips)]), T0_MS * 1_000_000)
        stats0, dump0 = eng.state_stats(), eng.state_dump()
        assert stats0["arena_capacity"] > 1 << 16
        for sel, found in (({"ips": ["9.9.9.9", "2001:db8::1", "", "172.16.0"]}, 0),
                           ({"name": "never-interned"}, 0),
                           ({"name": "never-interned", "ips": ips[:3]}, 3),
                           ({"min_start_ns": 5, "max_start_ns": 4}, 0),
                           ({"min_start_ns": 5, "max_start_ns": 4, "ips": ips[5:7] + ["9.9.9.9"] + ips[5:6]}, 2),
                           ({"ip": ips[0], "ips": ips[1:4]}, 3),
                           ({"ip": "9.9.9.9"}, 0),
                           ({"min_hits": 2}, 0),
                           ({"name": "r", "max_start_ns": T0_MS * 1_000_000 - 1, "ips": ips[::1000]}, 30)):
            s = eng.state_remove(**sel)
            assert (s["states_dropped"], s["ips_dropped"], s["ips_found"]) == (0, 0, found), (sel, s)
            assert (s["states_before"], s["ips_before"]) == (n, n)
            assert s["arena_bytes_after"] == s["arena_bytes_before"] == stats0["arena_bytes"]
            assert s["device_bytes_after"] == s["device_bytes_before"] == stats0["device_bytes"]
            st = eng.state_stats()
            for k in stats0:
                assert st[k] == stats0[k], (sel, k)
        assert eng.state_dump() == dump0
        run.compare_states(ips=ips[::997], dump=False)
        # and the engine goes on counting
        run.feed(H.lines([(3_000 + k, ip) for k, ip in enumerate(ips[::500])]), (T0_MS + 3_000) * 1_000_000)
        run.compare_states(ips=ips[::250], dump=False)
    finally:
        eng.close()


def test_everything_selected_equals_a_clear(engine, stream):
    run = Run(H.CFG, engine)
    for data, now in stream[:2]:
        run.feed(data, now)
    stats0 = engine.state_stats()
    s = engine.state_remove()
    assert (s["states_dropped"], s["ips_dropped"]) == (stats0["states"], stats0["ips"]) and s["arena_bytes_after"] == 0
    assert s["ips_found"] == 0
    st = engine.state_stats()
    assert engine.state_len() == 0 and engine.state_dump() == ""
    assert (st["ips"], st["states"], st["arena_bytes"]) == (0, 0, 0)
    assert st["rehashes"] == stats0["rehashes"]
    # ids restart at 0: the next batch equals the oracle on a fresh state
    data, now = stream[2]
    fresh = O.State()
    oflags, ores, oconsumed = fresh.consume(run.ocfg, data, now, cap=(H.PER + 1) * 5)
    compare_batch(oflags, ores, oconsumed, engine.process(run.rs, data, now, copy_results=True))
    assert engine.state_len() == len(fresh)
    for ip in POOL[:40] + POOL[-40:]:
        for n in run.names:
            assert engine.state_get(ip, n) == fresh.get(ip, n)


def test_forced_hash_collisions(engine):
    """Every IP on one of two hash values: two long probe chains, the listed
    IPs in their middle.  A listed IP comes back as a new IP, an unlisted one
    goes on counting; listed IPs that are not held but look like held ones (the
    same first 15 bytes and length, all but the last byte) drop nothing."""
    engine.debug_set_ip_hash_mask(0x2)
    try:
        run = Run(H.one_rule(), engine)
        ips = POOL[:40] + POOL[-40:]
        random.Random(9).shuffle(ips)
        middle = ips[20:60]
        stay = [ip for ip in ips if ip not in middle]
        long_stay = [ip for ip in stay if len(ip) > 15]
        short_stay = [ip for ip in stay if len(ip) <= 15]
        a, b = long_stay[0], long_stay[-1]
        near = [a[:-1] + ("0" if a[-1] != "0" else "1"),   # all but the last byte
                b[:15] + ("f" if b[15] != "f" else "e") + b[16:],  # the first 15 bytes (the whole key16) and the length
                a[:15], a + "0", short_stay[0] + "00", "0" + short_stay[1]]
        assert not set(near) & set(ips) and len(near[0]) == len(a) and len(near[1]) == len(b)
        ev = [(k, ip) for k, ip in enumerate(ips)]
        ev += [(500 + k, ip) for k, ip in enumerate(stay)]  # InsideInterval: 2 hits
        run.feed(H.lines(ev), T0_MS * 1_000_000)
        s, _ = run.remove(ips=near[:3] + middle + near[3:])
        assert (s["ips_dropped"], s["ips_found"], s["states_dropped"]) == (40, 40, 40)
        out = run.feed(H.lines([(1_000 + k, ip) for k, ip in enumerate(ips)]), (T0_MS + 1_000) * 1_000_000)
        for r, ip in zip(out.results, ips):
            assert (r.seen_ip, r.match_type) == ((0, 0) if ip in middle else (1, 2)), ip
        for ip in ips:
            assert engine.state_get(ip, "r")[0] == (1 if ip in middle else 3)
        run.compare_states(dump=False)
        # (IPs of one batch that share a 64-bit hash get their ids after the
        # batch's other new IPs, so the dump is compared without its order)
        assert sorted(engine.state_dump().split("\n\n")) == sorted(run.model.dump().split("\n\n"))
    finally:
        engine.debug_set_ip_hash_mask(0)


def test_list_sizes_and_scan_tiles(engine):
    """40,000 IPs with one state each; lists of 1, 64, 65, 257 and 13,001 IPs
    taken at stride through the ids that are left: one lane, a full wave, one
    more, past a block, many blocks -- and several tiles of the id scan."""
    n = 40_000
    ips = ["10.%d.%d.%d" % (k >> 16, (k >> 8) & 255, k & 255) if k % 5 else "2001:db8:aaaa:bbbb::%x:%x" % (k >> 8, k & 255)
           for k in range(n)]
    run = Run(H.one_rule(60, 100), engine)
    run.feed(H.lines([(j // 40, ip) for j, ip in enumerate(ips)]), T0_MS * 1_000_000)
    left = n
    for size in (1, 64, 65, 257, 13_001):
        cur = list(run.model.st)
        lst = cur[3::len(cur) // size][:size]
        assert len(lst) == size
        s, _ = run.remove(ips=lst)
        left -= size
        assert (s["ips_found"], s["ips_dropped"], s["states_dropped"]) == (size, size, size)
        assert engine.state_len() == left
        gone = set(lst)
        survivors = [ip for ip in cur[::991] + cur[-3:] + cur[:5] if ip not in gone]
        run.compare_states(ips=lst[::max(1, size // 40)] + survivors, dump=False)
    assert H.dump_ips(engine.state_dump()) == list(run.model.st)


def test_order_of_survivors_and_newcomers(engine):
    run = Run(H.one_rule(), engine)
    old = POOL[:30] + POOL[-30:]
    random.Random(5).shuffle(old)
    run.feed(H.lines([(k, ip) for k, ip in enumerate(old)]), T0_MS * 1_000_000)
    s, _ = run.remove(ips=old[1::2])
    assert s["ips_dropped"] == 30
    assert list(run.model.st) == old[::2]
    new = POOL[100:120] + old[1::4]  # unseen IPs and some of the removed, after the survivors
    run.feed(H.lines([(1_000 + k, ip) for k, ip in enumerate(new + old[:6:2])]), (T0_MS + 1_000) * 1_000_000)
    assert list(run.model.st) == old[::2] + new
    assert H.dump_ips(engine.state_dump()) == old[::2] + new
    run.compare_states()


def test_hot_key_and_slot_cache(engine, monkeypatch):
    """The first global rule matches every line (hot_name and the ip_st slot
    cache in use), one IP takes the long-run path.  Half of the quiet IPs go by
    list between two batches and the hot IP stays; then the hot IP goes by ip=."""
    monkeypatch.setenv("BJX_CHECK", "1")
    monkeypatch.setenv("BJX_SORT2", "1")
    engine.debug_set_slot_cache(1)
    try:
        run = Run(H.HOT_CFG, engine)
        run.feed(H.hot_lines(T0_MS, 30_000), T0_MS * 1_000_000)
        assert engine.scan_stats()["long_runs"] > 0
        quiet = H.hot_quiet_ips()
        s, _ = run.remove(ips=quiet[::2])
        assert s["ips_found"] == s["ips_dropped"] == len(quiet[::2]) == 30 and s["ips_dropped"] < s["ips_before"] - 1
        assert engine.state_get("6.6.6.6", "every") is not None
        run.compare_states(dump=True)
        run.feed(H.hot_lines(T0_MS + 30_000, 30_000), (T0_MS + 30_000) * 1_000_000)
        assert engine.scan_stats()["long_runs"] > 0
        run.compare_states(dump=True)
        s, _ = run.remove(ip="6.6.6.6")
        assert (s["ips_dropped"], s["states_dropped"], s["ips_found"]) == (1, 2, 0)
        assert engine.state_get("6.6.6.6", "every") is None
        run.feed(H.hot_lines(T0_MS + 60_000, 30_000), (T0_MS + 60_000) * 1_000_000)
        assert engine.scan_stats()["long_runs"] > 0
        run.compare_states(dump=True)
    finally:
        engine.debug_set_slot_cache(-1)


def test_growth_and_rollback_after_removal():
    """A small arena grows with the first batch and shrinks back with the
    removal; then new IPs arrive with a claim budget small enough to roll the
    first claim pass back."""
    eng = Engine(ip_arena_bytes=1 << 16)
    try:
        n = 30_000
        ips = ["172.%d.%d.%d" % (16 + (k >> 16), (k >> 8) & 255, k & 255) for k in range(n)]
        run = Run(H.one_rule(60, 100), eng)
        run.feed(H.lines([(k // 10, ip) for k, ip in enumerate(ips)]), T0_MS * 1_000_000)
        re0 = eng.state_stats()["rehashes"]
        s, _ = run.remove(ips=ips[:-1000])  # the last 1000 IPs stay
        assert s["ips_dropped"] == s["ips_found"] == n - 1000
        assert s["device_bytes_after"] < s["device_bytes_before"]
        st = eng.state_stats()
        assert st["rehashes"] == re0 and st["device_bytes"] == s["device_bytes_after"]
        eng.debug_set_claim_budget(64)
        new = ["192.168.%d.%d" % (k >> 8, k & 255) for k in range(5000)]
        run.feed(H.lines([(3_000 + k // 10, ip) for k, ip in enumerate(new + ips[-1500:])]), (T0_MS + 3_000) * 1_000_000)
        eng.debug_set_claim_budget(0)
        assert eng.state_len() == 1000 + 5000 + 500
        run.compare_states(ips=new[::97] + ips[-1500::53] + ips[:3], dump=False)
        assert eng.state_dump() == run.model.dump()
    finally:
        eng.close()


def test_refused_inside_an_open_batch(engine, stream):
    """Between bjx_match_batch and the bjx_finish_batch* that closes it the
    removal is BJX_ERR_ARG and touches nothing; the next whole batch closes it."""
    import torch
    run = Run(H.CFG, engine)
    data, now = stream[0]
    run.feed(data, now)
    before = engine.state_dump()
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    engine.match(run.rs, now, buf.data_ptr(), len(data))
    for sel in ({}, {"ips": POOL[:3]}, {"name": "mid"}):
        with pytest.raises(BanjaxGpuError) as ei:
            engine.state_remove(**sel)
        assert ei.value.code == -2
    assert engine.state_dump() == before
    data, now = stream[1]
    run.feed(data, now)
    run.remove(**H.selection(0, now))
    run.compare_states()


def test_bad_arguments_with_an_engine(engine):
    """The BJX_ERR_ARG cases that need a live handle: the message names the argument."""
    import ctypes as C
    from banjax_amd import _lib
    L = _lib.lib()
    f = _lib.StateFilter(_lib.Str(None, 0), _lib.Str(None, 0), INT64_MIN, INT64_MIN, INT64_MAX, 0, 0)
    assert L.bjx_state_remove(engine._h, None, None, 0, None) == _lib.ERR_ARG
    assert L.bjx_state_remove(engine._h, C.byref(f), None, 2, None) == _lib.ERR_ARG
    assert b"no list" in L.bjx_engine_last_error(engine._h)
    bad = (_lib.Str * 2)(_lib.Str(b"1.2.3.4", 7), _lib.Str(None, 5))
    assert L.bjx_state_remove(engine._h, C.byref(f), bad, 2, None) == _lib.ERR_ARG
    big = (_lib.Str * 2)(_lib.Str(b"1.2.3.4", 1 << 31), _lib.Str(b"1.2.3.4", 1 << 31))  # only the lengths are read
    assert L.bjx_state_remove(engine._h, C.byref(f), big, 2, None) == _lib.ERR_ARG
    assert b"2^32" in L.bjx_engine_last_error(engine._h)


def test_node_equals_single_engine(engine, stream):
    """Three engines on device 0: the same stream and selections through
    Node.state_remove give the single engine's results and summed stats."""
    _, single = H.parity_run(engine, stream)
    node = Node([0, 0, 0])
    try:
        _, sharded = H.parity_run(node, stream, compare_dump=False)
        for (a, _), (b, _) in zip(single, sharded):
            for k in COUNTS:
                assert a[k] == b[k], (k, a, b)
    finally:
        node.close()
