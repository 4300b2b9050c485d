"""Evicting the oldest state down to a budget on the device (bjx_state_trim,
include/banjax_gpu.h).

Expected values (tests/state_trim.py): banjax_amd.state_trim.trim -- the trim's
pure-Python model -- gives the cutoff, the bound, budget_met, the counts and the
survivors of a logical state, which is loaded by state_import of
snapshot.build(...).  The engine must equal the model on the stats of a dry run
and of the real call and, byte for byte, on the snapshot afterwards, which must
also be that of an engine that ran state_expire at the same cutoff.  Across
batches the Model of tests/test_gpu_state_expire.py replays the oracle's events
with expire(C) at the same boundaries.  tests/test_state_trim_cpu.py shows that
these inputs are telling."""
import ctypes as C

import pytest

from banjax_amd import Engine, Node, _lib, snapshot, state_trim
from banjax_amd._lib import BanjaxGpuError
from tests import state_remove as R
from tests import state_trim as H
from tests.state_trim import COUNTS, INT64_MAX, INT64_MIN
from tests.test_gpu_state_snapshot import _owner

pytestmark = pytest.mark.gpu
LOGICAL = ("ips", "states", "arena_bytes")


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
def case():
    """the sample, its snapshot, the 200 budgets and the model's stats for each (computed once)"""
    ips, states = H.sample()
    buds = H.budgets(states)
    return ips, states, snapshot.build(ips, states), buds, [state_trim.trim(ips, states, **b) for b in buds]


def _load(eng, blob):
    eng.state_clear()
    eng.state_import(blob)


def _check(got, want):
    assert {k: got[k] for k in COUNTS} == want, (got, want)


def test_dry_run_equals_the_model_and_changes_nothing(engine, case):
    ips, states, blob, buds, expected = case
    _load(engine, blob)
    stats0 = engine.state_stats()
    assert engine.state_export() == blob
    for bud, (_, _, want) in zip(buds, expected):
        got = engine.state_trim(dry_run=True, **bud)
        _check(got, want)
        assert got["device_bytes_after"] == got["device_bytes_before"] == stats0["device_bytes"]
        assert got["select_ms"] >= 0 and got["device_ms"] >= got["select_ms"]
        assert engine.state_stats() == stats0
        assert engine.state_export() == blob


def test_real_trim_equals_model_snapshot_and_expiry(engine, engine_b, case):
    ips, states, blob, buds, expected = case
    picked = H.real_subset([st for _, _, st in expected])
    assert {expected[k][2]["bound"] for k in picked} == {0, 1, 2, 3}
    for k in picked:
        kept_ips, kept, want = expected[k]
        _load(engine, blob)
        _load(engine_b, blob)
        stats0 = engine.state_stats()
        got = engine.state_trim(**buds[k])
        _check(got, want)
        after = engine.state_stats()
        assert after["rehashes"] == stats0["rehashes"] and got["device_bytes_after"] == after["device_bytes"]
        if not want["states_dropped"]:
            assert after == stats0  # no rebuild
        assert engine.state_export() == snapshot.build(kept_ips, kept)
        s = engine_b.state_expire(want["cutoff_ns"])
        assert engine_b.state_export() == snapshot.build(kept_ips, kept)
        assert (s["states_dropped"], s["ips_dropped"], s["arena_bytes_after"]) == \
            (want["states_dropped"], want["ips_dropped"], want["arena_bytes_after"])
        sb = engine_b.state_stats()
        for f in after:  # the expiry's sizing rule
            assert after[f] == sb[f], f
        # the budget holds (budget_met) and a second trim finds nothing to do
        if want["budget_met"]:
            assert not buds[k]["max_states"] or after["states"] <= buds[k]["max_states"]
            assert not buds[k]["max_ips"] or after["ips"] <= buds[k]["max_ips"]
        again = engine.state_trim(**buds[k])
        assert again["states_dropped"] == 0 and engine.state_stats() == after


@pytest.mark.parametrize("d", range(8))
def test_digit_positions(engine, d):
    """300 states whose starts differ only in byte d, a budget that cuts in the middle"""
    ips, states = H.flat_state(H.byte_starts(d))
    _load(engine, snapshot.build(ips, states))
    for bud in ({"max_states": 150}, {"max_ips": 77}):
        _check(engine.state_trim(dry_run=True, **bud), state_trim.trim(ips, states, **bud)[2])
    kept_ips, kept, want = state_trim.trim(ips, states, max_states=150)
    assert 100 < want["states_dropped"] < 200
    _check(engine.state_trim(max_states=150), want)
    assert engine.state_export() == snapshot.build(kept_ips, kept)


def test_all_equal_and_saturated(engine):
    ips, states = H.flat_state([H.T0 + 5] * 300, names=("a", "b", "c"))
    _load(engine, snapshot.build(ips, states))
    got = engine.state_trim(max_states=1)
    _check(got, state_trim.trim(ips, states, max_states=1)[2])
    assert (got["cutoff_ns"], got["states_dropped"], got["ips_dropped"], got["budget_met"]) == (H.T0 + 6, 300, 100, 1)
    assert engine.state_len() == 0 and engine.state_dump() == ""
    # two states at INT64_MAX and a budget of one: both stay
    ips, states = H.flat_state([INT64_MAX, 7, INT64_MAX, -3])
    _load(engine, snapshot.build(ips, states))
    kept_ips, kept, want = state_trim.trim(ips, states, max_states=1)
    got = engine.state_trim(max_states=1)
    _check(got, want)
    assert (got["cutoff_ns"], got["budget_met"], got["states_dropped"], got["bound"]) == (INT64_MAX, 0, 2, _lib.TRIM_BY_STATES)
    assert engine.state_export() == snapshot.build(kept_ips, kept) and engine.state_stats()["states"] == 2
    got = engine.state_trim(max_ips=1)
    assert (got["cutoff_ns"], got["budget_met"], got["states_dropped"], got["bound"]) == (INT64_MAX, 0, 0, _lib.TRIM_BY_IPS)


def test_exact_sizes_and_no_rebuild():
    """One state; then an arena that has grown past its floor (a rebuild would
    shrink it): a budget equal to what is held moves nothing, one below it drops
    the oldest tie group and rebuilds."""
    eng = Engine(ip_arena_bytes=1 << 16)
    try:
        ips, states = H.flat_state([H.T0])
        _load(eng, snapshot.build(ips, states))
        for bud in ({"max_states": 1}, {"max_ips": 1}, {"max_states": 1, "max_ips": 1, "floor_cutoff_ns": H.T0}):
            got = eng.state_trim(**bud)
            _check(got, state_trim.trim(ips, states, **bud)[2])
            assert got["states_dropped"] == 0 and eng.state_len() == 1
        got = eng.state_trim(floor_cutoff_ns=H.T0 + 1)
        assert (got["states_dropped"], got["bound"], eng.state_len()) == (1, _lib.TRIM_BY_FLOOR, 0)

        n = 30_000
        ips = ["172.%d.%d.%d" % (16 + (k >> 16), (k >> 8) & 255, k & 255) for k in range(n)]
        run = R.Run(R.one_rule(60, 100), eng)
        run.feed(R.lines([(k // 10, ip) for k, ip in enumerate(ips)]), R.T0_MS * 1_000_000)
        stats0, dump0 = eng.state_stats(), eng.state_dump()
        assert stats0["arena_capacity"] > 1 << 16 and stats0["states"] == n
        for bud in ({"max_states": n}, {"max_ips": n}, {"max_states": n, "max_ips": n + 5, "floor_cutoff_ns": R.T0_MS * 1_000_000},
                    {"max_states": n + 1}, {}):
            got = eng.state_trim(**bud)
            assert (got["states_dropped"], got["ips_dropped"], got["budget_met"]) == (0, 0, 1), (bud, got)
            assert got["device_bytes_after"] == got["device_bytes_before"] == stats0["device_bytes"]
            assert got["arena_bytes_after"] == got["arena_bytes_before"] == stats0["arena_bytes"]
            assert eng.state_stats() == stats0
        assert eng.state_dump() == dump0
        got = eng.state_trim(max_states=n - 1)  # ten IPs share the oldest millisecond
        assert (got["states_dropped"], got["ips_dropped"], got["cutoff_ns"]) == (10, 10, R.T0_MS * 1_000_000 + 1)
        assert got["device_bytes_after"] < got["device_bytes_before"]
        st = eng.state_stats()
        assert st["rehashes"] == stats0["rehashes"] and st["device_bytes"] == got["device_bytes_after"]
        run.model.remove(max_start_ns=got["cutoff_ns"] - 1)
        run.compare_states(ips=ips[:30] + ips[::997], dump=False)
        assert eng.state_dump() == run.model.dump()
    finally:
        eng.close()


def test_grid_stride_wraps(engine, case):
    """One block, and three, walk the whole state table and all the IPs."""
    ips, states, blob, buds, expected = case
    _load(engine, blob)
    try:
        for blocks in (1, 3):
            engine.debug_set_trim_grid(blocks)
            for k in H.real_subset([st for _, _, st in expected], per_bound=2):
                _check(engine.state_trim(dry_run=True, **buds[k]), expected[k][2])
    finally:
        engine.debug_set_trim_grid(0)


def test_forced_hash_collisions(engine, case):
    """Every IP on one of two hash values: the trim's rebuild re-inserts two long probe chains."""
    ips, states, blob, buds, expected = case
    engine.debug_set_ip_hash_mask(0x2)
    try:
        k = next(k for k in range(len(buds)) if expected[k][2]["bound"] == _lib.TRIM_BY_IPS and expected[k][2]["ips_dropped"] > 100)
        kept_ips, kept, want = expected[k]
        _load(engine, blob)
        _check(engine.state_trim(**buds[k]), want)
        assert engine.state_export() == snapshot.build(kept_ips, kept)
        for ip in ips[::23]:
            for n in H.NAMES:
                w = kept.get(ip.encode(), {}).get(n.encode())
                assert engine.state_get(ip, n) == w, (ip, n)
    finally:
        engine.debug_set_ip_hash_mask(0)
        engine.state_clear()


def test_after_a_batch_that_rolled_claims_back(engine):
    """The first claim pass of the batch is rolled back (claim budget) and run
    again, so the state table has held claimed slots without a state; the trim
    after it counts live states only, and the next batch goes on from the survivors."""
    run = H.Run(engine, R.one_rule(60, 100))
    ips = ["192.168.%d.%d" % (k >> 8, k & 255) for k in range(3000)]
    engine.debug_set_claim_budget(64)
    try:
        run.feed(R.lines([(k // 7, ip) for k, ip in enumerate(ips)]), R.T0_MS * 1_000_000)
    finally:
        engine.debug_set_claim_budget(0)
    want = run.trim(max_ips=1000, floor_cutoff_ns=R.T0_MS * 1_000_000)
    assert want["bound"] == _lib.TRIM_BY_IPS and 2000 <= want["ips_dropped"] < 2007 and want["states_dropped_live"] == want["states_dropped"]
    assert engine.state_dump() == run.model.dump()
    out = run.feed(R.lines([(1_000 + k, ip) for k, ip in enumerate(ips[::100] + ips[-5:])]), (R.T0_MS + 1_000) * 1_000_000)
    assert {r.seen_ip for r in out.results} == {0, 1}
    assert engine.state_dump() == run.model.dump()


def test_across_batches(engine, monkeypatch):
    """A trim at each batch boundary with a budget small enough to drop live
    states: every RuleResult, the trips and the dump equal the expiry test's
    Model with expire(C) at the same boundaries, the batches under BJX_CHECK=1."""
    monkeypatch.setenv("BJX_CHECK", "1")
    run, done = H.stream_run(engine)
    assert all(st["states_dropped_live"] > 0 for st in done)
    assert run.diff_first > 0 and run.diff_seen > 0
    assert engine.state_len() == len(run.model.st)
    for ip in H.POOL[::7]:
        for n in run.names:
            w = run.model.st.get(ip, {}).get(n)
            assert engine.state_get(ip, n) == (tuple(w) if w else None)


def test_refusals_leave_the_engine_usable(engine, case):
    import torch
    ips, states, blob, buds, expected = case
    L = _lib.lib()
    _load(engine, blob)
    out = _lib.TrimStats()
    assert L.bjx_state_trim(engine._h, None, C.byref(out)) == _lib.ERR_ARG
    assert b"no budget" in L.bjx_engine_last_error(engine._h)
    for flags in (2, 3, 1 << 31):
        bad = _lib.TrimBudget(10, 10, INT64_MIN, flags, 0)
        assert L.bjx_state_trim(engine._h, C.byref(bad), C.byref(out)) == _lib.ERR_ARG
        assert b"flag" in L.bjx_engine_last_error(engine._h)
    ok = _lib.TrimBudget(10, 10, INT64_MIN, _lib.TRIM_DRY_RUN, 0)
    assert L.bjx_state_trim(engine._h, C.byref(ok), None) == _lib.OK  # out may be NULL
    assert engine.state_export() == blob
    # inside an open batch
    run = H.Run(engine)
    data, now = H._stream()[0]
    run.feed(data, now)
    before = engine.state_dump()
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    engine.match(run.rs, now, buf.data_ptr(), len(data))
    for kw in ({"max_states": 5}, {"max_ips": 5, "dry_run": True}, {"floor_cutoff_ns": INT64_MAX}):
        with pytest.raises(BanjaxGpuError) as ei:
            engine.state_trim(**kw)
        assert ei.value.code == -2
    assert engine.state_dump() == before
    data, now = H._stream()[1]
    run.feed(data, now)  # the next whole batch closes the open one
    run.trim(max_states=200)
    assert engine.state_dump() == run.model.dump()


def test_limiter_bound_states(engine):
    """RegexRateLimiter.bound_states: the trim with the expiry's transparent cutoff as the floor."""
    from banjax_amd import Config, MockBanner, RegexRateLimiter
    from banjax_amd.regex_rate_limiter import expire_cutoff_ns
    cfg = Config.from_yaml(H.CFG)
    engine.state_clear()
    lim = RegexRateLimiter(cfg, engine=engine, banner=MockBanner())
    data, now = H._stream()[0]
    lim.consume_lines(data, now)
    ips, states = snapshot.parse(engine.state_export())
    n = len(H.all_starts(states))
    later = now + 100 * H.S
    floor = expire_cutoff_ns(later, cfg)
    assert min(H.all_starts(states)) < floor < max(H.all_starts(states))
    kept_ips, kept, want = state_trim.trim(ips, states, max_states=n // 2, floor_cutoff_ns=floor)
    assert 0 < want["states_dropped_live"] < want["states_dropped"]
    _check(lim.bound_states(later, max_states=n // 2, dry_run=True), want)
    _check(lim.bound_states(later, max_states=n // 2), want)
    assert engine.state_export() == snapshot.build(kept_ips, kept)
    assert lim.bound_states(later, max_states=n // 2)["states_dropped"] == 0


def test_node_trims_at_one_cutoff(case):
    """Three engines on device 0: the node's cutoff is the largest of the
    engines' own, every engine ends within the budget, the result is that of a
    node that expired at that cutoff, and the summed stats are the model's over
    the parts the owner function makes."""
    ips, states, blob, buds, expected = case
    node, node_b = Node([0, 0, 0]), Node([0, 0, 0])
    try:
        node.state_import(blob)
        node_b.state_import(blob)
        parts = [([ip for ip in ips if _owner(ip, 3) == k], {ip: states[ip] for ip in ips if _owner(ip, 3) == k})
                 for k in range(3)]
        for k in range(3):
            assert node.engine(k).state_export() == snapshot.build(*parts[k])
        bud = {"max_states": 300, "max_ips": 130, "floor_cutoff_ns": -(1 << 61)}
        survivors, want = state_trim.node_trim(parts, **bud)
        own = [node.engine(k).state_trim(dry_run=True, **bud) for k in range(3)]
        assert len({s["cutoff_ns"] for s in own}) > 1  # the engines disagree: the node has to choose
        dry = node.state_trim(dry_run=True, **bud)
        _check(dry, want)
        assert dry["cutoff_ns"] == max(s["cutoff_ns"] for s in own)
        assert dry["bound"] == next(s["bound"] for s in own if s["cutoff_ns"] == dry["cutoff_ns"])
        assert dry["device_bytes_after"] == dry["device_bytes_before"] and node.state_export() == node_b.state_export()
        got = node.state_trim(**bud)
        _check(got, want)
        for k in range(3):
            st = node.engine(k).state_stats()
            assert st["states"] <= 300 and st["ips"] <= 130
            assert node.engine(k).state_export() == snapshot.build(*survivors[k])
        node_b.state_expire(want["cutoff_ns"])
        assert node.state_export() == node_b.state_export()
        assert node.state_trim(**bud)["states_dropped"] == 0  # idempotent
        with pytest.raises(BanjaxGpuError) as ei:
            bad = _lib.TrimBudget(1, 1, INT64_MIN, 4, 0)
            node._check(_lib.lib().bjx_node_state_trim(node._h, C.byref(bad), None), "node_state_trim")
        assert ei.value.code == -2
    finally:
        node.close()
        node_b.close()
