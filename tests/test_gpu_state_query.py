"""bjx_state_query / bjx_node_state_query (include/banjax_gpu.h): top-K, counts
and Get(ip) over the state in HBM.

States are loaded with snapshot.build + state_import, so hits and starts are
arbitrary, or computed by batches that the oracle checks (Run, from the
snapshot tests).  The expected answer is always banjax_amd/state_query.select
on the same structures, never the engine."""
import random

import pytest

from banjax_amd import Config, Engine, MockBanner, Node, RegexRateLimiter, _lib, snapshot, state_query
from banjax_amd._lib import BanjaxGpuError
from tests.test_gpu_state_snapshot import (CFG, CFG_OTHER_ORDER, Run, _dump_ips, _engine_major, _lines, _one_rule,
                                           _other_name_order, _stream)

pytestmark = pytest.mark.gpu
S = 1_000_000_000
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
T0_MS = 1_700_000_000_000
T0 = T0_MS * 1_000_000
BY_HITS, BY_START = state_query.BY_HITS, state_query.BY_START
NAMES = ("mid", "fast", "slow", "a", "ab", "")


@pytest.fixture(scope="module")
def engine():
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def stream():
    return _stream()


def _load(eng, ips, states):
    eng.state_clear()
    got = eng.state_import(snapshot.build(ips, states))
    assert got["states"] == sum(len(d) for d in states.values())


def _ask(t, **flt):
    a = t.state_query(**flt)
    assert a["device_ms"] >= 0
    return a["n_matched"], a["n_ips_matched"], a["rows"]


def _same(t, ips, states, **flt):
    want = state_query.select(ips, states, **flt)
    got = _ask(t, **flt)
    assert got[:2] == want[:2], (flt, got[:2], want[:2])
    assert got[2] == want[2], (flt, [k for k, (a, b) in enumerate(zip(got[2], want[2])) if a != b][:3])
    return want


def _sample(seed, n_ips, names=NAMES, hits=5, band=10):
    rng = random.Random(seed)
    ips = ["10.%d.%d.%d" % (seed, k >> 8, k & 255) if k % 3 else "2001:db8:85a3:%x:0:8a2e:370:%x" % (seed, k)
           for k in range(n_ips)]
    rng.shuffle(ips)
    states = {}
    for ip in ips:
        use = rng.sample(list(names), rng.randrange(1, len(names) + 1))
        states[ip] = {n: (rng.randrange(0, hits), T0 + rng.randrange(0, band)) for n in use}
    return ips, states


def test_parity_sweep(engine):
    """300 IPs, 1 to 6 names each, hits 0..4, starts in a band of 10 ns: every
    combination of name filter, min_hits, start window, order and limit."""
    ips, states = _sample(1, 300)
    _load(engine, ips, states)
    n_q = 0
    for name in (None, "mid"):
        for min_hits in (INT64_MIN, 2):
            for lo, hi in ((INT64_MIN, INT64_MAX), (T0 + 3, T0 + 6)):
                flt = dict(name=name, min_hits=min_hits, min_start_ns=lo, max_start_ns=hi)
                n = state_query.select(ips, states, **flt)[0]
                assert n > 30  # every combination leaves something to rank
                for order in (BY_HITS, BY_START):
                    for limit in (0, 1, 2, 63, 64, 65, 255, 256, 257, n - 1, n, n + 1, 65536):
                        want = _same(engine, ips, states, order=order, limit=limit, **flt)
                        assert len(want[2]) == min(limit, n)
                        n_q += 1
    assert n_q == 2 * 2 * 2 * 2 * 13


def test_tie_selection():
    """Equal primaries: the radix select has to go on into the tie word."""
    eng = Engine()
    try:
        # names interned zz_unrelated, slow, mid, fast: ids in no sorted order
        _other_name_order(eng)
        names = ("fast", "mid", "slow", "zz_unrelated")
        # 5,000 states all with equal hits: the first 100 in (IP first-seen, name) order
        ips = ["10.9.%d.%d" % (k >> 8, k & 255) for k in range(1250)]
        random.Random(4).shuffle(ips)
        states = {ip: {n: (3, T0 + k) for n in names} for k, ip in enumerate(ips)}
        _load(eng, ips, states)
        want = _same(eng, ips, states, limit=100)
        assert want[0] == 5000 and want[2] == [(ips[k // 4].encode(), names[k % 4].encode(), 3, T0 + k // 4) for k in range(100)]
        _same(eng, ips, states, limit=100, name="mid")
        _same(eng, ips, states, limit=4097)
        # the group tied at the threshold straddles the limit, with larger values above it
        rng = random.Random(5)
        flat = [(ip, n) for ip in ips for n in names]
        rng.shuffle(flat)
        states = {ip: {} for ip in ips}
        for k, (ip, n) in enumerate(flat):
            states[ip][n] = (9 if k < 40 else 5 if k < 3040 else 1, T0 + (7 if k < 3040 else k))
        _load(eng, ips, states)
        for order in (BY_HITS, BY_START):
            for limit in (39, 40, 41, 100, 3039, 3040, 3041):
                want = _same(eng, ips, states, order=order, limit=limit)
        assert [r[2] for r in _ask(eng, limit=100)[2]] == [9] * 40 + [5] * 60
        # equal primaries whose ties differ only in the name rank: one IP's states
        few = ips[:3]
        states = {ip: {n: (2, T0) for n in names} for ip in few}
        _load(eng, few, states)
        for limit in (1, 2, 3, 4, 5, 12):
            want = _same(eng, few, states, limit=limit)
        assert [r[1] for r in want[2][:4]] == [b"fast", b"mid", b"slow", b"zz_unrelated"]
    finally:
        eng.close()


def test_key_transform(engine):
    """hits and starts that are negative, zero and at both int64 ends, both
    orders.  state_import refuses none of them (it checks the snapshot's form,
    not the values), so the whole range is here."""
    vals = [INT64_MIN, INT64_MIN + 1, -(1 << 40), -1, 0, 1, 1 << 40, INT64_MAX - 1, INT64_MAX]
    ips, states = [], {}
    for a, h in enumerate(vals):
        ip = "10.7.0.%d" % a
        ips.append(ip)
        states[ip] = {"n%d" % b: (h, s) for b, s in enumerate(vals)}
    random.Random(6).shuffle(ips)
    _load(engine, ips, states)
    n = len(vals) ** 2
    for order in (BY_HITS, BY_START):
        for limit in (0, 1, 9, 10, n - 1, n, 65536):
            _same(engine, ips, states, order=order, limit=limit)
        for v in vals:
            _same(engine, ips, states, order=order, limit=n, min_hits=v)
            _same(engine, ips, states, order=order, limit=n, min_start_ns=v)
            _same(engine, ips, states, order=order, limit=n, max_start_ns=v)
    want = _same(engine, ips, states, order=BY_START, limit=n)
    assert [r[3] for r in want[2][:9]] == [INT64_MAX] * 9 and [r[3] for r in want[2][-9:]] == [INT64_MIN] * 9


def _forty_thousand():
    n = 40_000
    ips = ["10.%d.%d.%d" % (k >> 16, (k >> 8) & 255, k & 255) if k % 5 else "2001:db8:aaaa:bbbb::%x:%x" % (k >> 8, k & 255)
           for k in range(n)]
    rng = random.Random(3)
    rng.shuffle(ips)
    return ips, {ip: {"r": (rng.randrange(0, 1000), T0 + rng.randrange(0, 10 ** 9))} for ip in ips}


@pytest.mark.parametrize("small", [False, True])
def test_several_blocks_and_partial_tiles(engine, small):
    """40,000 IPs with one state each: several blocks of every pass and a
    partial one; on a default engine and on one created with small capacities
    (which the engine raises to its floor of 2^22 slots; the import sizes the
    tables itself)."""
    ips, states = _forty_thousand()
    eng = Engine(ip_capacity=1024, state_capacity=1024, ip_arena_bytes=4096) if small else engine
    try:
        _load(eng, ips, states)
        assert eng.state_stats()["states"] == len(ips)
        for order in (BY_HITS, BY_START):
            for limit in (1, 4096, 65536):
                _same(eng, ips, states, order=order, limit=limit)
        _same(eng, ips, states, limit=4096, min_hits=500, max_start_ns=T0 + 5 * 10 ** 8)
        _same(eng, ips, states, limit=0, min_hits=990)
    finally:
        if small:
            eng.close()


IP_SHAPES = ["", "7", "a1", "1.2", "123.123.123.123", "2001:db8::12:345", "2001:db8::123:456", "f" * 300,
             # neighbours that differ only past byte 15 / in the last byte
             "2001:db8::12:346", "2001:db8::123:457", "f" * 299 + "e", "123.123.123.124"]


@pytest.mark.parametrize("mask", [0, 0x2])
def test_get_ip(mask):
    """Get(ip): IPs of 0, 1, 2, 3, 15, 16, 17 and 300 bytes and their
    neighbours, several names each; with mask 0x2 every IP sits in one of two
    probe chains."""
    assert [len(x) for x in IP_SHAPES[:8]] == [0, 1, 2, 3, 15, 16, 17, 300]
    rng = random.Random(8)
    states = {ip: {n: (rng.randrange(0, 4), T0 + rng.randrange(0, 5)) for n in rng.sample(NAMES, 4)} for ip in IP_SHAPES}
    eng = Engine()
    try:
        eng.debug_set_ip_hash_mask(mask)
        _load(eng, IP_SHAPES, states)
        for ip in IP_SHAPES:
            for order in (BY_HITS, BY_START):
                want = _same(eng, IP_SHAPES, states, ip=ip, order=order, limit=100)
                assert want[0] == 4 and want[1] == 1
            _same(eng, IP_SHAPES, states, ip=ip, limit=2)
            _same(eng, IP_SHAPES, states, ip=ip, limit=0, min_hits=2)
            for name in NAMES:
                want = _same(eng, IP_SHAPES, states, ip=ip, name=name, limit=5)
                assert want[0] == (1 if name in states[ip] else 0)
        for unknown in ("9.9.9.9", "f" * 298, "2001:db8::12:347", "123.123.123.12"):
            assert _ask(eng, ip=unknown, limit=10) == (0, 0, [])
        assert _ask(eng, ip=IP_SHAPES[4], name="never interned", limit=10) == (0, 0, [])
        assert _ask(eng, name="never interned", limit=10) == (0, 0, [])
    finally:
        eng.debug_set_ip_hash_mask(0)
        eng.close()


def test_get_all_returns_a_state_whose_name_left_the_ruleset():
    """RegexRateLimitStates.get_all is the reference's whole-map Get: a state
    kept under a rule name that a reload removed (and the process restarted
    from a snapshot since) is returned; get(), which asks name by name for the
    names its limiter has seen, does not return it."""
    eng = Engine()
    try:
        lim = RegexRateLimiter(Config.from_yaml(_one_rule()), engine=eng, banner=MockBanner())
        eng.state_import(snapshot.build(["1.2.3.4", "5.6.7.8"], {"1.2.3.4": {"r": (2, T0), "gone": (7, T0 - S)},
                                                                  "5.6.7.8": {"gone": (1, T0)}}))
        assert lim.states.get("1.2.3.4") == {"r": (2, T0)}
        assert lim.states.get_all("1.2.3.4") == {"r": (2, T0), "gone": (7, T0 - S)}
        assert lim.states.get("5.6.7.8") is None and lim.states.get_all("5.6.7.8") == {"gone": (1, T0)}
        assert lim.states.get_all("9.9.9.9") is None
    finally:
        eng.close()


def _model_states(run):
    return list(run.model.st), {ip: {n: tuple(s) for n, s in d.items()} for ip, d in run.model.st.items()}


QUERIES = [dict(limit=0), dict(limit=10), dict(limit=65536, order=BY_START), dict(name="mid", limit=50),
           dict(min_hits=2, limit=300), dict(ip="10.1.0.3", limit=10), dict(name="slow", order=BY_START, limit=7)]


def test_engine_unchanged(engine, stream):
    """state_export, the dump and the stats are equal before and after a
    series of queries, and the next batch is bit-exact against the oracle."""
    run = Run(CFG, engine)
    for data, now in stream[:2]:
        run.feed(data, now)
    blob, dump, stats = engine.state_export(), engine.state_dump(), engine.state_stats()
    ips, states = _model_states(run)
    for q in QUERIES:
        _same(engine, ips, states, **q)
    for bad in (dict(limit=65537), dict(order=2)):
        with pytest.raises(BanjaxGpuError):
            engine.state_query(**bad)
    assert engine.state_export() == blob == run.oracle_blob()
    assert engine.state_dump() == dump and engine.state_stats() == stats
    data, now = stream[2]
    run.feed(data, now)  # RuleResults, line flags and trips against the oracle
    run.compare_states()
    assert engine.state_export() == run.oracle_blob()
    ips, states = _model_states(run)
    for q in QUERIES:
        _same(engine, ips, states, **q)


def test_after_the_tables_move(stream):
    """The query equals the model after an expiry, after a clear and re-import,
    and after both tables grew; the count-only preview of a cutoff equals the
    states_dropped of the expiry that follows."""
    eng = Engine(ip_capacity=1024, state_capacity=1024, ip_arena_bytes=4096)
    try:
        run = Run(CFG, eng)
        for data, now in stream[:2]:
            run.feed(data, now)
        ips, states = _model_states(run)
        for q in QUERIES:
            _same(eng, ips, states, **q)
        cutoff = stream[1][1] + 45 * S
        preview = _same(eng, ips, states, max_start_ns=cutoff - 1, limit=0)
        got = eng.state_expire(cutoff)
        ds, di, partial = run.model.expire(cutoff)
        assert preview[0] == got["states_dropped"] == ds > 0 and got["ips_dropped"] == di
        ips, states = _model_states(run)
        for q in QUERIES:
            _same(eng, ips, states, **q)
        blob = eng.state_export()
        eng.state_clear()
        assert _ask(eng, limit=10) == (0, 0, [])
        eng.state_import(blob)
        for q in QUERIES:
            _same(eng, ips, states, **q)
        # batches of new IPs on top (the oracle checks them): ids and slots past the imported ones
        run2 = Run(_one_rule(60, 100), eng)
        new = ["10.%d.%d.%d" % (50 + (k >> 16), (k >> 8) & 255, k & 255) for k in range(6000)]
        random.Random(12).shuffle(new)
        for b in range(2):
            part = new[b * 3000:(b + 1) * 3000]
            run2.feed(_lines([(b * 1000 + j // 10, ip) for j, ip in enumerate(part + part[:500])]), (T0_MS + b * 1000) * 1_000_000)
        ips, states = _model_states(run2)
        for q in (dict(limit=0), dict(limit=100), dict(limit=65536, order=BY_START), dict(min_hits=2, limit=1000),
                  dict(ip=new[10], limit=5)):
            _same(eng, ips, states, **q)
    finally:
        eng.close()


def test_after_growth_of_both_tables():
    """Both tables are created with 2^22 slots whatever capacity is asked for,
    so only millions of IPs make them grow: 3.3M new IPs in two batches, one
    line and so one state {1, line time} each (rule r: 100 hits per 60 s).
    The model is evaluated on the states that can pass the filter -- the last
    5,000 IPs for a start window that begins at their first timestamp, one IP
    for Get(ip) -- in their first-seen order; states outside a filter do not
    reach its answer."""
    from banjax_amd import Ruleset
    n, per = 3_300_000, 1_650_000
    eng = Engine()
    try:
        rs = Ruleset(Config.from_yaml(_one_rule(60, 100)))

        def ts(k):
            t = T0_MS + k // 1000
            return "%d.%03d" % (t // 1000, t % 1000)

        def ip(k):
            return "11.%d.%d.%d" % (k >> 16, (k >> 8) & 255, k & 255)

        for b in range(2):
            data = "".join(["%s %s GET h.com GET /x HTTP/1.1 ua\n" % (ts(k), ip(k)) for k in range(b * per, (b + 1) * per)])
            out = eng.process(rs, data.encode(), T0)
            assert out.n_lines == per
        st = eng.state_stats()
        assert st["ips"] == st["states"] == n and st["ip_slots"] > 1 << 22 and st["state_slots"] > 1 << 22 and st["rehashes"] >= 2
        assert _ask(eng, limit=0)[:2] == (n, n)
        tail = list(range(n - 5000, n))
        ips = [ip(k) for k in tail]
        states = {ip(k): {"r": (1, int(float(ts(k)) * 1e9))} for k in tail}
        cut = states[ips[0]]["r"][1]
        assert cut > int(float(ts(n - 5001)) * 1e9)
        for order in (BY_HITS, BY_START):
            for limit in (0, 1, 100, 4999, 5000, 65536):
                _same(eng, ips, states, min_start_ns=cut, order=order, limit=limit)
        _same(eng, ips, states, min_start_ns=cut, max_start_ns=states[ips[2500]]["r"][1], limit=3000)
        # every state has hits 1, so by hits the order is first-seen order: the
        # rows (not the counts) are the model's over the first 100 IPs
        head = {ip(k): {"r": (1, int(float(ts(k)) * 1e9))} for k in range(100)}
        assert _ask(eng, limit=100)[2] == state_query.select([ip(k) for k in range(100)], head, limit=100)[2]
        for k in (0, 5, per - 1, per, n - 1):
            one = {ip(k): {"r": (1, int(float(ts(k)) * 1e9))}}
            _same(eng, [ip(k)], one, ip=ip(k), limit=5)
    finally:
        eng.close()


def test_refusals(engine, stream):
    import torch
    ips, states = _sample(2, 50)
    _load(engine, ips, states)
    for bad in (dict(limit=65537), dict(order=2), dict(order=0xFFFFFFFF)):
        with pytest.raises(BanjaxGpuError) as ei:
            engine.state_query(**bad)
        assert ei.value.code == _lib.ERR_ARG
    assert len(_ask(engine, limit=65536)[2]) == sum(len(d) for d in states.values())
    # min_start_ns > max_start_ns: zero rows, rc 0
    assert _ask(engine, min_start_ns=T0 + 5, max_start_ns=T0 + 4, limit=10) == (0, 0, [])
    # between match_batch and finish_batch: refused, nothing touched; the next whole batch closes it
    run = Run(CFG)
    data, now = stream[0]
    small = b"\n".join(data.split(b"\n")[:400]) + b"\n"
    buf = torch.frombuffer(bytearray(small), dtype=torch.uint8).to("cuda:0")
    engine.match(run.rs, now, buf.data_ptr(), len(small))
    with pytest.raises(BanjaxGpuError) as ei:
        engine.state_query(limit=1)
    assert ei.value.code == _lib.ERR_ARG and "between" in str(ei.value)
    engine.process(run.rs, small, now)
    assert _ask(engine, limit=0)[0] >= sum(len(d) for d in states.values())
    # an empty engine gives zeros
    engine.state_clear()
    for q in (dict(limit=0), dict(limit=10), dict(ip="1.2.3.4", limit=10), dict(name="mid", limit=10)):
        assert _ask(engine, **q) == (0, 0, [])


def test_node():
    """Three engines on device 0: rows and counts equal the model evaluated
    with the IPs in the node's dump order (engine-major)."""
    ips, states = _sample(3, 240, hits=3, band=4)
    node = Node([0, 0, 0])
    try:
        node.state_import(snapshot.build(ips, states))
        order = _dump_ips(node.state_dump())
        assert order == _engine_major(ips, 3) and sorted(order) == sorted(ips)
        for by in (BY_HITS, BY_START):
            for limit in (0, 1, 17, 300, 65536):
                _same(node, order, states, order=by, limit=limit)
                _same(node, order, states, order=by, limit=limit, name="ab", min_hits=1)
            for ip in (ips[0], ips[1], ips[77], order[0], order[-1]):
                want = _same(node, order, states, ip=ip, order=by, limit=10)
                assert want[0] == len(states[ip])
            assert _ask(node, ip="9.9.9.9", order=by, limit=10) == (0, 0, [])
        for bad in (dict(limit=65537), dict(order=2)):
            with pytest.raises(BanjaxGpuError) as ei:
                node.state_query(**bad)
            assert ei.value.code == _lib.ERR_ARG
    finally:
        node.close()
