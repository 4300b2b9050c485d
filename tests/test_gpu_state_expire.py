"""Explicit expiry of stale rate-limit state (bjx_state_expire, include/banjax_gpu.h).

Expected values: the oracle says which (line, rule) pairs are events (its
RuleResults with skip_host == 0, in reference order); a Python restatement of
RegexRateLimitStates.Apply (reference internal/rate_limit.go:37-78) plus "drop
every state whose start < cutoff, and every IP left without one" replays them,
with an expiry at the same batch boundaries as the engine.  The engine must
equal that model on every RuleResult, on the trips, on state_get and on the
state dump (IPs in first-seen order)."""
import random

import pytest

from oracle import oracle as O

import workloads as W
from banjax_amd import Config, Engine, MockBanner, Node, RegexRateLimiter, Ruleset
from banjax_amd._lib import BanjaxGpuError
from tests.parity import compare_batch, oracle_config

pytestmark = pytest.mark.gpu
S = 1_000_000_000
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
T0_MS = 1_700_000_000_000


class Model:
    """RegexRateLimitStates with expiry: {ip: {rule name: [NumHits, IntervalStartTime ns]}},
    both levels in insertion order."""

    def __init__(self):
        self.st = {}

    def apply(self, ip, rule, t):
        """Apply, rate_limit.go:37-78 -> (seenIp, MatchType, Exceeded)."""
        states = self.st.get(ip)
        if states is None:                                  # :48-51
            seen, mt = 0, 0
            state = [1, t]
            self.st[ip] = {rule.rule: state}
        else:
            seen = 1
            state = states.get(rule.rule)
            if state is not None:
                if t - state[1] > rule.interval:            # :56-58 OutsideInterval
                    mt = 1
                    state[0], state[1] = 1, t
                else:                                       # :59-61 InsideInterval
                    mt = 2
                    state[0] += 1
            else:                                           # :63-66 FirstTime
                mt = 0
                state = [1, t]
                states[rule.rule] = state
        if state[0] > rule.hits_per_interval:               # :70-72
            state[0] = 0
            return seen, mt, 1
        return seen, mt, 0

    def expire(self, cutoff):
        """-> (states dropped, IPs dropped, IPs that lost some but not all states)"""
        ds = di = partial = 0
        for ip in list(self.st):
            keep = {n: s for n, s in self.st[ip].items() if s[1] >= cutoff}
            ds += len(self.st[ip]) - len(keep)
            if not keep:
                di += 1
                del self.st[ip]
            else:
                partial += len(keep) != len(self.st[ip])
                self.st[ip] = keep  # (the IP keeps its place)
        return ds, di, partial

    def n_states(self):
        return sum(len(d) for d in self.st.values())

    def dump(self):
        """bjx_state_dump's text: IPs in first-seen order, rule names sorted."""
        out = []
        for ip, d in self.st.items():
            out.append(ip + ":\n")
            for n in sorted(d):
                out.append("\t%s:\n\t\t{%d %d}\n" % (n, d[n][0], d[n][1]))
            out.append("\n")
        return "".join(out)


class Run:
    """One config over an engine (or node), the oracle and the model."""

    def __init__(self, cfg_yaml, target):
        self.cfg = Config.from_yaml(cfg_yaml)
        self.rules = self.cfg.all_rules()
        self.names = sorted(set(r.rule for r in self.rules))
        self.rs = Ruleset(self.cfg)
        self.ocfg = oracle_config(self.cfg)
        self.ost = O.State()
        self.model = Model()
        self.t = target
        self.t.state_clear()
        self.diff_first = self.diff_seen = 0  # events the model answers differently from the never-expiring oracle

    def expected(self, data, now_ns):
        """(oracle results, the model's (line, rule, seen, match type, exceeded) per result)"""
        lines = data.split(b"\n")
        _, ores, _ = self.ost.consume(self.ocfg, data, now_ns, cap=(len(lines) + 1) * (len(self.rules) + 1))
        want = []
        for o in ores:
            if o.skip_host:
                want.append((o.line_idx, o.rule_id, o.seen_ip, o.match_type, o.exceeded))
                continue
            f = lines[o.line_idx].split(b" ", 2)
            seen, mt, ex = self.model.apply(f[1].decode(), self.rules[o.rule_id], int(float(f[0]) * 1e9))
            self.diff_first += mt == 0 and o.match_type != 0 and seen == 1
            self.diff_seen += seen == 0 and o.seen_ip == 1
            want.append((o.line_idx, o.rule_id, seen, mt, ex))
        return ores, want

    def feed(self, data, now_ns):
        _, want = self.expected(data, now_ns)
        out = self.t.process(self.rs, data, now_ns, copy_results=True)
        got = [(r.line_idx, r.rule_idx, r.seen_ip, r.match_type, r.exceeded) for r in out.results]
        if got != want:
            bad = next(k for k in range(min(len(got), len(want))) if got[k] != want[k]) if len(got) == len(want) else -1
            raise AssertionError("RuleResults differ (%d vs %d), first at %d: engine %s model %s"
                                 % (len(got), len(want), bad, got[bad] if bad >= 0 else None, want[bad] if bad >= 0 else None))
        assert [(t.line_idx, t.rule_idx) for t in out.trips] == [(w[0], w[1]) for w in want if w[4]]
        return out

    def expire(self, cutoff):
        """expiry on both sides; the engine's stats must be the model's counts"""
        ips0, st0 = len(self.model.st), self.model.n_states()
        ds, di, partial = self.model.expire(cutoff)
        s = self.t.state_expire(cutoff)
        assert (s["states_before"], s["states_dropped"], s["ips_before"], s["ips_dropped"]) == (st0, ds, ips0, di), s
        assert s["arena_bytes_after"] == sum(len(ip) for ip in self.model.st)
        assert s["device_bytes_after"] <= s["device_bytes_before"]
        return s, partial

    def compare_states(self, ips=None, dump=True):
        assert self.t.state_len() == len(self.model.st)
        for ip in (self.model.st if ips is None else ips):
            for n in self.names:
                want = self.model.st.get(ip, {}).get(n)
                got = self.t.state_get(ip, n)
                assert got == (tuple(want) if want else None), (ip, n, got, want)
        if dump:
            assert self.t.state_dump() == self.model.dump()


CFG = """
regexes_with_rates:
  - {rule: "fast", regex: 'GET', interval: 1, hits_per_interval: 0, decision: challenge}
  - {rule: "mid", regex: 'POST', interval: 5, hits_per_interval: 2, decision: nginx_block}
  - {rule: "slow", regex: '/login', interval: 60, hits_per_interval: 10, decision: iptables_block}
per_site_regexes_with_rates:
  site.com:
    - {rule: "mid", regex: '/api', interval: 5, hits_per_interval: 2, decision: challenge}
expiring_decision_ttl_seconds: 10
"""
N_BATCH, PER, STEP_MS = 4, 5000, 20  # 4 batches of 100 s
# dotted IPv4 (<= 15 bytes: the inline key16 compare) and full IPv6 text (the arena compare)
POOL = ["10.1.%d.%d" % (k >> 8, k & 255) for k in range(200)] + \
       ["2001:db8:85a3:%x:0:8a2e:370:%x" % (k, 0x7000 + k) for k in range(100)]


def _stream():
    """Rising timestamps; a third of the IPs send throughout, a third only in
    the first 35% of every batch, a third only in batches 0 and 2."""
    rng = random.Random(20240611)
    always, early, alt = POOL[0::3], POOL[1::3], POOL[2::3]
    batches = []
    for b in range(N_BATCH):
        out = []
        for k in range(PER):
            t = T0_MS + (b * PER + k) * STEP_MS
            pool = always + (early if k < PER * 35 // 100 else []) + (alt if b % 2 == 0 else [])
            m = rng.choice(("GET", "POST", "HEAD"))
            out.append("%d.%03d %s %s %s %s %s HTTP/1.1 ua" % (t // 1000, t % 1000, rng.choice(pool), m,
                                                               rng.choice(("site.com", "h.com")), m,
                                                               rng.choice(("/login", "/api/x", "/x"))))
        batches.append((("\n".join(out) + "\n").encode(), (T0_MS + b * PER * STEP_MS) * 1_000_000))
    return batches


@pytest.fixture(scope="module")
def stream():
    return _stream()


@pytest.fixture(scope="module")
def engine():
    e = Engine()
    yield e
    e.close()


def _mid_cutoff(now_ns):
    """inside the batch that started at now_ns: states last started in its first 45 s die"""
    return now_ns + 45 * S


def _parity_run(target, stream):
    run = Run(CFG, target)
    stats = []
    for b, (data, now) in enumerate(stream):
        run.feed(data, now)
        if b < N_BATCH - 1:
            s, partial = run.expire(_mid_cutoff(now))
            stats.append(s)
            # some states die, some survive; some IPs lose everything, some a part
            assert s["states_dropped"] > 0 and s["states_dropped"] < s["states_before"]
            assert s["ips_dropped"] > 0 and partial > 0
            run.compare_states(dump=not isinstance(target, Node))
    # the input really met both situations: a dropped rule of a known IP came
    # back FirstTime with seen_ip 1, a fully dropped IP came back with seen_ip 0
    assert run.diff_first > 0 and run.diff_seen > 0
    run.compare_states(dump=not isinstance(target, Node))
    return run, stats


def test_model_parity_arbitrary_cutoffs(engine, stream):
    _parity_run(engine, stream)


def test_trip_transparency(engine, stream):
    """RegexRateLimiter.expire_states after every batch: trips, decision lists
    and ban log equal the oracle's run that never expires.  RuleResults differ
    only where a dropped state's OutsideInterval reads FirstTime, and in
    seen_ip (1 -> 0) of the first event of an IP that lost every state: that
    event is FirstTime on the engine, and OutsideInterval on the oracle, or
    FirstTime there too when it is the IP's first event of that rule."""
    cfg = Config.from_yaml(CFG)
    ocfg, ost = oracle_config(cfg), O.State()
    engine.state_clear()
    lim = RegexRateLimiter(cfg, engine=engine, banner=MockBanner())
    dropped = changed = 0
    for data, now in stream:
        oflags, ores, oconsumed = ost.consume(ocfg, data, now, cap=(PER + 1) * 5)
        _, out = lim.consume_lines(data, now)
        assert out.consumed_bytes == oconsumed and list(out.line_flags) == oflags and out.n_results == len(ores)
        for g, o in zip(out.results, ores):
            assert (g.line_idx, g.rule_idx, g.rule_pos, g.skip_host, g.exceeded) == \
                (o.line_idx, o.rule_id, o.rule_pos, o.skip_host, o.exceeded)
            if g.match_type != o.match_type:
                changed += 1
                assert o.match_type == 1 and g.match_type == 0 and g.seen_ip <= o.seen_ip, (g.line_idx, g.rule_idx)
            elif g.seen_ip != o.seen_ip:
                assert (o.seen_ip, g.seen_ip, g.match_type) == (1, 0, 0), (g.line_idx, g.rule_idx)
        assert [(t.line_idx, t.rule_idx) for t in out.trips] == [(o.line_idx, o.rule_id) for o in ores if o.exceeded]
        s = lim.expire_states(now)
        dropped += s["states_dropped"]
    assert dropped > 0 and changed > 0  # not vacuous: states went, and their next events showed it
    dl = lim.banner.decision_lists.expiring
    assert len(dl) == ost.decisions_len() and len(dl) > 0
    for ip, d in dl.items():
        od = ost.decision(ip)
        assert od is not None and (od[0], od[1], od[2]) == (d.decision, d.expires_ns, d.domain), (ip, od, d)
    assert lim.banner.banned_ip == ost.banned_ip()
    assert ["0 " + l for l in lim.banner.ban_log] == [l for l in ost.ban_log().split("\n") if l]


def test_identity_and_totality(engine, stream):
    run = Run(CFG, engine)
    for data, now in stream[:2]:
        run.feed(data, now)
    before, stats0 = engine.state_dump(), engine.state_stats()
    s = engine.state_expire(INT64_MIN)
    assert s["states_dropped"] == 0 and s["ips_dropped"] == 0 and s["arena_bytes_after"] == s["arena_bytes_before"]
    assert (s["states_before"], s["ips_before"]) == (stats0["states"], stats0["ips"])
    assert engine.state_dump() == before == run.model.dump()
    run.compare_states(dump=False)
    s = engine.state_expire(INT64_MAX)
    assert (s["states_dropped"], s["ips_dropped"]) == (stats0["states"], stats0["ips"]) and s["arena_bytes_after"] == 0
    st = engine.state_stats()
    assert engine.state_len() == 0 and engine.state_dump() == ""
    assert (st["ips"], st["states"], st["arena_bytes"]) == (0, 0, 0)
    assert st["rehashes"] == stats0["rehashes"]
    # ids restart at 0: the next batch equals the oracle on a fresh state
    data, now = stream[2]
    fresh = O.State()
    oflags, ores, oconsumed = fresh.consume(run.ocfg, data, now, cap=(PER + 1) * 5)
    compare_batch(oflags, ores, oconsumed, engine.process(run.rs, data, now, copy_results=True))
    assert engine.state_len() == len(fresh)
    for ip in POOL[:40] + POOL[-40:]:
        for n in run.names:
            assert engine.state_get(ip, n) == fresh.get(ip, n)


def test_refused_inside_an_open_batch(engine, stream):
    """Between bjx_match_batch and the bjx_finish_batch* that closes it the
    expiry is BJX_ERR_ARG and touches nothing; the next whole batch closes it."""
    import torch
    run = Run(CFG, engine)
    data, now = stream[0]
    run.feed(data, now)
    before = engine.state_dump()
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    engine.match(run.rs, now, buf.data_ptr(), len(data))
    with pytest.raises(BanjaxGpuError) as ei:
        engine.state_expire(INT64_MAX)
    assert ei.value.code == -2
    assert engine.state_dump() == before
    data, now = stream[1]
    run.feed(data, now)
    run.expire(_mid_cutoff(now))
    run.compare_states()


def _one_rule(interval_s=5, hits=100):
    return """
regexes_with_rates:
  - {rule: "r", regex: 'GET', interval: %d, hits_per_interval: %d, decision: challenge}
expiring_decision_ttl_seconds: 10
""" % (interval_s, hits)


def _lines(events):
    """events: (ms since T0_MS, ip)"""
    return ("".join("%d.%03d %s GET h.com GET /x HTTP/1.1 ua\n" % ((T0_MS + ms) // 1000, (T0_MS + ms) % 1000, ip)
                    for ms, ip in events)).encode()


def test_order_of_survivors_and_newcomers(engine):
    run = Run(_one_rule(), engine)
    old = POOL[:30] + POOL[-30:]
    random.Random(5).shuffle(old)
    # every IP once, then every other one again 20 s later (its window restarts)
    run.feed(_lines([(k, ip) for k, ip in enumerate(old)] + [(20_000 + k, ip) for k, ip in enumerate(old[::2])]),
             T0_MS * 1_000_000)
    s, _ = run.expire((T0_MS + 10_000) * 1_000_000)
    assert s["ips_dropped"] == 30
    assert list(run.model.st) == old[::2]
    new = POOL[100:120] + old[1::4]  # unseen IPs and some of the dropped, after the survivors
    run.feed(_lines([(21_000 + k, ip) for k, ip in enumerate(new + old[:6:2])]), (T0_MS + 21_000) * 1_000_000)
    assert list(run.model.st) == old[::2] + new
    dump_ips = [l[:-1] for l in engine.state_dump().split("\n") if l.endswith(":") and not l.startswith("\t")]
    assert dump_ips == old[::2] + new
    run.compare_states()


def test_forced_hash_collisions(engine):
    """Every IP on one of two hash values: two long probe chains, expired in
    the middle.  Survivors are still found (InsideInterval goes on counting),
    the dropped come back as new IPs."""
    engine.debug_set_ip_hash_mask(0x2)
    try:
        run = Run(_one_rule(), engine)
        ips = POOL[:40] + POOL[-40:]
        random.Random(9).shuffle(ips)
        middle = set(ips[20:60])
        ev = [(k, ip) for k, ip in enumerate(ips)]
        ev += [(8_000 + k, ip) for k, ip in enumerate(ips) if ip not in middle]  # OutsideInterval: start moves on
        ev += [(8_500 + k, ip) for k, ip in enumerate(ips) if ip not in middle]  # InsideInterval: 2 hits
        run.feed(_lines(ev), T0_MS * 1_000_000)
        s, _ = run.expire((T0_MS + 4_000) * 1_000_000)
        assert s["ips_dropped"] == len(middle) == 40
        out = run.feed(_lines([(9_000 + k, ip) for k, ip in enumerate(ips)]), (T0_MS + 9_000) * 1_000_000)
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


def test_scan_tiles(engine):
    """40,000 IPs, one event each, every third one older than the cutoff:
    several tiles of the id scan and a partial one."""
    n = 40_000
    ips = ["10.%d.%d.%d" % (k >> 16, (k >> 8) & 255, k & 255) if k % 5 else "2001:db8:aaaa:bbbb::%x:%x" % (k >> 8, k & 255)
           for k in range(n)]
    run = Run(_one_rule(60, 100), engine)
    # the old third first (timestamps rise), interleaved by id: k % 3 == 0 is old
    order = [k for k in range(n) if k % 3 == 0]
    young = [k for k in range(n) if k % 3]
    data = _lines([(j // 40, ips[k]) for j, k in enumerate(order)] + [(5_000 + j // 40, ips[k]) for j, k in enumerate(young)])
    run.feed(data, T0_MS * 1_000_000)
    s, _ = run.expire((T0_MS + 3_000) * 1_000_000)
    assert s["ips_dropped"] == len(order) and engine.state_len() == len(young)
    sample = sorted(set(list(range(0, n, 997)) + list(range(255, n, 256 * 9)) + [1, 2, 3, n - 3, n - 2, n - 1]))
    run.compare_states(ips=[ips[k] for k in sample], dump=False)
    dump_ips = [l[:-1] for l in engine.state_dump().split("\n") if l.endswith(":") and not l.startswith("\t")]
    assert dump_ips == list(run.model.st)


def test_growth_and_rollback_after_expiry():
    """A small arena grows with the first batch and shrinks back with the
    expiry (the tables themselves start at their floor); then new IPs arrive
    with a claim budget small enough to roll the first claim pass back."""
    eng = Engine(ip_arena_bytes=1 << 16)
    try:
        n = 30_000
        ips = ["172.%d.%d.%d" % (16 + (k >> 16), (k >> 8) & 255, k & 255) for k in range(n)]
        run = Run(_one_rule(60, 100), eng)
        run.feed(_lines([(k // 10, ip) for k, ip in enumerate(ips)]), T0_MS * 1_000_000)
        re0 = eng.state_stats()["rehashes"]
        s, _ = run.expire((T0_MS + 2_900) * 1_000_000)  # the last 1000 IPs stay
        assert s["ips_dropped"] == n - 1000
        assert s["device_bytes_after"] < s["device_bytes_before"]
        st = eng.state_stats()
        assert st["rehashes"] == re0 and st["device_bytes"] == s["device_bytes_after"]
        eng.debug_set_claim_budget(64)
        new = ["192.168.%d.%d" % (k >> 8, k & 255) for k in range(5000)]
        run.feed(_lines([(3_000 + k // 10, ip) for k, ip in enumerate(new + ips[-1500:])]), (T0_MS + 3_000) * 1_000_000)
        eng.debug_set_claim_budget(0)
        assert eng.state_len() == 1000 + 5000 + 500
        run.compare_states(ips=new[::97] + ips[-1500::53] + ips[:3], dump=False)
        assert eng.state_dump() == run.model.dump()
    finally:
        eng.close()


def test_tables_shrink_at_scale():
    """The tables are created with 2^22 slots and never shrink below that, so
    only millions of IPs can show a table that shrinks: 3.6M IPs grow both
    tables, an expiry of the older half brings them back to 2^22 slots, and
    every sampled survivor is still found under the smaller mask."""
    eng = Engine()
    try:
        w = W.replace(W.CFG5, n_lines=3_600_000, n_ips=3_600_000, ipv6_pct=0)
        lim = RegexRateLimiter(Config.from_yaml(w.rules_yaml), engine=eng, banner=MockBanner())
        per, samples, nows = 1_800_000, [], []
        for b in range(2):
            data = w.host_lines(b * per, per)
            nows.append(w.now_ns(b * per, per))
            lim.consume_lines(data, nows[-1], want_results=False)
            lines = data.split(b"\n", 2001)
            samples.append([l.split(b" ")[1].decode() for l in lines[:2000:40]])
        st0 = eng.state_stats()
        assert st0["ips"] == 2 * per and st0["ip_slots"] > 1 << 22 and st0["state_slots"] > 1 << 22
        # half a millisecond before the second batch's first timestamp (lines
        # carry milliseconds): the first batch goes, the second stays
        s = eng.state_expire(nows[1] - 500_000)
        st = eng.state_stats()
        assert s["ips_dropped"] == per and st["ips"] == per == eng.state_len()
        assert st["ip_slots"] == 1 << 22 and st["state_slots"] == 1 << 22 and st["rehashes"] == st0["rehashes"]
        assert s["device_bytes_after"] == st["device_bytes"] < s["device_bytes_before"] == st0["device_bytes"]
        for ip in samples[0]:
            assert eng.state_get(ip, "flood10") is None, ip
        for ip in samples[1]:
            assert eng.state_get(ip, "flood10") is not None, ip
    finally:
        eng.close()


HOT_CFG = """
regexes_with_rates:
  - {rule: "every", regex: '.*', interval: 0.25, hits_per_interval: -1, decision: challenge}
  - {rule: "shared", regex: 'GET', interval: 2, hits_per_interval: 37, decision: challenge}
  - {rule: "shared", regex: 'POST', interval: 2, hits_per_interval: 37, decision: nginx_block}
expiring_decision_ttl_seconds: 10
"""


def _hot_lines(t0_ms, n):
    """as test_gpu_hotkey: 6.6.6.6 sends nine lines of ten (a k_long_* run)"""
    out = []
    for k in range(n):
        t = t0_ms + k
        m = "POST" if k % 7 == 0 else "GET"
        ip = "6.6.6.6" if k % 10 else "7.7.%d.%d" % (k % 3, k % 200)
        out.append("%d.%03d %s %s h.com %s /x HTTP/1.1 ua" % (t // 1000, t % 1000, ip, m, m))
    return ("\n".join(out) + "\n").encode()


def test_hot_key_and_slot_cache(engine, monkeypatch):
    """The first global rule matches every line (hot_name and the ip_st slot
    cache in use), one IP takes the long-run path; the expiry between the two
    batches drops the quiet IPs' older states and keeps the hot IP."""
    monkeypatch.setenv("BJX_CHECK", "1")
    monkeypatch.setenv("BJX_SORT2", "1")
    engine.debug_set_slot_cache(1)
    try:
        run = Run(HOT_CFG, engine)
        run.feed(_hot_lines(T0_MS, 30_000), T0_MS * 1_000_000)
        assert engine.scan_stats()["long_runs"] > 0
        # a quiet IP sends every 600 ms: those silent for the last 300 ms go
        s, _ = run.expire((T0_MS + 29_700) * 1_000_000)
        assert s["states_dropped"] > 0 and s["ips_dropped"] > 0 and s["ips_dropped"] < s["ips_before"] - 1
        assert engine.state_get("6.6.6.6", "every") is not None
        run.compare_states(dump=True)
        run.feed(_hot_lines(T0_MS + 30_000, 30_000), (T0_MS + 30_000) * 1_000_000)
        assert engine.scan_stats()["long_runs"] > 0
        run.compare_states(dump=True)
    finally:
        engine.debug_set_slot_cache(-1)


def test_node_equals_single_engine(engine, stream):
    """Three engines on device 0: the same stream and cutoffs through
    Node.state_expire give the single engine's results and drop counts."""
    _, single = _parity_run(engine, stream)
    node = Node([0, 0, 0])
    try:
        _, sharded = _parity_run(node, stream)
        for a, b in zip(single, sharded):
            for k in ("states_before", "states_dropped", "ips_before", "ips_dropped", "arena_bytes_before",
                      "arena_bytes_after"):
                assert a[k] == b[k], (k, a, b)
    finally:
        node.close()
