"""Snapshot and restore of the rate-limit state (bjx_state_export /
bjx_state_import, include/banjax_gpu.h; format: banjax_amd/snapshot.py).

Expected values: the oracle runs the whole stream without interruption and
gives every RuleResult, line flag and trip and (State.get) every stored state;
a Python restatement of RegexRateLimitStates.Apply (reference
internal/rate_limit.go:37-78) replays the oracle's events to keep the IPs in
first-seen order and to apply the min_start_ns filter; snapshot.build turns
either into the expected bytes.  Nothing expected comes from the engine."""
import random
import struct

import pytest

from oracle import oracle as O

import workloads as W
from banjax_amd import Config, Engine, MockBanner, Node, RegexRateLimiter, Ruleset, snapshot
from banjax_amd._lib import BanjaxGpuError
from tests.parity import compare_batch, oracle_config

pytestmark = pytest.mark.gpu
S = 1_000_000_000
INT64_MIN = -(1 << 63)
T0_MS = 1_700_000_000_000
ERR_ARG, ERR_CAPACITY = -2, -6


class Model:
    """RegexRateLimitStates: {ip: {rule name: [NumHits, IntervalStartTime ns]}}, both levels in insertion order."""

    def __init__(self):
        self.st = {}

    def apply(self, ip, rule, t):
        """Apply, rate_limit.go:37-78 -> (seenIp, MatchType, Exceeded)."""
        states = self.st.get(ip)
        if states is None:
            seen, mt = 0, 0
            state = [1, t]
            self.st[ip] = {rule.rule: state}
        else:
            seen = 1
            state = states.get(rule.rule)
            if state is not None:
                if t - state[1] > rule.interval:
                    mt = 1
                    state[0], state[1] = 1, t
                else:
                    mt = 2
                    state[0] += 1
            else:
                mt = 0
                state = [1, t]
                states[rule.rule] = state
        if state[0] > rule.hits_per_interval:
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
                self.st[ip] = keep
        return ds, di, partial

    def copy(self):
        m = Model()
        m.st = {ip: {n: list(s) for n, s in d.items()} for ip, d in self.st.items()}
        return m

    def n_states(self):
        return sum(len(d) for d in self.st.values())

    def blob(self, order=None):
        return snapshot.build(list(self.st) if order is None else order,
                              {ip: {n: tuple(s) for n, s in d.items()} for ip, d in self.st.items()})

    def dump(self, order=None):
        out = []
        for ip in (self.st if order is None else order):
            d = self.st[ip]
            out.append(ip + ":\n")
            for n in sorted(d):
                out.append("\t%s:\n\t\t{%d %d}\n" % (n, d[n][0], d[n][1]))
            out.append("\n")
        return "".join(out)


class Run:
    """One config over the oracle, the model and (unless target is None) an engine or node."""

    def __init__(self, cfg_yaml, target=None, clear=True):
        self.cfg = Config.from_yaml(cfg_yaml)
        self.rules = self.cfg.all_rules()
        self.names = sorted(set(r.rule for r in self.rules))
        self.rs = Ruleset(self.cfg)
        self.ocfg = oracle_config(self.cfg)
        self.ost = O.State()
        self.model = Model()
        self.t = target
        if target is not None and clear:
            target.state_clear()

    def feed(self, data, now_ns, targets=None):
        """the batch through the oracle (once) and every target: RuleResults, line flags and trips must be equal"""
        lines = data.split(b"\n")
        oflags, ores, oconsumed = self.ost.consume(self.ocfg, data, now_ns, cap=(len(lines) + 1) * (len(self.rules) + 1))
        for o in ores:
            if o.skip_host:
                continue
            f = lines[o.line_idx].split(b" ", 2)
            got = self.model.apply(f[1].decode(), self.rules[o.rule_id], int(float(f[0]) * 1e9))
            assert got == (o.seen_ip, o.match_type, o.exceeded), (o.line_idx, o.rule_id)  # the model restates the oracle
        out = None
        for t in ([self.t] if self.t is not None else []) if targets is None else targets:
            out = t.process(self.rs, data, now_ns, copy_results=True)
            assert out.n_results == len(ores)
            compare_batch(oflags, ores, oconsumed, out)
            assert [(x.line_idx, x.rule_idx) for x in out.trips] == [(o.line_idx, o.rule_id) for o in ores if o.exceeded]
        return out

    def oracle_states(self):
        st = {}
        for ip in self.model.st:
            st[ip] = {n: self.ost.get(ip, n) for n in self.names if self.ost.get(ip, n) is not None}
        return st

    def oracle_blob(self, order=None):
        """the oracle's stored states, IPs in first-seen order (or the order given)"""
        return snapshot.build(list(self.model.st) if order is None else order, self.oracle_states())

    def oracle_dump(self, order=None):
        st, out = self.oracle_states(), []
        for ip in (self.model.st if order is None else order):
            out.append(ip + ":\n")
            for n in sorted(st[ip]):
                out.append("\t%s:\n\t\t{%d %d}\n" % (n, st[ip][n][0], st[ip][n][1]))
            out.append("\n")
        return "".join(out)

    def compare_states(self, ips=None):
        assert self.t.state_len() == len(self.ost) == len(self.model.st)
        for ip in (self.model.st if ips is None else ips):
            for n in self.names:
                assert self.t.state_get(ip, n) == self.ost.get(ip, n), (ip, n)


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
# the same names met in another order, after one the snapshot does not know
CFG_OTHER_ORDER = """
regexes_with_rates:
  - {rule: "zz_unrelated", regex: 'ua', interval: 1, hits_per_interval: 100, decision: challenge}
  - {rule: "slow", regex: '/login', interval: 60, hits_per_interval: 10, decision: iptables_block}
  - {rule: "mid", regex: 'POST', interval: 5, hits_per_interval: 2, decision: nginx_block}
  - {rule: "fast", regex: 'GET', interval: 1, hits_per_interval: 0, decision: challenge}
expiring_decision_ttl_seconds: 10
"""
N_BATCH, PER, STEP_MS = 4, 5000, 20  # 4 batches of 100 s
POOL = ["10.1.%d.%d" % (k >> 8, k & 255) for k in range(200)] + \
       ["2001:db8:85a3:%x:0:8a2e:370:%x" % (k, 0x7000 + k) for k in range(100)]


def _stream():
    """As tests/test_gpu_state_expire.py: rising timestamps; a third of the IPs
    send throughout, a third only in the first 35% of every batch, a third only
    in batches 0 and 2."""
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


@pytest.fixture(scope="module")
def engine_b():
    e = Engine()
    yield e
    e.close()


def _mid_cutoff(now_ns):
    """inside the batch that started at now_ns: states last started in its first 45 s die"""
    return now_ns + 45 * S


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


def _dump_ips(text):
    return [l[:-1] for l in text.split("\n") if l.endswith(":") and not l.startswith("\t")]


def _other_name_order(eng):
    """eng interns zz_unrelated, slow, mid, fast in that order, then holds no state"""
    rs = Ruleset(Config.from_yaml(CFG_OTHER_ORDER))
    eng.process(rs, b"%d.000 9.9.9.9 POST h.com POST /login HTTP/1.1 ua\n" % (T0_MS // 1000), T0_MS * 1_000_000)
    assert eng.state_len() == 1
    eng.state_clear()


def test_continuation_parity_and_round_trip(engine, engine_b, stream):
    """Tests 1 and 2 of the issue: the export is the oracle's state byte for
    byte; an engine that interned the names in another order imports it and
    goes on exactly as the uninterrupted oracle does; exporting changes
    nothing in the exporter; export(import(x)) == x."""
    run = Run(CFG, engine)
    for data, now in stream[:2]:
        run.feed(data, now)
    dump0, stats0 = engine.state_dump(), engine.state_stats()
    blob = engine.state_export()
    assert blob == run.oracle_blob()
    assert len(blob) <= engine.state_export_bound() <= len(blob) + 64  # (every interned name is in use here)
    s = engine.snapshot_stats
    assert (s["ips"], s["states"], s["names"], s["bytes"]) == (len(run.model.st), run.model.n_states(), 3, len(blob))
    assert (s["ips_skipped"], s["states_skipped"]) == (0, 0)
    assert snapshot.parse(blob)[0] == [ip.encode() for ip in run.model.st]
    # purity: the exporter is as it was, and its next batch still equals the oracle
    assert engine.state_dump() == dump0 == run.oracle_dump() and engine.state_stats() == stats0

    _other_name_order(engine_b)
    got = engine_b.state_import(blob)
    assert (got["ips"], got["states"], got["names"], got["bytes"]) == (s["ips"], s["states"], 3, len(blob))
    assert (got["ips_skipped"], got["states_skipped"]) == (0, 0)
    assert engine_b.state_dump() == dump0
    assert engine_b.state_export() == blob
    run.compare_states()
    run.t = engine_b
    run.compare_states()

    # batch 2 on the exporter and the importer, batch 3 on the importer
    data, now = stream[2]
    run.feed(data, now, targets=[engine, engine_b])
    data, now = stream[3]
    run.feed(data, now)
    run.compare_states()
    assert engine_b.state_dump() == run.oracle_dump()
    assert engine_b.state_export() == run.oracle_blob()


def test_min_start_filter(engine, stream):
    run = Run(CFG, engine)
    for data, now in stream[:2]:
        run.feed(data, now)
    cutoff = _mid_cutoff(stream[1][1])
    kept = run.model.copy()
    ds, di, partial = kept.expire(cutoff)
    assert 0 < ds < run.model.n_states() and di > 0 and partial > 0
    before = engine.state_dump()
    blob = engine.state_export(cutoff)
    assert blob == kept.blob()
    s = engine.snapshot_stats
    assert (s["ips_skipped"], s["states_skipped"]) == (di, ds)
    assert (s["ips"], s["states"]) == (len(kept.st), kept.n_states())
    assert engine.state_dump() == before  # nothing expired
    # the limiter's wrapper: expire_cutoff_ns of the config
    lim = RegexRateLimiter(run.cfg, engine=engine, banner=MockBanner())
    from banjax_amd.regex_rate_limiter import expire_cutoff_ns
    now = stream[1][1] + 120 * S
    kept2 = run.model.copy()
    kept2.expire(expire_cutoff_ns(now, run.cfg))
    assert lim.export_states(now) == kept2.blob() and lim.export_states() == run.oracle_blob()


def _small_blob(stream):
    run = Run(CFG)
    data = b"\n".join(stream[0][0].split(b"\n")[:600]) + b"\n"
    run.feed(data, stream[0][1])
    return run, run.oracle_blob()


def _sections(blob):
    magic, ver, hb, total, n_names, names_bytes, n_ips, ip_bytes, n_states = struct.unpack_from("<8sII6Q", blob)
    return (n_names, n_ips, ip_bytes, n_states) + snapshot.layout(n_names, names_bytes, n_ips, ip_bytes, n_states)


def _poke(blob, off, fmt, v):
    b = bytearray(blob)
    struct.pack_into(fmt, b, off, v)
    return bytes(b)


def _bad_blobs(blob):
    n_names, n_ips, ip_bytes, n_states, _, _, o_ip_off, o_ips, o_recs, _ = _sections(blob)
    bad = {"ip = n_ips": _poke(blob, o_recs + 24 * 9, "<I", n_ips)}
    r = [blob[o_recs + 24 * k:o_recs + 24 * (k + 1)] for k in (20, 21)]
    bad["swapped records"] = blob[:o_recs + 24 * 20] + r[1] + r[0] + blob[o_recs + 24 * 22:]
    bad["ip_off not monotone"] = _poke(blob, o_ip_off + 8 * 5, "<Q", struct.unpack_from("<Q", blob, o_ip_off + 8 * 4)[0] - 1)
    # IP 3 stays in the IP section, its records go (n_states and total_bytes follow)
    recs = [struct.unpack_from("<IIqq", blob, o_recs + 24 * j) for j in range(n_states)]
    kept = [x for x in recs if x[0] != 3]
    assert 0 < len(kept) < n_states
    body = b"".join(struct.pack("<IIqq", *x) for x in kept)
    hdr = list(struct.unpack_from("<8sII6Q", blob))
    hdr[8] = len(kept)
    hdr[3] = o_recs + len(body)
    bad["an IP with no record"] = struct.pack("<8sII6Q", *hdr) + blob[64:o_recs] + body
    return bad


def _dup_blob(pair):
    """two IPs of equal length, then the second one's bytes overwritten with the first's"""
    a, b = pair
    assert len(a) == len(b)
    blob = snapshot.build([a, b], {a: {"fast": (1, T0_MS * 1_000_000)}, b: {"fast": (2, T0_MS * 1_000_000)}})
    o_ips = _sections(blob)[7]
    return blob[:o_ips + len(a)] + a.encode() + blob[o_ips + 2 * len(a):]


def _refused(eng, blob, run, data, now, word=None):
    with pytest.raises(BanjaxGpuError) as ei:
        eng.state_import(blob)
    assert ei.value.code == ERR_ARG, ei.value
    if word:
        assert word in str(ei.value), ei.value
    # empty and usable: the next batch equals a fresh oracle
    assert eng.state_len() == 0 and eng.state_dump() == ""
    fresh = O.State()
    oflags, ores, oconsumed = fresh.consume(run.ocfg, data, now, cap=(data.count(b"\n") + 1) * 5)
    compare_batch(oflags, ores, oconsumed, eng.process(run.rs, data, now, copy_results=True))
    assert eng.state_len() == len(fresh)
    eng.state_clear()


def test_refusals(engine, engine_b, stream):
    import torch
    run, blob = _small_blob(stream)
    data, now = stream[0]
    small = b"\n".join(data.split(b"\n")[:400]) + b"\n"
    # import into a non-empty engine: refused, state untouched
    engine.state_clear()
    engine.state_import(blob)
    before = engine.state_dump()
    assert before == run.oracle_dump()
    with pytest.raises(BanjaxGpuError) as ei:
        engine.state_import(blob)
    assert ei.value.code == ERR_ARG and engine.state_dump() == before
    # cap one byte short: BJX_ERR_CAPACITY with the length set
    with pytest.raises(BanjaxGpuError) as ei:
        engine.state_export(cap=len(blob) - 1)
    assert ei.value.code == ERR_CAPACITY and ei.value.needed == len(blob)
    assert engine.state_export(cap=len(blob)) == blob
    # inside an open batch: both refused, nothing touched; the next whole batch closes it
    buf = torch.frombuffer(bytearray(small), dtype=torch.uint8).to("cuda:0")
    engine.match(run.rs, now, buf.data_ptr(), len(small))
    with pytest.raises(BanjaxGpuError) as ei:
        engine.state_export()
    assert ei.value.code == ERR_ARG
    engine.process(run.rs, small, now)
    engine_b.state_clear()
    engine_b.match(run.rs, now, buf.data_ptr(), len(small))
    with pytest.raises(BanjaxGpuError) as ei:
        engine_b.state_import(blob)
    assert ei.value.code == ERR_ARG and "between" in str(ei.value)
    engine_b.process(run.rs, small, now)
    engine_b.state_clear()
    # snapshots the device checks refuse
    for what, bad in _bad_blobs(blob).items():
        _refused(engine_b, bad, run, small, now)
    _refused(engine_b, _dup_blob(("10.1.2.3", "10.3.2.1")), run, small, now, "twice")
    _refused(engine_b, _dup_blob((POOL[-1], POOL[-2])), run, small, now, "twice")
    _refused(engine_b, blob[:-8], run, small, now, "total_bytes")
    with pytest.raises(BanjaxGpuError) as ei:
        engine_b.state_import(blob, part=2, n_parts=2)
    assert ei.value.code == ERR_ARG
    # and the good one still goes in
    engine_b.state_import(blob)
    assert engine_b.state_dump() == run.oracle_dump()


def test_ip_shapes(engine, engine_b):
    """IP fields of 0, 1, 2, 3, 15, 16 and 17 bytes (the inline key16 and its
    edge) and one of 300 (the len >= 255 branch of the arena compare)."""
    ips = ["", "7", "a1", "1.2", "123.123.123.123", "2001:db8::12:345", "2001:db8::123:456", "f" * 300]
    assert [len(x) for x in ips] == [0, 1, 2, 3, 15, 16, 17, 300]
    # neighbours that differ only past byte 15 / in the last byte
    ips += ["2001:db8::12:346", "2001:db8::123:457", "f" * 299 + "e", "123.123.123.124"]
    run = Run(_one_rule(), engine)
    run.feed(_lines([(k, ip) for k, ip in enumerate(ips)]), T0_MS * 1_000_000)
    blob = engine.state_export()
    assert blob == run.oracle_blob()
    engine_b.state_clear()
    engine_b.state_import(blob)
    assert engine_b.state_export() == blob and engine_b.state_dump() == run.oracle_dump()
    run.t = engine_b
    run.compare_states()
    out = run.feed(_lines([(100 + k, ip) for k, ip in enumerate(ips)]), (T0_MS + 100) * 1_000_000)
    assert [(r.seen_ip, r.match_type) for r in out.results] == [(1, 2)] * len(ips)  # each one found: InsideInterval
    run.compare_states()
    assert engine_b.state_dump() == run.oracle_dump()


def test_empty_state(engine_b):
    """An engine without state exports the 80-byte empty snapshot and takes it back."""
    engine_b.state_clear()
    blob = engine_b.state_export()
    assert blob == snapshot.build([], {}) and len(blob) == 80
    got = engine_b.state_import(blob)
    assert (got["ips"], got["states"], got["names"]) == (0, 0, 0)
    assert engine_b.state_len() == 0 and engine_b.state_dump() == "" and engine_b.state_export() == blob


def test_scan_tiles(engine, engine_b):
    """40,000 IPs with one state each, every fifth one IPv6: several tiles of
    the id scans and a partial one, on both sides."""
    n = 40_000
    ips = ["10.%d.%d.%d" % (k >> 16, (k >> 8) & 255, k & 255) if k % 5 else "2001:db8:aaaa:bbbb::%x:%x" % (k >> 8, k & 255)
           for k in range(n)]
    order = list(range(n))
    random.Random(3).shuffle(order)
    run = Run(_one_rule(60, 100), engine)
    run.feed(_lines([(j // 40, ips[k]) for j, k in enumerate(order)]), T0_MS * 1_000_000)
    blob = engine.state_export()
    assert blob == run.model.blob()
    engine_b.state_clear()
    got = engine_b.state_import(blob)
    assert (got["ips"], got["states"]) == (n, n) and engine_b.state_len() == n
    assert _dump_ips(engine_b.state_dump()) == list(run.model.st) == [ips[k] for k in order]
    sample = sorted(set(list(range(0, n, 997)) + list(range(255, n, 256 * 9)) + [1, 2, 3, n - 3, n - 2, n - 1]))
    run.t = engine_b
    run.compare_states(ips=[ips[k] for k in sample])
    assert engine_b.state_export() == blob


def test_forced_hash_collisions(engine_b):
    """Every imported IP on one of two hash values: two probe chains built by
    the import.  The format carries no hash, so the blob is the unmasked
    engine's, and comes back out equal."""
    ips = POOL[:40] + POOL[-40:]
    random.Random(9).shuffle(ips)
    run = Run(_one_rule())
    run.feed(_lines([(k, ip) for k, ip in enumerate(ips)]), T0_MS * 1_000_000)
    blob = run.oracle_blob()
    engine_b.state_clear()
    engine_b.debug_set_ip_hash_mask(0x2)
    try:
        engine_b.state_import(blob)
        assert engine_b.state_export() == blob
        run.t = engine_b
        new = POOL[100:120]
        out = run.feed(_lines([(500 + k, ip) for k, ip in enumerate(ips + new)]), (T0_MS + 500) * 1_000_000)
        for r, ip in zip(out.results, ips + new):
            assert (r.seen_ip, r.match_type) == ((1, 2) if ip in ips else (0, 0)), ip
        for ip in ips:
            assert engine_b.state_get(ip, "r")[0] == 2
        run.compare_states()
        # (IPs of one batch that share a 64-bit hash get their ids after the
        # batch's other new IPs, so the dump is compared without its order)
        assert sorted(engine_b.state_dump().split("\n\n")) == sorted(run.oracle_dump().split("\n\n"))
    finally:
        engine_b.debug_set_ip_hash_mask(0)
        engine_b.state_clear()


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


def test_hot_key_and_slot_cache(engine, engine_b, monkeypatch):
    """The first global rule matches every line (hot_name and the ip_st slot
    cache in use) and one IP takes the long-run path, on the importer too."""
    monkeypatch.setenv("BJX_CHECK", "1")
    monkeypatch.setenv("BJX_SORT2", "1")
    engine.debug_set_slot_cache(1)
    engine_b.debug_set_slot_cache(1)
    try:
        run = Run(HOT_CFG, engine)
        engine_b.state_clear()
        # the importer has bound the ruleset and used its slot cache before the import
        engine_b.process(run.rs, _hot_lines(T0_MS - 5_000, 2_000), (T0_MS - 5_000) * 1_000_000)
        engine_b.state_clear()
        run.feed(_hot_lines(T0_MS, 30_000), T0_MS * 1_000_000)
        assert engine.scan_stats()["long_runs"] > 0
        blob = engine.state_export()
        assert blob == run.oracle_blob()
        engine_b.state_import(blob)
        run.t = engine_b
        run.feed(_hot_lines(T0_MS + 30_000, 30_000), (T0_MS + 30_000) * 1_000_000)
        assert engine_b.scan_stats()["long_runs"] > 0
        run.compare_states()
        assert engine_b.state_dump() == run.oracle_dump()
    finally:
        engine.debug_set_slot_cache(-1)
        engine_b.debug_set_slot_cache(-1)


def test_arena_growth_and_rollback_after_import():
    """30,000 IPs into an engine created with a 64 KiB arena (the import sizes
    the arena itself); then new IPs arrive with a claim budget small enough to
    roll the first claim pass back."""
    eng = Engine(ip_arena_bytes=1 << 16)
    try:
        n = 30_000
        ips = ["172.%d.%d.%d" % (16 + (k >> 16), (k >> 8) & 255, k & 255) for k in range(n)]
        run = Run(_one_rule(60, 100))
        run.feed(_lines([(k // 10, ip) for k, ip in enumerate(ips)]), T0_MS * 1_000_000)
        blob = run.model.blob()
        got = eng.state_import(blob)
        st = eng.state_stats()
        assert got["ips"] == n == st["ips"] and st["arena_bytes"] == sum(len(ip) for ip in ips)
        assert st["arena_capacity"] >= 2 * st["arena_bytes"]
        run.t = eng
        eng.debug_set_claim_budget(64)
        new = ["192.168.%d.%d" % (k >> 8, k & 255) for k in range(5000)]
        run.feed(_lines([(3_000 + k // 10, ip) for k, ip in enumerate(new + ips[-1500:])]), (T0_MS + 3_000) * 1_000_000)
        eng.debug_set_claim_budget(0)
        assert eng.state_len() == n + 5000
        run.compare_states(ips=new[::97] + ips[-1500::53] + ips[:3])
        assert eng.state_dump() == run.model.dump() == run.oracle_dump()
    finally:
        eng.close()


M32 = 0xFFFFFFFF


def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def _hash_bytes(p: bytes) -> int:
    """bjx::hash_bytes (banjax_amd/csrc/bjx_common.h), restated: the node's owner is (hash >> 32) % n"""
    n = len(p)
    a, b = 0x9E3779B9 ^ n, (0x7F4A7C15 + n * 0x85EBCA6B) & M32
    i = 0
    while i + 4 <= n:
        w = int.from_bytes(p[i:i + 4], "little")
        a = (_rotl(a ^ w, 7) * 0x27D4EB2D) & M32
        b = (_rotl((b + w) & M32, 13) * 0x165667B1) & M32
        i += 4
    t = int.from_bytes(p[i:], "little")
    a = (_rotl(a ^ t ^ 0xA5A5A5A5, 7) * 0x27D4EB2D) & M32
    b = (_rotl((b + t) & M32, 13) * 0x165667B1) & M32
    a ^= b >> 16; a = (a * 0x85EBCA6B) & M32; a ^= a >> 13; a = (a * 0xC2B2AE35) & M32; a ^= a >> 16
    b ^= a >> 15; b = (b * 0x2C1B3C6D) & M32; b ^= b >> 12; b = (b * 0x297A2D39) & M32; b ^= b >> 15
    h = (a << 32) | b
    return 0x1234567 if h in (0, (1 << 64) - 1) else h


def _owner(ip, n):
    return (_hash_bytes(ip.encode()) >> 32) % n


def _engine_major(ips, n):
    return [ip for k in range(n) for ip in ips if _owner(ip, n) == k]


def test_resharding(stream):
    """3 engines -> 1 engine -> 2 engines, each continuing at parity with the
    oracle; a node snapshot lists the IPs engine-major."""
    run = Run(CFG)
    node3, one, node2, again = Node([0, 0, 0]), Engine(), Node([0, 0]), Node([0, 0, 0])
    try:
        run.t = node3
        for data, now in stream[:2]:
            run.feed(data, now)
        order3 = _engine_major(list(run.model.st), 3)
        blob3 = node3.state_export()
        assert blob3 == run.oracle_blob(order3)
        assert _dump_ips(node3.state_dump()) == order3
        s3 = node3.snapshot_stats
        assert (s3["ips"], s3["states"], s3["bytes"]) == (len(run.model.st), run.model.n_states(), len(blob3))

        # the same size again, part by part: every IP has one owner
        parts = [again.engine(k).state_import(blob3, k, 3) for k in range(3)]
        assert sum(p["ips"] for p in parts) == s3["ips"] and sum(p["states"] for p in parts) == s3["states"]
        for k, p in enumerate(parts):
            assert p["ips"] == sum(1 for ip in run.model.st if _owner(ip, 3) == k) > 0
            assert p["ips_skipped"] == sum(q["ips"] for j, q in enumerate(parts) if j != k)
            assert p["states_skipped"] == sum(q["states"] for j, q in enumerate(parts) if j != k)
        assert again.state_export() == blob3
        again.state_clear()
        tot = again.state_import(blob3)
        assert (tot["ips"], tot["states"], tot["ips_skipped"], tot["states_skipped"]) == (s3["ips"], s3["states"], 0, 0)
        assert again.state_export() == blob3
        with pytest.raises(BanjaxGpuError) as ei:
            again.state_import(blob3)
        assert ei.value.code == ERR_ARG and again.state_export() == blob3

        # into one engine: snapshot order kept, batches 2-3 at parity
        one.state_import(blob3)
        assert one.state_export() == blob3 and _dump_ips(one.state_dump()) == order3
        run.t = one
        for data, now in stream[2:]:
            run.feed(data, now)
        run.compare_states()
        new = [ip for ip in run.model.st if ip not in set(order3)]
        order1 = order3 + new
        blob1 = one.state_export()
        assert blob1 == run.oracle_blob(order1)

        # into two engines, and batch 3 once more on the oracle and the node
        node2.state_import(blob1)
        order2 = _engine_major(order1, 2)
        assert _dump_ips(node2.state_dump()) == order2
        assert node2.state_export() == run.oracle_blob(order2)
        run.t = node2
        run.compare_states()
        data, now = stream[3]
        run.feed(data, now)
        run.compare_states()
        assert node2.state_export() == run.oracle_blob(order2)
    finally:
        for x in (node3, one, node2, again):
            x.close()


def test_tables_above_their_floor():
    """The tables are created with 2^22 slots, so only millions of IPs make the
    import size them itself: 3.6M IPs exported and imported into a default
    engine, whose tables come out as the growth rule gives for those counts."""
    a, b = Engine(), Engine()
    try:
        w = W.replace(W.CFG5, n_lines=3_600_000, n_ips=3_600_000, ipv6_pct=0)
        lim = RegexRateLimiter(Config.from_yaml(w.rules_yaml), engine=a, banner=MockBanner())
        per, samples = 1_800_000, []
        for k in range(2):
            data = w.host_lines(k * per, per)
            lim.consume_lines(data, w.now_ns(k * per, per), want_results=False)
            lines = data.split(b"\n", 2001)
            samples += [l.split(b" ")[1].decode() for l in lines[:2000:40]]
        st0 = a.state_stats()
        assert st0["ips"] == 2 * per
        blob = lim.export_states()
        s = a.snapshot_stats
        assert (s["ips"], s["states"], s["bytes"]) == (st0["ips"], st0["states"], len(blob))
        assert a.state_stats() == st0
        assert b.state_stats()["ip_slots"] == 1 << 22 and b.state_stats()["state_slots"] == 1 << 22
        got = b.state_import(blob)
        st = b.state_stats()
        assert (got["ips"], got["states"]) == (st0["ips"], st0["states"]) == (st["ips"], st["states"])

        def rule(n):
            p = 1
            while p < n * 4 // 3 + 1024:
                p <<= 1
            return p
        assert st["ip_slots"] == rule(st["ips"]) > 1 << 22 and st["state_slots"] == rule(st["states"]) > 1 << 22
        assert st["arena_bytes"] == st0["arena_bytes"] and st["rehashes"] == 0
        assert len(samples) == 100
        for ip in samples:
            assert b.state_get(ip, "flood10") is not None and b.state_get(ip, "flood10") == a.state_get(ip, "flood10"), ip
        assert b.state_export() == blob
    finally:
        a.close()
        b.close()
