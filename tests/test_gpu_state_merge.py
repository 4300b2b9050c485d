"""bjx_state_merge: a snapshot folded into an engine that holds state
(include/banjax_gpu.h; model: banjax_amd/state_merge.py).

Where the expected values come from.  Engine-side states: small batches fed
through the oracle (Run / Model, restated from tests/test_gpu_state_snapshot.py),
whose stored states snapshot.build turns into the engine's expected export.
Snapshots: snapshot.build of hand-made states, or of the oracle's states varied
by hand.  Expected blobs and counts after a merge: the model.  Expected
RuleResults of a batch after a merge: the matches (line, rule, position) of a
fresh oracle state over that batch, with seen_ip / match_type / exceeded from
the Python restatement of Apply (rate_limit.go:37-78) seeded with the merged
states.  Nothing expected comes from the engine.

The issue's case 9 (a key held with valid == 0) is not here: no hook leaves
such a slot reachable.  A batch that overruns bjx_debug_set_claim_budget is
rolled back (k_st_rollback empties every claimed slot with valid == 0) and
claimed again, and a finished batch has applied an event to every slot it
claimed, so between two calls no state slot has valid == 0."""
import ctypes
import random
import re
import struct

import numpy as np
import pytest

from oracle import oracle as O

from banjax_amd import Config, Engine, Node, Ruleset, _lib, snapshot, state_merge
from banjax_amd._lib import BanjaxGpuError
from banjax_amd.state_merge import KEEP, NEWER, REPLACE
from tests.parity import compare_batch, oracle_config

pytestmark = pytest.mark.gpu
S = 1_000_000_000
MS = 1_000_000
INT64_MIN = -(1 << 63)
T0_MS = 1_700_000_000_000
T0 = T0_MS * MS
ERR_ARG = -2
COUNTS = ("states_added", "states_replaced", "states_kept", "states_skipped")
POLICIES = {"newer": NEWER, "keep": KEEP, "replace": REPLACE}


class Model:
    """RegexRateLimitStates: {ip: {rule name: [NumHits, IntervalStartTime ns]}}, both levels in insertion order."""

    def __init__(self):
        self.st = {}

    @classmethod
    def from_blob(cls, blob):
        m = cls()
        ips, states = snapshot.parse(blob)
        for ip in ips:
            m.st[ip.decode()] = {n.decode(): list(v) for n, v in states[ip].items()}
        return m

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

    def states(self):
        return {ip: {n: tuple(s) for n, s in d.items()} for ip, d in self.st.items()}

    def blob(self):
        return snapshot.build(list(self.st), self.states())

    def dump(self):
        out = []
        for ip, d in self.st.items():
            out.append(ip + ":\n")
            for n in sorted(d):
                out.append("\t%s:\n\t\t{%d %d}\n" % (n, d[n][0], d[n][1]))
            out.append("\n")
        return "".join(out)


def _line_t(line):
    """the reference's timestamp of a line: float64 seconds times 1e9, truncated"""
    return int(float(line.split(b" ", 1)[0]) * 1e9)


def _t(ms):
    """_line_t of a line written ms after T0_MS"""
    return _line_t(b"%d.%03d " % ((T0_MS + ms) // 1000, (T0_MS + ms) % 1000))


class Run:
    """One config over the oracle, the model and (unless target is None) an engine or node."""

    def __init__(self, cfg_yaml, target=None):
        self.cfg = Config.from_yaml(cfg_yaml)
        self.rules = self.cfg.all_rules()
        self.names = sorted(set(r.rule for r in self.rules))
        self.rs = Ruleset(self.cfg)
        self.ocfg = oracle_config(self.cfg)
        self.ost = O.State()
        self.model = Model()
        self.t = target
        if target is not None:
            target.state_clear()

    def feed(self, data, now_ns):
        """the batch through the oracle, the model and the target: RuleResults, line flags and trips must be equal"""
        lines = data.split(b"\n")
        oflags, ores, oconsumed = self.ost.consume(self.ocfg, data, now_ns, cap=(len(lines) + 1) * (len(self.rules) + 1))
        for o in ores:
            assert not o.skip_host
            ip = lines[o.line_idx].split(b" ", 2)[1].decode()
            got = self.model.apply(ip, self.rules[o.rule_id], _line_t(lines[o.line_idx]))
            assert got == (o.seen_ip, o.match_type, o.exceeded), (o.line_idx, o.rule_id)  # the model restates the oracle
        if self.t is not None:
            out = self.t.process(self.rs, data, now_ns, copy_results=True)
            compare_batch(oflags, ores, oconsumed, out)

    def oracle_states(self):
        st = {}
        for ip in self.model.st:
            st[ip] = {n: self.ost.get(ip, n) for n in self.names if self.ost.get(ip, n) is not None}
        return st

    def oracle_blob(self, order=None):
        """the oracle's stored states, IPs in first-seen order (or the order given)"""
        return snapshot.build(list(self.model.st) if order is None else order, self.oracle_states())

    def after_merge(self, target, merged_blob, data, now_ns):
        """One more batch on a target that holds merged_blob.  The matches come
        from a fresh oracle state, the outcomes from Apply on the merged states.
        -> the model after the batch."""
        lines = data.split(b"\n")
        oflags, ores, oconsumed = O.State().consume(self.ocfg, data, now_ns, cap=(len(lines) + 1) * (len(self.rules) + 1))
        m = Model.from_blob(merged_blob)
        want = []
        for o in ores:
            assert not o.skip_host
            ip = lines[o.line_idx].split(b" ", 2)[1].decode()
            want.append((o.line_idx, o.rule_id, o.rule_pos, 0) + m.apply(ip, self.rules[o.rule_id], _line_t(lines[o.line_idx])))
        out = target.process(self.rs, data, now_ns, copy_results=True)
        assert out.consumed_bytes == oconsumed and list(out.line_flags) == oflags
        got = [(g.line_idx, g.rule_idx, g.rule_pos, g.skip_host, g.seen_ip, g.match_type, g.exceeded) for g in out.results]
        assert got == want
        assert [(t.line_idx, t.rule_idx) for t in out.trips] == [(w[0], w[1]) for w in want if w[6]]
        return m


CFG = """
regexes_with_rates:
  - {rule: "every", regex: '.*', interval: 5, hits_per_interval: 6, decision: challenge}
  - {rule: "mid", regex: 'POST', interval: 5, hits_per_interval: 2, decision: nginx_block}
  - {rule: "slow", regex: '/login', interval: 60, hits_per_interval: 10, decision: iptables_block}
expiring_decision_ttl_seconds: 10
"""
ONE_RULE = """
regexes_with_rates:
  - {rule: "r", regex: 'GET', interval: 5, hits_per_interval: 3, decision: challenge}
expiring_decision_ttl_seconds: 10
"""


def _lines(events):
    """events: (ms since T0_MS, ip, method, path)"""
    return ("".join("%d.%03d %s %s h.com %s %s HTTP/1.1 ua\n" % ((T0_MS + ms) // 1000, (T0_MS + ms) % 1000, ip, m, m, p)
                    for ms, ip, m, p in events)).encode()


def _get_lines(events):
    return _lines([(ms, ip, "GET", "/x") for ms, ip in events])


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


def _query_rows(eng):
    return [eng.state_query(order=o, limit=10)[k] for o in ("hits", "start") for k in ("n_matched", "n_ips_matched", "rows")]


def _merge_and_check(eng, ref, before, snap, policy=NEWER, **opts):
    """eng holds `before` (an expected blob, not the engine's word).  Merge
    snap: the counts are the model's, the export is the model's blob, and
    everything else a caller can read equals ref after it imported that blob.
    -> (the model's blob, the call's stats)"""
    want, ws = state_merge.merge(before, snap, policy, **opts)
    st0 = eng.state_stats()
    got = eng.state_merge(snap, policy, **opts)
    for k, v in ws.items():
        assert got[k] == v, (k, got[k], v)
    assert sum(got[k] for k in COUNTS) == got["snap_states"]
    assert got["device_bytes_before"] == st0["device_bytes"]
    st1 = eng.state_stats()
    assert got["device_bytes_after"] == st1["device_bytes"] and st1["rehashes"] == st0["rehashes"]
    assert (st1["ips"], st1["arena_bytes"]) == (ws["ips_before"] + ws["ips_added"], ws["arena_bytes_after"])
    assert st1["states"] == ws["states_before"] + ws["states_added"]
    assert st1["ip_slots"] >= st0["ip_slots"] and st1["state_slots"] >= st0["state_slots"]  # a merge never shrinks
    assert st1["arena_capacity"] >= st0["arena_capacity"]
    assert eng.state_export() == want
    ref.state_clear()
    ref.state_import(want)
    assert eng.state_dump() == ref.state_dump() == Model.from_blob(want).dump()
    assert eng.state_len() == ref.state_len() == len(snapshot.parse(want)[0])
    assert _query_rows(eng) == _query_rows(ref)
    return want, got


# ---- case 1: equivalence under each policy, and the batch after

E_IPS = ["10.1.0.%d" % k for k in range(40)]
S_NEW = ["10.2.0.%d" % k for k in range(16)] + ["2001:db8:85a3:%x::8a2e:370:%x" % (k, 0x7000 + k) for k in range(4)]


def _batch1():
    rng = random.Random(11)
    ev = []
    for k, ip in enumerate(E_IPS):
        for j in range(1 + k % 4):
            ev.append((rng.randrange(0, 2000), ip, rng.choice(("GET", "POST")), rng.choice(("/login", "/x"))))
    ev.sort(key=lambda e: e[0])
    return _lines(ev), T0


def _snapshot_for(run):
    """E_IPS[20:] shared, S_NEW new.  Each shared key in one of six relations
    to the engine's record: equal, same window with more / fewer hits, a later
    window, an earlier one, absent; every third shared IP brings a name the
    engine has never interned."""
    ost = run.oracle_states()
    states, order = {}, []
    for i, ip in enumerate(E_IPS[20:]):
        d = {}
        for j, (n, (hits, start)) in enumerate(sorted(ost[ip].items())):
            v = (3 * i + j) % 6
            if v < 5:
                d[n] = [(hits, start), (hits + 1, start), (hits - 1, start), (1, start + S), (5, start - S)][v]
        for n in run.names:
            if n not in ost[ip] and i % 2:
                d[n] = (2, T0 + 1500 * MS)
        if i % 3 == 0:
            d["zz_new"] = (2, T0)
        states[ip] = d
    for k, ip in enumerate(S_NEW):
        states[ip] = {"every": (k % 7, T0 + k * 100 * MS)}
        if k % 2:
            states[ip]["mid"] = (2, T0 + 2500 * MS)
    order = S_NEW[:10] + E_IPS[:19:-1] + S_NEW[10:]  # new and shared IPs interleaved, the shared ones backwards
    blob = snapshot.build(order, states)
    assert all(states[ip] for ip in order)
    return blob


def _batch2():
    rng = random.Random(12)
    ips = E_IPS[:10] + E_IPS[20:30] + S_NEW[:8] + S_NEW[-2:] + ["10.3.0.%d" % k for k in range(5)]
    ev = []
    for ip in ips:
        for j in range(rng.randrange(1, 6)):
            ev.append((3000 + rng.randrange(0, 1500), ip, rng.choice(("GET", "POST")), rng.choice(("/login", "/x"))))
    ev.sort(key=lambda e: e[0])
    return _lines(ev), T0 + 3000 * MS


@pytest.mark.parametrize("policy", sorted(POLICIES))
def test_equivalence_and_the_batch_after(engine, engine_b, policy):
    for cache in (1, 0):
        engine.debug_set_slot_cache(cache)
        try:
            run = Run(CFG, engine)
            run.feed(*_batch1())
            before = run.oracle_blob()
            assert engine.state_export() == before
            snap = _snapshot_for(run)
            want, got = _merge_and_check(engine, engine_b, before, snap, POLICIES[policy])
            assert got["ips_added"] == len(S_NEW) and got["states_kept"] > 0 and got["states_added"] > len(S_NEW)
            assert (got["states_replaced"] > 0) == (policy != "keep")
            assert got["snap_names"] == 4
            data, now = _batch2()
            m = run.after_merge(engine, want, data, now)
            assert engine.state_export() == m.blob() and engine.state_dump() == m.dump()
            assert any(ip.startswith("10.3.") for ip in m.st)
        finally:
            engine.debug_set_slot_cache(-1)


# ---- case 2: the IP shapes where the lookup can go wrong

# (an IP the engine holds, an IP that must not be taken for it)
PAIRS = [
    ("2001:db8::12:345", "2001:db8::12:346"),      # 16 bytes, equal in the first 15
    ("2001:db8::123:456", "2001:db8::123:457"),    # 17 bytes, equal in the first 16
    ("123456789012345", "1234567890123456"),       # 15 and 16 bytes, equal in bytes 0..14
    ("123456789012345x", "123456789012345xy"),     # 16 and 17
    ("f" * 255, "f" * 256),                        # key16 holds min(len, 255) for both
    ("f" * 300, "f" * 299 + "e"),
    ("e" * 39, "e" * 38 + "d"),
    ("7", "8"),
    ("123.123.123.123", "123.123.123.124"),        # 15 bytes: the inline key decides
]
SINGLES = ["", "a1", "1.2", "g" * 16, "g" * 17, "h" * 39, "i" * 255, "i" * 257]


@pytest.mark.parametrize("mask", [0, 0xF, 1])
def test_ip_shapes(engine, engine_b, mask):
    """Every shape once new and once shared, with all hashes distinct, on
    eight chains, and on one.  The engine first holds the second IP of every
    pair; the first ones and the singles arrive as new IPs next to their
    look-alikes, then everything arrives again as shared."""
    assert sorted(set(len(x) for p in PAIRS for x in p) | set(len(x) for x in SINGLES))[:8] == [0, 1, 2, 3, 15, 16, 17, 39]
    held = [b for _, b in PAIRS]
    new = [a for a, _ in PAIRS] + SINGLES
    run = Run(ONE_RULE)
    run.feed(_get_lines([(k, ip) for k, ip in enumerate(held)]), T0)
    before = run.oracle_blob()
    for eng in (engine, engine_b):
        eng.state_clear()
        eng.debug_set_ip_hash_mask(mask)
    try:
        engine.state_import(before)
        snap1 = snapshot.build(new, {ip: {"r": (2, T0 + 100 * MS)} for ip in new})
        want1, got = _merge_and_check(engine, engine_b, before, snap1)
        assert (got["ips_added"], got["states_added"], got["states_kept"]) == (len(new), len(new), 0)
        everything = held + new
        random.Random(5).shuffle(everything)
        snap2 = snapshot.build(everything, {ip: {"r": (3, T0 + (200 + k) * MS)} for k, ip in enumerate(everything)})
        want2, got = _merge_and_check(engine, engine_b, want1, snap2)
        assert (got["ips_added"], got["states_added"], got["states_replaced"]) == (0, 0, len(everything))
        assert snapshot.parse(want2)[0] == [ip.encode() for ip in held + new]
        for k, ip in enumerate(everything):
            assert engine.state_get(ip, "r") == (3, T0 + (200 + k) * MS), ip
        # each one found by the next batch: hits 3 + 1 trips the rule
        data = _get_lines([(1000 + k, ip) for k, ip in enumerate(everything + ["9.9.9.9"])])
        m = run.after_merge(engine, want2, data, T0 + 1000 * MS)
        assert engine.state_len() == len(everything) + 1
        assert snapshot.parse(engine.state_export())[1] == snapshot.parse(m.blob())[1]
        for ip in everything:
            assert engine.state_get(ip, "r") == (0, T0 + (200 + everything.index(ip)) * MS)
    finally:
        for eng in (engine, engine_b):
            eng.debug_set_ip_hash_mask(0)
            eng.state_clear()


# ---- case 3: growth

def test_a_merge_that_fits_keeps_the_capacities_and_one_that_does_not_grows_the_arena(engine_b):
    eng = Engine(ip_arena_bytes=1 << 14)
    try:
        run = Run(ONE_RULE, eng)
        run.feed(_get_lines([(k, "10.4.0.%d" % k) for k in range(30)]), T0)
        before = run.oracle_blob()
        st0 = eng.state_stats()
        small = ["10.4.0.%d" % k for k in range(20, 45)]
        snap = snapshot.build(small, {ip: {"r": (1, T0 + S)} for ip in small})
        want, got = _merge_and_check(eng, engine_b, before, snap)
        st1 = eng.state_stats()
        assert got["ips_added"] == 15 and got["device_bytes_after"] == got["device_bytes_before"]
        assert [st1[k] for k in ("ip_slots", "state_slots", "arena_capacity")] == \
            [st0[k] for k in ("ip_slots", "state_slots", "arena_capacity")]
        # 40 IPs of 300 bytes: the arena passes the load its size allows (2 * bytes + 4096 <= capacity)
        long_ips = ["%03d" % k + "z" * 297 for k in range(40)]
        snap = snapshot.build(long_ips + small[:5], {ip: {"r": (2, T0 + 2 * S)} for ip in long_ips + small[:5]})
        want, got = _merge_and_check(eng, engine_b, want, snap)
        st2 = eng.state_stats()
        assert got["device_bytes_after"] > got["device_bytes_before"] and st2["rehashes"] == st0["rehashes"]
        assert st2["arena_capacity"] > st1["arena_capacity"] and st2["arena_capacity"] >= 2 * st2["arena_bytes"] + 4096
        assert (st2["ip_slots"], st2["state_slots"]) == (st1["ip_slots"], st1["state_slots"])
        data = _get_lines([(3000 + k, ip) for k, ip in enumerate(long_ips[::7] + small[::5] + ["10.4.0.1", "10.9.9.9"])])
        m = run.after_merge(eng, want, data, T0 + 3000 * MS)
        assert eng.state_export() == m.blob()
    finally:
        eng.close()


def _np_blob(ids, hits, starts):
    """snapshot.build for IPs "%08d" % id with one state each under the name "r", from numpy arrays"""
    n = len(ids)
    digits = (np.asarray(ids, dtype=np.int64)[:, None] // 10 ** np.arange(7, -1, -1, dtype=np.int64)) % 10 + 48
    recs = np.zeros(n, dtype=np.dtype([("ip", "<u4"), ("name", "<u4"), ("hits", "<i8"), ("start", "<i8")]))
    recs["ip"], recs["hits"], recs["start"] = np.arange(n), hits, starts
    total = snapshot.layout(1, 1, n, 8 * n, n)[-1]
    blob = struct.pack("<8sII6Q", snapshot.MAGIC, 1, 64, total, 1, 1, n, 8 * n, n) + struct.pack("<2Q", 0, 1) + b"r" + b"\0" * 7 + \
        (np.arange(n + 1, dtype="<u8") * 8).tobytes() + digits.astype(np.uint8).tobytes() + recs.tobytes()
    assert len(blob) == total
    return blob


def test_table_growth(engine_b):
    """The tables are created with 2^22 slots, so only a union of more than
    3.1M IPs and states passes their 3/4 load.  50 IPs fed through the oracle,
    then a snapshot of 3.3M IPs, 25 of them shared: the model's rule in numpy
    (the Python model would take minutes), checked against the model on the
    first 1,000 IPs of the same snapshot."""
    n, first = 3_300_000, 25
    eng = Engine(ip_arena_bytes=1 << 24)
    try:
        run = Run(ONE_RULE, eng)
        run.feed(_get_lines([(k, "%08d" % k) for k in range(50)]), T0)
        before = run.oracle_blob()
        assert eng.state_export() == before
        e_ids = np.arange(50)
        e_hits, e_starts = np.ones(50, dtype=np.int64), np.array([_t(k) for k in range(50)], dtype=np.int64)
        assert _np_blob(e_ids, e_hits, e_starts) == before
        s_ids = np.arange(first, first + n)
        s_hits, s_starts = s_ids % 5, T0 + (s_ids % 3 - 1) * S  # a third older, a third the engine's second, a third newer

        def merged(k):
            """NEWER over the first k snapshot IPs: a shared key goes to the larger (start, hits)"""
            sh = slice(first, 50)
            h, t = e_hits.copy(), e_starts.copy()
            win = (s_starts[:25] > t[sh]) | ((s_starts[:25] == t[sh]) & (s_hits[:25] > h[sh]))
            h[sh], t[sh] = np.where(win, s_hits[:25], h[sh]), np.where(win, s_starts[:25], t[sh])
            return _np_blob(np.concatenate([e_ids, s_ids[25:k]]), np.concatenate([h, s_hits[25:k]]),
                            np.concatenate([t, s_starts[25:k]])), int(win.sum())
        assert merged(1000)[0] == state_merge.merge(before, _np_blob(s_ids[:1000], s_hits[:1000], s_starts[:1000]))[0]
        want, replaced = merged(n)
        st0 = eng.state_stats()
        assert st0["ip_slots"] == st0["state_slots"] == 1 << 22
        got = eng.state_merge(_np_blob(s_ids, s_hits, s_starts))
        assert (got["ips_added"], got["states_added"], got["states_replaced"], got["states_kept"], got["states_skipped"]) == \
            (n - 25, n - 25, replaced, 25 - replaced, 0)
        st = eng.state_stats()

        def rule(k):
            p = 1
            while p < k * 4 // 3 + 1024:
                p <<= 1
            return p
        assert st["ips"] == st["states"] == n + 25 and st["ip_slots"] == st["state_slots"] == rule(n + 25) > 1 << 22
        assert st["arena_bytes"] == 8 * (n + 25) and st["arena_capacity"] > st0["arena_capacity"]
        assert got["device_bytes_after"] == st["device_bytes"] > got["device_bytes_before"] == st0["device_bytes"]
        assert st["rehashes"] == st0["rehashes"]
        assert eng.state_export() == want
        for k in (0, 24, 25, 49, 50, n // 2, first + n - 1):
            rec = eng.state_get("%08d" % k, "r")
            assert rec is not None and rec[1] in (_t(k), T0 + (k % 3 - 1) * S), k
        # the batch after: shared, engine-only, snapshot-only and brand-new IPs (a snapshot of the touched IPs stands for the 3.3M)
        touched = [0, 24, 25, 26, 27, 49, 50, 51, 52, n // 2, first + n - 1]
        small_ids = np.array([k for k in touched if k >= first])
        small = state_merge.merge(before, _np_blob(small_ids, small_ids % 5, T0 + (small_ids % 3 - 1) * S))[0]
        data = _get_lines([(1200 + j, "%08d" % k) for j, k in enumerate(touched + [99_999_999])])
        m = run.after_merge(eng, small, data, T0 + 1200 * MS)
        for k in touched + [99_999_999]:
            assert eng.state_get("%08d" % k, "r") == tuple(m.st["%08d" % k]["r"]), k
        assert eng.state_len() == n + 26
    finally:
        eng.close()


# ---- case 4: nothing to change

def test_nothing_to_change(engine):
    run = Run(CFG, engine)
    run.feed(*_batch1())
    before = run.oracle_blob()
    assert engine.state_export() == before
    shared = snapshot.build(E_IPS[5:25], {ip: {n: (v[0] + 3, v[1] + S) for n, v in d.items()}
                                          for ip, d in run.oracle_states().items()})
    old = snapshot.build(["10.8.0.1", E_IPS[3]], {"10.8.0.1": {"every": (9, T0 - S), "new_name": (1, T0 - 1)},
                                                  E_IPS[3]: {"every": (9, T0 - 2)}})
    cases = [(before, NEWER, INT64_MIN), (before, KEEP, INT64_MIN), (before, REPLACE, INT64_MIN), (old, REPLACE, T0),
             (shared, KEEP, INT64_MIN), (snapshot.build([], {}), NEWER, INT64_MIN)]
    for snap, policy, cut in cases:
        st0, bound0 = engine.state_stats(), engine.state_export_bound()
        want, ws = state_merge.merge(before, snap, policy, cut)
        assert want == before and ws["states_added"] == ws["states_replaced"] == 0
        got = engine.state_merge(snap, policy, cut)
        for k, v in ws.items():
            assert got[k] == v, (k, got[k], v)
        assert got["ips_added"] == got["states_added"] == got["states_replaced"] == 0
        assert got["arena_bytes_after"] == got["arena_bytes_before"] == st0["arena_bytes"]
        assert got["device_bytes_after"] == got["device_bytes_before"] == st0["device_bytes"]
        assert engine.state_stats() == st0  # field by field: the capacities, device_bytes and rehashes too
        assert engine.state_export() == before and engine.state_export_bound() == bound0
    # and the engine goes on as the uninterrupted oracle does
    data, now = _batch2()
    run.feed(data, now)
    assert engine.state_export() == run.oracle_blob()


def test_an_empty_engine_merges_as_it_imports(engine, engine_b):
    run = Run(CFG)
    run.feed(*_batch1())
    snap = _snapshot_for(run)
    engine.state_clear()
    want, got = _merge_and_check(engine, engine_b, snapshot.build([], {}), snap, KEEP)
    assert want == snap and (got["ips_before"], got["states_before"], got["states_added"]) == (0, 0, got["snap_states"])
    m = run.after_merge(engine, want, *_batch2())
    assert engine.state_export() == m.blob()


# ---- case 5: dry run

def test_dry_run(engine, engine_b):
    run = Run(CFG, engine)
    run.feed(*_batch1())
    before = run.oracle_blob()
    snap = _snapshot_for(run)
    for policy in (NEWER, KEEP, REPLACE):
        st0, bound0 = engine.state_stats(), engine.state_export_bound()
        dry = engine.state_merge(snap, policy, dry_run=True)
        assert dry["device_bytes_after"] == dry["device_bytes_before"] == st0["device_bytes"]
        assert engine.state_stats() == st0 and engine.state_export() == before
        assert engine.state_export_bound() == bound0  # the snapshot's new name is not interned either
        ws = state_merge.merge(before, snap, policy)[1]
        for k, v in ws.items():
            assert dry[k] == v, (k, dry[k], v)
    want, real = _merge_and_check(engine, engine_b, before, snap, NEWER)
    engine.state_clear()
    engine.state_import(before)
    dry = engine.state_merge(snap, NEWER, dry_run=True)
    real = engine.state_merge(snap, NEWER)
    assert real["device_bytes_after"] == real["device_bytes_before"]  # this merge fits, so every field but the time is equal
    assert {k: v for k, v in dry.items() if k != "device_ms"} == {k: v for k, v in real.items() if k != "device_ms"}
    assert engine.state_export() == want
    # a dry run refuses what the real call refuses
    with pytest.raises(BanjaxGpuError) as ei:
        engine.state_merge(_dup_blob(("10.77.0.1", "10.77.0.2")), NEWER, dry_run=True)
    assert ei.value.code == ERR_ARG and "twice" in str(ei.value) and engine.state_export() == want


# ---- case 6: parts

def test_parts(engine, engine_b):
    third = Engine()
    try:
        engs = [engine, engine_b, third]
        own = ["10.5.0.%d" % k for k in range(12)]
        befores = []
        for k, eng in enumerate(engs):
            mine = own[k::2]  # overlapping: the engines' own IPs are whoever's
            b = snapshot.build(mine, {ip: {"mid": (1, T0)} for ip in mine})
            eng.state_clear()
            eng.state_import(b)
            befores.append(b)
        ips = ["10.5.0.%d" % k for k in range(6, 60)] + ["2001:db8::%x" % k for k in range(30)]
        snap = snapshot.build(ips, {ip: {"mid": (2, T0 + S), "slow": (1, T0)} for ip in ips})
        seen = {}
        for k, eng in enumerate(engs):
            want, ws = state_merge.merge(befores[k], snap, NEWER, INT64_MIN, k, 3)
            got = eng.state_merge(snap, part=k, n_parts=3)
            for f, v in ws.items():
                assert got[f] == v, (k, f)
            assert eng.state_export() == want
            held = snapshot.parse(eng.state_export())[1]
            for ip in ips:
                if held.get(ip.encode(), {}).get(b"slow") == (1, T0):
                    assert ip not in seen and state_merge.owner(ip.encode(), 3) == k, ip
                    seen[ip] = k
            assert got["ips_skipped"] == sum(1 for ip in ips if state_merge.owner(ip.encode(), 3) != k) > 0
        assert sorted(seen) == sorted(ips) and set(seen.values()) == {0, 1, 2}
    finally:
        third.close()


# ---- case 7: node

def test_node(engine_b):
    node = Node([0, 0, 0])
    try:
        run = Run(CFG, node)
        run.feed(*_batch1())
        snap = _snapshot_for(run)
        shard_before = []
        for k in range(3):
            mine = [ip for ip in run.model.st if state_merge.owner(ip.encode(), 3) == k]
            shard_before.append(run.oracle_blob(mine))
            assert node.engine(k).state_export() == shard_before[k] and mine
        wants = [state_merge.merge(shard_before[k], snap, REPLACE, T0 - S, k, 3) for k in range(3)]
        with pytest.raises(BanjaxGpuError) as ei:
            node.state_merge(snap, REPLACE, T0 - S, 1, 3)
        assert ei.value.code == ERR_ARG
        dry = node.state_merge(snap, REPLACE, T0 - S, dry_run=True)
        assert [node.engine(k).state_export() for k in range(3)] == shard_before
        got = node.state_merge(snap, REPLACE, T0 - S)
        for f in wants[0][1]:
            v = wants[0][1][f] if f.startswith("snap_") else sum(w[1][f] for w in wants)
            assert got[f] == dry[f] == v, f
        assert got["states_added"] > 0 and got["states_replaced"] > 0 and got["ips_added"] == len(S_NEW)
        for k in range(3):
            assert node.engine(k).state_export() == wants[k][0]
        # the node's view: every IP once, readable through the node
        for ip, d in snapshot.parse(snap)[1].items():
            for n, rec in d.items():
                if rec[1] >= T0 - S:
                    assert node.state_get(ip, n) == rec
        assert node.state_len() == len(E_IPS) + len(S_NEW)
        again = node.state_merge(snap, REPLACE, T0 - S)  # idempotent: the repeat finds nothing to do
        assert again["states_added"] == again["states_replaced"] == again["ips_added"] == 0
        assert [node.engine(k).state_export() for k in range(3)] == [w[0] for w in wants]
    finally:
        node.close()


# ---- case 8: refusals leave the engine as it was

def _sections(blob):
    magic, ver, hb, total, n_names, names_bytes, n_ips, ip_bytes, n_states = struct.unpack_from("<8sII6Q", blob)
    return (n_names, n_ips, ip_bytes, n_states) + snapshot.layout(n_names, names_bytes, n_ips, ip_bytes, n_states)


def _poke(blob, off, fmt, v):
    b = bytearray(blob)
    struct.pack_into(fmt, b, off, v)
    return bytes(b)


def _bad_blobs(blob):
    """the snapshots bjx_state_import refuses (tests/test_gpu_state_snapshot.py), and which check names each"""
    n_names, n_ips, ip_bytes, n_states, o_name_off, o_names, o_ip_off, o_ips, o_recs, _ = _sections(blob)
    bad = {"records: ip index out of range": _poke(blob, o_recs + 24 * 9, "<I", n_ips)}
    r = [blob[o_recs + 24 * k:o_recs + 24 * (k + 1)] for k in (20, 21)]
    bad["records: not strictly ascending by (ip, name)"] = blob[:o_recs + 24 * 20] + r[1] + r[0] + blob[o_recs + 24 * 22:]
    bad["ip_off: not monotone from 0"] = _poke(blob, o_ip_off + 8 * 5, "<Q", struct.unpack_from("<Q", blob, o_ip_off + 8 * 4)[0] - 1)
    bad["ip_off: does not end at ip_bytes"] = _poke(blob, o_ip_off + 8 * n_ips, "<Q", ip_bytes - 1)
    bad["records: name index out of range"] = _poke(blob, o_recs + 24 * 9 + 4, "<I", n_names)
    recs = [struct.unpack_from("<IIqq", blob, o_recs + 24 * j) for j in range(n_states)]
    kept = [x for x in recs if x[0] != 3]
    assert 0 < len(kept) < n_states
    body = b"".join(struct.pack("<IIqq", *x) for x in kept)
    hdr = list(struct.unpack_from("<8sII6Q", blob))
    hdr[8] = len(kept)
    hdr[3] = o_recs + len(body)
    bad["records: an IP without a record"] = struct.pack("<8sII6Q", *hdr) + blob[64:o_recs] + body
    bad["total_bytes: does not equal the length given"] = blob[:-8]
    bad["magic: not BJXSTATE"] = b"X" + blob[1:]
    bad["version: not 1"] = _poke(blob, 8, "<I", 2)
    bad["names: not sorted"] = _poke(blob, o_names, "<B", ord("z"))  # "zvery" before "mid"
    return bad


def _dup_blob(pair):
    """two IPs of equal length, then the second one's bytes overwritten with the first's"""
    a, b = pair
    assert len(a) == len(b)
    blob = snapshot.build([a, b], {a: {"every": (1, T0)}, b: {"every": (2, T0)}})
    o_ips = _sections(blob)[7]
    return blob[:o_ips + len(a)] + a.encode() + blob[o_ips + 2 * len(a):]


def _message(exc, call):
    m = re.search(r"%s: (.*) \(code -?\d+\)$" % call, str(exc), re.S)
    assert m, str(exc)
    return m.group(1)


def test_refusals(engine, engine_b):
    import torch
    run = Run(CFG, engine)
    run.feed(*_batch1())
    before = run.oracle_blob()
    assert engine.state_export() == before
    good = _snapshot_for(run)
    st0 = engine.state_stats()

    def refused(snap, word=None, **kw):
        with pytest.raises(BanjaxGpuError) as ei:
            engine.state_merge(snap, **kw)
        assert ei.value.code == ERR_ARG, ei.value
        if word:
            assert word in str(ei.value), ei.value
        assert engine.state_export() == before and engine.state_stats() == st0
        return ei.value

    # every snapshot import refuses, for the same reason in the same words
    engine_b.state_clear()
    for why, bad in _bad_blobs(good).items():
        with pytest.raises(BanjaxGpuError) as ei:
            engine_b.state_import(bad)
        assert ei.value.code == ERR_ARG and _message(ei.value, "bjx_state_import") == why, (why, ei.value)
        assert _message(refused(bad), "bjx_state_merge") == why
        assert _message(refused(bad, dry_run=True), "bjx_state_merge") == why
    # an IP twice: one the engine holds (both short and long), one it does not
    for pair in ((E_IPS[3], E_IPS[4]), ("10.66.0.1", "10.66.0.2"), ("q" * 40 + "1", "q" * 40 + "2")):
        with pytest.raises(BanjaxGpuError) as ei:
            engine_b.state_import(_dup_blob(pair))
        assert _message(refused(_dup_blob(pair), "twice"), "bjx_state_merge") == _message(ei.value, "bjx_state_import")
    # ... and with other IPs around it, new and shared
    ips = ["10.66.1.%d" % k for k in range(30)] + E_IPS[10:14]
    crowd = snapshot.build(ips, {ip: {"mid": (1, T0)} for ip in ips})
    o_ips = _sections(crowd)[7]
    refused(crowd[:o_ips + 9 * 9] + b"10.66.1.2" + crowd[o_ips + 10 * 9:], "twice")  # 10.66.1.9 overwritten
    refused(good, "policy", policy=3)
    for flags in (2, 3, 1 << 31):
        o = _lib.MergeOptions(INT64_MIN, 0, 1, 0, flags)
        assert _lib.lib().bjx_state_merge(engine._h, good, len(good), ctypes.byref(o), None) == ERR_ARG
        assert engine.state_export() == before
    for part, n_parts in ((2, 2), (0, 0), (0, 257), (5, 3)):
        refused(good, "part", part=part, n_parts=n_parts)
    # out may be NULL
    o = _lib.MergeOptions(INT64_MIN, 0, 1, 0, 0)
    assert _lib.lib().bjx_state_merge(engine._h, None, len(good), ctypes.byref(o), None) == ERR_ARG
    assert _lib.lib().bjx_state_merge(engine._h, good, len(good), None, None) == ERR_ARG
    assert engine.state_export() == before
    # inside an open batch; the next whole batch closes it, and finds the state the oracle has
    data, now = _batch2()
    buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    engine.match(run.rs, now, buf.data_ptr(), len(data))
    with pytest.raises(BanjaxGpuError) as ei:
        engine.state_merge(good)
    assert ei.value.code == ERR_ARG and "between" in str(ei.value)
    run.feed(data, now)
    before2 = run.oracle_blob()
    assert engine.state_export() == before2
    # and the good one still goes in, with no stats asked for
    assert _lib.lib().bjx_state_merge(engine._h, good, len(good), ctypes.byref(o), None) == 0
    assert engine.state_export() == state_merge.merge(before2, good)[0]
