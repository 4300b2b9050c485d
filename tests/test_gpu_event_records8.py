"""The 8-byte event records of the rate-limit sort (engine_types.h EvRec8: a
millisecond offset, the rule index, the first-event bit and the event index in
one 64-bit word) against the oracle and against the 12- and 16-byte forms.

Which form a batch took is scan_stats()["record_bytes"].  The 8-byte form is
tried when the ruleset and the batch fit its fields; an event whose timestamp
is not the reference's value of a whole-millisecond text, or lies outside the
span, sends the whole batch to the 12-byte form (and from there to the 16-byte
one), and the following BJX_REC_HOLD batches start at the form that worked.
Results must not depend on the form: the same input under no hook, BJX_REC12=1
and BJX_REC16=1 gives identical results, trips and state, on every apply path
(buckets, full sort, runs crossing an apply chunk, oversized buckets) and in
node mode.
"""
import pytest

import workloads as W
from banjax_amd import Config, Engine, Node, Ruleset
from tests import bucket_plan as P
from tests.parity import Pair

pytestmark = pytest.mark.gpu

S = 1_000_000_000
HOOKS = ("BJX_REC12", "BJX_REC16", "BJX_REC_HOLD", "BJX_SORT2", "BJX_SORT2_MIN", "BJX_SORT2_HOLD", "BJX_WAVE_RUNS", "BJX_CHECK")
FORMS = ((None, 8), ("BJX_REC12", 12), ("BJX_REC16", 16))
PER = 10_000


@pytest.fixture
def eng(monkeypatch):
    for h in HOOKS:
        monkeypatch.delenv(h, raising=False)
    e = Engine()
    yield e
    e.close()


def rec_bytes(e):
    return e.scan_stats()["record_bytes"]


def batch(w, b):
    return w.host_lines(b * PER, PER), w.now_ns(b * PER, PER)


def with_fraction_digit(data, line_no):
    """The batch with one more fractional digit on one line's timestamp
    (S.mmm -> S.mmm4): not a whole millisecond."""
    lines = data.split(b"\n")
    tok, rest = lines[line_no].split(b" ", 1)
    assert len(tok.split(b".")[1]) == 3
    lines[line_no] = tok + b"4 " + rest
    return b"\n".join(lines)


def test_plain_batches_take_8(eng):
    """(a) scaled cfg3, state carried across the batches."""
    w = W.scaled(W.CFG3, 3 * PER, n_ips=2_000)
    pair = Pair(w.rules_yaml, eng)
    for b in range(3):
        pair.feed(*batch(w, b), want_results=b < 2)
        assert rec_bytes(eng) == 8
    pair.compare_state([ln.split(b" ")[1].decode() for ln in w.host_lines(0, 50).split(b"\n")[:50] if ln])


def test_non_ms_line_falls_back_and_holds(eng, monkeypatch):
    """(b) one line of ....1234 sends its whole batch to the 12-byte form; the
    next BJX_REC_HOLD batches start there, then the 8-byte form is back."""
    monkeypatch.setenv("BJX_REC_HOLD", "2")
    w = W.scaled(W.CFG3, 6 * PER, n_ips=2_000)
    pair = Pair(w.rules_yaml, eng)
    want = [8, 12, 12, 12, 8, 8]
    for b in range(6):
        data, now = batch(w, b)
        if b == 1:
            data = with_fraction_digit(data, PER // 2)
        pair.feed(data, now, want_results=b in (1, 2, 4))
        assert rec_bytes(eng) == want[b], b
    pair.compare_state()


def test_batch_three_hours_past_its_clock_takes_16(eng):
    """(c) outside the 8-byte span (2^23 ms either way) and the 12-byte one."""
    w = W.scaled(W.CFG3, 3 * PER, n_ips=2_000)
    pair = Pair(w.rules_yaml, eng)
    pair.feed(*batch(w, 0))
    assert rec_bytes(eng) == 8
    data, now = batch(w, 1)
    pair.feed(data, now - 3 * 3600 * S)
    assert rec_bytes(eng) == 16
    pair.feed(*batch(w, 2), want_results=False)   # held at the form that worked
    assert rec_bytes(eng) == 16
    pair.compare_state()


def site_rules_yaml(n_hosts, per_host):
    out = ["regexes_with_rates:",
           "  - rule: 'g'\n    regex: 'GET'\n    interval: 1\n    hits_per_interval: 40\n    decision: challenge",
           "per_site_regexes_with_rates:"]
    for h in range(n_hosts):
        out.append("  h%d.example.com:" % h)
        for k in range(per_host):
            out.append("    - rule: 's%d_%d'\n      regex: '\\/p%d\\/'\n      interval: 2\n      hits_per_interval: %d\n"
                       "      decision: nginx_block" % (h, k, k, k % 3))
    return "\n".join(out) + "\n"


@pytest.mark.parametrize("per_host,want", [(64, 12), (63, 8)])
def test_ruleset_past_the_rule_field(eng, per_host, want):
    """(d) 1 + 32 * 64 = 2,049 rules: one past the 11-bit rule field, so the
    12-byte form; 1 + 32 * 63 = 2,017 rules take the 8-byte form, the site
    rules' indices up in the field's top bits."""
    n_hosts = 32
    pair = Pair(site_rules_yaml(n_hosts, per_host), eng)
    assert pair.n_rules == 1 + n_hosts * per_host
    t0 = 1_700_000_000_000
    for b in range(2):
        lines = []
        for j in range(4000):
            ms = t0 + b * 500 + j // 8
            lines.append("%d.%03d 10.2.%d.%d GET h%d.example.com GET /p%d/x HTTP/1.1 ua" % (
                ms // 1000, ms % 1000, j % 5, j % 31, (j * 7) % n_hosts, (j * 13) % per_host))
        pair.feed(("\n".join(lines) + "\n").encode(), (t0 + b * 500) * 1_000_000)
        assert rec_bytes(eng) == want
    pair.compare_state(["10.2.%d.%d" % (a, c) for a in range(5) for c in range(31)][::5])


def test_lowered_event_limit(eng):
    """(e) the event index field's gate, lowered by the debug setter to just
    under the batch's events."""
    w = W.scaled(W.CFG3, 3 * PER, n_ips=2_000)
    pair = Pair(w.rules_yaml, eng)
    n_ev = pair.feed(*batch(w, 0)).n_events
    assert rec_bytes(eng) == 8 and n_ev > 1000
    eng.debug_set_rec8_max_events(1000)
    pair.feed(*batch(w, 1))
    assert rec_bytes(eng) == 12
    eng.debug_set_rec8_max_events(0)
    pair.feed(*batch(w, 2))
    assert rec_bytes(eng) == 8     # a gate is no fallback: nothing is held
    pair.compare_state()


def run_stream(e, rs, batches, compact=False):
    """The batches on a cleared engine -> (per-batch outputs, record sizes, state dump)."""
    e.state_clear()
    outs, forms = [], []
    for data, now in batches:
        out = e.process(rs, data, now, copy_results=not compact, compact_trips=compact)
        forms.append(rec_bytes(e))
        if compact:
            outs.append(out.trips_compact().tolist())
        else:
            outs.append((out.line_flags,
                         [(r.line_idx, r.rule_idx, r.rule_pos, r.skip_host, r.seen_ip, r.match_type, r.exceeded) for r in out.results],
                         [(t.line_idx, t.rule_idx, t.line_offset, t.line_len) for t in out.trips]))
    return outs, forms, e.state_dump()


def test_three_forms_agree(eng, monkeypatch):
    """(f) no hook, BJX_REC12=1, BJX_REC16=1: identical results, trips (full
    and compact) and state; the unhooked run is the oracle's."""
    w = W.scaled(W.CFG3, 3 * PER, n_ips=2_000)
    batches = [batch(w, b) for b in range(3)]
    pair = Pair(w.rules_yaml, eng)
    for data, now in batches:
        pair.feed(data, now)
        assert rec_bytes(eng) == 8
    pair.compare_state()
    rs = Ruleset(Config.from_yaml(w.rules_yaml))
    got = {}
    for hook, size in FORMS:
        if hook:
            monkeypatch.setenv(hook, "1")
        full = run_stream(eng, rs, batches)
        comp = run_stream(eng, rs, batches, compact=True)
        if hook:
            monkeypatch.delenv(hook)
        assert full[1] == comp[1] == [size] * 3, hook
        assert full[2] == comp[2]
        got[size] = (full[0], comp[0], full[2])
    assert sum(len(t) for t in got[8][1]) > 100
    assert got[8] == got[12] == got[16]
    for (flags, res, trips), words in zip(*got[8][:2]):
        assert [(off << 24) | r for _, r, off, _ in trips] == words


# ---- (g) the apply paths, on batches planned by tests/bucket_plan.py

N_IPS = 20_000
BACK_MS = 5_000


def ip_of(k):
    return "10.%d.%d.%d" % (k >> 16, (k >> 8) & 255, k & 255)


def priming(t0_ms):
    """One line per (ip, rule name), 16 lines per ms -> (bytes, now_ns, end ms)."""
    rows, k = [], 0
    for i in range(N_IPS):
        for name in P.NAMES:
            ms = t0_ms + k // 16
            rows.append("%d.%03d %s GET h.com GET /%s HTTP/1.1" % (ms // 1000, ms % 1000, ip_of(i), P.TOKENS[name][0]))
            k += 1
    return ("\n".join(rows) + "\n").encode(), (t0_ms + k // 16) * 1_000_000, t0_ms + k // 16


def plan_lines_ms(pl, t0_ms, per_ms=8):
    """Plan.lines with whole-millisecond stamps: the runs take turns, one line
    each; line k is stamped t0 + k // per_ms ms, every third run's events 1 mod
    3 lie BACK_MS earlier; a "b" state alternates between its two rules."""
    runs = [r for _, _, _, rr in pl.jobs for r in rr]
    left = [r[3] for r in runs]
    alive = list(range(len(runs)))
    out, k = [], 0
    while alive:
        nxt = []
        for i in alive:
            ip, name, _, length = runs[i]
            j = length - left[i]
            ms = t0_ms + k // per_ms - (BACK_MS if i % 3 == 2 and j % 3 == 1 else 0)
            toks = P.TOKENS[name]
            out.append("%d.%03d %s GET h.com GET /%s HTTP/1.1" % (ms // 1000, ms % 1000, ip, toks[(j // 5 + i) % len(toks)]))
            k += 1
            left[i] -= 1
            if left[i]:
                nxt.append(i)
        alive = nxt
    assert k // per_ms + BACK_MS < 10_000, "the batch would reach the OldLine bound"
    return ("\n".join(out) + "\n").encode(), (t0_ms + k // per_ms) * 1_000_000


PATHS = {
    # name: (BJX_SORT2, bucket bits, plan targets, compositions)
    "buckets": ("2", 7, (1, 2, 17, 257, 1025, 4000), ("mixed", "tail")),
    "full_sort": ("0", 0, (1, 2, 17, 257, 1025), ("mixed", "tail")),
    "long_run": ("0", 0, (17, 5000), ("tail",)),
    "oversized": ("2", 7, (17, 257, 5000), ("tail",)),
}


@pytest.mark.parametrize("path", list(PATHS))
def test_apply_paths_agree(eng, path, monkeypatch):
    """(g) (f) on each apply path: the 8-byte run against the oracle, once more
    under BJX_CHECK=1 (every sorted outcome written once, the event indices a
    permutation), then the 12- and 16-byte forms."""
    sort2, bucket_bits, targets, comps = PATHS[path]
    monkeypatch.setenv("BJX_SORT2", sort2)
    eng.debug_set_bucket_bits(bucket_bits)
    t0_ms = 1_700_000_000_000
    prime, prime_now, t1_ms = priming(t0_ms)
    pair = Pair(P.RULES_YAML, eng)
    pair.feed(prime, prime_now, want_results=False)
    assert rec_bytes(eng) == 8
    keys = [(ip_of(i), name) for i in range(N_IPS) for name in P.NAMES]
    slots = dict(zip(keys, eng.debug_state_slots([k[0] for k in keys], [k[1] for k in keys]).tolist()))
    pl = P.plan(slots, 15, targets=targets, comps=comps)
    data, now = plan_lines_ms(pl, t1_ms + 2 * P.LONGEST_INTERVAL_US // 1000)
    out = pair.feed(data, now)
    assert out.n_events == pl.n_events
    st = eng.scan_stats()
    assert st["record_bytes"] == 8
    if path == "buckets":
        assert st["grouping"] == 1
    elif path == "oversized":
        assert st["grouping"] == 1 + pl.oversized > 4096
    else:
        assert st["grouping"] == 0 and (path != "long_run" or st["long_runs"] >= 1)
    ips = pl.touched_ips()
    pair.compare_state(ips[::max(1, len(ips) // 100)])
    rs = Ruleset(Config.from_yaml(P.RULES_YAML))
    batches = [(prime, prime_now), (data, now)]
    ref = None
    for hook, check, size in ((None, False, 8), (None, True, 8), ("BJX_REC12", False, 12), ("BJX_REC16", False, 16)):
        for h in ([hook] if hook else []) + (["BJX_CHECK"] if check else []):
            monkeypatch.setenv(h, "1")
        outs, forms, dump = run_stream(eng, rs, batches)
        for h in ("BJX_REC12", "BJX_REC16", "BJX_CHECK"):
            monkeypatch.delenv(h, raising=False)
        assert forms == [size, size], (hook, check)
        if ref is None:
            ref = (outs, dump)
            assert [(t[0], t[1]) for t in outs[1][2]] == [(t.line_idx, t.rule_idx) for t in out.trips]
        else:
            assert (outs, dump) == ref, (hook, check)


def test_node_of_two_engines(eng):
    """(h) two engines on one GPU behind a node: the owners' rate-limit stages
    take the 8-byte form from the records they receive, and the node's trips
    are one engine's."""
    w = W.scaled(W.CFG3, 3 * PER, n_ips=2_000)
    rs = Ruleset(Config.from_yaml(w.rules_yaml))
    node = Node([0, 0])
    want, got, n = [], [], 0
    eng.state_clear()
    for b in range(3):
        data, now = batch(w, b)
        o1 = eng.process(rs, data, now, copy_results=True)
        o2 = node.process(rs, data, now, copy_results=True)
        assert rec_bytes(eng) == 8
        assert [rec_bytes(node.engine(k)) for k in range(2)] == [8, 8]
        want.append([(t.line_idx, t.rule_idx) for t in o1.trips])
        got.append([(t.line_idx, t.rule_idx) for t in o2.trips])
        assert [(r.match_type, r.exceeded, r.seen_ip) for r in o1.results] == \
            [(r.match_type, r.exceeded, r.seen_ip) for r in o2.results]
        n += o1.n_trips
    assert got == want and n > 50
    assert node.state_len() == eng.state_len()
    node.close()
