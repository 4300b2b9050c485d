"""Per-rule statistics of a batch (BJX_RULE_STATS: bjx_batch_rule_stats,
bjx_rule_stats_total, bjx_rule_stats_reset and their node calls).

The expected rows are always banjax_amd.rule_stats.count over the ORACLE's
RuleResults for the same bytes (oracle.State().consume, as tests/parity.py's
Pair.feed runs it), never anything the engine returned: matches, SkipHost
matches and trips per ruleset rule index.  Compared exactly; there is no
tolerance in a count.
"""
import functools

import numpy as np
import pytest

import workloads as W
from banjax_amd import CHALLENGE, NGINX_BLOCK, Config, Engine, MockBanner, Node, RegexRateLimiter, RegexWithRate, Ruleset, _lib
from banjax_amd import rule_stats as RS
from oracle import oracle as O
from tests import wide_scopes as WS
from tests.parity import oracle_config
from tests.test_gpu_parity import TEST_CONSUME_LINE_CFG

pytestmark = pytest.mark.gpu
FIELDS = ("matches", "skip_host", "trips")
UA = "AppleWebKit/537.36 (KHTML, like Gecko) Chrome/51.0.2704.103 Safari/537.36 -"


@pytest.fixture(scope="module")
def engine():
    e = Engine()
    yield e
    e.close()


@pytest.fixture(params=[0, 1], ids=["lds", "global"])
def bins(request, engine):
    """Both homes of the bins: LDS (the default), and straight into the global
    counters, which any ruleset of two or more rules reaches with the LDS path
    limited to rulesets of one rule (bjx_debug_set_rule_stats_lds).  Yields the
    path the test must find in engine.debug_rule_stats_path() after a batch
    with results."""
    engine.debug_set_rule_stats_lds(request.param)
    yield "global" if request.param else "lds"
    engine.debug_set_rule_stats_lds(0)


class Model:
    """The oracle side: one state fed the same batches, its RuleResults counted by the model."""

    def __init__(self, cfg: Config):
        self.cfg, self.ocfg, self.st = cfg, oracle_config(cfg), O.State()
        self.n_rules = len(cfg.all_rules())
        self.last = None

    def feed(self, data: bytes, now_ns: int):
        _, self.last, _ = self.st.consume(self.ocfg, data, now_ns, cap=(data.count(b"\n") + 1) * (self.n_rules + 1))
        return RS.as_rows(*RS.count(self.last, self.n_rules))


def same(got, want):
    assert got.dtype.names == FIELDS and len(got) == len(want), (got.dtype, len(got), len(want))
    for f in FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert len(bad) == 0, (f, bad[:10], got[f][bad[:10]], want[f][bad[:10]])


def add(a, b):
    out = a.copy()
    for f in FIELDS:
        out[f] += b[f]
    return out


def check_sums(out, rows):
    """What the library checks itself: the rows add up to the batch's own counts."""
    assert int(rows["matches"].sum()) == out.n_results
    assert int(rows["matches"].sum() - rows["skip_host"].sum()) == out.n_events
    assert int(rows["trips"].sum()) == out.n_trips


def limiter(cfg_yaml, engine):
    engine.state_clear()
    engine.rule_stats_reset()
    cfg = Config.from_yaml(cfg_yaml)
    return cfg, RegexRateLimiter(cfg, engine=engine, banner=MockBanner())


# ---- 1. the reference's sequences

def consume_line_lines():
    """The seven lines of regex_rate_limiter_test.go TestConsumeLine (tests/test_gpu_parity.py)."""
    t0 = 1700000000.123456
    get = " 1.2.3.4 GET example.com GET /whatever HTTP/1.1 " + UA
    post = " 1.2.3.4 POST example.com POST /whatever HTTP/1.1 " + UA
    lines = ["%f" % t0 + get, "%f" % (t0 + 4) + get, "%f" % (t0 + 5.5) + get, "%f" % (t0 + 6.5) + post,
             "%f" % (t0 + 7.0) + post,
             "%f 1.6.6.6 GET per-site.com GET /blockme/?a HTTP/1.1 %s" % (t0 + 20, UA),
             "%f 1.6.6.7 GET no-per-site.com GET /blockme/?a HTTP/1.1 %s" % (t0 + 22, UA)]
    return [ln.encode() + b"\n" for ln in lines], int(t0 * 1e9)


def test_reference_sequence_one_batch(engine):
    lines, now = consume_line_lines()
    cfg, lim = limiter(TEST_CONSUME_LINE_CFG, engine)
    want = Model(cfg).feed(b"".join(lines), now)
    _, out = lim.consume_lines(b"".join(lines), now, rule_stats=True)
    st = engine.rule_stats()
    same(st["rules"], want)
    check_sums(out, st["rules"])
    assert (st["n_batches"], st["n_lines"]) == (1, 7)
    # rule indices: the two global rules, then per-site.com's; its line is counted there, and trips at once
    assert [r.rule for r in cfg.all_rules()] == ["rule1", "rule2", "instant block"]
    assert tuple(int(st["rules"][2][f]) for f in FIELDS) == (1, 0, 1)
    assert tuple(int(st["rules"][0][f]) for f in FIELDS) == (3, 0, 0)
    assert tuple(int(st["rules"][1][f]) for f in FIELDS) == (2, 0, 1)
    tot = engine.rule_stats(total=True)
    same(tot["rules"], want)
    assert (tot["n_batches"], tot["n_lines"]) == (1, 7)
    assert lim.rule_stats() == {"rule1": {"matches": 3, "skip_host": 0, "events": 3, "trips": 0},
                                "rule2": {"matches": 2, "skip_host": 0, "events": 2, "trips": 1},
                                "instant block": {"matches": 1, "skip_host": 0, "events": 1, "trips": 1}}


def test_reference_sequence_seven_batches(engine):
    lines, now = consume_line_lines()
    cfg, lim = limiter(TEST_CONSUME_LINE_CFG, engine)
    model = Model(cfg)
    total = RS.as_rows(*RS.count([], model.n_rules))
    for k, ln in enumerate(lines):
        want = model.feed(ln, now)
        _, out = lim.consume_lines(ln, now, want_results=bool(k & 1), rule_stats=True)
        st = engine.rule_stats()
        same(st["rules"], want)
        check_sums(out, st["rules"])
        assert (st["n_batches"], st["n_lines"]) == (1, 1)
        total = add(total, want)
        tot = engine.rule_stats(total=True)
        same(tot["rules"], total)
        assert (tot["n_batches"], tot["n_lines"]) == (k + 1, k + 1)
        assert tot["device_ms"] >= st["device_ms"] >= 0
    assert engine.rule_stats(total=True)["n_batches"] == 7
    assert int(total["matches"][2]) == 1  # the per-site.com line, under the per-site rule's index


# ---- 2. SkipHost only

SKIP_CFG = r"""
regexes_with_rates:
  - decision: nginx_block
    rule: 'rule1'
    regex: '%s'
    interval: 5
    hits_per_interval: 2
    hosts_to_skip:
      skiphost.com: true
"""
# TestConsumeLineHostsToSkip's own regex is anchored at the start of rest, where the method
# and the host stand ("GET skiphost.com GET http://x ..."), so no line of skiphost.com can
# match it: that config gives zero rows (checked below).  The same rule without the anchor
# is what a skiphost.com line can match.
SKIP_REGEX_REFERENCE = r"^GET https?:\/\/\.*"
SKIP_REGEX = r"GET https?:\/\/\.*"


def test_skip_host_only(engine):
    t = 1700000000.5
    now = int(t * 1e9)
    skip = b"".join(b"%f 1.2.3.%d GET skiphost.com GET http://x HTTP/1.1 x\n" % (t, k % 5) for k in range(300))
    cfg, lim = limiter(SKIP_CFG % SKIP_REGEX_REFERENCE, engine)
    want = Model(cfg).feed(skip, now)
    _, out = lim.consume_lines(skip, now, want_results=False, rule_stats=True)
    assert out.n_results == 0 and int(want["matches"].sum()) == 0
    same(engine.rule_stats()["rules"], want)

    cfg, lim = limiter(SKIP_CFG % SKIP_REGEX, engine)
    model = Model(cfg)
    want = model.feed(skip, now)
    _, out = lim.consume_lines(skip, now, want_results=False, rule_stats=True)
    st = engine.rule_stats()
    assert out.n_results == 300 and out.n_events == 0 and out.n_trips == 0
    same(st["rules"], want)
    assert int(st["rules"]["matches"][0]) == int(st["rules"]["skip_host"][0]) == 300 and int(st["rules"]["trips"][0]) == 0
    assert engine.state_len() == 0  # nothing reached Apply

    mixed = b"".join(b"%f 1.2.3.%d GET %s GET http://x HTTP/1.1 x\n" % (t, k % 5, b"skiphost.com" if k % 3 else b"other.com")
                     for k in range(301))
    want2 = model.feed(mixed, now)
    _, out = lim.consume_lines(mixed, now, want_results=True, rule_stats=True)
    st = engine.rule_stats()
    same(st["rules"], want2)
    check_sums(out, st["rules"])
    assert 0 < int(want2["skip_host"][0]) < int(want2["matches"][0]) and int(want2["trips"][0]) > 0
    same(engine.rule_stats(total=True)["rules"], add(want, want2))


# ---- 3. no results, empty input, no flag

def test_no_results_and_empty_input(engine):
    _, now = consume_line_lines()
    cfg, lim = limiter(TEST_CONSUME_LINE_CFG, engine)
    zeros = RS.as_rows(*RS.count([], 3))
    nothing = b"".join(b"%f 9.9.9.%d PUT other.com PUT /x HTTP/1.1 x\n" % (now / 1e9, k) for k in range(40))
    want = Model(cfg).feed(nothing, now)
    same(want, zeros)
    _, out = lim.consume_lines(nothing, now, want_results=False, rule_stats=True)
    assert out.n_lines == 40 and out.n_results == 0
    assert engine.debug_rule_stats_path() == "none"  # nothing to count, nothing launched
    st = engine.rule_stats()
    same(st["rules"], zeros)
    assert (st["n_batches"], st["n_lines"]) == (1, 40)
    for data in (b"", b"no newline yet"):
        out = engine.process(lim.ruleset, data, now, rule_stats=True)
        assert out.n_lines == 0
        st = engine.rule_stats()
        same(st["rules"], zeros)
        assert (st["n_batches"], st["n_lines"]) == (1, 0)
    tot = engine.rule_stats(total=True)
    same(tot["rules"], zeros)
    assert (tot["n_batches"], tot["n_lines"]) == (3, 40)
    engine.process(lim.ruleset, nothing, now)
    with pytest.raises(_lib.BanjaxGpuError) as ei:
        engine.rule_stats()
    assert ei.value.code == _lib.ERR_ARG and "BJX_RULE_STATS" in str(ei.value)
    assert engine.rule_stats(total=True)["n_batches"] == 3  # the unflagged batch changed nothing


# ---- 4. one bin, many lanes

ONE_RULE = """
regexes_with_rates:
  - {rule: everything, regex: '.*', interval: 30, hits_per_interval: 0, decision: nginx_block}
"""
# A ruleset of one rule is within any LDS limit the hook can set (1 <= 1), so the runs on the
# global counters get a second rule that no line matches: the one bin that counts is the same.
ONE_RULE_AND_A_DEAD_ONE = ONE_RULE + \
    "  - {rule: never, regex: 'no line holds this', interval: 30, hits_per_interval: 0, decision: nginx_block}\n"


@functools.lru_cache(maxsize=None)
def one_rule_case(n_lines, n_ips, cfg_yaml):
    t = 1700000000
    data = b"".join(b"%d.%06d 10.0.0.%d GET h.example.com GET /p%d HTTP/1.1 ua\n" % (t, k % 1000000, k % n_ips, k)
                    for k in range(n_lines))
    cfg = Config.from_yaml(cfg_yaml)
    return data, t * 10 ** 9, Model(cfg).feed(data, t * 10 ** 9)


@pytest.mark.parametrize("n_lines,n_ips", [(256 * 3 + 37, 1), (70_000, 3)])
def test_one_bin_many_lanes(engine, bins, n_lines, n_ips):
    """Every lane of every wave hits the same bin, twice: the `.*` rule matches every line and,
    with hits_per_interval 0, every event trips.  More than one block and a partial last wave;
    then many blocks and a grid-stride tail."""
    cfg_yaml = ONE_RULE if bins == "lds" else ONE_RULE_AND_A_DEAD_ONE
    data, now, want = one_rule_case(n_lines, n_ips, cfg_yaml)
    cfg, lim = limiter(cfg_yaml, engine)
    _, out = lim.consume_lines(data, now, want_results=False, rule_stats=True)
    assert engine.debug_rule_stats_path() == bins
    st = engine.rule_stats()
    same(st["rules"], want)
    assert len(st["rules"]) == (1 if bins == "lds" else 2)
    assert tuple(int(st["rules"][0][f]) for f in FIELDS) == (n_lines, 0, n_lines)
    assert out.n_trips == n_lines and st["n_lines"] == n_lines


# ---- 5. workload shapes

@functools.lru_cache(maxsize=None)
def workload_case(name, n_lines):
    w = W.scaled(W.ALL[name], n_lines, n_ips=min(W.ALL[name].n_ips, n_lines // 3 + 1))
    cfg = Config.from_yaml(w.rules_yaml)
    model = Model(cfg)
    per = (n_lines + 1) // 2
    batches = []
    for first in (0, per):
        data, now = w.host_lines(first, min(per, n_lines - first)), w.now_ns(first, min(per, n_lines - first))
        batches.append((data, now, model.feed(data, now)))
    return w.rules_yaml, batches


@pytest.mark.parametrize("name,n_lines", [("cfg3", 20_000), ("cfg2", 20_000), ("cfg5", 20_000), ("cfg4", 1_500)])
def test_workload_shapes(engine, name, n_lines):
    """Two batches, with RuleResult copies and trips-only on a fresh state: the same rows, the
    oracle's; and the flag changes nothing else a batch returns or leaves in the state."""
    rules_yaml, batches = workload_case(name, n_lines)
    runs = {}
    for run, (copy, flag) in {"copy": (True, True), "trips": (False, True), "plain": (False, False)}.items():
        cfg, lim = limiter(rules_yaml, engine)
        seen = []
        for data, now, want in batches:
            _, out = lim.consume_lines(data, now, want_results=copy, rule_stats=flag)
            rows = engine.rule_stats()["rules"] if flag else None
            if flag:
                same(rows, want)
                check_sums(out, rows)
            seen.append((out.n_lines, out.n_results, out.n_events, [(t.line_idx, t.rule_idx) for t in out.trips], rows))
        if flag:
            tot = engine.rule_stats(total=True)
            same(tot["rules"], add(batches[0][2], batches[1][2]))
            assert tot["n_batches"] == 2 and tot["n_lines"] == sum(s[0] for s in seen)
        runs[run] = (seen, engine.state_dump())
    assert sum(int(b[2]["trips"].sum()) for b in batches) > 0 and sum(int(b[2]["matches"].sum()) for b in batches) > 0
    for run in ("copy", "trips"):
        assert [s[:4] for s in runs[run][0]] == [s[:4] for s in runs["plain"][0]], run
        assert runs[run][1] == runs["plain"][1], run
    for a, b in zip(runs["copy"][0], runs["trips"][0]):
        same(a[4], b[4])


# ---- 6. scopes past 128 positions

@functools.lru_cache(maxsize=None)
def wide_case(kind):
    b = WS.batch(kind, 1)
    cfg = Config.from_yaml(WS.rules_yaml(kind))
    model = Model(cfg)
    want = model.feed(b.data, b.now_ns)
    far = [r for r in model.last if r.rule_pos >= 128]
    return b.data, b.now_ns, want, len(far), sum(1 for r in far if r.skip_host)


@pytest.mark.parametrize("kind", ["MIX", "SITE", "WNFA"])
def test_wide_scopes(engine, bins, kind):
    """Three and more mask words, is_skip past position 127, lines without a host, the
    k_parse_match / decide_wide path and wide-NFA matches added by atomicOr."""
    data, now, want, n_far, n_far_skip = wide_case(kind)
    # without these the test shows nothing: a counted rule at a position >= 128, a SkipHost count
    assert n_far > 0 and int(want["skip_host"].sum()) > 0, (n_far, int(want["skip_host"].sum()))
    cfg, lim = limiter(WS.rules_yaml(kind), engine)
    _, out = lim.consume_lines(data, now, want_results=False, rule_stats=True)
    assert engine.debug_rule_stats_path() == bins
    st = engine.rule_stats()
    same(st["rules"], want)
    check_sums(out, st["rules"])
    cfg, lim = limiter(WS.rules_yaml(kind), engine)
    _, out = lim.consume_lines(data, now, want_results=True, rule_stats=True)
    assert engine.debug_rule_stats_path() == bins
    same(engine.rule_stats()["rules"], want)


def test_wide_scopes_skip_past_127():
    """is_skip's own ground: some batch has a SkipHost RuleResult at a position >= 128."""
    assert any(wide_case(kind)[4] > 0 for kind in ("MIX", "SITE", "WNFA"))


# ---- 7b. bins past the 64 KB of dynamic LDS a kernel has by default

@functools.lru_cache(maxsize=None)
def many_rules_case():
    """8,301 rules, 66,408 B of bins: one global rule and 83 hosts x 100 site rules (a line's
    scope stays at 101 positions, so the oracle and the line kernel stay quick)."""
    hosts, per = 83, 100
    cfg = Config()
    cfg.regexes_with_rates = [RegexWithRate("everything", ".*", 30 * 10 ** 9, 5, CHALLENGE)]
    for h in range(hosts):
        cfg.per_site_regexes_with_rates["h%d.example.com" % h] = [
            RegexWithRate("s%d_%d" % (h, k), "GET /p%d/" % k, 10 * 10 ** 9, k % 3, NGINX_BLOCK) for k in range(per)]
    t = 1700000000
    data = b"".join(b"%d.%06d 10.0.%d.%d GET h%d.example.com GET /p%d/x HTTP/1.1 ua\n"
                    % (t, j, j % 7, j % 11, (j * 7) % hosts, (j * 13) % per) for j in range(3000))
    # the last rule of the ruleset: its bins are the last bytes of each plane
    data += b"".join(b"%d.9%05d 10.1.0.%d GET h%d.example.com GET /p%d/x HTTP/1.1 ua\n" % (t, j, j, hosts - 1, per - 1)
                     for j in range(5))
    return cfg, data, t * 10 ** 9, Model(cfg).feed(data, t * 10 ** 9)


def test_bins_past_64k_of_lds(engine):
    """Rulesets of 8,193 to 16,384 rules keep their bins in LDS, which the kernel has to be
    allowed first (hipFuncAttributeMaxDynamicSharedMemorySize); the last rule index sits in
    the last bytes of it."""
    cfg, data, now, want = many_rules_case()
    assert 8 * len(want) > 64 * 1024 and int(want["matches"][-1]) > 0 and int(want["trips"].sum()) > 0
    engine.state_clear()
    engine.rule_stats_reset()
    engine.debug_set_rule_stats_lds(0)
    engine.set_decision_lists([])
    rs = Ruleset(cfg)
    out = engine.process(rs, data, now, rule_stats=True)
    assert engine.debug_rule_stats_path() == "lds"
    st = engine.rule_stats()
    same(st["rules"], want)
    check_sums(out, st["rules"])
    out = engine.process(rs, data, now, rule_stats=True)  # the attribute already raised
    assert engine.debug_rule_stats_path() == "lds"
    check_sums(out, engine.rule_stats()["rules"])


# ---- 8. reload

def test_reload_restarts_totals(engine):
    lines, now = consume_line_lines()
    engine.state_clear()
    engine.rule_stats_reset()
    empty = engine.rule_stats(total=True)
    assert len(empty["rules"]) == 0 and empty["n_batches"] == 0 and empty["n_lines"] == 0
    cfg_a, cfg_b = Config.from_yaml(TEST_CONSUME_LINE_CFG), Config.from_yaml(SKIP_CFG % SKIP_REGEX)
    rs_a, rs_b = Ruleset(cfg_a), Ruleset(cfg_b)
    ma = Model(cfg_a)
    a1, a2 = b"".join(lines[:4]), b"".join(lines[4:])
    w1 = ma.feed(a1, now)
    engine.process(rs_a, a1, now, rule_stats=True)
    engine.process(rs_a, a1, now)  # unflagged, in between: counted nowhere
    ma.feed(a1, now)
    w2 = ma.feed(a2, now)
    engine.process(rs_a, a2, now, copy_results=True, rule_stats=True)
    same(engine.rule_stats()["rules"], w2)
    tot = engine.rule_stats(total=True)
    same(tot["rules"], add(w1, w2))
    assert (tot["n_batches"], tot["n_lines"]) == (2, 7)
    # another ruleset with another rule count: the totals are its batch alone
    t = now / 1e9
    # (other IPs than A's lines: B's rule shares the name rule1, and state is keyed by name)
    data_b = b"".join(b"%f 7.7.7.%d GET %s GET http://x HTTP/1.1 x\n" % (t, k % 5, b"skiphost.com" if k % 2 else b"o.com")
                      for k in range(50))
    engine.process(rs_b, data_b, now)  # unflagged under B: the totals are still A's
    same(engine.rule_stats(total=True)["rules"], add(w1, w2))
    mb = Model(cfg_b)
    mb.feed(data_b, now)
    wb = mb.feed(data_b, now)
    engine.process(rs_b, data_b, now, rule_stats=True)
    tot = engine.rule_stats(total=True)
    same(tot["rules"], wb)
    assert len(tot["rules"]) == 1 and (tot["n_batches"], tot["n_lines"]) == (1, 50)
    # a ruleset compiled anew from the same config is another ruleset
    rs_b2 = Ruleset(cfg_b)
    wb2 = mb.feed(data_b, now)
    engine.process(rs_b2, data_b, now, rule_stats=True)
    tot = engine.rule_stats(total=True)
    same(tot["rules"], wb2)
    assert tot["n_batches"] == 1
    engine.rule_stats_reset()
    tot = engine.rule_stats(total=True)
    assert len(tot["rules"]) == 0 and tot["n_batches"] == 0 and tot["n_lines"] == 0 and tot["device_ms"] == 0
    same(engine.rule_stats()["rules"], wb2)  # the last batch's rows are not the totals


# ---- 9. node

@functools.lru_cache(maxsize=None)
def node_case(name):
    n_lines, per = 6_000, 3_000
    w = W.scaled(W.ALL[name], n_lines, n_ips=2000)
    cfg = Config.from_yaml(w.rules_yaml)
    model = Model(cfg)
    batches = []
    for first in (0, per):
        data, now = w.host_lines(first, per), w.now_ns(first, per)
        batches.append((data, now, model.feed(data, now)))
    return cfg, batches


def _prepare(h, cfg):
    h.set_decision_lists(cfg.decision_entries)
    h.set_ban_options(cfg.expiring_decision_ttl_seconds)


@pytest.mark.parametrize("copy", [True, False], ids=["finish", "finish_trips"])
@pytest.mark.parametrize("n_engines", [2, 3])
@pytest.mark.parametrize("name", ["cfg3", "cfg5"])
def test_node(engine, name, n_engines, copy):
    """Engines sharing GPU 0: bjx_finish_batch (copy) and bjx_finish_batch_trips close the
    batches.  The node's rows are one engine's over the whole batch and the oracle's, and the
    sum of its engines' own rows."""
    cfg, batches = node_case(name)
    rs = Ruleset(cfg)
    node = Node([0] * n_engines)
    _prepare(node, cfg)
    engine.state_clear()
    engine.rule_stats_reset()
    _prepare(engine, cfg)
    total = None
    with pytest.raises(_lib.BanjaxGpuError):
        node.rule_stats()
    assert len(node.rule_stats(total=True)["rules"]) == 0
    for data, now, want in batches:
        out = node.process(rs, data, now, copy_results=copy, rule_stats=True)
        one = engine.process(rs, data, now, copy_results=copy, rule_stats=True)
        st = node.rule_stats()
        same(st["rules"], want)
        same(engine.rule_stats()["rules"], want)
        check_sums(out, st["rules"])
        assert (out.n_results, out.n_events, out.n_trips) == (one.n_results, one.n_events, one.n_trips)
        assert (st["n_batches"], st["n_lines"]) == (1, out.n_lines)
        parts = [node.engine(k).rule_stats() for k in range(n_engines)]
        acc = parts[0]["rules"]
        for p in parts[1:]:
            acc = add(acc, p["rules"])
        same(acc, st["rules"])
        assert sum(p["n_lines"] for p in parts) == out.n_lines
        assert st["device_ms"] == max(p["device_ms"] for p in parts)
        total = want if total is None else add(total, want)
    assert int(total["trips"].sum()) > 0
    tot = node.rule_stats(total=True)
    same(tot["rules"], total)
    same(engine.rule_stats(total=True)["rules"], total)
    assert (tot["n_batches"], tot["n_lines"]) == (2, 6000)
    node.process(rs, batches[0][0], batches[0][1], copy_results=copy)  # unflagged
    with pytest.raises(_lib.BanjaxGpuError):
        node.rule_stats()
    same(node.rule_stats(total=True)["rules"], total)
    node.rule_stats_reset()
    assert len(node.rule_stats(total=True)["rules"]) == 0
    node.close()
