"""Shared by tests/test_state_remove_cpu.py and tests/test_gpu_state_remove.py
(not collected): the inputs and the expected values of bjx_state_remove.

Expected values: the oracle says which (line, rule) pairs are events (its
RuleResults with skip_host == 0, in reference order); a Python restatement of
RegexRateLimitStates.Apply (reference internal/rate_limit.go:37-78) replays
them over a state from which banjax_amd.state_remove.remove -- the removal's
pure-Python model -- takes the selected states at the same batch boundaries as
the engine.  With a target (an Engine or a Node) every RuleResult, the trips,
the stats, state_get and the dump must equal that model; without one (the CPU
tests) the model alone runs, which is how the inputs are shown to be telling."""
import random

from oracle import oracle as O

from banjax_amd import Config, Ruleset, state_remove
from tests.parity import oracle_config

S = 1_000_000_000
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
T0_MS = 1_700_000_000_000
COUNTS = ("states_before", "states_dropped", "ips_before", "ips_dropped", "ips_found", "arena_bytes_before",
          "arena_bytes_after")


class Model:
    """RegexRateLimitStates with removal: {ip: {rule name: [NumHits, IntervalStartTime ns]}},
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

    def snapshot_args(self):
        """(ips_in_order, states) as snapshot.build and state_remove.remove take them"""
        return list(self.st), {ip: {n: tuple(v) for n, v in d.items()} for ip, d in self.st.items()}

    def remove(self, **sel):
        """-> (the model's counts, IPs that lost some but not all states)"""
        before = {ip: len(d) for ip, d in self.st.items()}
        ips, kept, counts = state_remove.remove(*self.snapshot_args(), **sel)
        self.st = {ip.decode(): {n.decode(): list(v) for n, v in kept[ip].items()} for ip in ips}
        partial = sum(1 for ip, d in self.st.items() if len(d) != before[ip])
        return counts, partial

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
    """One config over the oracle and the model, and over an engine or node when one is given."""

    def __init__(self, cfg_yaml, target=None):
        self.cfg = Config.from_yaml(cfg_yaml)
        self.rules = self.cfg.all_rules()
        self.names = sorted(set(r.rule for r in self.rules))
        self.ocfg = oracle_config(self.cfg)
        self.ost = O.State()
        self.model = Model()
        self.t = target
        if target is not None:
            self.rs = Ruleset(self.cfg)
            target.state_clear()
        # events the model answers differently from the oracle, which never forgets
        self.diff_first = self.diff_seen = 0

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

    def feed(self, data, now_ns, targets=None):
        """the batch through the model once and through every target (default: the run's own)"""
        _, want = self.expected(data, now_ns)
        out = None
        for t in ([self.t] if targets is None else targets):
            if t is not None:
                out = self._process(t, data, now_ns, want)
        return out

    def _process(self, target, data, now_ns, want):
        out = target.process(self.rs, data, now_ns, copy_results=True)
        got = [(r.line_idx, r.rule_idx, r.seen_ip, r.match_type, r.exceeded) for r in out.results]
        if got != want:
            bad = next(k for k in range(min(len(got), len(want))) if got[k] != want[k]) if len(got) == len(want) else -1
            raise AssertionError("RuleResults differ (%d vs %d), first at %d: engine %s model %s"
                                 % (len(got), len(want), bad, got[bad] if bad >= 0 else None, want[bad] if bad >= 0 else None))
        assert [(t.line_idx, t.rule_idx) for t in out.trips] == [(w[0], w[1]) for w in want if w[4]]
        return out

    def remove(self, **sel):
        """removal on both sides; the engine's stats must be the model's counts
        -> (the engine's stats, or the counts without a target; partial)"""
        counts, partial = self.model.remove(**sel)
        if self.t is None:
            return counts, partial
        s = self.t.state_remove(**sel)
        assert {k: s[k] for k in COUNTS} == counts, (s, counts)
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
NOT_HELD = ["10.9.9.1", "2001:db8:85a3:ffff:0:8a2e:370:1", ""]


def stream():
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


def selection(b, now_ns):
    """The removal after batch b (0, 1, 2), which started at now_ns.
    0: a list of 40 entries, short and long IPs mixed, three of them not held
       and two given twice
    1: one rule name
    2: min_hits and a start window, restricted to a list"""
    if b == 0:
        held = POOL[5:23] + POOL[-17:]
        lst = held[:20] + NOT_HELD + held[20:] + [held[3], held[-2]]
        assert len(lst) == 40
        return {"ips": lst}
    if b == 1:
        return {"name": "mid"}
    return {"min_hits": 2, "min_start_ns": now_ns + 20 * S, "max_start_ns": now_ns + 95 * S, "ips": POOL[::2] + NOT_HELD[:1]}


def parity_run(target, batches, compare_dump=True):
    """The stream with a removal after each of the first three batches -> (run,
    [(stats or counts, partial)] per removal)."""
    run = Run(CFG, target)
    done = []
    for b, (data, now) in enumerate(batches):
        run.feed(data, now)
        if b < N_BATCH - 1:
            done.append(run.remove(**selection(b, now)))
            if target is not None:
                run.compare_states(dump=compare_dump)
    if target is not None:
        run.compare_states(dump=compare_dump)
    return run, done


def one_rule(interval_s=5, hits=100):
    return """
regexes_with_rates:
  - {rule: "r", regex: 'GET', interval: %d, hits_per_interval: %d, decision: challenge}
expiring_decision_ttl_seconds: 10
""" % (interval_s, hits)


def lines(events):
    """events: (ms since T0_MS, ip)"""
    return ("".join("%d.%03d %s GET h.com GET /x HTTP/1.1 ua\n" % ((T0_MS + ms) // 1000, (T0_MS + ms) % 1000, ip)
                    for ms, ip in events)).encode()


def dump_ips(text):
    return [l[:-1] for l in text.split("\n") if l.endswith(":") and not l.startswith("\t")]


HOT_CFG = """
regexes_with_rates:
  - {rule: "every", regex: '.*', interval: 0.25, hits_per_interval: -1, decision: challenge}
  - {rule: "shared", regex: 'GET', interval: 2, hits_per_interval: 37, decision: challenge}
  - {rule: "shared", regex: 'POST', interval: 2, hits_per_interval: 37, decision: nginx_block}
expiring_decision_ttl_seconds: 10
"""


def hot_lines(t0_ms, n):
    """6.6.6.6 sends nine lines of ten (a k_long_* run); 60 quiet IPs share the rest"""
    out = []
    for k in range(n):
        t = t0_ms + k
        m = "POST" if k % 7 == 0 else "GET"
        ip = "6.6.6.6" if k % 10 else "7.7.%d.%d" % (k % 3, k % 200)
        out.append("%d.%03d %s %s h.com %s /x HTTP/1.1 ua" % (t // 1000, t % 1000, ip, m, m))
    return ("\n".join(out) + "\n").encode()


def hot_quiet_ips():
    return sorted({"7.7.%d.%d" % (k % 3, k % 200) for k in range(0, 30_000, 10)})
