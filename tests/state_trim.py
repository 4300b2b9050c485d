"""Shared by tests/test_state_trim_cpu.py and tests/test_gpu_state_trim.py (not
collected): the inputs and the expected values of bjx_state_trim.

Expected values: banjax_amd.state_trim -- the trim's pure-Python model -- gives
the cutoff, the bound, the counts and the survivors of a logical state; across
batches the oracle says which (line, rule) pairs are events and the Model of
tests/test_gpu_state_expire.py (Apply restated, plus expire(C)) replays them
with the model's cutoff applied at the same batch boundaries as the engine."""
import random

from oracle import oracle as O

from banjax_amd import Config, Ruleset, state_trim
from tests.parity import oracle_config
from tests.test_gpu_state_expire import CFG, N_BATCH, PER, POOL, Model, _stream  # noqa: F401

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
S = 1_000_000_000
T0 = 1_700_000_000 * S
NAMES = ("fast", "mid", "slow", "a", "")
SPECIAL = (INT64_MIN, INT64_MIN + 1, -1, 0, 1, INT64_MAX - 1)
COUNTS = ("cutoff_ns", "bound", "budget_met", "states_before", "states_dropped", "states_dropped_live", "ips_before",
          "ips_dropped", "arena_bytes_before", "arena_bytes_after")


def sample(seed=1, n_ips=600):
    """About 600 IPs (short and long text) and 1,500 states: half of the starts
    on 64 tied values one second apart, 30 % spread over 2^40 ns, 10 % negative
    down to -2^62, 10 % from SPECIAL.  -> (ips_in_order, states)"""
    rng = random.Random(seed)
    ips = ["10.7.%d.%d" % (k >> 8, k & 255) if k % 3 else "2001:db8:85a3:%x:0:8a2e:370:%x" % (k, 0x7000 + k)
           for k in range(n_ips)]
    rng.shuffle(ips)

    def start():
        r = rng.random()
        if r < 0.5:
            return T0 + rng.randrange(64) * S
        if r < 0.8:
            return T0 + rng.randrange(1 << 40)
        if r < 0.9:
            return -rng.randrange(1, (1 << 62) + 1)
        return rng.choice(SPECIAL)

    states = {ip: {n: (rng.randrange(0, 9), start()) for n in rng.sample(NAMES, rng.choice((1, 2, 2, 3, 3, 4)))}
              for ip in ips}
    return ips, states


def all_starts(states):
    return [s[1] for d in states.values() for s in d.values()]


def budgets(states, n=200, seed=7):
    """Seeded budgets: max_states and max_ips each 0 with probability 1/4, else
    uniform in [1, count + 20); the floor INT64_MIN or an existing start +- 1,
    clamped to int64.  -> [{max_states, max_ips, floor_cutoff_ns}]"""
    rng = random.Random(seed)
    starts = sorted(set(all_starts(states)))
    n_st, n_ips = len(all_starts(states)), sum(1 for d in states.values() if d)
    out = []
    for _ in range(n):
        floor = INT64_MIN
        if rng.random() < 0.5:
            floor = min(INT64_MAX, max(INT64_MIN, rng.choice(starts) + rng.choice((-1, 1))))
        out.append({"max_states": 0 if rng.random() < 0.25 else rng.randrange(1, n_st + 20),
                    "max_ips": 0 if rng.random() < 0.25 else rng.randrange(1, n_ips + 20),
                    "floor_cutoff_ns": floor})
    return out


def real_subset(expected, per_bound=5):
    """indices of about 20 budgets for the real trim: some of each bound, no-ops among them"""
    pick, seen = [], {}
    for k, st in enumerate(expected):
        if seen.get(st["bound"], 0) < per_bound:
            seen[st["bound"]] = seen.get(st["bound"], 0) + 1
            pick.append(k)
    return pick


def byte_starts(d, n=300, seed=3):
    """n starts that differ only in byte d (byte 7: negative and positive values)"""
    rng = random.Random(seed + d)
    base = 0x0102030405060708 & ~(0xFF << (8 * d))
    vals = [rng.randrange(256) for _ in range(n)]
    out = []
    for v in vals:
        u = base | (v << (8 * d))
        out.append(u - (1 << 64) if u >= 1 << 63 else u)
    return out


def flat_state(starts, names=("r",)):
    """one IP per start (several names: one IP per group of len(names) starts)"""
    ips, states = [], {}
    for k in range(0, len(starts), len(names)):
        ip = "10.9.%d.%d" % (k >> 8, k & 255)
        ips.append(ip)
        states[ip] = {n: (1, s) for n, s in zip(names, starts[k:k + len(names)])}
    return ips, states


# ---- across batches: the expiry test's stream with a trim at each boundary
TRIM_BUDGETS = ({"max_states": 300}, {"max_ips": 90}, {"max_states": 400, "max_ips": 150})


class Run:
    """One config (default: the expiry test's) over the oracle and the expiry
    test's Model, and over an engine when one is given; trim() applies the
    model's cutoff to the Model."""

    def __init__(self, target=None, cfg_yaml=CFG):
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
        self.diff_first = self.diff_seen = 0  # events the model answers differently from the never-forgetting oracle

    def feed(self, data, now_ns):
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
        if self.t is None:
            return None
        out = self.t.process(self.rs, data, now_ns, copy_results=True)
        got = [(r.line_idx, r.rule_idx, r.seen_ip, r.match_type, r.exceeded) for r in out.results]
        assert got == want
        assert [(t.line_idx, t.rule_idx) for t in out.trips] == [(w[0], w[1]) for w in want if w[4]]
        return out

    def trim(self, floor_cutoff_ns=INT64_MIN, **budget):
        """-> the model's stats; with a target its stats must equal them"""
        ips = list(self.model.st)
        states = {ip: {n: tuple(v) for n, v in d.items()} for ip, d in self.model.st.items()}
        _, _, want = state_trim.trim(ips, states, floor_cutoff_ns=floor_cutoff_ns, **budget)
        self.model.expire(want["cutoff_ns"])
        if self.t is not None:
            got = self.t.state_trim(floor_cutoff_ns=floor_cutoff_ns, **budget)
            assert {k: got[k] for k in COUNTS} == want, (got, want)
        return want


def stream_run(target=None):
    """-> (run, the stats of the trims): a trim after each of the first three
    batches, the floor at the batch's start (every state dropped above it is live)"""
    run, done = Run(target), []
    for b, (data, now) in enumerate(_stream()):
        run.feed(data, now)
        if b < N_BATCH - 1:
            done.append(run.trim(floor_cutoff_ns=now, **TRIM_BUDGETS[b]))
            if target is not None:
                assert target.state_dump() == run.model.dump()
    if target is not None:
        assert target.state_dump() == run.model.dump()
    return run, done
