"""Planner for tests/test_gpu_bucket_shapes.py, in plain Python: from the
state-table slot of every known (ip, rule name) state it builds one batch of
log lines that puts an exact number of rate-limit events, in runs of exact
lengths, into chosen buckets of the two-level grouping (k_bucket_apply: one
block per bucket of 2^L state slots, bucket = slot >> L; a run is the events
of one state, i.e. of one slot).

Every line matches exactly one rule of RULES_YAML (it carries one token), so
it produces exactly one event, on the state (its ip, that rule's name): the
events per bucket and per run are decided here and nowhere else.  The two
rules named "b" share a state and differ in hits_per_interval, so a run on a
"b" state mixes rules and the wave-per-run chunks holding both take the
event-by-event path.  The limits are 0, 2, 3, -1: Exceeded resets many times
inside a run.

tests/test_bucket_plan_cpu.py checks the planner against itself: the counts
recomputed from the emitted lines equal the plan."""
from __future__ import annotations

from collections import Counter

RULES_YAML = """
regexes_with_rates:
  - rule: "a"
    regex: 'AAA'
    interval: 0.2
    hits_per_interval: 0
    decision: challenge
  - rule: "b"
    regex: 'BBB'
    interval: 0.3
    hits_per_interval: 2
    decision: challenge
  - rule: "b"
    regex: 'CCC'
    interval: 0.3
    hits_per_interval: 3
    decision: nginx_block
  - rule: "d"
    regex: 'DDD'
    interval: 0.7
    hits_per_interval: -1
    decision: challenge
expiring_decision_ttl_seconds: 10
"""
NAMES = ("a", "b", "d")
TOKENS = {"a": ("AAA",), "b": ("BBB", "CCC"), "d": ("DDD",)}
NAME_OF_TOKEN = {t: n for n, ts in TOKENS.items() for t in ts}
LONGEST_INTERVAL_US = 700_000

CAP = 4096  # k_bucket_apply's events per bucket; more go the oversized way
TARGETS = (1, 2, 15, 16, 17, 255, 256, 257, 1023, 1024, 1025, 4079, 4080, 4081, 4095, 4096, 4097, 5000)
COMPOSITIONS = ("flat", "pairs", "mixed", "tail")
MIXED = (1, 2, 7, 8, 9, 15, 16, 17, 63, 64, 65, 129)

STEP_US = 20        # between consecutive lines of a batch
BACK_US = 5_000_000  # how far back the non-monotone events lie (OldLine is 10 s)


def run_lengths(comp, n, m):
    """The run lengths of a bucket with m known states and n events: at most
    m runs, each >= 1, summing to n."""
    assert n >= 1 and m >= 1
    if comp == "pairs" and m >= (n + 1) // 2:
        return [2] * (n // 2) + [1] * (n % 2)
    if comp == "mixed":
        lens, left = [], n
        while left and len(lens) < m - 1:
            k = min(MIXED[len(lens) % len(MIXED)], left)
            lens.append(k)
            left -= k
        if left:
            lens.append(left)
        return lens
    if comp == "tail":
        k = min(m - 1, n // 2)
        return [n - k] + [1] * k
    assert comp in ("flat", "pairs"), comp
    k = min(n, m)
    return [n // k + (1 if i < n % k else 0) for i in range(k)]


def want_states(comp, n):
    """How many states the composition would like for n events."""
    if comp == "flat":
        return min(n, CAP)
    if comp == "pairs":
        return (n + 1) // 2
    if comp == "tail":
        return n // 2 + 1
    return len(run_lengths("mixed", n, n + 1))


def buckets_of(slots, L):
    """{bucket: [(slot, ip, name)], highest slot first}: a state whose low L
    bits are all ones (its low key equals k_bucket_apply's padding key) is
    used before the others of its bucket."""
    out = {}
    for (ip, name), slot in slots.items():
        if slot >= 0:
            out.setdefault(slot >> L, []).append((slot, ip, name))
    for v in out.values():
        v.sort(reverse=True)
    return out


class Plan:
    """jobs: [(bucket, n, comp, [(ip, name, slot, run length)])], one per
    planned bucket; events: {bucket: n}; runs: {bucket: sorted run lengths}."""

    def __init__(self, L, jobs):
        self.L = L
        self.jobs = jobs
        self.events = {b: n for b, n, _, _ in jobs}
        self.runs = {b: sorted(r[3] for r in runs) for b, _, _, runs in jobs}
        self.n_events = sum(self.events.values())
        self.oversized = sum(n for n in self.events.values() if n > CAP)

    def touched_ips(self):
        seen = {}
        for _, _, _, runs in self.jobs:
            for ip, _, _, _ in runs:
                seen.setdefault(ip, None)
        return list(seen)

    def lines(self, t0_us):
        """-> (the batch's bytes, now_ns).  All runs of the batch take turns,
        one line each, until each has sent its length (rank order within a
        bucket differs from position order); line k is stamped t0 + k *
        STEP_US, and in every third run every event whose index in the run is
        1 mod 3 lies BACK_US earlier.  A "b" state's events alternate between
        its two rules in blocks of five, every other run starting with the
        second rule."""
        runs = []
        for _, _, _, rr in self.jobs:
            runs.extend(rr)
        left = [r[3] for r in runs]
        alive = list(range(len(runs)))
        out, k = [], 0
        while alive:
            nxt = []
            for i in alive:
                ip, name, _, length = runs[i]
                j = length - left[i]
                t = t0_us + k * STEP_US
                if i % 3 == 2 and j % 3 == 1:
                    t -= BACK_US
                toks = TOKENS[name]
                tok = toks[(j // 5 + i) % len(toks)]
                out.append("%d.%06d %s GET h.com GET /%s HTTP/1.1" % (t // 1_000_000, t % 1_000_000, ip, tok))
                k += 1
                left[i] -= 1
                if left[i]:
                    nxt.append(i)
            alive = nxt
        assert k * STEP_US + BACK_US < 10_000_000, "the batch would reach the OldLine bound"
        return ("\n".join(out) + "\n").encode(), (t0_us + k * STEP_US) * 1000


def plan(slots, L, targets=TARGETS, comps=COMPOSITIONS, extra=(), exclude=(), pad=None, known=None):
    """slots: {(ip, name): state-table slot}.  Every (target, composition) gets
    a bucket of its own: the jobs that want the most states take the buckets
    with the most known states.  extra: [(bucket, n, comp)] placed where they
    say; exclude: buckets left empty; pad = (mod, rem): one more "flat" bucket
    sized so that the batch's events are rem modulo mod; known: buckets_of(slots,
    L), when the caller has it already."""
    if known is None:
        known = buckets_of(slots, L)
    taken = set(exclude)
    jobs = []

    def add(b, n, comp):
        assert b not in taken and b in known, (b, n, comp)
        taken.add(b)
        st = known[b]
        lens = run_lengths(comp, n, len(st))
        jobs.append((b, n, comp, [(ip, name, slot, k) for (slot, ip, name), k in zip(st, lens)]))

    for b, n, comp in extra:
        add(b, n, comp)
    free = sorted((b for b in known if b not in taken), key=lambda b: (-len(known[b]), b))
    auto = sorted(((n, c) for n in targets for c in comps), key=lambda j: (-want_states(j[1], j[0]), j[0], j[1]))
    assert len(auto) + (1 if pad else 0) <= len(free), "not enough buckets with a known state"
    for (n, comp), b in zip(auto, free):
        add(b, n, comp)
    if pad:
        mod, rem = pad
        total = sum(n for _, n, _, _ in jobs)
        add(free[len(auto)], (rem - total - 1) % mod + 1, "flat")
    return Plan(L, jobs)


def recount(data, slots, L):
    """({bucket: events}, {bucket: sorted run lengths}) of a batch's lines,
    from the lines alone: each line's ip and token name its state."""
    per_state = Counter()
    for line in data.decode().splitlines():
        w = line.split(" ")
        per_state[(w[1], NAME_OF_TOKEN[w[5][1:]])] += 1
    events, runs = Counter(), {}
    for key, k in per_state.items():
        b = slots[key] >> L
        events[b] += k
        runs.setdefault(b, []).append(k)
    return dict(events), {b: sorted(v) for b, v in runs.items()}
