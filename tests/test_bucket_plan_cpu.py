"""tests/bucket_plan.py against itself, on synthetic slot maps (no GPU): the
events per bucket and the run lengths recomputed from the emitted lines equal
the plan, for every composition; the lines are interleaved, partly
non-monotone and inside the OldLine bound; and a table filled as the GPU
test's is yields the buckets its L = 15 cases assert."""
import random

import pytest

from tests import bucket_plan as P

SLOTS = 1 << 22
T0_US = 1_700_000_000_000_000


def slot_map(n_states, seed, buckets=None, L=None):
    """n_states states on distinct random slots of a 2^22-slot table (of the
    given buckets of 2^L slots only, when asked)."""
    rnd = random.Random(seed)
    if buckets is None:
        used = rnd.sample(range(SLOTS), n_states)
    else:
        per = n_states // len(buckets)
        used = [(b << L) | s for b in buckets for s in rnd.sample(range(1 << L), per)]
    return {("10.%d.%d.%d" % (k >> 16, (k >> 8) & 255, k & 255), P.NAMES[k % 3]): s for k, s in enumerate(used)}


@pytest.fixture(scope="module")
def sparse():
    return slot_map(60_000, 1)


@pytest.fixture(scope="module")
def dense15():
    """80 of the 128 buckets of L = 15 at the GPU test's load (525,000 states
    in 2^22 slots: ~4,100 per bucket), the last bucket among them."""
    buckets = list(range(1, 80)) + [127]
    return slot_map(80 * 4102, 2, buckets, 15)


@pytest.mark.parametrize("comp", P.COMPOSITIONS)
@pytest.mark.parametrize("m", [1, 2, 3, 20, 153, 2048, 4096, 6000])
def test_run_lengths(comp, m):
    for n in P.TARGETS:
        lens = P.run_lengths(comp, n, m)
        assert sum(lens) == n and 1 <= len(lens) <= m and min(lens) >= 1, (comp, n, m)
        if comp == "flat":
            assert len(lens) == min(n, m) and max(lens) - min(lens) <= 1
            assert m < n or lens == [1] * n
        elif comp == "pairs":
            if m >= (n + 1) // 2:
                assert lens == [2] * (n // 2) + [1] * (n % 2)
            else:
                assert lens == P.run_lengths("flat", n, m)
        elif comp == "mixed":
            cyc = [P.MIXED[i % len(P.MIXED)] for i in range(len(lens))]
            assert lens[:-1] == cyc[:len(lens) - 1]
            assert lens[-1] <= cyc[-1] or len(lens) == m
        else:
            k = len(lens) - 1
            assert lens == [n - k] + [1] * k and k == min(m - 1, n // 2)


def check(pl, slots, L):
    data, now_ns = pl.lines(T0_US)
    events, runs = P.recount(data, slots, L)
    assert events == pl.events and runs == pl.runs
    assert len(pl.events) == len(pl.jobs)  # a bucket per job
    assert pl.n_events == data.count(b"\n") == sum(pl.events.values())
    for b, n, comp, rr in pl.jobs:
        assert all(slot >> L == b and slots[(ip, name)] == slot for ip, name, slot, _ in rr)
        assert len(set(slot for _, _, slot, _ in rr)) == len(rr)
    return data, now_ns


@pytest.mark.parametrize("L", [6, 9, 12])
def test_plan_matches_lines_sparse(sparse, L):
    pl = P.plan(sparse, L)
    assert sorted(n for _, n, _, _ in pl.jobs) == sorted(P.TARGETS * 4)
    assert [c for _, _, c, _ in pl.jobs].count("mixed") == len(P.TARGETS)
    assert pl.oversized == 4 * (4097 + 5000)
    check(pl, sparse, L)


def test_plan_matches_lines_dense(dense15):
    pl = P.plan(dense15, 15)
    check(pl, dense15, 15)
    by = {(n, c): rr for _, n, c, rr in pl.jobs}
    assert [r[3] for r in by[(4096, "flat")]] == [1] * 4096
    assert [r[3] for r in by[(4096, "pairs")]] == [2] * 2048
    lens = [r[3] for r in by[(4081, "mixed")]]
    assert min(lens) < 8 and any(8 <= k < 16 for k in lens) and max(lens) >= 16
    assert [r[3] for r in by[(4095, "tail")]] == [2048] + [1] * 2047


def test_extra_exclude_and_padding(sparse):
    L = 6
    nb = SLOTS >> L
    known = P.buckets_of(sparse, L)
    last = max(known)
    ones = [b for b, st in known.items() if st[0][0] & 63 == 63]
    assert ones
    for mod, rem in ((4, 0), (4, 1), (4, 2), (4, 3), (256, 0), (1024, 0)):
        pl = P.plan(sparse, L, targets=(1, 2, 17, 257), comps=("flat", "mixed"), extra=[(last, 3, "flat"), (ones[0], 2, "tail")],
                    pad=(mod, rem), known=known)
        assert pl.n_events % mod == rem and pl.events[last] == 3 and pl.events[ones[0]] == 2
        assert len(pl.jobs) == 8 + 2 + 1
        check(pl, sparse, L)
        # the state whose low bits are all ones is used first
        assert [r for b, _, _, rr in pl.jobs if b == ones[0] for r in rr][0][2] & 63 == 63
        top = [b for b in known if b >= nb - 4096]
        pl = P.plan(sparse, L, targets=(1, 2, 17, 257), comps=("flat",), exclude=top, pad=(mod, rem), known=known)
        assert pl.n_events % mod == rem and not set(pl.events) & set(top) and max(pl.events) < nb - 4096
        check(pl, sparse, L)


def test_lines_interleaved_and_partly_backwards(sparse):
    pl = P.plan(sparse, 12, targets=(17, 300, 1025))
    data, now_ns = pl.lines(T0_US)
    rows = [l.split(" ") for l in data.decode().splitlines()]
    n_runs = sum(len(rr) for _, _, _, rr in pl.jobs)
    # round robin: the first lines are one per run
    assert len(set((w[1], P.NAME_OF_TOKEN[w[5][1:]]) for w in rows[:n_runs])) == n_runs
    seq = {}
    for w in rows:
        assert len(w) == 7  # "ts ip" and five more words: no ban-log line (it needs six)
        sec, us = w[0].split(".")
        t = int(sec) * 1_000_000 + int(us)
        assert 0 <= now_ns // 1000 - t < 10_000_000
        seq.setdefault((w[1], P.NAME_OF_TOKEN[w[5][1:]]), []).append((t, w[5][1:]))
    back = sum(1 for v in seq.values() if [t for t, _ in v] != sorted(t for t, _ in v))
    long_runs = sum(1 for v in seq.values() if len(v) >= 2)
    assert long_runs // 3 - 1 <= back <= long_runs // 3 + 1 and back > 0
    # runs on a "b" state of more than five events use both of its rules
    assert all(len(set(k for _, k in v)) == 2 for (ip, name), v in seq.items() if name == "b" and len(v) > 5)
    assert all(len(set(k for _, k in v)) == 1 for (ip, name), v in seq.items() if name != "b")
