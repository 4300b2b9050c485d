"""k_bucket_apply and k_bucket_bounds at every bucket width L = 6..15 and at
exact bucket sizes, bit-exact against the oracle's sequential
RegexRateLimitStates.Apply (reference internal/rate_limit.go:37-78).

The engine's own tables reach L = 6 only (2^22 slots, 16 bucket bits), and a
test-sized batch leaves its 65,536 buckets nearly empty.  Here
bjx_debug_set_bucket_bits moves the split (bucket bits 16..7 give L = 6..15
with the same 2^22 slots), one priming batch creates ~525,000 states,
bjx_debug_state_slots tells the slot of each, and tests/bucket_plan.py then
writes batches that put 1, 2, 15 ... 4,095, 4,096 (the block's capacity),
4,097 and 5,000 (the oversized way) events into chosen buckets, as singletons,
pairs, mixed run lengths and one long run with a tail of singletons, the
states' lines interleaved and partly 5 s back in time.  A wrong or unstable
rank, a wrong s_ord region or a wrong bucket bound changes MatchType /
Exceeded of some event, which compare_batch sees.

All cases continue on the one primed state (a slot keeps its index until a
rebuild, which every case checks did not happen); after a failed case the
engine and the oracle have diverged, so the rest are skipped.

The fixture (priming 525,000 lines through oracle and engine, one slot
lookup) takes about 6 s, nearly all of it the oracle and the Python Banner
replay of the priming trips; the lookup itself is one launch of a few ms."""
import itertools
import os
import time

import pytest

from banjax_amd import Engine, _lib
from tests import bucket_plan as P
from tests.parity import Pair

pytestmark = pytest.mark.gpu

N_IPS = 175_000
SLOT_BITS = 22
T0_US = 1_700_000_000_000_000
WAVE_RUNS = (None, "0", "2", "16")
BOUNDS_TARGETS = (1, 2, 16, 17, 255, 256, 257, 1023, 1025)
# the batch's events modulo 4, a multiple of 256 that is none of 1,024, a multiple of 1,024
PADS = ((4, 0), (4, 1), (4, 2), (4, 3), (1024, 256), (1024, 0))


def ip_of(k):
    return "10.%d.%d.%d" % (k >> 16, (k >> 8) & 255, k & 255)


class World:
    def __init__(self):
        self.engine = Engine()
        self.pair = Pair(P.RULES_YAML, self.engine)
        self.failed = False
        self.cases = 0
        self._known = (None, None)
        t = time.time()
        rows, k = [], 0
        for i in range(N_IPS):
            ip = ip_of(i)
            for name in P.NAMES:
                us = T0_US + 10 * k
                rows.append("%d.%06d %s GET h.com GET /%s HTTP/1.1" % (us // 1_000_000, us % 1_000_000, ip, P.TOKENS[name][0]))
                k += 1
        self.t_us = T0_US + 10 * k
        self.pair.feed(("\n".join(rows) + "\n").encode(), self.t_us * 1000, want_results=False)
        t1 = time.time()
        keys = [(ip_of(i), name) for i in range(N_IPS) for name in P.NAMES]
        got = self.engine.debug_state_slots([ip for ip, _ in keys], [n for _, n in keys])
        t2 = time.time()
        print("bucket shapes fixture: priming %.2f s, slot lookup of %d states %.2f s" % (t1 - t, len(keys), t2 - t1))
        self.stats = self.engine.state_stats()
        assert self.stats["state_slots"] == 1 << SLOT_BITS and self.stats["states"] == len(keys)
        assert int(got.min()) >= 0 and int(got.max()) < 1 << SLOT_BITS and len(set(got.tolist())) == len(keys)
        self.slots = dict(zip(keys, got.tolist()))

    def known(self, L):
        if self._known[0] != L:
            self._known = (L, P.buckets_of(self.slots, L))
        return self._known[1]

    def ones_bucket(self, L, avoid):
        """A bucket with a state whose low L bits are all ones (the padding
        key), or None."""
        mask = (1 << L) - 1
        for b, st in sorted(self.known(L).items()):
            if st[0][0] & mask == mask and b not in avoid:
                return b
        return None

    def run(self, L, bits=None, **kw):
        """One planned batch for buckets of 2^L slots (bucket bits 22 - L, or
        as given): results, trips, a sample of the states, and the tables not
        rebuilt.  -> (the plan, scan_stats' grouping)."""
        if self.failed:
            pytest.skip("an earlier case failed: the engine's and the oracle's states have diverged")
        self.failed = True
        self.engine.debug_set_bucket_bits(SLOT_BITS - L if bits is None else bits)
        pl = P.plan(self.slots, L, known=self.known(L), **kw)
        # the clock passes the longest interval before every other case: stored windows Outside and Inside
        self.cases += 1
        t0 = self.t_us + (2 * P.LONGEST_INTERVAL_US if self.cases % 2 else 100)
        data, now_ns = pl.lines(t0)
        out = self.pair.feed(data, now_ns)
        assert out.n_events == pl.n_events == out.n_results
        grouping = self.engine.scan_stats()["grouping"]
        ips = pl.touched_ips()
        self.pair.compare_state(ips[::max(1, len(ips) // 200)])
        now = self.engine.state_stats()
        assert (now["state_slots"], now["rehashes"], now["states"]) == \
            (self.stats["state_slots"], self.stats["rehashes"], self.stats["states"])
        self.t_us = now_ns // 1000 + 1
        self.failed = False
        return pl, grouping

    def close(self):
        self.engine.close()


@pytest.fixture(scope="module")
def world():
    keep = {k: os.environ.get(k) for k in ("BJX_SORT2", "BJX_WAVE_RUNS", "BJX_REC16", "BJX_CHECK")}
    for k in keep:
        os.environ.pop(k, None)
    os.environ["BJX_SORT2"] = "2"
    w = World()
    yield w
    w.close()
    for k, v in keep.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def set_wave_runs(monkeypatch, wave_runs):
    if wave_runs is None:
        monkeypatch.delenv("BJX_WAVE_RUNS", raising=False)
    else:
        monkeypatch.setenv("BJX_WAVE_RUNS", wave_runs)


def lens_of(pl, n, comp):
    return [[r[3] for r in rr] for _, m, c, rr in pl.jobs if (m, c) == (n, comp)][0]


@pytest.mark.parametrize("L,wave_runs", list(itertools.product(range(6, 16), WAVE_RUNS)))
def test_bucket_shapes(world, L, wave_runs, monkeypatch):
    """Every target size in every composition, each in a bucket of its own;
    the last bucket, and bucket 0 in every other case; a state whose low key
    equals the padding key in a bucket below the cap, its run long ("tail") or
    a singleton ("mixed")."""
    set_wave_runs(monkeypatch, wave_runs)
    nb = 1 << (SLOT_BITS - L)
    known = world.known(L)
    with_zero = wave_runs in ("0", "16")
    extra, exclude = [], set()
    if nb - 1 in known:
        extra.append((nb - 1, 257, "mixed"))
    if with_zero and 0 in known:
        extra.append((0, 255, "tail"))
    else:
        exclude.add(0)
    ones = world.ones_bucket(L, {0, nb - 1})
    if ones is not None:
        extra.append((ones, 1025, "tail" if wave_runs in (None, "0") else "mixed"))
    if L == 15:  # what a bucket of 2^15 slots must bring, from the plan
        assert nb - 1 in known and 0 in known and ones is not None
    pl, grouping = world.run(L, extra=extra, exclude=exclude)
    assert grouping == 1 + pl.oversized and pl.oversized == 4 * (4097 + 5000)
    if L == 15:
        mask = (1 << L) - 1
        assert pl.events[nb - 1] == 257 and (pl.events.get(0) == 255 if with_zero else 0 not in pl.events)
        assert pl.events[ones] == 1025 < P.CAP and [r for b, _, _, rr in pl.jobs if b == ones for r in rr][0][2] & mask == mask
        assert lens_of(pl, 4096, "flat") == [1] * 4096              # nh = 4,096
        assert lens_of(pl, 4096, "pairs") == [2] * 2048             # BJX_WAVE_RUNS=2: nh = nwv = 2,048
        for n in (4079, 4080, 4081, 4095, 4096):                    # BJX_WAVE_RUNS=16: all three regions of s_ord
            lens = lens_of(pl, n, "mixed")
            assert sum(lens) >= 3585 and min(lens) < 8 and any(8 <= k < 16 for k in lens) and max(lens) >= 16


@pytest.mark.parametrize("L,last,pad", [(L, last, pad) for L in (6, 15) for last in ("filled", "empty") for pad in PADS])
def test_bucket_bounds_edges(world, L, last, pad, monkeypatch):
    """k_bucket_bounds: the batch's events modulo 4 (the four-key load and its
    tail), whole blocks (256 lanes x 4 keys), with events in the last bucket
    (bstart[nb] written by the lane past the last event alone) and with the last
    sixteenth of the buckets empty (the gap fill up to nb); bucket 0 is empty.
    At L = 6 the ~40 filled buckets lie among 65,536."""
    set_wave_runs(monkeypatch, None)
    nb = 1 << (SLOT_BITS - L)
    if last == "filled":
        assert nb - 1 in world.known(L)
        kw = dict(extra=[(nb - 1, 3, "flat")], exclude={0})
    else:
        kw = dict(exclude={0} | set(range(nb - nb // 16, nb)))
    pl, grouping = world.run(L, targets=BOUNDS_TARGETS, pad=pad, **kw)
    assert pl.n_events % pad[0] == pad[1] and grouping == 1
    assert (max(pl.events) == nb - 1) if last == "filled" else (max(pl.events) < nb - nb // 16)


@pytest.mark.parametrize("L,wave_runs,hook", [(L, w, h) for L in (6, 12, 15) for w in (None, "16")
                                              for h in ("BJX_REC16", "BJX_CHECK")])
def test_bucket_shapes_hooks(world, L, wave_runs, hook, monkeypatch):
    """BJX_REC16=1: the 16-byte event records; BJX_CHECK=1: every sorted
    position written exactly once, by whichever path took it."""
    set_wave_runs(monkeypatch, wave_runs)
    monkeypatch.setenv(hook, "1")
    pl, grouping = world.run(L)
    assert grouping == 1 + pl.oversized


def test_bucket_bits_gate(world, monkeypatch):
    """Bucket bits 6 would be L = 16: the gate keeps the full sort, and the
    batch still matches the oracle.  Bad arguments are refused and change
    nothing."""
    set_wave_runs(monkeypatch, None)
    pl, grouping = world.run(16, comps=("flat", "mixed"))  # 64 buckets of 2^16 slots
    assert grouping == 0 and pl.n_events == 2 * sum(P.TARGETS)
    world.engine.debug_set_bucket_bits(7)
    for bad in (17, 32, 1 << 31):
        with pytest.raises(_lib.BanjaxGpuError) as x:
            world.engine.debug_set_bucket_bits(bad)
        assert x.value.code == _lib.ERR_ARG
    # still 7 bucket bits: 5,000 events on ~4,100 slots are one oversized bucket of 2^15 slots (and ~500 small ones of 64)
    pl, grouping = world.run(15, bits=7, targets=(17, 5000), comps=("flat",))
    assert grouping == 1 + 5000


@pytest.mark.parametrize("sort2", ["2", None])
def test_bucket_bits_back_to_default(world, sort2, monkeypatch):
    """Back at 0 the engine groups as it does without the hook: buckets of 64
    slots under BJX_SORT2=2, and without it the default policy's full sort for
    a batch this small."""
    set_wave_runs(monkeypatch, None)
    if sort2 is None:
        monkeypatch.delenv("BJX_SORT2")
    pl, grouping = world.run(6, bits=0)
    assert pl.oversized and grouping == (1 + pl.oversized if sort2 else 0)
