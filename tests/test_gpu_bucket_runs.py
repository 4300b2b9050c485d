"""k_bucket_apply's wave-per-run path (runs of at least 8 events of one (ip,
rule name) state, a whole wave per run in chunks of 64 events, closed form
where the chunk's rules agree, event by event where they do not) against the
oracle's sequential RegexRateLimitStates.Apply (reference
internal/rate_limit.go:37-78), bit-exact, through the two-level grouping
(BJX_SORT2=2).  Every case runs with the wave path (BJX_WAVE_RUNS unset) and
with every run on the lane-per-run loop (BJX_WAVE_RUNS=0).

Each IP of a group sends an exact number of lines per batch, so its runs
straddle the wave threshold (7, 8, 9) and the chunk edges (63 ... 129, 200).
Every line matches the `.*` rule and one of the two rules sharing the name
"shared", so each IP has two runs of that length."""
import pytest

from banjax_amd import Engine
from tests.parity import Pair

pytestmark = pytest.mark.gpu

CFG = """
regexes_with_rates:
  - rule: "shared"
    regex: 'GET'
    interval: 0.25
    hits_per_interval: %d
    decision: challenge
  - rule: "shared"
    regex: 'POST'
    interval: 0.25
    hits_per_interval: %d
    decision: nginx_block
  - rule: "every"
    regex: '.*'
    interval: 0.25
    hits_per_interval: %d
    decision: challenge
expiring_decision_ttl_seconds: 10
"""

COUNTS = (1, 7, 8, 9, 63, 64, 65, 127, 128, 129, 200)
T0 = 1700000000_000  # ms


@pytest.fixture(scope="module")
def engine():
    e = Engine()
    yield e
    e.close()


def ip_of(group, count):
    return "10.%d.%d.%d" % (group, count >> 8, count & 255)


def lines(t0_ms, groups, counts=COUNTS, post_every=7, back_every=97):
    """The IPs of `groups` take turns, one line per ms, until each has sent
    its count: an IP's lines are as many ms apart as IPs are still sending
    (a 0.25 s window holds ~23 events while all eleven send, so a chunk of 64
    holds several windows; 250 at the end, when only the 200-line IP is left).
    The 128-line IPs' lines are 0.3 s late from their 64th on and the 129-line
    IPs' from their 65th on: a window opens on the last lane of the first
    chunk and on the first lane of the second.  Every `back_every`-th line
    is 5 s back."""
    left = {(g, c): c for g in groups for c in counts}
    out, k = [], 0
    while left:
        for key in sorted(left):
            g, c = key
            sent = c - left[key]
            t = t0_ms + k
            if (c == 128 and sent >= 63) or (c == 129 and sent >= 64):
                t += 300
            if back_every and k % back_every == back_every - 1:
                t -= 5000
            m = "POST" if k % post_every == 0 else "GET"
            out.append("%d.%03d %s %s h.com %s /x HTTP/1.1 ua" % (t // 1000, t % 1000, ip_of(g, c), m, m))
            k += 1
            left[key] -= 1
            if not left[key]:
                del left[key]
    return ("\n".join(out) + "\n").encode(), k


def feed_batches(pair):
    """Three batches that continue each other's windows (the second and third
    bring new IPs, whose first event -- seenIp false -- opens a long run), then
    one that lies outside every stored window."""
    t = T0
    for groups in ((1,), (1, 2), (1, 2, 3)):
        data, n = lines(t, groups)
        pair.feed(data, t * 1_000_000)
        t += n + 1  # the next batch starts 1 ms after this one's last line
    t += 60_000
    data, n = lines(t, (1, 2, 3))
    pair.feed(data, t * 1_000_000)
    pair.compare_state([ip_of(g, c) for g in (1, 2, 3) for c in COUNTS])


@pytest.mark.parametrize("wave_runs", [None, "0"])
@pytest.mark.parametrize("lim_get,lim_post,lim_every", [
    (3, 3, 2),     # small limits: Exceeded resets many times inside a run
    (0, 0, -1),    # every hit trips
    (-1, -1, 0),
    (5, 2, 1),     # the rules sharing the name differ: chunks with both are walked event by event
])
def test_bucket_runs(engine, lim_get, lim_post, lim_every, wave_runs, monkeypatch):
    monkeypatch.setenv("BJX_SORT2", "2")
    if wave_runs is None:
        monkeypatch.delenv("BJX_WAVE_RUNS", raising=False)
    else:
        monkeypatch.setenv("BJX_WAVE_RUNS", wave_runs)
    engine.state_clear()
    pair = Pair(CFG % (lim_get, lim_post, lim_every), engine)
    feed_batches(pair)
    assert engine.scan_stats()["grouping"] == 1  # two-level, no oversized bucket


@pytest.mark.parametrize("wave_runs", [None, "0"])
@pytest.mark.parametrize("hook", ["BJX_CHECK", "BJX_REC16"])
def test_bucket_runs_hooks(engine, hook, wave_runs, monkeypatch):
    """BJX_CHECK=1: every sorted position is written exactly once, by either
    path; BJX_REC16=1: the 16-byte event records."""
    monkeypatch.setenv("BJX_SORT2", "2")
    monkeypatch.setenv(hook, "1")
    if wave_runs is None:
        monkeypatch.delenv("BJX_WAVE_RUNS", raising=False)
    else:
        monkeypatch.setenv("BJX_WAVE_RUNS", wave_runs)
    engine.state_clear()
    pair = Pair(CFG % (3, 3, 2), engine)
    feed_batches(pair)


@pytest.mark.parametrize("wave_runs", [None, "0"])
def test_full_and_oversized_bucket(engine, wave_runs, monkeypatch):
    """One IP with exactly 4,096 lines: its runs fill a bucket to the block's
    capacity (64 chunks of one run).  One with 4,097: its buckets overflow and
    take the full sort on their own (grouping > 1)."""
    monkeypatch.setenv("BJX_SORT2", "2")
    monkeypatch.setenv("BJX_CHECK", "1")
    if wave_runs is None:
        monkeypatch.delenv("BJX_WAVE_RUNS", raising=False)
    else:
        monkeypatch.setenv("BJX_WAVE_RUNS", wave_runs)
    engine.state_clear()
    pair = Pair(CFG % (37, 37, 5), engine)
    data, n = lines(T0, (4,), counts=(4096, 9))
    pair.feed(data, T0 * 1_000_000)
    assert engine.scan_stats()["grouping"] >= 1
    t = T0 + n + 1
    data, n = lines(t, (5,), counts=(4097, 9))
    out = pair.feed(data, t * 1_000_000)
    g = engine.scan_stats()["grouping"]
    assert g > 1 and g - 1 >= 2 * 4097, (g, out.n_events)  # both of the IP's runs went through the oversized-bucket path
    t += n + 1
    data, n = lines(t, (4, 5), counts=(4096, 4097, 9))
    pair.feed(data, t * 1_000_000)
    pair.compare_state([ip_of(g, c) for g in (4, 5) for c in (4096, 4097, 9)])
