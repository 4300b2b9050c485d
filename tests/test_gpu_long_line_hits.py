"""GPU parity and repeatability on lines whose literal hits overflow, or race
for, the scan pass's four hit slots (tests/long_lines.py; its batches are
checked on the host by tests/test_long_lines_cpu.py).

A long line's hits get their slots from atomics, in an order that differs
between runs, so which hits are exact and which are summarised differs too;
the results may not.  Bit-exact against the oracle on every ruleset class
(literal counts that switch Bind::cfirst and Bind::lits_small, literal ids
past 32, the per-line kernel k_lines, the wide kernel), and identical across
repeated feeds of one batch."""
import pytest

import workloads as W
from banjax_amd import Engine
from tests import long_lines as LL
from tests.parity import Pair

pytestmark = pytest.mark.gpu
TILE_BYTES = LL.TILE
IPS = LL.IPS + ["AhrefsBot", "Firefox/7", "Scrapy", "Macintosh", "haystack12x", "needle3", "sitelit", "ab=token", "Mechanize"]


@pytest.fixture(scope="module")
def engine():
    e = Engine()
    yield e
    e.close()


# ruleset, seed, the bind-time switch to set, the per-line kernel that must have run.
# BJX_NO_LINES2 (as in test_gpu_parity.py test_fallback_paths) is the switch that
# keeps k_lines inside a test process: BJX_LINES is read once per process.
CASES = [("A", 1, None, "k_lines2"), ("B", 1, None, "k_lines2"), ("C1", 2, None, "k_lines2"), ("C2", 2, None, "k_lines2"),
         ("A", 2, "BJX_NO_LINES2", "k_lines"), ("B", 2, "BJX_NO_LINES2", "k_lines"), ("D", 1, None, "k_parse_match")]


@pytest.mark.parametrize("kind,seed,switch,kernel", CASES, ids=["%s-%s" % (c[0], c[3]) for c in CASES])
def test_layouts(engine, kind, seed, switch, kernel, monkeypatch):
    b = LL.batch(seed)
    eng = engine
    if switch:
        monkeypatch.setenv(switch, "1")
        eng = Engine(0)
    try:
        pair = Pair(LL.rules_yaml(kind), eng)
        out = pair.feed(b.data, b.now_ns)
        assert eng.line_kernel()[0] == kernel
        st = eng.scan_stats()
        # every layout line but the 3- and 4-hit ones overflows its slots
        assert st["literal_hits"] > 4 * len(b.lines), st
        # overflowed lines send their literal rules to the automata (the wide
        # kernel decides every pair itself and emits no DFA jobs)
        if kernel != "k_parse_match":
            assert st["dfa_jobs"] > 0, st
        # lines handed to the per-line fallback: the headers past k_lines2's window
        # (k_lines reads every line from HBM and hands none over)
        if kernel != "k_lines":
            assert st["fallback_lines"] > 0, st
        assert out.n_trips > 50
        # the same bytes a few bytes on: every hit lands on other tile offsets
        k = 5 + 6 * seed + len(kind)
        pair.feed(b"\n" * k + b.data, b.now_ns)
        assert eng.line_kernel()[0] == kernel
        pair.compare_state(IPS)
    finally:
        if switch:
            eng.close()


def _digest(out):
    return ([(r.line_idx, r.rule_idx, r.rule_pos, r.skip_host, r.seen_ip, r.match_type, r.exceeded) for r in out.results],
            [(t.line_idx, t.rule_idx) for t in out.trips], out.n_results, out.n_events, out.n_lines)


@pytest.mark.parametrize("kind,seed", [("A", 2), ("C1", 1)])
def test_repeatable(engine, kind, seed):
    """One batch three times through one engine, the state cleared between:
    results, trips, counts and the recorded hits are the same every time (the
    DFA-job count may differ: it follows which hits got slots).  Each feed is
    also compared with the oracle, so the common value is the right one."""
    b = LL.batch(seed)
    seen = []
    for _ in range(3):
        pair = Pair(LL.rules_yaml(kind), engine)  # clears the engine's state, fresh oracle state
        out = pair.feed(b.data, b.now_ns)
        assert engine.line_kernel()[0] == "k_lines2"
        seen.append((_digest(out), engine.scan_stats()["literal_hits"]))
    assert seen[0][1] > 4 * len(b.lines)
    assert seen[1] == seen[0] and seen[2] == seen[0]


@pytest.mark.parametrize("kind", ["A", "C1"])
def test_tile_start_lines_recorded_once(engine, kind):
    """A line that starts on a tile's first byte and ends in that tile's halo:
    the tile has no '\\n', so the next tile takes the line for one begun earlier
    and records the hits past the tile's end itself.  The first tile once did
    too, from LDS: those hits were recorded twice, and its plain store of the hit
    count raced with the next tile's atomicAdd, so that now and then a slot
    held a later hit in place of an earlier one (workload cfg4 lost one or two
    events of 92M that way).  Every hit of this batch is a true literal clear of
    the tile edges, so the scan must record exactly the occurrences counted on
    the host; the results are compared with the oracle as everywhere."""
    b = LL.tile_start_batch(3)
    pair = Pair(LL.rules_yaml(kind), engine)
    want = LL.count_hits(b.data, LL.literals(kind))
    for shift in (0, TILE_BYTES):
        pair.feed(b"\n" * shift + b.data, b.now_ns)
        assert engine.line_kernel()[0] == "k_lines2"
        assert engine.scan_stats()["literal_hits"] == want
    pair.compare_state(LL.IPS)


def test_cfg4_tile_start_lines(engine):
    """The lines of workload cfg4 that take that path (tests/golden/long_line_hits.json.gz),
    verbatim, each on a tile's first byte again: oracle parity over two feeds, and
    every hit recorded once (all of them lie in lines one wave verifies whole)."""
    b = LL.golden_batch()
    pair = Pair(W.CFG4.rules_yaml, engine)
    want = LL.count_hits(b.data, LL.literals("A"))
    for shift in (0, TILE_BYTES):
        out = pair.feed(b"\n" * shift + b.data, b.now_ns)
        assert engine.scan_stats()["literal_hits"] == want
    assert out.n_results > len(b.lines)
    pair.compare_state(sorted({ln.text.split(b" ")[1].decode() for ln in b.lines}))


def test_cfg4_slice_repeatable(engine):
    """4,000 lines of workload cfg4 (about 20 MB of 2-8 KB lines), twice."""
    w = W.scaled(W.CFG4, 4_000)
    data, now = w.host_lines(), w.now_ns()
    seen = []
    for _ in range(2):
        pair = Pair(w.rules_yaml, engine)
        out = pair.feed(data, now)
        seen.append((_digest(out), engine.scan_stats()["literal_hits"]))
    assert seen[0] == seen[1]
    assert seen[0][0][2] > 0
