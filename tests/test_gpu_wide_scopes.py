"""GPU parity on scopes of more than 128 positions (tests/wide_scopes.py; its
rulesets and batches are checked on the host by tests/test_wide_scopes_cpu.py).

decide_wide, the per-line fallback's rule walk for such scopes, looks only at
the rules a line's literal hits name, where the reference tries every rule
(regex_rate_limiter.go:175-211); a wrong skip in one of its branches drops a
match without any other sign.  Each ruleset kind reaches other branches: the
mixed regime where only one host's scope is wide (k_lines decides the other
hosts' lines and lists that host's for the fallback), every scope wide with
and without the line pass, site positions past 128, no prefilter literal at
all, wide-NFA rules listed for k_nfa_wide, and as a control the same lines in
scopes k_lines2 decides.  Bit-exact against the oracle over two batches with
the state carried between them, then the trips-only path on a cleared state."""
import pytest

from banjax_amd import Engine
from tests import wide_scopes as WS
from tests.parity import Pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    e = Engine()
    yield e
    e.close()


def _run(engine, kind, kernel, fallback=None):
    """Two batches (the second clock 3 s later, the hosts in another order, so a line index
    that was wide is narrow now), every result, trip and state compared; then the first batch
    on a cleared state without RuleResult copies."""
    pair = Pair(WS.rules_yaml(kind), engine)
    outs = []
    for seed in WS.SEEDS:
        b = WS.batch(kind, seed)
        outs.append(pair.feed(b.data, b.now_ns, check=True))
        assert engine.line_kernel()[0] == kernel
        # the events counted per line (by the kernel that decided it) are the ones emitted
        assert outs[-1].n_events == sum(1 for r in outs[-1].results if not r.skip_host)
        if fallback is not None:
            assert engine.scan_stats()["fallback_lines"] == fallback(b), seed
    assert min(o.n_trips for o in outs) >= 20
    pair.compare_state(WS.IPS)
    pair = Pair(WS.rules_yaml(kind), engine)  # clears the engine's state, fresh oracle state
    b = WS.batch(kind, WS.SEEDS[0])
    out = pair.feed(b.data, b.now_ns, want_results=False)
    assert out.n_trips == outs[0].n_trips
    pair.compare_state(WS.IPS)
    return outs


# MIX first: the switch between k_lines and k_lines2 is read once per process, at the first
# batch with a line pass, and must not be read under BJX_LINES=1

def test_mix(engine):
    """Only big's scope is wide: k_lines decides the other hosts' lines with three mask words
    and lists big's lines, and the lines with an exotic timestamp, for the fallback."""
    _run(engine, "MIX", "k_lines", lambda b: b.fallback_lines())


def test_site(engine):
    """150 site rules: site positions in all three mask words, every global position past 149."""
    _run(engine, "SITE", "k_lines", lambda b: b.fallback_lines())


def test_narrow(engine):
    """The control: the lines of MIX, the far ones among them, in scopes of at most 120 positions."""
    _run(engine, "NARROW", "k_lines2")


def test_all(engine):
    """More than 128 global rules: no line pass, the fallback parses and decides every line."""
    _run(engine, "ALL", "k_parse_match", lambda b: b.n_lines)


def test_all_with_line_pass(engine, monkeypatch):
    """The same through k_lines, which lists every line with four spaces."""
    monkeypatch.setenv("BJX_LINES", "1")
    _run(engine, "ALL", "k_lines", lambda b: sum(1 for ln in b.lines if ln.spaces4))


@pytest.mark.parametrize("line_pass", [True, False])
def test_nolit(engine, line_pass, monkeypatch):
    """No prefilter literal in the ruleset: the fallback tries every rule of the scope and
    writes three mask words.  130 global rules make every scope wide, so the line pass, and
    with it k_lines, runs only with BJX_LINES=1; without it the fallback takes every line
    from its own parse."""
    if line_pass:
        monkeypatch.setenv("BJX_LINES", "1")
    _run(engine, "NOLIT", "k_lines" if line_pass else "k_parse_match",
         (lambda b: sum(1 for ln in b.lines if ln.spaces4)) if line_pass else (lambda b: b.n_lines))


def test_wnfa(engine):
    """Wide-NFA rules in a wide scope: decide_wide lists them for k_nfa_wide under their
    pattern's first rule, which sets the bit and counts the event.  Two rules of one
    pattern differ in hosts_to_skip (in both orders) and a site rule shares it: the event
    count must follow the line's own rule at that position, as k_emit does."""
    outs = _run(engine, "WNFA", "k_parse_match", lambda b: b.n_lines)
    assert all(o.n_results > o.n_events > 0 for o in outs)  # skipped results: RuleResults without events


@pytest.mark.parametrize("kind,kernel", [("MIX", "k_lines"), ("NARROW", "k_lines2")])
def test_engine_self_checks(engine, kind, kernel, monkeypatch):
    """BJX_CHECK=1: the engine's own per-batch checks (each line's RuleResult count against its
    mask words where there are at most two, every event its own RuleResult, the sorted
    rate-limit records) raise nothing on these batches."""
    monkeypatch.setenv("BJX_CHECK", "1")
    pair = Pair(WS.rules_yaml(kind), engine)
    for seed in WS.SEEDS:
        b = WS.batch(kind, seed)
        pair.feed(b.data, b.now_ns)
        assert engine.line_kernel()[0] == kernel
    pair.compare_state(WS.IPS)
