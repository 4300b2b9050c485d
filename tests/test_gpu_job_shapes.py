"""The DFA job stage (emit_job -> job sort -> k_dfa / k_dfa_legacy / k_nfa<WT> /
k_nfa_wide, with k_rule_bounds' ranges) at the exact shapes tests/job_shapes.py
plans, bit for bit against the oracle.

Every batch goes through a tests.parity.Pair (line flags, RuleResults, trips,
and the states carried from batch to batch), and after every batch
Engine.debug_job_counts() must equal the plan's windowed and legacy jobs of
every rule exactly, their sum scan_stats' dfa_jobs, and the per-line pass must
have run once.  So a case proves both that the kernels saw the planned block
compositions and that they decided them as the oracle does.

When the oracle and the engine disagree, explain() also evaluates the rule on
that text with bjx_debug_rule_match_host: host tables that agree with the
oracle point at a kernel, host tables that disagree at the rule compiler.

What the net catches, tried on scratch builds with one logic edit each:
k_rule_bounds writing last[r] = i fails every case (the hook's counts and the
NFA ranges are one short); dfa_line keeping `skip` past the first chunk fails
every dfa_line case; k_dfa starting every job in R.start fails the cases with
the `^GET .*<lit>.{k}y` rule (text edges S, mixed, last line), whose jobs
begin in the skip state.  The `n_states <= B.dfa_acc` test of k_dfa matters
only for class L (transitions staged, accel words not): its uniform blocks
are in text_edges_uniform[L] and block_compositions[kinds].

test_job_buffer_growth runs on an engine of its own: the first batch plans
more jobs than the fresh job buffers hold, so the per-line pass runs twice.
"""
import pytest

from banjax_amd import Engine, _lib
from tests import job_shapes as J
from tests.parity import Pair, compare_batch

pytestmark = pytest.mark.gpu
S = 1_000_000_000
NOW = J.T0 * S
CASES = [n for n, c in J.cases().items() if not c.no_lines2 and c.items]
CASES_NL2 = [n for n, c in J.cases().items() if c.no_lines2]
LAST_RULES = (1, 3, 4, 5, 7, 9, 10, 13)   # S `.{k}y`, S `.*d`, S `x+...*d` (no lead), T, A, L, N, S `^GET .*...`


def explain(pair, data, ores, out):
    """Which side the host tables take for the first (line, rule) pairs the engine and the oracle decide differently."""
    lines = data.split(b"\n")
    gset = {(r.line_idx, r.rule_idx) for r in out.results}
    oset = {(o.line_idx, o.rule_id) for o in ores}
    rs = pair.lim._snap.ruleset
    for line, rule in sorted(gset ^ oset)[:8]:
        rest = lines[line].split(b" ", 2)[2] if lines[line].count(b" ") >= 2 else b""
        host = _lib.lib().bjx_debug_rule_match_host(rs.handle, rule, rest, len(rest))
        orc = (line, rule) in oset
        print("line %d rule %d (%s): oracle %s, engine %s, host tables %s -> %s; rest=%r"
              % (line, rule, rs.rules[rule].regex, orc, (line, rule) in gset, bool(host),
                 "a kernel bug (the host tables agree with the oracle)" if bool(host) == orc
                 else "a compiler bug (the host tables disagree with the oracle)", rest[:200]), flush=True)


def feed(pair, data, now_ns, device=False):
    """Pair.feed with explain() on a mismatch; device: the batch in a tensor of exactly its size."""
    oflags, ores, oconsumed = pair.ost.consume(pair.ocfg, data, now_ns, cap=(data.count(b"\n") + 1) * (pair.n_rules + 1))
    if device:
        import torch
        t = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        torch.cuda.synchronize()
        assert t.numel() == len(data)
        _, out = pair.lim.consume_device_batch(data, t.data_ptr(), len(data), now_ns)
    else:
        _, out = pair.lim.consume_lines(data, now_ns)
    try:
        compare_batch(oflags, ores, oconsumed, out)
    except AssertionError:
        explain(pair, data, ores, out)
        raise
    return out, ores


def check_jobs(eng, want, kernel, runs=1):
    w, g, n = eng.debug_job_counts()
    st = eng.scan_stats()
    assert eng.line_kernel()[0] == kernel, eng.line_kernel()
    bad = [(r, w[r], want[0][r], g[r], want[1][r]) for r in range(len(w)) if (w[r], g[r]) != (want[0][r], want[1][r])]
    assert len(w) == len(want[0]) and not bad, "(rule, windowed, planned, legacy, planned): %s" % bad[:20]
    assert sum(w) + sum(g) == st["dfa_jobs"], (sum(w), sum(g), st)
    assert n == runs, n


def set_lines2(monkeypatch, on):
    if on:
        monkeypatch.delenv("BJX_NO_LINES2", raising=False)
    else:
        monkeypatch.setenv("BJX_NO_LINES2", "1")   # read when the ruleset is bound: at the Pair's first batch
    return "k_lines2" if on else "k_lines"


@pytest.fixture(scope="module")
def engine():
    e = Engine(0)
    yield e
    e.close()


def run_case(eng, name, kernel):
    c = J.cases()[name]
    b = c.batch()
    pair = Pair(J.rules_yaml(c.ruleset), eng)
    for k in range(2):
        out, _ = feed(pair, b.data, NOW + k * S)
        assert out.n_lines == len(b.lines)
        check_jobs(eng, c.counts, kernel)
    pair.compare_state(J.IPS[::5])
    return out


@pytest.mark.parametrize("name", CASES)
def test_block_compositions(engine, name, monkeypatch):
    """k_lines2's jobs: runs of 1..513 jobs of a staged (S) and a never staged (T) rule from a block's first lane,
    runs of 257 from lanes 1, 128 and 255, totals of 0, 1 and 255 modulo 256, one job alone, and in "kinds" every key
    kind: uniform and mixed blocks of the A and L rules, the block with the last windowed and the first legacy
    jobs, a uniform legacy block, DFA legacy jobs beside NFA jobs, NFA ranges of 1, 256 and 257 jobs of the lowest
    and the highest rule and of adjacent rules, wide-NFA ranges of 1 and 257."""
    run_case(engine, name, set_lines2(monkeypatch, True))


@pytest.mark.parametrize("name", CASES_NL2)
def test_block_compositions_no_lines2(engine, name, monkeypatch):
    """Every job a legacy one (k_lines, dfa_text); rules256: one block of 256 different rules."""
    run_case(engine, name, set_lines2(monkeypatch, False))


def test_no_jobs_after_many(engine, monkeypatch):
    """A batch without a job directly after one with 2,700: the sorted buffers still hold the older batch's keys."""
    kernel = set_lines2(monkeypatch, True)
    cs = J.cases()
    pair = Pair(J.rules_yaml("MAIN"), engine)
    for k, name in enumerate(("kinds", "nojobs", "single", "nojobs")):
        b = cs[name].batch()
        out, _ = feed(pair, b.data, NOW + k * S)
        check_jobs(engine, cs[name].counts, kernel)
        if name == "nojobs":
            assert out.n_results == 0 and engine.scan_stats()["dfa_jobs"] == 0
    pair.compare_state(J.IPS[::5])


@pytest.mark.parametrize("lines2", [True, False], ids=["dfa_line", "dfa_text"])
@pytest.mark.parametrize("cls", list(J.EDGE_RULES))
def test_text_edges_uniform(engine, cls, lines2, monkeypatch):
    """Each edge rule's lines alone (every block its own): see job_shapes.EDGE_KINDS."""
    kernel = set_lines2(monkeypatch, lines2)
    pair = Pair(J.rules_yaml("EDGE"), engine)
    rs = J.EDGE_RULES[cls]
    for k, r in enumerate(rs + rs[:1] if len(rs) == 1 else rs):
        b = J.edge_uniform(r)
        out, ores = feed(pair, b.data, NOW + k * S)
        check_jobs(engine, J.edge_counts(b, not lines2), kernel)
        n = sum(1 for ln in b.lines if ln.rule == r)
        assert 0 < len(ores) < n, (len(ores), n)   # both outcomes, as the oracle has it
    pair.compare_state(J.IPS[::5])


@pytest.mark.parametrize("lines2", [True, False], ids=["dfa_line", "dfa_text"])
def test_text_edges_mixed(engine, lines2, monkeypatch):
    """The same edges with every rule's jobs in blocks they share with other rules."""
    kernel = set_lines2(monkeypatch, lines2)
    pair = Pair(J.rules_yaml("EDGE"), engine)
    for k, b in enumerate(J.edge_mixed()):
        feed(pair, b.data, NOW + k * S)
        check_jobs(engine, J.edge_counts(b, not lines2), kernel)
    pair.compare_state(J.IPS[::5])


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("lines2", [True, False], ids=["dfa_line", "dfa_text"])
def test_last_line_of_batch(engine, lines2, device, monkeypatch):
    """The job's line ends the batch, whose length modulo 16 takes every value (the n_buf guard of the 16-byte
    loads): from host memory, and from a device tensor of exactly the batch's size; the job alone in its block and
    beside another rule's."""
    kernel = set_lines2(monkeypatch, lines2)
    pair = Pair(J.rules_yaml("EDGE"), engine)
    k, seen = 0, set()
    for r in LAST_RULES:
        for mixed in (False, True):
            for b in J.last_line_batches(r, mixed):
                k += 1
                out, ores = feed(pair, b.data, NOW + k * 1000, device)
                check_jobs(engine, J.edge_counts(b, not lines2), kernel)
                seen.add((r, any(o.rule_id == r for o in ores)))
    assert seen == {(r, m) for r in LAST_RULES for m in (True, False)}
    pair.compare_state(J.IPS[::5])


def test_job_buffer_growth(monkeypatch):
    """A fresh engine's job buffers hold (lines + 2^20) * 5 / 4 jobs; 44,000 lines with 32 jobs each pass that, so
    the buffers grow and the per-line pass runs again: nothing of the first pass may be counted twice."""
    set_lines2(monkeypatch, True)
    eng = Engine(0)
    try:
        b = J.grow_batch()
        pair = Pair(J.rules_yaml("GROW"), eng)
        n = len(b.lines)
        assert n * 32 > (n + J.JOB_SLACK) * 5 // 4
        first = None
        for k, runs in enumerate((2, 1)):
            out, ores = feed(pair, b.data, NOW + k * S)
            w, g, n_runs = eng.debug_job_counts()
            assert eng.line_kernel()[0] == "k_lines2"
            assert n_runs == runs, n_runs
            assert eng.scan_stats()["dfa_jobs"] == n * 32 == sum(w) + sum(g)
            assert [w[r] + g[r] for r in range(32)] == [n] * 32
            assert out.n_results == len(ores) == 2 * n - sum(1 for i in range(n) if i % 32 == (7 * i + 3) % 32)
            assert out.n_events == len(ores)
            got = [(r.line_idx, r.rule_idx) for r in out.results]
            if first is None:
                first = got
            assert got == first
        pair.compare_state(["10.4.0.0", "10.4.3.5", "10.4.7.7"])
    finally:
        eng.close()
