"""The generated rule corpus (tests/rule_corpus.py, swept on the host by
tests/test_rule_plans_cpu.py) through the device's decision paths: every
RuleResult bit for bit against the oracle.

Every text of a rule becomes log lines in five layouts (rule_corpus.LAYOUTS:
at rest[0], at the line's end, straddling k_lines2's 112-byte window, past the
inline automata's 64 steps, behind more literal hits than a line has hit
slots), and every line is judged against every rule of its ruleset.  The
rulesets are cut from the corpus so that the bind takes each literal-count
path: A at most 8 interned literals (Bind::cfirst), B 9-32 (lits_small), C
past 32 with the rules under test behind 34 one-literal rules (literal ids
past 32: kJiBigLit), D more than 128 global rules (the wide per-line kernel).
B and C also run under the bind-time switches and the forced per-lane NFA.

A change that decides more rules from their hits has to pass this file and
tests/test_rule_plans_cpu.py."""
import collections
import functools
import os
import subprocess
import sys
from dataclasses import dataclass

import pytest

from banjax_amd import Config, Engine, Ruleset, _lib
from oracle import oracle as O
from tests import rule_corpus as RC
from tests.parity import Pair
from tests.test_rule_plans_cpu import corpus

pytestmark = pytest.mark.gpu
S = 1_000_000_000
IPS = ["9.9.0.0", "9.9.1.1", "9.9.2.17", "9.9.3.60", "9.9.1.33"]


@dataclass
class Set:
    kind: str
    idx: list      # corpus indices, in rule order
    budget: list   # per rule: (matching texts, non-matching texts, window offsets per text)
    lines: list = None

    @property
    def yaml(self):
        entries = corpus()[0]
        y = ["regexes_with_rates:"]
        for k, i in enumerate(self.idx):
            y.append("  - rule: 'p%d'\n    regex: '%s'\n    interval: 1\n    hits_per_interval: 1000000\n"
                     "    decision: challenge" % (k, entries[i].rule.pattern.replace("'", "''")))
        return "\n".join(y) + "\n"


def _rest(line):
    return line.split(b" ", 2)[2]


@functools.lru_cache(maxsize=None)
def _world():
    """(entries, pool, eligible): pool = literals other rules' overflow lines are
    padded with; eligible[i] = the oracle finds, among the lines of rule i's
    first matching and first non-matching text alone, both outcomes in every
    layout (an anchored rule: in the start layout, the only one that puts a text
    at rest[0]), so the rule can be shown wrong in both directions wherever it
    is placed."""
    entries = corpus()[0]
    pool = []
    for e in entries:
        if e.rule.shape == "pure" and e.plan.equiv and len(e.plan.pref) == 1 and not e.plan.pref[0].any_ci:
            pool.append(e.plan.pref[0])
        if len(pool) == 12:
            break
    elig = []
    for i, e in enumerate(entries):
        if e.violation or "'" in e.rule.pattern:
            elig.append(False)
            continue
        if e.decided:
            elig.append(True)
            continue
        ore = O.Regex(e.rule.pattern)
        seen = collections.defaultdict(set)
        for ln in _lines_of(entries, i, 0, (1, 1, 1), tuple(pool)):
            seen[ln.layout].add(ore.match(_rest(ln.data)))
        need = ("start",) if e.plan.mode == RC.MODE_ANCHORED else RC.LAYOUTS
        elig.append(all(len(seen[k]) == 2 for k in need))
    return entries, tuple(pool), elig


def _lines_of(entries, i, owner, budget, pool):
    e = entries[i]
    return RC.rule_lines(owner, e.rule, e.plan, e.texts, e.want, i, budget[0], budget[1], budget[2], list(pool))


def _n_literals(entries, idx):
    return len({(l.s, l.ci) for i in idx for l in entries[i].plan.literals})


@functools.lru_cache(maxsize=None)
def ruleset(kind) -> Set:
    entries, pool, elig = _world()
    used = set()

    def pick(n, pred, max_lits=6, exact=True):
        out = []
        for i, e in enumerate(entries):
            if len(out) == n:
                break
            if elig[i] and i not in used and len(e.plan.pref) <= max_lits and pred(e, set(e.classes)):
                used.add(i)
                out.append(i)
        assert len(out) == n or not exact, (kind, n, len(out))
        return out

    one = lambda e: len(e.plan.pref) == 1  # noqa: E731
    if kind == "A":
        idx = (pick(2, lambda e, c: "pref_lead" in c and one(e)) + pick(1, lambda e, c: "pref_equiv" in c and "pref_ci" in c and one(e))
               + pick(1, lambda e, c: "pref_equiv" in c and one(e)) + pick(1, lambda e, c: "pref_lead" in c and len(e.plan.pref) == 2)
               + pick(1, lambda e, c: "pref_nolead" in c and one(e)) + pick(2, lambda e, c: "scan" in c)
               + pick(1, lambda e, c: "always" in c) + pick(1, lambda e, c: "never" in c))
        budget = [(3, 3, 6)] * len(idx)
    elif kind == "B":
        idx = (pick(6, lambda e, c: "pref_lead" in c, 2) + pick(5, lambda e, c: "pref_equiv" in c, 2)
               + pick(4, lambda e, c: "pref_nolead" in c, 2) + pick(4, lambda e, c: "pref_lead0" in c and "pref_equiv" not in c, 2)
               + pick(3, lambda e, c: "pref_ci" in c, 1) + pick(3, lambda e, c: "pref_fold_ks" in c, 1)
               + pick(1, lambda e, c: "anchored_eq" in c and len(e.plan.anchor) == 1 and not e.plan.anchor[0].any_ci)
               + pick(20, lambda e, c: "scan" in c) + pick(1, lambda e, c: "always" in c) + pick(1, lambda e, c: "never" in c))
        budget = [(6, 6, 8)] * len(idx)
    elif kind == "C":
        fill, lits = [], set()
        for i in pick(200, lambda e, c: "pref_equiv" in c and one(e) and not e.plan.pref[0].any_ci, exact=False):
            if len(fill) < 34 and entries[i].plan.pref[0].s not in lits:
                lits.add(entries[i].plan.pref[0].s)
                fill.append(i)
        assert len(fill) == 34
        used.clear()
        used.update(fill)
        idx = (fill + pick(20, lambda e, c: "pref_lead" in c) + pick(14, lambda e, c: "pref_equiv" in c)
               + pick(10, lambda e, c: "pref_nolead" in c) + pick(8, lambda e, c: "pref_multi" in c, 32)
               + pick(5, lambda e, c: "pref_fold_ks" in c) + pick(1, lambda e, c: "anchored_eq" in c)
               + pick(1, lambda e, c: "anchored_ne" in c) + pick(1, lambda e, c: "anchored_none" in c)
               + pick(1, lambda e, c: "anchored_eq" in c and len(e.plan.anchor) == 1 and not e.plan.anchor[0].any_ci)
               + pick(1, lambda e, c: "anchored_ne" in c and len(e.plan.anchor) > 1 and min(len(l.s) for l in e.plan.anchor) < 4)
               + pick(14, lambda e, c: "scan" in c) + pick(1, lambda e, c: "always" in c) + pick(1, lambda e, c: "never" in c))
        budget = [(1, 1, 1)] * len(fill) + [(4, 4, 4)] * (len(idx) - len(fill))
    else:
        focus = pick(14, lambda e, c: "pref_lead" in c) + pick(14, lambda e, c: "pref_equiv" in c)
        anch = (pick(2, lambda e, c: "anchored_eq" in c) + pick(2, lambda e, c: "anchored_ne" in c)
                + pick(2, lambda e, c: "anchored_none" in c))
        rest = pick(126, lambda e, c: e.plan.mode != RC.MODE_ANCHORED, 32)
        idx = focus + anch + rest
        budget = [(4, 4, 3)] * len(focus) + [(2, 2, 2)] * (len(idx) - len(focus))
    s = Set(kind, idx, budget)
    s.lines = [ln for k, i in enumerate(idx) for ln in _lines_of(entries, i, k, budget[k], pool)]
    return s


def test_rulesets_take_each_literal_path():
    """The literal counts that select Bind::cfirst, Bind::lits_small and the
    ids past 32, by the bind's own count (as test_long_lines_cpu.py does)."""
    entries = corpus()[0]
    L = _lib.lib()
    for kind in "ABCD":
        s = ruleset(kind)
        rs = Ruleset(Config.from_yaml(s.yaml))
        n = L.bjx_debug_ruleset_literals(rs.handle)
        assert n == _n_literals(entries, s.idx), kind
        classes = collections.Counter(c for i in s.idx for c in entries[i].classes)
        assert classes["pref_lead"] >= 2 and classes["pref_equiv"] >= 2 and classes["pref_nolead"] >= 1, (kind, classes)
        if kind == "A":
            assert n <= 8
        elif kind == "B":
            assert 9 <= n <= 32 and len(s.idx) <= 64 and len({entries[i].plan.mode for i in s.idx}) == 5
        elif kind == "C":
            assert n > 32 and len(s.idx) <= 120
            for k in range(34):  # one literal each, so the ids of the rules under test are 34 and up
                p = RC.read_plan(L, rs.handle, k)
                assert len(p.literals) == 1 and p.equiv
            assert len({RC.read_plan(L, rs.handle, k).pref[0].s for k in range(34)}) == 34
        else:
            assert len(s.idx) > 128
        for k, i in enumerate(s.idx):  # the ruleset compiles each rule to the plan the corpus recorded
            assert RC.read_plan(L, rs.handle, k) == entries[i].plan, entries[i].rule.pattern


def _check_outcomes(s, out):
    """What the oracle found (the results compared equal to it): no error line,
    and both outcomes, per layout, for at least 95 % of the undecided rules."""
    entries = corpus()[0]
    assert out.n_lines == len(s.lines)
    assert not any(f & O.LINE_ERROR for f in out.line_flags)
    n_in = collections.Counter(ln.layout for ln in s.lines)
    hit = collections.Counter((s.lines[r.line_idx].layout, r.rule_idx) for r in out.results)
    undecided = [k for k, i in enumerate(s.idx) if not entries[i].decided]
    for lay in RC.LAYOUTS:
        both = [k for k in undecided if 0 < hit[(lay, k)] < n_in[lay]]
        print("ruleset %s layout %s: %d lines, both outcomes for %d of %d rules" % (s.kind, lay, n_in[lay], len(both), len(undecided)))
        assert len(both) >= 0.95 * len(undecided), (s.kind, lay, [entries[s.idx[k]].rule.pattern for k in undecided if k not in both])
    for k, i in enumerate(s.idx):
        if entries[i].plan.mode == RC.MODE_ALWAYS:
            assert sum(hit[(lay, k)] for lay in RC.LAYOUTS) == len(s.lines)
        if entries[i].plan.mode == RC.MODE_NEVER:
            assert sum(hit[(lay, k)] for lay in RC.LAYOUTS) == 0


def run_case(kind, eng, kernel):
    s = ruleset(kind)
    data = RC.batch(s.lines)
    pair = Pair(s.yaml, eng)
    out = pair.feed(data, RC.TS * S)
    assert eng.line_kernel()[0] == kernel, eng.line_kernel()
    st = eng.scan_stats()
    print("ruleset %s: %d rules, %d lines, %d results, stats %s" % (kind, len(s.idx), len(s.lines), out.n_results, st))
    assert st["literal_hits"] > 0, st
    if kernel != "k_parse_match":  # the wide kernel decides every pair itself and emits no jobs
        assert st["dfa_jobs"] > 0, st
    _check_outcomes(s, out)
    pair.feed(data, (RC.TS + 1) * S)
    assert eng.line_kernel()[0] == kernel
    pair.compare_state(IPS)


@pytest.fixture(scope="module")
def engine():
    e = Engine()
    yield e
    e.close()


@pytest.fixture
def forced_nfa():
    L = _lib.lib()
    assert L.bjx_debug_set_dfa_state_cap(1) == 0
    yield
    L.bjx_debug_set_dfa_state_cap(0)


@pytest.mark.parametrize("kind,kernel", [("A", "k_lines2"), ("B", "k_lines2"), ("C", "k_lines2"), ("D", "k_parse_match")])
def test_default_path(engine, kind, kernel):
    run_case(kind, engine, kernel)


SHORT_ANCHORS = [r"^(HEAD|k) /.*sitemap", r"^ab[0-9]", r"^k /x", r"(?i)^ab\d", r"^(?:a|bc|defgh)-[0-9]", r"^x.*", r"^(?:no|yes).*",
                 r"^a(?:b|cd)\b", r"^(?i:e)noy"]


@pytest.mark.parametrize("wide", [False, True], ids=["k_lines2", "k_parse_match"])
def test_short_anchor_literals(engine, wide):
    """Anchor literals of 1-3 bytes (found by the corpus: `^(HEAD|k) /.*sitemap`
    missed `k /sitemap`).  literal_at compares a whole word first, and the bind
    gave these literals a check window 253-255 bytes in and zero padding, so a
    rule with several anchor literals, or one that is not equivalent, lost every
    match that began with a short one.  Both per-line kernels."""
    pats = SHORT_ANCHORS + ["zq%dzq" % k for k in range(130 if wide else 0)]
    y = ["regexes_with_rates:"]
    for k, p in enumerate(pats):
        y.append("  - rule: 's%d'\n    regex: '%s'\n    interval: 1\n    hits_per_interval: 1000000\n    decision: challenge" % (k, p))
    heads = [b"k /sitemap", b"k /x", b"HEAD /a sitemap", b"ab7", b"AB7", b"aB", b"ab", b"a-1", b"bc-2", b"defgh-3", b"defg-3", b"x", b"xyz",
             b"no", b"yes sir", b"ye", b"abc", b"abcd", b"Enoy", b"enoy", b"eno", b"k", b"k /", b"", b"\xe2\x84\xaa /x", b"zq5zq"]
    lines = []
    for j, h in enumerate(heads):
        lines.append(b"%d 9.9.0.%d " % (RC.TS, j) + h + b" - -")
        lines.append(b"%d 9.9.1.%d " % (RC.TS, j) + h + b" a b")
        lines.append(b"%d 9.9.2.%d GET h.com " % (RC.TS, j) + h)
        if b" " in h:
            lines.append(b"%d 9.9.3.%d " % (RC.TS, j) + h + b" ")
    pair = Pair("\n".join(y) + "\n", engine)
    out = pair.feed(b"\n".join(lines) + b"\n", RC.TS * S)
    assert engine.line_kernel()[0] == ("k_parse_match" if wide else "k_lines2")
    hit = collections.Counter(r.rule_idx for r in out.results)
    assert all(hit[k] > 0 for k in range(len(SHORT_ANCHORS))), hit
    pair.compare_state(["9.9.0.0", "9.9.0.3"])


@pytest.mark.parametrize("kind", ["B", "C"])
@pytest.mark.parametrize("switch,kernel", [("BJX_NO_LINES2", "k_lines"), ("BJX_NO_PLAN", "k_lines2"), ("BJX_NO_DFA_SKIP", "k_lines2")])
def test_bind_switches(kind, switch, kernel, monkeypatch):
    """A bind-time switch is set before the engine and the ruleset exist."""
    monkeypatch.setenv(switch, "1")
    eng = Engine(0)
    try:
        run_case(kind, eng, kernel)
    finally:
        eng.close()


@pytest.mark.parametrize("kind", ["B", "C"])
def test_forced_nfa(engine, forced_nfa, kind):
    """Every rule that fits on the per-lane bit-parallel NFA."""
    s = ruleset(kind)
    rs = Ruleset(Config.from_yaml(s.yaml))
    assert sum(1 for k in range(len(s.idx)) if rs.rule_info(k)[2] & 4) > len(s.idx) // 2
    run_case(kind, engine, "k_lines2")


@pytest.mark.parametrize("kind", ["B", "C"])
def test_line_pass_k_lines(kind):
    """BJX_LINES=1: the engine reads it once per process, so the case runs in a
    process of its own (this file as a program)."""
    env = dict(os.environ, BJX_LINES="1")
    r = subprocess.run([sys.executable, "-m", "tests.test_gpu_rule_plans", kind], env=env, capture_output=True, text=True,
                       cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "case %s k_lines ok" % kind in r.stdout


if __name__ == "__main__":
    assert os.environ.get("BJX_LINES") == "1"
    _eng = Engine(0)
    run_case(sys.argv[1], _eng, "k_lines")
    _eng.close()
    print("case %s k_lines ok" % sys.argv[1])
