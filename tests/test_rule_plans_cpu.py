"""The rule compiler's plan claims as properties, swept over a generated corpus
(tests/rule_corpus.py): what compile_regex (banjax_amd/csrc/regex_compiler.cpp)
says about a pattern beyond its automaton -- the mode, pref_equivalent, the
anchor literals, the lead distance, the per-byte ci flags, gram_off -- checked
on the host against the oracle (Go regexp restated) on texts built to sit on
the edges of each claim.  tests/test_lead_cpu.py holds the named examples;
this is the sweep, and tests/test_gpu_rule_plans.py takes the same corpus
through the device.

For every text T of a rule, M = the oracle's answer on the whole of T:
  P0  bjx_debug_rule_match_host(T) == M (the tables the kernels read)
  P1  ALWAYS: M on every T, the empty one included; NEVER: never M
  P2  PREFILTER: literals of >= 4 bytes, gram_off + 4 <= len, ci only under a
      letter other than k / s; M implies that a pref literal occurs in T
  P3  pref_equivalent: a literal occurring implies M
  P4  ANCHORED with anchor rows: M implies T starts with one; with ^= rows T
      starting with one implies M
  P5  ANCHORED: a match starts at 0: for every matching T and every filler
      prefix p (rule_corpus.PREFIXES) the host tables decide p + T as the
      oracle does, and T[1:] too: the automaton from its start state on T[1:]
      reports only what T[1:] has
  P6  lead >= 0: no pref literal in T implies not M; else with f the first
      occurrence, match_host(T[max(0, f - lead - 3):]) == M (the job start of
      engine.hip lead_bound / slot_lead_start)
"""
import collections
import functools
from dataclasses import dataclass

from banjax_amd import _lib
from oracle import oracle as O
from tests import rule_corpus as RC
from tests.test_cpu_boundary import _one_rule_ruleset

SEED = 20260
N_PATTERNS = 1600
FLOOR = 20  # rules per plan class, at least

# Rules that once violated a property, each with a text that showed it: (pattern, text).
# They are checked on that text and on the texts the corpus would give them.
REGRESSIONS = []


class Violation(Exception):
    pass


@dataclass
class Entry:
    rule: RC.Rule
    plan: RC.Plan
    texts: list          # [(kind, bytes)]
    want: list           # the oracle's answer per text
    violation: str = None

    @property
    def classes(self):
        return RC.plan_classes(self.rule.pattern, self.plan)

    @property
    def decided(self):
        return self.plan.mode in (RC.MODE_ALWAYS, RC.MODE_NEVER)


def _check_plan_shape(plan):
    """The static half of P2."""
    if plan.mode != RC.MODE_PREFILTER:
        return
    if not plan.pref:
        raise Violation("P2: prefilter rule without a literal")
    for l in plan.pref:
        if len(l.s) < 4 or l.gram_off + 4 > len(l.s):
            raise Violation("P2: literal %r, gram_off %d" % (l.s, l.gram_off))
        for c, ci in zip(l.s, l.ci):
            if ci and not (0x61 <= (c | 0x20) <= 0x7A and (c | 0x20) not in b"ks"):
                raise Violation("P2: ci flag under byte %r of %r" % (bytes([c]), l.s))


def _check_text(L, handle, ore, plan, t, m):
    def host(b):
        return bool(L.bjx_debug_rule_match_host(handle, 0, b, len(b)))

    if host(t) != m:
        raise Violation("P0: host tables say %s, the oracle %s" % (not m, m))
    if plan.mode == RC.MODE_ALWAYS and not m:
        raise Violation("P1: an ALWAYS rule the oracle does not match")
    if plan.mode == RC.MODE_NEVER and m:
        raise Violation("P1: a NEVER rule the oracle matches")
    if plan.mode == RC.MODE_PREFILTER:
        f = RC.first_hit(t, plan.pref)
        if f >= 0:
            assert any(RC.lit_at(t, f, l) for l in plan.pref)  # the two occurrence tests agree
        if m and f < 0:
            raise Violation("P2: a match without any pref literal")
        if plan.equiv and f >= 0 and not m:
            raise Violation("P3: equivalent, a literal occurs at %d, no match" % f)
        if plan.lead >= 0 and f >= 0:
            p = max(0, f - plan.lead - 3)
            if host(t[p:]) != m:
                raise Violation("P6: first hit at %d, job start %d decides %s, the whole text %s" % (f, p, not m, m))
    if plan.mode == RC.MODE_ANCHORED:
        starts = any(RC.lit_at(t, 0, l) for l in plan.anchor)
        if plan.anchor and m and not starts:
            raise Violation("P4: a match that starts with no anchor literal")
        if plan.anchor and plan.anchor_equiv and starts and not m:
            raise Violation("P4: ^= and the text starts with an anchor literal, no match")
        if m:
            for p in RC.PREFIXES:
                pt = p + t
                if host(pt) != ore.match(pt):
                    raise Violation("P5: prefix %r: host tables and oracle differ" % p)
            if host(t[1:]) != ore.match(t[1:]):
                raise Violation("P5: T[1:]: host tables and oracle differ")


def check_rule(pattern, plan, texts, extra=()):
    """(the oracle's answers, the first violation or None)."""
    rs = _one_rule_ruleset(pattern)
    L = _lib.lib()
    ore = O.Regex(pattern)
    want = [ore.match(t) for _, t in texts]
    try:
        _check_plan_shape(plan)
        for (kind, t), m in list(zip(texts, want)) + [(("regression", t), ore.match(t)) for t in extra]:
            try:
                _check_text(L, rs.handle, ore, plan, t, m)
            except Violation as v:
                raise Violation("%s on text %r (%s)" % (v, t, kind))
    except Violation as v:
        return want, "%s  pattern %r  plan %r" % (v, pattern, plan)
    return want, None


def _plan_of(pattern):
    rs = _one_rule_ruleset(pattern)
    return RC.read_plan(_lib.lib(), rs.handle, 0)


@functools.lru_cache(maxsize=None)
def corpus(seed=SEED, n=N_PATTERNS):
    """(entries, dropped): every generated rule with its plan, texts, the oracle's
    answers and its first violation.  A rule that is neither ALWAYS nor NEVER and
    for which the oracle does not find both a matching and a non-matching text is
    dropped: nothing could show a claim about it wrong in one of the directions."""
    entries, dropped = [], []
    for k, rule in enumerate(RC.patterns(seed, n, compiles=lambda p: O.compile_error(p) is None)):
        plan = _plan_of(rule.pattern)
        texts = RC.rule_texts(rule, plan, seed * 100003 + k)
        want, bad = check_rule(rule.pattern, plan, texts)
        e = Entry(rule, plan, texts, want, bad)
        if not e.decided and not bad and (all(want) or not any(want)):
            dropped.append(e)
        else:
            entries.append(e)
    return entries, dropped


def test_properties_hold_on_every_rule():
    entries, _ = corpus()
    bad = [e.violation for e in entries if e.violation]
    assert not bad, "%d of %d rules:\n%s" % (len(bad), len(entries), "\n".join(bad))


def test_regressions():
    for pat, text in REGRESSIONS:
        plan = _plan_of(pat)
        rule = next((r for r in RC.patterns(SEED, N_PATTERNS) if r.pattern == pat), None)
        texts = RC.rule_texts(rule, plan, 1) if rule else []
        _, bad = check_rule(pat, plan, texts, extra=[text])
        assert not bad, bad


def class_counts(entries):
    c = collections.Counter()
    for e in entries:
        c.update(e.classes)
    return c


def test_every_plan_class_is_present():
    entries, dropped = corpus()
    assert len(entries) >= 1500
    counts = class_counts(entries)
    print("rules per plan class:", {k: counts[k] for k in RC.PLAN_CLASSES})
    for k in RC.PLAN_CLASSES:
        assert counts[k] >= FLOOR, (k, counts)
    shapes = collections.Counter(e.rule.shape for e in entries)
    for name, _, _ in RC.SHAPES:
        assert shapes[name] >= FLOOR, (name, shapes)


def test_both_outcomes():
    """Every kept rule that the plan does not decide outright has a matching and
    a non-matching text; few rules had to be dropped for having only one."""
    entries, dropped = corpus()
    print("dropped:", [(e.rule.pattern, any(e.want)) for e in dropped])
    assert len(dropped) <= 0.02 * N_PATTERNS, [e.rule.pattern for e in dropped]
    for e in entries:
        if not e.decided:
            assert any(e.want) and not all(e.want), e.rule.pattern


def test_texts_sit_on_the_edges():
    """Equivalent rules are shown near misses of their literals that do not
    match; lead rules with a distance are shown matches with a non-ASCII byte
    or a cut rune inside the bytes a job starts before the hit."""
    entries, _ = corpus()
    near = lead = n_texts = 0
    for e in entries:
        n_texts += len(e.texts)
        assert not any(b"\n" in t for _, t in e.texts)
        if "pref_equiv" in e.classes:
            near += sum(1 for (kind, _), m in zip(e.texts, e.want) if kind in RC.NEAR_MISS and not m)
        if "pref_lead" in e.classes:
            for (_, t), m in zip(e.texts, e.want):
                f = RC.first_hit(t, e.plan.pref)
                if m and f > 0 and any(b >= 0x80 for b in t[max(0, f - e.plan.lead - 3):f]):
                    lead += 1
    print("texts:", n_texts, "near misses on equivalent rules:", near, "lead matches behind non-ASCII bytes:", lead)
    assert near > 0 and lead > 0


def test_occurrence_tests_agree():
    """lit_find (a compiled search) against lit_at (the definition) at every offset."""
    entries, _ = corpus()
    n = 0
    for e in entries[::7]:
        for l in e.plan.literals:
            for _, t in e.texts[::5]:
                want = next((i for i in range(len(t)) if RC.lit_at(t, i, l)), -1)
                assert RC.lit_find(t, l) == want, (l, t)
                n += 1
    assert n > 1000
