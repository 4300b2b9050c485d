"""tests/job_shapes.py against itself and against the rule compiler (no GPU):
the rule classes from Ruleset.rule_info, the planned job counts recounted from
the emitted bytes, every block composition the plan has to contain, and the
text-edge generator's offsets recomputed from the bytes."""
import collections
import ctypes as C

import pytest

from banjax_amd import Config, Ruleset, _lib
from oracle import oracle as O
from tests import job_shapes as J


def _compiled(ruleset):
    return Ruleset(Config.from_yaml(J.rules_yaml(ruleset)))


def _literal(rs, i):
    buf = C.create_string_buffer(256)
    n = _lib.lib().bjx_debug_rule_literal(rs.handle, i, buf, 256)
    return buf.raw[:n]


@pytest.mark.parametrize("ruleset", ["MAIN", "EDGE", "BIG", "GROW"])
def test_rule_classes(ruleset):
    """The classes as the issue defines them, from the compiled rules; one literal per rule, the planned one."""
    rules = J.rules(ruleset)
    rs = _compiled(ruleset)
    assert len(rs) == len(rules)
    assert _lib.lib().bjx_debug_ruleset_literals(rs.handle) == len(rules)
    for i, R in enumerate(rules):
        st, ncls, fl = rs.rule_info(i)
        if R.cls == "S":
            assert ncls * st <= 8192 and st <= 2048 and not fl & 12, (i, R.regex, st, ncls)
        elif R.cls == "T":
            assert ncls * st > 8192 and st <= 2048 and not fl & 12, (i, R.regex, st, ncls)
        elif R.cls == "A":
            assert 2048 < st <= 4096 and ncls * st > 8192 and not fl & 12, (i, R.regex, st, ncls)
        elif R.cls == "L":
            assert 2048 < st <= 4096 and ncls * st <= 8192 and ncls <= 3 and not fl & 12, (i, R.regex, st, ncls)
        elif R.cls == "N":
            assert fl & 4 and not fl & 8, (i, R.regex, fl)
        else:
            assert fl & 8, (i, R.regex, fl)
        assert J.class_of(st, ncls, fl) == R.cls
        lead = _lib.lib().bjx_debug_rule_lead(rs.handle, i)
        if R.kind == "anchored":
            assert b"GET " in _literal(rs, i) and st >= 256 and lead == -1
        else:
            assert R.lit in _literal(rs, i) and lead == (-1 if R.kind == "xstar" else 0), (i, R.regex, lead)
    if ruleset == "MAIN":
        nfa = sorted(rs.rule_info(i)[0] for i, R in enumerate(rules) if R.cls == "N")
        assert nfa[-1] > 10 * nfa[0]                       # two NFA sizes: 2 and 16 state words
        assert rules[0].cls == "N" and rules[-1].cls == "N" and rules[35].cls == rules[36].cls == "N"
        assert max(collections.Counter(R.host for R in rules).values()) <= 128
        assert {R.cls for R in rules[32:35]} == {"S", "T", "A"}  # DFA rules with literal ids past 32


def _line_starts(data):
    out, s = [], 0
    for t in data.split(b"\n")[:-1]:
        out.append((s, t))
        s += len(t) + 1
    return out


def _occurrences(text, lit):
    n, i = 0, text.find(lit)
    while i >= 0:
        n, i = n + 1, text.find(lit, i + 1)
    return n


def _recount(b, no_lines2=False):
    """(windowed, legacy) per rule from the batch's bytes alone: which rule's literal each line spells, and how often."""
    rules = b.rules
    w, g = [0] * len(rules), [0] * len(rules)
    hosts = {R.host for R in rules}
    assert len(_line_starts(b.data)) == len(b.lines)
    for (s, text), ln in zip(_line_starts(b.data), b.lines):
        assert (s, text) == (ln.start, ln.text)
        f = text.split(b" ")
        if len(f) < 3:
            assert ln.rule < 0
            continue
        rest = text.split(b" ", 2)[2]
        hits = {i: _occurrences(rest, R.lit) for i, R in enumerate(rules) if R.lit in rest}
        if f[3].decode() not in hosts:
            assert ln.rule < 0
            continue
        own = [i for i in hits if rules[i].host == f[3].decode()]
        if b.ruleset == "GROW":
            assert sorted(hits) == list(range(32)) and set(hits.values()) == {1}
            for i in hits:
                g[i] += 1
            continue
        anchored = [i for i, R in enumerate(rules) if R.kind == "anchored" and R.host == f[3].decode() and rest.startswith(b"GET ")]
        if anchored:
            assert ln.rule == anchored[0]
            (g if no_lines2 else w)[ln.rule] += 1
            continue
        assert list(hits) == own and len(own) <= 1, (text, hits)
        if not own:
            assert ln.rule < 0
            continue
        r = own[0]
        assert ln.rule == r and hits[r] in (1, 2, 5), (text, hits)
        overflow = hits[r] > 4
        if overflow or no_lines2 or b.ruleset == "BIG" or rules[r].nfa or r >= 32:
            g[r] += 1
        else:
            w[r] += 1
    return w, g


@pytest.mark.parametrize("name", list(J.cases()))
def test_planned_counts_recounted(name):
    c = J.cases()[name]
    b = c.batch()
    assert _recount(b, c.no_lines2) == c.counts
    per = collections.Counter()
    for it in c.items:
        per[it.rule] += it.n
    assert per == collections.Counter(ln.rule for ln in b.lines if ln.rule >= 0)
    assert len(b.lines) <= 10_000
    assert sum(map(sum, c.counts)) == sum(bl.lanes for bl in c.blocks())


def _all_runs(pred_case=lambda c: True):
    return [(c, r) for c in J.cases().values() if pred_case(c) for r in c.runs()]


def _all_blocks(pred_case=lambda c: True):
    return [(c, bl) for c in J.cases().values() if pred_case(c) for bl in c.blocks()]


def test_classify_blocks_names():
    cls = ["S", "T", "N", "W"]
    kinds = lambda w, g: [(b.kind, b.cls, b.lanes) for b in J.classify_blocks((w, g), cls)]  # noqa: E731
    assert kinds([256, 1, 0, 0], [0, 0, 0, 0]) == [("uniform", "S", 256), ("uniform", "T", 1)]
    assert kinds([255, 2, 0, 0], [0, 0, 0, 0]) == [("mixed", "S", 256), ("uniform", "T", 1)]
    assert kinds([10, 0, 0, 0], [5, 0, 0, 0]) == [("windowed+legacy", "S", 15)]
    assert kinds([0, 0, 0, 0], [5, 5, 7, 0]) == [("legacy+nfa", "S", 17)]
    assert kinds([0, 0, 0, 0], [0, 0, 256, 3]) == [("nfa", "N", 256), ("nfa", "W", 3)]
    assert kinds([0, 0, 0, 0], [0, 0, 0, 0]) == []


def test_plan_contains_every_composition():
    """Every composition the job kernels branch on; none may be missing."""
    k2 = lambda c: not c.no_lines2  # noqa: E731
    runs = _all_runs(k2)
    for cls in "ST":   # runs from a block's first lane, windowed
        for n in J.SIZES:
            assert any(r.cls == cls and r.n == n and r.start % 256 == 0 and not r.legacy for _, r in runs), (cls, n)
    for lane in (1, 128, 255):
        assert any(r.n == 257 and r.start % 256 == lane and not r.legacy for _, r in runs), lane
    blocks = _all_blocks()
    assert any(len({p[1] for p in bl.parts}) == 256 and bl.lanes == 256 for _, bl in blocks)   # 256 rules, one job each
    totals = {sum(map(sum, c.counts)) for c in J.cases().values() if k2(c)}
    assert {t % 256 for t in totals if t} >= {0, 1, 255} and 1 in totals and 0 in totals
    k2b = _all_blocks(k2)
    assert any(bl.kind == "windowed+legacy" for _, bl in k2b)
    assert any(bl.kind == "uniform" and bl.legacy and bl.lanes == 256 and bl.cls in "ST" for _, bl in k2b)
    assert any(bl.kind == "legacy+nfa" for _, bl in k2b)
    nfa = [r for c, r in runs if r.cls == "N"]
    assert {1, 256, 257} <= {r.n for r in nfa}
    n_rules = len(J.rules("MAIN"))
    assert {0, n_rules - 1} <= {r.rule for r in nfa}
    by_case = collections.defaultdict(list)
    for c, r in runs:
        by_case[c.name].append(r)
    assert any(a.cls == "N" and b.cls == "N" and b.rule == a.rule + 1 for rr in by_case.values() for a, b in zip(rr, rr[1:]))
    assert {1, 257} <= {r.n for _, r in runs if r.cls == "W"}
    for cls in "AL":
        assert any(bl.kind == "uniform" and bl.cls == cls and not bl.legacy and bl.lanes == 256 for _, bl in k2b), cls
        assert any(bl.kind == "mixed" and cls in {p[2] for p in bl.parts} for _, bl in k2b), cls
    # the three sources of legacy DFA jobs
    assert any(r.legacy and r.rule < 32 and r.cls in "STAL" for _, r in _all_runs(lambda c: c.no_lines2))
    assert any(r.legacy and r.rule >= 32 and r.cls in "STA" for _, r in runs)
    assert any(it.overflow for c in J.cases().values() if k2(c) for it in c.items)
    # every class under BJX_NO_LINES2 too
    assert {r.cls for _, r in _all_runs(lambda c: c.no_lines2)} >= set("STALNW")


def _job_from_bytes(R, start, text):
    rest_off = len(text) - len(text.split(b" ", 2)[2])
    if R.kind == "xstar":
        return start + rest_off
    if R.kind == "anchored":
        return start + rest_off + 4
    return start + rest_off + text[rest_off:].index(R.lit)


@pytest.mark.parametrize("r", [r for rs in J.EDGE_RULES.values() for r in rs])
def test_edge_offsets_from_bytes(r):
    b = J.edge_uniform(r)
    R = b.rules[r]
    assert _recount(b) == J.edge_counts(b)
    ore = O.Regex(R.regex)
    jobs = [(ln, s) for (s, _), ln in zip(_line_starts(b.data), b.lines) if ln.rule == r]
    by_kind = collections.defaultdict(list)
    for ln, s in jobs:
        assert ln.job == _job_from_bytes(R, s, ln.text)
        by_kind[ln.kind].append(ln)
    assert set(by_kind) <= set(J.EDGE_KINDS)
    L = len(R.lit)
    for kind, lns in by_kind.items():
        if kind != "rune_cut":
            assert {ln.job % 16 for ln in lns} >= (set(range(16)) if kind in ("len", "esc_in_skip", "dollar_late") else {0}), kind
    nl = [(ln, ln.start + len(ln.text)) for ln in by_kind["len"]]
    if R.kind in ("xstar", "anchored"):
        assert {e % 16 for _, e in nl} == set(range(16))
    else:
        first = {e % 16 for ln, e in nl if e >> 4 == ln.job >> 4}
        second = {e % 16 for ln, e in nl if e >> 4 == (ln.job >> 4) + 1}
        assert first == set(range(L, 16)) and second == set(range(16)), (first, second)
    rest = lambda ln: ln.text.split(b" ", 2)[2]  # noqa: E731
    if R.kind in ("dotk", "dollar", "L", "anchored"):
        # the match completes on the last byte before the '\n', at every start offset
        done = {ln.job % 16 for ln in by_kind["len"] if ore.match(rest(ln)) and not ore.match(rest(ln)[:-1])}
        assert done == set(range(16))
    if R.kind == "dollar":
        assert len(by_kind["dollar_late"]) == 16
        assert all(not ore.match(rest(ln)) and ore.match(rest(ln)[:-1]) for ln in by_kind["dollar_late"])
    hi = {(ln.start + ln.text.index(b"\xc3")) % 16 for ln in by_kind["nonascii"]}
    assert hi == set(range(16)), hi
    if R.kind != "anchored":
        assert any(ln.text.endswith(b"\xe2\x84") for ln in by_kind["rune_cut"])
    outcomes = collections.defaultdict(set)
    for ln, _ in jobs:
        outcomes[ln.kind].add(ore.match(rest(ln)))
    if R.kind in ("star", "xstar"):
        if R.kind == "star":
            assert {ln.job % 16 for ln in by_kind["esc_before"]} >= set(range(1, 16))
            assert all(b.data[ln.job - 1:ln.job] == b"d" for ln in by_kind["esc_before"])
        assert outcomes["esc_before"] == {False} and outcomes["esc_next_line"] == {False}
        for ln in by_kind["esc_next_line"]:
            e = ln.start + len(ln.text)
            assert b.data[e:e + 2] == b"\nd"
        at = collections.Counter()
        for ln in by_kind["esc_in_skip"]:
            t = ln.text[ln.text.index(R.lit) + L:]
            assert len(t) >= 64
            at[min(i for i in range(len(t)) if t[i:i + 1] in (b"d", b"q"))] += 1
        assert set(at) == {1, 16, 17}
        assert outcomes["esc_in_skip"] == {True, False}
    assert outcomes["len"] == {True, False} and outcomes["nonascii"] == {True, False}


def test_edge_texts_host_tables_agree_with_oracle():
    """Every edge line through the rule's compiled tables on the host: the rule compiler, without a GPU."""
    rs = _compiled("EDGE")
    L = _lib.lib()
    n = 0
    for rr in J.EDGE_RULES.values():
        for r in rr:
            ore = O.Regex(J.rules("EDGE")[r].regex)
            for ln in J.edge_uniform(r).lines:
                if ln.rule == r:
                    t = ln.text.split(b" ", 2)[2]
                    assert L.bjx_debug_rule_match_host(rs.handle, r, t, len(t)) == int(ore.match(t)), (r, t)
                    n += 1
    assert n > 8000


@pytest.mark.parametrize("no_lines2", [False, True])
def test_edge_blocks_uniform_and_mixed(no_lines2):
    classes = [R.cls for R in J.rules("EDGE")]
    jobs = collections.Counter()
    for b in J.edge_mixed():
        cnt = J.edge_counts(b, no_lines2)
        assert _recount(b, no_lines2) == cnt
        assert len(b.lines) <= 10_000
        blocks = J.classify_blocks(cnt, classes)
        assert blocks and not any(bl.kind == "uniform" for bl in blocks), [(bl.kind, bl.cls, bl.lanes) for bl in blocks]
        jobs.update({r: cnt[0][r] + cnt[1][r] for r in range(len(classes))})
    for rr in J.EDGE_RULES.values():
        for r in rr:
            b = J.edge_uniform(r)
            assert jobs[r] == sum(1 for ln in b.lines if ln.rule == r)   # every spec is in some mixed batch
            assert {bl.kind for bl in J.classify_blocks(J.edge_counts(b, no_lines2), classes)} <= {"uniform", "nfa"}


def test_last_line_batches():
    for r in (1, 4, 10, 13):
        for mixed in (False, True):
            bs = J.last_line_batches(r, mixed)
            assert sorted(len(b.data) % 16 for b in bs) == list(range(16))
            for b in bs:
                assert b.lines[-1].rule == r and b.data.endswith(b.lines[-1].text + b"\n")
                cnt = J.edge_counts(b)
                assert _recount(b) == cnt and sum(map(sum, cnt)) == (2 if mixed else 1)


def test_growth_batch_passes_the_fresh_job_buffers():
    """engine.hip match_phase: jline.ensure(max(n, lines + 2^20)), DevBuf::ensure allocates want + want / 4."""
    n = J.GROW_LINES
    assert n * 32 > (n + (1 << 20)) * 5 // 4
    b = J.grow_batch()
    assert len(b.lines) == n == b.data.count(b"\n")
    w, g = _recount(b)
    assert w == [0] * 32 and g == [n] * 32
    ore = [O.Regex(R.regex) for R in b.rules]
    for i in (0, 1, 31, 4321):
        rest = b.lines[i].text.split(b" ", 2)[2]
        assert [k for k in range(32) if ore[k].match(rest)] == sorted({i % 32, (7 * i + 3) % 32})
