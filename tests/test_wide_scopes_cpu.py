"""Self-check of the wide-scope generator (tests/wide_scopes.py), on the host:
every ruleset compiles into the rule modes, literals and scope sizes it is
meant to have, and the oracle alone finds, in both batches of every kind,
enough matching and non-matching lines of every rule kind, position band and
line class, so the GPU tests built on these batches
(tests/test_gpu_wide_scopes.py) cannot pass on an empty class."""
import pytest

from banjax_amd import Config, Ruleset, _lib
from oracle import oracle as O
from tests import long_lines as LL
from tests import rule_corpus as RC
from tests import wide_scopes as WS
from tests.parity import oracle_config


def _compiled(kind):
    cfg = Config.from_yaml(WS.rules_yaml(kind))
    return cfg, Ruleset(cfg)


@pytest.mark.parametrize("kind", WS.KINDS)
def test_rulesets_compile_as_meant(kind):
    cfg, rs = _compiled(kind)
    want = WS.all_rules(kind)
    assert [r.rule for r in cfg.all_rules()] == [r.name for r in want] and len(rs) == len(want)
    L = _lib.lib()
    n_pref = 0
    for i, r in enumerate(want):
        buf = RC.read_plan(L, rs.handle, i)
        mode, equiv = buf.mode, buf.equiv
        assert mode == r.mode, (r.name, r.regex, buf)
        lits = [(l.s, l.any_ci) for l in buf.literals]
        assert lits == r.lits, (r.name, r.regex, buf)
        if mode == WS.MODE_PREFILTER:
            n_pref += 1
            assert bool(equiv) == r.equiv, (r.name, buf)
        if mode == WS.MODE_ANCHORED and r.lits:
            assert buf.anchor and buf.anchor_equiv == r.equiv, (r.name, buf)  # ^= rows or ^~ rows
        if r.letter == "i":  # the literal spells the rule's own host; the scan looks for the host-free piece
            assert r.site.encode() in lits[0][0] and WS.piece_of(lits[0][0], r.site) in (b" POST /xmlrpc.php", b" GET /wp-login.php HTTP/",
                                                                                        b" POST /xmlrpcB.php", b" GET /wp-loginB.php HTTP/")
        assert bool(rs.rule_info(i)[2] & 8) == r.wide, (r.name, rs.rule_info(i))
    # the interned literals: every prefilter literal, the split rules' full literals and their
    # pieces, the anchor literals.  The pieces of the pair every host has are the two global
    # piece rules' own literals, so they add nothing.
    ids = set()
    for r in want:
        ids |= set(r.lits)
        if r.letter == "i":
            ids.add((WS.piece_of(r.lits[0][0], r.site), False))
    assert L.bjx_debug_ruleset_literals(rs.handle) == len(ids)
    if kind in ("MIX", "ALL", "NARROW", "SITE"):
        pieces = {(WS.piece_of(r.lits[0][0], r.site), False) for r in want if r.letter == "i" and r.name.endswith(("001", "002"))}
        assert pieces == {tuple(r.lits[0]) for r in want if r.letter == "p"}
    glob, sites = WS.rules(kind)
    if kind == "NOLIT":
        assert n_pref == 0 and not WS.scan_literals(kind)
    else:
        assert n_pref > 100
    if kind != "NARROW":
        assert len(WS.scope(kind, WS.BIG)) > 128
    else:
        assert max(len(WS.scope(kind, h)) for h in WS.HOSTS) <= 128
    if kind in ("MIX", "NARROW", "SITE"):
        assert len(glob) <= 128
    if kind in ("MIX", "SITE"):
        assert WS.wide_hosts(kind) == [WS.BIG]  # the mixed regime: the other hosts' lines stay with k_lines
    if kind == "WNFA":
        # one wide pattern, three rules; the first of them decides which rule the job list names
        names = [r.name for r in want]
        assert names.index("w_one_plain") < names.index("w_one_skip") < names.index("w_one_big")
        assert names.index("w_two_skip") < names.index("w_two_plain") < names.index("w_two_big")
        assert sum(1 for r in want if r.wide) == 9


def test_fill_alphabet_spells_no_literal():
    for kind in WS.KINDS:
        for s, _ in WS.scan_literals(kind):
            assert not set(s.lower()) <= set(LL.FILL.lower()), s


_runs = {}


def oracle_run(kind):
    """Both batches through one oracle state: per batch (flags, results), and the
    (ip, rule) states that a result of batch 2 found already there."""
    if kind not in _runs:
        cfg = Config.from_yaml(WS.rules_yaml(kind))
        oc = oracle_config(cfg)
        st = O.State()
        out = []
        for seed in WS.SEEDS:
            b = WS.batch(kind, seed)
            before = len(st)
            flags, res, consumed = st.consume(oc, b.data, b.now_ns, cap=b.n_lines * 40)
            assert consumed == len(b.data) and len(flags) == b.n_lines
            out.append((b, flags, res, before))
        _runs[kind] = (out, oc.rule_names)
    return _runs[kind]


def _band(pos):
    return min(pos // 64, 2)


@pytest.mark.parametrize("kind", ["MIX", "ALL", "SITE", "NARROW"])
def test_every_rule_kind_matches_and_misses_in_every_band(kind):
    """Per rule kind a-j, origin (big's site rules, the global rules) and 64-position band
    of big's scope: on big's lines, at least 5 that match a rule of the cell and at least 5
    that hold a token aimed at one (a hit token of another variant, a half token or a near
    miss) without a match.  ALWAYS rules cannot miss: only their matches are counted."""
    runs, names = oracle_run(kind)
    rules = WS.all_rules(kind)
    assert names == [r.name for r in rules]
    big = WS.scope(kind, WS.BIG)
    cell = {}
    for pos, r in enumerate(big):
        if r.letter in "abcdefghij":
            cell[r.name] = (r.letter, "site" if r.site else "global", _band(pos))
    cells = set(cell.values())
    letters = set("abcdefghij")
    for origin in ("site", "global"):
        bands = {c[2] for c in cells if c[1] == origin}
        if origin == "site":
            assert bands == ({0, 1, 2} if kind == "SITE" else {0})
        else:
            assert 2 in bands if kind != "NARROW" else 1 in bands
        for bd in ((0, 1, 2) if (origin, kind) == ("site", "SITE") else ((2,) if kind != "NARROW" else (1,)) if origin == "global" else (0,)):
            have = {c[0] for c in cells if c[1] == origin and c[2] == bd}
            want = letters - ({"i"} if origin == "global" else set())  # split rules are site rules
            if kind == "SITE" and bd == 1:
                want = want - {"i"}  # SITE's split pairs lie at positions 16-17 and 144-145
            assert want <= have, (origin, bd, want - have)
    hit = {c: 0 for c in cells}
    miss = {c: 0 for c in cells}
    for b, flags, res, _ in runs:
        matched = {}
        for x in res:
            matched.setdefault(x.line_idx, set()).add(names[x.rule_id])
        for ln in b.lines:
            if ln.host != WS.BIG or flags[ln.index]:
                continue
            m = matched.get(ln.index, set())
            for c in {cell[n] for n in m if n in cell}:
                hit[c] += 1
            for c in {cell[n] for n in ln.targets if n in cell and n not in m}:
                miss[c] += 1
    for c in sorted(cells):
        assert hit[c] >= 5, (c, hit[c])
        only_always = all(r.sub == "d" for r in big if cell.get(r.name) == c)
        assert only_always or miss[c] >= 5, (c, miss[c])


@pytest.mark.parametrize("kind", ["MIX", "ALL", "SITE"])
def test_skipped_results_overflow_trips_and_carried_state(kind):
    runs, names = oracle_run(kind)
    lits = WS.scan_literals(kind)
    skip_hi = skip_lo = ovf = ovf_big = ovf_big_site = carried = 0
    site_lits = [x for r in WS.rules(kind)[1][WS.BIG] if r.mode == WS.MODE_PREFILTER for x in [(WS.piece_of(r.lits[0][0], WS.BIG), r.lits[0][1])]]
    for k, (b, flags, res, before) in enumerate(runs):
        assert sum(1 for x in res if x.exceeded) >= 20
        for x in res:
            if x.skip_host:
                skip_hi += x.rule_pos >= 128
                skip_lo += x.rule_pos < 128
            if k == 1 and x.seen_ip and x.match_type != 0 and not x.skip_host:
                carried += 1
        for ln in b.lines:
            if flags[ln.index] or ln.cls == "far":
                continue
            rest = ln.text.split(b" ", 2)[2]
            n = LL.count_hits(rest, lits)
            if n > 4:
                ovf += 1
                ovf_big += ln.host == WS.BIG
                ovf_big_site += ln.host == WS.BIG and LL.count_hits(rest, site_lits) > 0
    assert skip_hi >= 20 and skip_lo >= 20, (skip_hi, skip_lo)
    assert ovf >= 150 and ovf_big >= 50 and ovf_big_site >= 25 and ovf_big - ovf_big_site >= 5, (ovf, ovf_big, ovf_big_site)
    # a state of batch 1 met again in batch 2: some (ip, rule) of a batch-2 result had a result in batch 1
    first = {(runs[0][0].lines[x.line_idx].text.split(b" ")[1], x.rule_id) for x in runs[0][2] if not x.skip_host}
    again = sum(1 for x in runs[1][2] if not x.skip_host and (runs[1][0].lines[x.line_idx].text.split(b" ")[1], x.rule_id) in first)
    assert again >= 1 and runs[1][3] > 0


@pytest.mark.parametrize("kind", ["MIX", "ALL", "SITE", "NARROW"])
def test_line_classes(kind):
    """The classes the batches are made of, by what the oracle says about them."""
    runs, names = oracle_run(kind)
    lits = WS.scan_literals(kind)
    by_name = {r.name: r for r in WS.all_rules(kind)}
    hosts_of = {}
    n_far = 0
    for k, (b, flags, res, _) in enumerate(runs):
        matched = {}
        for x in res:
            matched.setdefault(x.line_idx, set()).add(names[x.rule_id])
        by_cls = {}
        for ln in b.lines:
            by_cls.setdefault(ln.cls, []).append(ln)
            hosts_of.setdefault(ln.cls, set()).add(ln.host)
        assert all(flags[ln.index] == O.LINE_ERROR and not ln.spaces4 for ln in by_cls["short"])
        assert all(flags[ln.index] == O.LINE_OLD for ln in by_cls["old"])
        assert all(flags[ln.index] == O.LINE_EXEMPTED for ln in by_cls["allow"])
        assert all(flags[ln.index] == 0 and ln.exotic for ln in by_cls["exotic"]) and len(by_cls["exotic"]) >= 100
        for ln in by_cls["zero"]:
            assert LL.count_hits(ln.text.split(b" ", 2)[2], lits) == 0
        for ln in by_cls["near"]:
            assert not ({n for n in ln.targets if by_name[n].mode == WS.MODE_PREFILTER} & matched.get(ln.index, set())), ln.text[:200]
        assert sum(1 for ln in by_cls["hits"] if 1 <= LL.count_hits(ln.text.split(b" ", 2)[2], lits) <= 4) >= 400
        twice = 0
        for ln in by_cls["twice"]:
            rest = ln.text.split(b" ", 2)[2]
            twice += any(len(LL.hit_positions(rest, [x])) == 2 for x in lits) and LL.count_hits(rest, lits) <= 4
        assert twice >= 100, twice
        # the split rules: per host that has them, the true lines match both rules of the pair, the
        # others hit the piece (its global rule matches) without the site rule
        pair = {h: [r.name for r in WS.rules(kind)[1].get(h, []) if r.letter == "i"] for h in WS.HOSTS}
        t = {h: [0, 0] for h in WS.HOSTS}
        for ln in by_cls["split"]:
            m = matched.get(ln.index, set())
            assert m & {"gp1", "gp2"} or kind == "SITE" and b"B.php" in ln.text, ln.text[:200]
            t[ln.host][bool(m & set(pair[ln.host]))] += 1
        for h in WS.HOSTS:
            if pair[h]:
                assert t[h][0] >= 20 and t[h][1] >= 20, (h, t[h])
            else:
                assert t[h][0] >= 40 and t[h][1] == 0
        # far lines: the verdict the class predicts, and the hit where it is meant to be
        for ln in by_cls["far"]:
            n_far += 1
            rest = ln.text.split(b" ", 2)[2]
            pos = LL.hit_positions(rest, lits)
            assert flags[ln.index] == 0 and len(pos) <= 1 and (not pos or pos[0] in WS.FAR_OFFSETS), (ln.text[:80], pos)
            for name, verdict in ln.expect.items():
                assert (name in matched.get(ln.index, set())) == verdict, (name, verdict, ln.text[:80])
        assert len(by_cls["far"]) == 12
        if kind in ("MIX", "SITE"):
            wide = sum(1 for ln in b.lines if ln.host == WS.BIG and ln.spaces4)
            assert b.fallback_lines() == wide + sum(1 for ln in b.lines if ln.exotic and ln.host != WS.BIG and ln.spaces4)
    for cls in ("zero", "hits", "twice", "ovf_site", "ovf_glob", "shared", "near", "split", "exotic", "old", "short", "allow"):
        assert hosts_of[cls] == set(WS.HOSTS), cls
    assert hosts_of["far"] == {WS.BIG, WS.OTHER}
    # across the two batches every far offset comes as: split true, split with the wrong method, plain literal
    seen = set()
    for b, _, _, _ in runs:
        for ln in b.lines:
            if ln.cls == "far":
                rest = ln.text.split(b" ", 2)[2]
                pos = LL.hit_positions(rest, lits)
                off = pos[0] if pos else len(rest) - 7
                seen.add((off, "split" if b"xmlrpc" in rest else "plain", tuple(sorted(ln.expect.values())), ln.host))
    for off in WS.FAR_OFFSETS:
        got = {x[1:] for x in seen if x[0] == off}
        assert any(g[0] == "split" and g[2] == WS.BIG and False not in g[1] for g in got), (off, got)
        assert any(g[0] == "split" and g[2] == WS.BIG and False in g[1] for g in got), (off, got)
        assert any(g[0] == "split" and g[2] == WS.OTHER for g in got), (off, got)
        assert {g[1] for g in got if g[0] == "plain"} == {(True,), (False,)}, (off, got)
        assert {g[2] for g in got if g[0] == "plain"} == {WS.BIG, WS.OTHER}, (off, got)


def test_host_order_differs_between_the_batches():
    """A line index that is wide in one batch is narrow in the next (the mask words past
    the second are left as they were for a narrow line)."""
    a, b = WS.batch("MIX", 1), WS.batch("MIX", 2)
    flips = sum(1 for x, y in zip(a.lines, b.lines) if (x.host == WS.BIG) != (y.host == WS.BIG))
    assert flips >= 1000, flips


def test_nolit_and_wnfa_batches():
    runs, names = oracle_run("NOLIT")
    rules = WS.all_rules("NOLIT")
    for b, flags, res, _ in runs:
        assert 1400 <= b.n_lines <= 1600
        per_rule = {}
        for x in res:
            per_rule[x.rule_id] = per_rule.get(x.rule_id, 0) + 1
        assert len(per_rule) >= 100                                     # most of the 133 rules match somewhere
        assert sum(1 for x in res if x.rule_pos >= 128) >= 20           # the third mask word
        assert sum(1 for x in res if x.skip_host) >= 5
        assert sum(1 for x in res if x.exceeded) >= 20
        assert 3 * len(res) < b.n_lines * len(rules)
    runs, names = oracle_run("WNFA")
    wide = {r.name for r in WS.all_rules("WNFA") if r.wide}
    for b, flags, res, _ in runs:
        assert 380 <= b.n_lines <= 420
        hits = {n: [0, 0] for n in wide}  # on big, elsewhere
        for x in res:
            if names[x.rule_id] in wide:
                hits[names[x.rule_id]][b.lines[x.line_idx].host != WS.BIG] += 1
        for n, (on_big, off_big) in hits.items():
            assert on_big >= 5, (n, hits)
            assert (off_big >= 5) == (not n.endswith("_big") and n != "w_site_skip"), (n, hits)
        assert sum(1 for ln in b.lines if ln.cls == "wide_miss") >= 40
        # the trio's skipped results on big: what the event count must leave out
        assert sum(1 for x in res if x.skip_host and names[x.rule_id] in ("w_one_skip", "w_two_skip", "w_site_skip")) >= 15
        assert sum(1 for x in res if x.exceeded) >= 20
    # a line that misses by one byte matches no wide rule of its pattern
    b, flags, res, _ = runs[0]
    matched = {}
    for x in res:
        matched.setdefault(x.line_idx, set()).add(names[x.rule_id])
    n_clean = sum(1 for ln in b.lines if ln.cls == "wide_miss" and not (matched.get(ln.index, set()) & wide))
    assert n_clean >= 30, n_clean
