"""Self-check of the long-line generator (tests/long_lines.py), on the host:
every layout has the geometry and the hit counts it is meant to have, every
ruleset is of the literal-count class it is meant to be, and for every rule
the oracle finds both matching and non-matching lines in every layout that
holds the rule's literal, so the GPU tests built on these batches can fail in
either direction."""
import pytest

from banjax_amd import Config, Ruleset, _lib
from oracle import oracle as O
from tests import long_lines as LL
from tests import rule_corpus as RC
from tests.parity import oracle_config

SEEDS = (1, 2)  # the seeds tests/test_gpu_long_line_hits.py feeds
TILE, HALO = LL.TILE, LL.HALO


def _rule_literals(rs, i):
    """(mode, [(bytes, ci)]) of rule i from bjx_debug_rule_literal."""
    plan = RC.read_plan(_lib.lib(), rs.handle, i)
    return plan.mode, [(l.s, l.any_ci) for l in plan.literals]


@pytest.mark.parametrize("kind", LL.RULESETS)
def test_ruleset_literal_classes(kind):
    """The literal count selects the paths under test: at most 8 keeps a first
    candidate per literal (Bind::cfirst), at most 32 keeps the summary bits
    exact (Bind::lits_small); ids go in rule order, so C1's targets lie past 32."""
    cfg = Config.from_yaml(LL.rules_yaml(kind))
    rs = Ruleset(cfg)
    L = _lib.lib()
    n = L.bjx_debug_ruleset_literals(rs.handle)
    want = LL.literals(kind)
    got = set()
    for i in range(len(rs)):
        got |= set(_rule_literals(rs, i)[1])
    assert got == set(want), got ^ set(want)
    assert n == len(want)
    if kind == "A":
        assert n <= 8
    elif kind == "B":
        assert 9 <= n <= 32
    else:
        assert n > 32
    names = [r.rule for r in cfg.all_rules()]
    if kind == "C1":
        assert names[:40] == ["fill%d" % k for k in range(40)]
        for i in range(40):  # one literal each, so every target's ids are 40 and up
            assert _rule_literals(rs, i)[1] == [(LL.filler_literal(i), False)]
    if kind == "C2":
        assert names[:6] == ["mac firefox", "scrapers", "ahrefs", "any firefox", "hay", "lead"]
    if kind == "D":
        assert len(cfg.regexes_with_rates) > 128
    if kind != "A":
        assert L.bjx_debug_rule_lead(rs.handle, names.index("lead")) == 4
    assert L.bjx_debug_rule_lead(rs.handle, names.index("scrapers")) == 4
    assert L.bjx_debug_rule_lead(rs.handle, names.index("mac firefox")) == 0


def test_fill_alphabet_spells_no_literal():
    for kind in LL.RULESETS:
        for s, _ in LL.literals(kind):
            assert not set(s.lower()) <= set(LL.FILL.lower()), s


@pytest.mark.parametrize("seed", SEEDS)
def test_geometry(seed):
    b = LL.batch(seed)
    assert len(b.data) <= 12 << 20
    assert b.data.count(b"\n") == b.n_lines and b.data.endswith(b"\n")
    by_layout = {k: [ln for ln in b.lines if ln.layout == k] for k in LL.LAYOUTS}
    for k, lines in by_layout.items():
        assert len(lines) >= 100, k
    spread = [ln.start % TILE for ln in b.lines if ln.klass != "edge"]
    assert len(set(spread)) > 0.85 * len(spread)
    for ln in b.lines:
        s, n = ln.start, len(ln.text)
        assert b.data[s:s + n] == ln.text and b.data[s + n:s + n + 1] == b"\n" and (s == 0 or b.data[s - 1:s] == b"\n")
        assert b.data.count(b"\n", 0, s) == ln.index
        assert ln.text.split(b" ", 2)[2] == ln.text[ln.rest_off:]
        u = s % TILE
        if ln.klass == "two":
            assert 4700 <= n < 6000
        elif ln.klass == "mid":
            assert 9000 <= n < 13000
        elif ln.klass == "big":
            assert 19000 <= n < 21000
        elif ln.klass == "cap":
            # long through lk >= kLineCap: 128 or more lines start before it in its tile
            assert n == 300 and b.data.count(b"\n", s - u, s) >= LL.LINE_CAP + 1
        elif ln.klass == "edge":
            # no '\n' in the tile it starts with, yet it ends in that tile's halo
            assert u == 0 and TILE <= n < TILE + HALO
        else:
            assert ln.klass == "halo" and 600 <= n <= 4500 and TILE <= u + n < TILE + HALO
        if ln.klass in ("two", "mid", "big"):
            assert u + n >= TILE + HALO  # past the halo: several waves see it
    for k in LL.LAYOUTS:
        want = {"two", "mid", "big", "cap", "halo", "edge"} if k not in (4, 8, 9) else {"mid", "big"}
        assert want <= {ln.klass for ln in by_layout[k]}, k


def test_tile_start_batch():
    """Every line from a tile's first byte to its halo, every hit a true literal
    clear of the tile edges, and hits on both sides of the tile's end."""
    b = LL.tile_start_batch(3)
    n_after = n_sparse = 0
    for kind in LL.RULESETS:
        assert LL.count_hits(b.data, LL.literals(kind)) == sum(ln.expect_hits for ln in b.lines)
    for ln in b.lines:
        n = len(ln.text)
        assert ln.start % TILE == 0 and TILE <= n < TILE + HALO and b.data[ln.start:ln.start + n + 1] == ln.text + b"\n"
        pos = LL.hit_positions(ln.text, LL.literals("A"))
        assert len(pos) == ln.expect_hits
        assert all(p + 16 <= TILE or p >= TILE for p in pos)
        n_after += any(p >= TILE for p in pos)
        n_sparse += 0 < len(pos) <= LL.SLOTS and any(p >= TILE for p in pos)
    assert n_after >= 60 and n_sparse >= 30


def test_golden_cfg4_lines():
    """tests/golden/long_line_hits.json.gz (tests/test_golden.py runs it through
    the oracle and the engine): its long lines are lines of workload cfg4,
    verbatim, each on a tile's first byte and ending in that tile's halo."""
    import workloads as W
    b = LL.golden_batch()
    assert b.data == LL.cfg4_tile_start_log()
    assert len(b.lines) == len(LL.CFG4_TILE_START_LINES) >= 8
    n_after = 0
    for idx, ln in zip(LL.CFG4_TILE_START_LINES, b.lines):
        n = len(ln.text)
        assert W.CFG4.host_lines(idx, 1) == ln.text + b"\n"
        assert ln.start % TILE == 0 and TILE <= n < TILE + HALO and b.data[ln.start:ln.start + n + 1] == ln.text + b"\n"
        n_after += any(p >= TILE for p in LL.hit_positions(ln.text, LL.literals("A")))
    assert n_after >= 4  # hits past the tile's end: the ones that were recorded twice


@pytest.mark.parametrize("kind", LL.RULESETS)
@pytest.mark.parametrize("seed", SEEDS)
def test_hit_counts(seed, kind):
    b = LL.batch(seed)
    lits = LL.literals(kind)
    n_first_tile = n_three_tiles = n_long = 0
    for ln in b.lines:
        pos = LL.hit_positions(ln.text, lits)
        if ln.layout in (9, 10):
            assert len(pos) == ln.expect_hits and ln.expect_hits in (3, 4, 5), (ln.layout, ln.variant)
        else:
            assert len(pos) >= LL.SLOTS + 1, (ln.layout, ln.variant, ln.klass, len(pos))
        tiles = [(ln.start + p) // TILE for p in pos]
        if ln.layout == 9:
            assert len(set(tiles)) == len(tiles)
        if ln.layout == 10:
            assert len({ln.text[p:p + 5] for p in pos}) < len(pos)  # a literal repeats
        if ln.layout <= 7 and ln.klass in ("mid", "big"):
            # the hits race: several waves record them.  Two tiles is the floor per
            # line, three the rule: a 9 KB line that starts late in a tile has two whole
            # tiles and a few hundred bytes in the first and the last, where the
            # layout may put a near miss or nothing; the crowded variants put five
            # of their hits into one tile on purpose.  So three tiles are asserted
            # over the class (three lines in four), two per line.
            assert len(set(tiles)) >= 2, (ln.layout, ln.variant, tiles)
            n_long += 1
            n_three_tiles += len(set(tiles)) >= 3
        if ln.layout <= 7 and ln.klass in ("two", "mid", "big") and tiles.count(ln.start // TILE) >= 4:
            n_first_tile += 1
        if ln.layout == 8:
            assert len(pos) >= 300
            dense = [p for p in pos if ln.text[p:p + 9] == b"Firefox/ "]
            assert len(dense) == 300 and len({(ln.start + p) // TILE for p in dense}) == 1
            assert ln.text.count(b"Firefox/9") == ln.variant % 2
    assert n_three_tiles >= 0.75 * n_long and n_long >= 200 and n_first_tile >= 30, (n_three_tiles, n_long, n_first_tile)


@pytest.mark.parametrize("seed", SEEDS)
def test_layout_properties(seed):
    b = LL.batch(seed)
    seen = {"edge": 0, "halo_end": 0, "true": 0, "near": 0, "ip4": 0, "host4": 0, "rest_start": 0, "lead_edge": 0}
    ks = set()
    for ln in b.lines:
        o = LL.OWN[ln.own]
        lit, low, ro, n = o["lit"].lower(), ln.text.lower(), ln.rest_off, len(ln.text)
        own_pos = LL.hit_positions(ln.text, [(o["lit"], True)])
        if ln.layout == 1:
            assert lit in low[:ro]
            if ln.variant % 3 != 1:
                assert all(p < ro for p in own_pos)
            else:
                assert b" Macintosh.Firefox/1.example " in ln.text[ro:ro + 40]
        elif ln.layout == 2:
            assert all(p >= n - 16 for p in own_pos)
            assert own_pos or ln.variant % 3 == 2
        elif ln.layout == 3:
            assert all(ro <= p < LL.CERTAIN_GAP for p in own_pos) and ro < 64
            assert own_pos or ln.variant % 3 == 2
        elif ln.layout == 4:
            assert all(p >= LL.CERTAIN_GAP for p in own_pos)
            if ln.variant % 2:  # in the IP field: the header runs past kCertainGap
                assert ro > LL.CERTAIN_GAP and all(p < ro for p in own_pos)
                seen["ip4"] += bool(own_pos)
            else:
                host_end = ln.text.index(b" ", ln.text.index(b" ", ro) + 1)
                assert all(ro < p < host_end for p in own_pos)
                seen["host4"] += bool(own_pos)
        elif ln.layout == 5 and ln.straddle:
            B, k, t = ln.straddle
            assert 0 < k < len(t) and b.data[B - k:B - k + len(t)] == t and ln.start < B - k and B + len(t) < ln.start + n
            assert B % TILE in (0, HALO)
            seen["edge" if B % TILE == 0 else "halo_end"] += 1
            seen["true" if t in o["true"] else "near"] += 1
            ks.add(k)
        elif ln.layout == 6:
            cands = [ln.text.find(t) for t in o["near"] + o["half"] if t in ln.text]
            trues = [ln.text.rfind(t) for t in o["true"] if t in ln.text]
            assert cands and min(cands) < n // 2
            assert max(trues) > n // 2 if ln.variant % 3 else not trues
        elif ln.layout == 7:
            assert ln.own in ("scr", "tok", "mech")
            # a bounded-lead literal 0-4 bytes into rest: its bounded piece starts at or before rest
            lead_pos = LL.hit_positions(ln.text, [(b"crapy", True), (b"=token", False), (b"mechanize", True)])
            if any(ro <= p <= ro + 4 for p in lead_pos):
                seen["rest_start"] += 1
            if any((ln.start + p) % TILE == 0 for p in own_pos):
                seen["lead_edge"] += 1
    assert seen["edge"] >= 25 and seen["halo_end"] >= 15 and seen["true"] >= 20 and seen["near"] >= 10, seen
    assert seen["ip4"] >= 20 and seen["host4"] >= 20 and seen["rest_start"] >= 15 and seen["lead_edge"] >= 8, seen
    assert len(ks) >= 8
    for pre in (b"\xc3\xa9", b"\xc5\xbf", b"\xe2\x84\xaa", b"\xff"):
        assert sum(1 for ln in b.lines if ln.layout == 7 and (pre + b"crapy" in ln.text or pre + b"=token" in ln.text
                                                             or pre + b"mechanize" in ln.text)) >= 3, pre


_matches = {}


def oracle_matches(seed, kind):
    """{rule name: set of batch line indices the oracle matches}, and the rule names."""
    if (seed, kind) not in _matches:
        b = LL.batch(seed)
        cfg = Config.from_yaml(LL.rules_yaml(kind))
        oc = oracle_config(cfg)
        n_rules = len(cfg.all_rules())
        flags, res, consumed = O.State().consume(oc, b.data, b.now_ns, cap=(b.n_lines + 1) * 8 + 1024)
        assert consumed == len(b.data)
        assert not any(flags[ln.index] for ln in b.lines)  # only the one-byte lines are in error
        names = [r.rule for r in cfg.all_rules()]
        assert len(names) == n_rules == len(oc.rule_names)
        m = {nm: set() for nm in names}
        for r in res:
            m[oc.rule_names[r.rule_id]].add(r.line_idx)
        _matches[(seed, kind)] = (m, sum(1 for r in res if r.exceeded))
    return _matches[(seed, kind)]


RULE_LITS = {"mac firefox": [b"macintosh"], "scrapers": [b"crapy", b"mechanize"], "ahrefs": [b"ahrefsbot"],
             "semrush": [b"semrushbot"], "any firefox": [b"firefox/"], "hay": [b"haystack"], "lead": [b"=token"],
             "site": [b"sitelit"], "equiv": [b"needle"]}


@pytest.mark.parametrize("kind", LL.RULESETS)
@pytest.mark.parametrize("seed", SEEDS)
def test_every_rule_matches_and_misses_in_every_layout(seed, kind):
    b = LL.batch(seed)
    m, n_trips = oracle_matches(seed, kind)
    assert n_trips > 50  # the limits are low enough for trips
    checked = 0
    for rule, lits in RULE_LITS.items():
        if rule not in m:
            continue
        for k in LL.LAYOUTS:
            lines = [ln for ln in b.lines if ln.layout == k]
            if not any(t in ln.text.lower() for ln in lines for t in lits):
                continue
            hit = sum(1 for ln in lines if ln.index in m[rule])
            assert 0 < hit < len(lines), (rule, k, hit, len(lines))
            checked += 1
    assert checked >= (40 if kind == "A" else 60)
