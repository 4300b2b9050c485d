"""Lines whose literal hits overflow, or race for, the scan pass's hit slots.

k_scan gives a line that one wave sees whole (it fits the 4,096-byte tile plus
the 512-byte halo, and starts after fewer than 128 other lines of its tile)
its four hit slots from LDS, in position order.  Every other line is a long
line: its hits come from several waves, each taking slot indices from an
atomic counter, so WHICH four hits are kept exactly and which are folded into
the line's summary (CandMeta: occurrence bits, verified-and-far bits, the
lowest position) differs from run to run.  Every consumer of the slots
branches on that (lines2.h l2_job_rec and the hit loop of k_lines2;
engine.hip lead_start, lead_seek, eq_certain, decide_rules), and the result
must not.

batch(seed) builds one batch of such lines, LINES_PER_LAYOUT of each layout
below, each behind a filler line of random length so that every line starts at
another offset of its tile.  A line is `<ts> <ip> <method> <host> <method>
/<body>`; the header the engine skips is `<ts> <ip> ` (rest, the text the
rules see, begins at the first method field and holds the host).

Layouts (Line.layout):
  1  the own literal only in the header (the IP field), 5-12 other hits in rest;
     every third line's host is Macintosh.Firefox/1.example
  2  the own literal only in the line's last 16 bytes, other hits in every tile before
  3  the own literal in rest, less than 256 bytes (kCertainGap) into the line, the others far
  4  a host (in rest) or an IP field (header) of 300-700 bytes holding the own
     literal 256 bytes or more into the line; none of it elsewhere
  5  straddles: the own token, true or a near miss, crossing a tile edge or
     the end of a tile's halo by 1 .. len - 1 bytes
  6  false first: a near miss of the own literal early, the true one late
  7  bounded-lead rules: the bounded piece crossing the start of rest, crossing
     a tile edge, and non-ASCII bytes directly before the literal
  8  dense: 300 x "Firefox/ " inside one tile of a long line (past both per-round
     list caps of k_scan), with and without a final "Firefox/9"
  9  three or four hits in all, in distinct tiles (no overflow: only the slot order varies)
  10 exactly four and exactly five hits, with repeats of one literal

Length classes (Line.klass): "two" 4.7-6 KB, "mid" 9-13 KB, "big" about 20 KB,
"cap" 300 bytes after 140 one-byte lines of the same tile, "halo" 600-4,500
bytes ending in the halo of the tile they start in (the in-window control),
"edge" 4,096-4,600 bytes from a tile's first byte: the tile holds no '\n', so
the next tile takes the line for one begun earlier, though it ends in the halo.
"""
from __future__ import annotations

import random
from dataclasses import dataclass, field

TILE, HALO = 4096, 512
LINE_CAP, SLOTS, CERTAIN_GAP = 128, 4, 256
T0 = 1700000000
LINES_PER_LAYOUT = 100
LAYOUTS = tuple(range(1, 11))
# no byte sequence over this alphabet spells a literal of any ruleset below
FILL = b"bdgjkquvwz_-:;,+~. "
IPS = ["10.7.%d.%d" % (k // 8, k % 8) for k in range(40)]
BOUNDED_LEAD = r"[a-z]{1,4}=token"  # tests/test_lead_cpu.py CASES, distance 4

# own literal of a line -> its literal, tokens that make its rule match ("true"; "mac" also
# needs a Firefox/<digit> after it, "site" and "needle" the host h.com), tokens that hold the
# literal without a match ("half"), and near misses of the literal: first or last byte
# changed, a 4-byte gram kept ("near")
OWN = {
    "ahrefs": dict(lit=b"AhrefsBot", true=[b"AhrefsBot"], half=[], near=[b"AhrefsBoT", b"ahrefsBot"]),
    "ff": dict(lit=b"Firefox/", true=[b"Firefox/7", b"Firefox/42"], half=[b"Firefox/x"], near=[b"Firefox-7", b"firefox/7"]),
    "scr": dict(lit=b"crapy", true=[b"Scrapy", b"sCRAPY", b"\xc5\xbfcrapy"], half=[b"xcrapy", b"\xffcrapy"],
                near=[b"scrapz", b"sdrapy"]),
    "mac": dict(lit=b"Macintosh", true=[b"Macintosh"], half=[], near=[b"Macintosi", b"Nacintosh"]),
    "mech": dict(lit=b"mechanize", true=[b"Mechanize", b"mechaniZE"], half=[], near=[b"mechanizf", b"nechanize"]),
    "hay": dict(lit=b"haystack", true=[b"haystack12x"], half=[b"haystack12", b"haystackx"], near=[b"haystacl1x", b"iaystack1x"]),
    "needle": dict(lit=b"needle", true=[b"needle3"], half=[b"needlex"], near=[b"needlf3", b"oeedle3"]),
    "site": dict(lit=b"sitelit", true=[b"sitelit"], half=[], near=[b"sitelis", b"titelit"]),
    "tok": dict(lit=b"=token", true=[b"ab=token", b"z=token"], half=[b" =token", b"\xc3\xa9=token", b"\xff=token"],
                near=[b"ab=tokem", b"ab-token"]),
}
OWN_KINDS = ("ahrefs", "ff", "scr", "mac", "hay", "needle", "site", "tok", "mech")
# other hits: the first pool holds literals of every ruleset (so five of them overflow the slots anywhere)
OTHERS_A = [b"AhrefsBot", b"Firefox/x", b"Firefox/5", b"Macintosh", b"Scrapy", b"mechanize", b"xcrapy", b"MECHANIZE"]
OTHERS_X = [b"SemrushBot", b"haystack1x", b"haystack1", b"needlex", b"needle4", b"sitelit", b"q=token", b" =token",
            b"zq005zq", b"zq033zq", b"zq037zq", b"zq039zq"]

# (literal, case-insensitive) of each ruleset, checked against the compiled rules by the CPU test
LITS_A = [(b"Macintosh", False), (b"crapy", True), (b"mechanize", True), (b"AhrefsBot", False), (b"SemrushBot", False),
          (b"Firefox/", False)]
LITS_TARGETS = [(b"Macintosh", False), (b"crapy", True), (b"mechanize", True), (b"AhrefsBot", False), (b"Firefox/", False),
                (b"haystack", False), (b"=token", False), (b"sitelit", False), (b"needle", False)]


def filler_literal(k: int) -> bytes:
    return b"zq%03dzq" % k


def _rule(name, regex, interval, hits, decision, indent="  "):
    return ("%s- rule: '%s'\n%s  regex: '%s'\n%s  interval: %d\n%s  hits_per_interval: %d\n%s  decision: %s\n"
            % (indent, name, indent, regex.replace("'", "''"), indent, interval, indent, hits, indent, decision))


def _targets():
    return [_rule("mac firefox", r"Macintosh.*Firefox/\d+", 60, 6, "challenge"),
            _rule("scrapers", r"(?i)scrapy|mechanize", 10, 3, "nginx_block"),
            _rule("ahrefs", r"AhrefsBot", 60, 4, "nginx_block"),
            _rule("any firefox", r".*Firefox/\d+", 30, 9, "challenge"),
            _rule("hay", r"haystack[0-9]+x", 5, 2, "challenge"),
            _rule("lead", BOUNDED_LEAD, 5, 2, "nginx_block")]


def _fillers(n):
    return [_rule("fill%d" % k, filler_literal(k).decode(), 5, 1 + k % 3, "challenge") for k in range(n)]


_SITE = ("per_site_regexes_with_rates:\n  h.com:\n" + _rule("site", r"sitelit", 1, 0, "nginx_block", "    ") +
         _rule("equiv", r"needle\d", 1, 1, "challenge", "    "))
_TAIL = "expiring_decision_ttl_seconds: 10\n"
RULESETS = ("A", "B", "C1", "C2", "D")
N_FILLERS = {"B": 12, "C1": 40, "C2": 40, "D": 130}


def rules_yaml(kind: str) -> str:
    """A: the UA rules of workload cfg4 as they stand (6 literals: the scan keeps
    each literal's first candidate).  B: the targets and 12 one-literal fillers (9-32
    literals: a summary bit names one literal).  C1: 40 fillers, then the targets
    (their literal ids past 32).  C2: the targets, then 40 fillers (ids below 32, summary
    bits aliased).  D: C2 with 130 fillers (more than 128 global rules: the wide kernel)."""
    if kind == "A":
        import workloads
        return workloads.UA_RULES + _TAIL
    f = _fillers(N_FILLERS[kind])
    rules = f + _targets() if kind == "C1" else _targets() + f
    return "regexes_with_rates:\n" + "".join(rules) + _SITE + _TAIL


def literals(kind: str):
    if kind == "A":
        return list(LITS_A)
    return LITS_TARGETS + [(filler_literal(k), False) for k in range(N_FILLERS[kind])]


def hit_positions(text: bytes, lits) -> list:
    """Sorted offsets of the true occurrences (overlapping ones too) of the literals in text."""
    low = text.lower()
    out = []
    for s, ci in lits:
        hay, needle = (low, s.lower()) if ci else (text, s)
        i = hay.find(needle)
        while i >= 0:
            out.append(i)
            i = hay.find(needle, i + 1)
    return sorted(out)


def count_hits(text: bytes, lits) -> int:
    return len(hit_positions(text, lits))


@dataclass
class Line:
    layout: int
    variant: int
    klass: str
    own: str
    start: int          # batch offset of the line's first byte
    text: bytes         # without the '\n'
    rest_off: int
    index: int = 0      # line index in the batch
    # straddles: (batch offset of the boundary, bytes of the token before it, the token)
    straddle: tuple = None
    expect_hits: int = None  # layouts 9 and 10: the exact number of literal occurrences


@dataclass
class Batch:
    data: bytes
    lines: list = field(default_factory=list)  # the layout lines (fillers not listed)
    n_lines: int = 0
    now_ns: int = T0 * 1_000_000_000


class _Gen:
    def __init__(self, seed):
        self.rnd = random.Random(seed)
        self.block = bytes(self.rnd.choices(FILL, k=1 << 16))
        self.out = bytearray()
        self.n_lines = 0
        self.lines = []

    # ---- plumbing
    def fill(self, n):
        o = self.rnd.randrange(0, len(self.block) - n) if n < len(self.block) else 0
        return self.block[o:o + n]

    def emit(self, text: bytes):
        assert b"\n" not in text
        self.out += text + b"\n"
        self.n_lines += 1

    def filler_line(self, n):
        head = b"%d %s GET f.org GET /" % (T0, self.rnd.choice(IPS).encode())
        self.emit(head + self.fill(max(0, n - len(head))))

    def pad_to(self, u):
        """Filler lines until the next line starts u bytes into its tile."""
        gap = (u - len(self.out)) % TILE
        if gap < 48:
            gap += TILE
        while gap > 2200:
            n = self.rnd.randrange(60, 1100)
            self.filler_line(n - 1)
            gap -= n
        self.filler_line(gap - 1)
        assert len(self.out) % TILE == u

    def place(self, klass):
        """Emit what precedes a line of this class; returns its length."""
        r = self.rnd
        if klass == "cap":
            self.pad_to(r.randrange(0, TILE - 2 * 140 - 1))
            for _ in range(140):
                self.emit(b"x")
            return 300
        if klass == "halo":
            end = TILE + r.randrange(1, HALO - 8)  # tile-relative offset of the '\n'
            n = r.randrange(600, min(4500, end) + 1)
            self.pad_to(end - n)
            return n
        if klass == "edge":
            self.pad_to(0)
            return r.randrange(TILE, TILE + HALO - 8)
        self.filler_line(r.randrange(40, 900))
        return {"two": r.randrange(4700, 6000), "mid": r.randrange(9000, 13000), "big": r.randrange(19000, 21000)}[klass]

    def others(self, own, k, exact_pool=False):
        lit = OWN[own]["lit"].lower()
        ok = lambda t: lit not in t.lower()
        a = [t for t in OTHERS_A if ok(t)]
        x = [t for t in OTHERS_A + OTHERS_X if ok(t)]
        return [self.rnd.choice(a if (i < 6 or exact_pool) else x) for i in range(k)]

    def spread(self, lo, hi, toks, taken):
        """One token per equal segment of [lo, hi), clear of the taken spans."""
        r = self.rnd
        seg = (hi - lo) // max(1, len(toks))
        out = []
        for i, t in enumerate(toks):
            for _ in range(200):
                a = lo + i * seg
                p = r.randrange(a, max(a + 1, a + seg - len(t) - 1))
                if p + len(t) <= hi and all(p + len(t) + 1 <= q or p >= q + len(u) + 1 for q, u in taken + out):
                    out.append((p, t))
                    break
            else:
                raise AssertionError("no room for %r in [%d, %d)" % (t, lo, hi))
        return out

    def build(self, layout, variant, klass, own, n, plants, ip=None, host=None, method=b"GET", **meta):
        """plants: (line offset, token); every one must lie past the header fields."""
        r = self.rnd
        ip = (ip or r.choice(IPS).encode())
        host = host or r.choice([b"h.com", b"x.org", b"h.com", b"ua.example"])
        head = b"%d %s %s %s %s /" % (T0, ip, method, host, method)
        body = bytearray(self.fill(n - len(head)))
        spans = sorted(plants)
        for (p, t), (q, _) in zip(spans, spans[1:]):
            assert p + len(t) <= q, (layout, variant, spans)
        for p, t in spans:
            assert len(head) <= p and p + len(t) <= n, (layout, variant, klass, p, t, n, len(head))
            body[p - len(head):p - len(head) + len(t)] = t
        text = head + bytes(body)
        assert len(text) == n
        ln = Line(layout, variant, klass, own, len(self.out), text, len(b"%d %s " % (T0, ip)), self.n_lines, **meta)
        self.lines.append(ln)
        self.emit(text)
        return ln


def _classes(layout):
    if layout == 8:
        return ["mid", "big", "mid", "mid", "big"]
    if layout == 9:
        return ["mid", "big", "mid", "mid"]
    if layout == 4:
        return ["two"] * 5 + ["mid"] * 4 + ["big"] * 2 + ["halo"] * 4
    return ["two"] * 6 + ["mid"] * 5 + ["big"] * 2 + ["cap"] * 3 + ["halo"] * 4 + ["edge"] * 2


def _own_tok(g, own, v):
    """The own token of variant v: mostly true, every third a half or near one."""
    o = OWN[own]
    if v % 3 == 2:
        alt = o["half"] + o["near"]
        return alt[(v // 3) % len(alt)]
    return o["true"][(v // 3) % len(o["true"])]


def crowded_first_tile(variant: int) -> bool:
    """Layouts 1-7: the variants whose hits crowd the line's first tile
    instead of spreading one or two per tile."""
    return variant % 7 == 3


def _layout_line(g: _Gen, layout: int, v: int):
    r = g.rnd
    classes = _classes(layout)
    klass = classes[v % len(classes)]
    own = OWN_KINDS[(v // 2 + layout) % len(OWN_KINDS)]
    n = g.place(klass)
    s = len(g.out)
    hl = 64  # past any header of ordinary fields (the real one is shorter)
    o = OWN[own]
    def others_spread(k, lo, hi, taken, exact=False, extra=()):
        toks = g.others(own, k, exact) + list(extra)
        if crowded_first_tile(v) and klass != "cap" and layout <= 7:
            # five or six of them inside the line's first tile, two or more past it
            toks += g.others(own, 2, exact)
            m = min(len(toks) - 2, r.randrange(5, 7))
            lim = min(hi, max(lo + 400, min(hi, TILE - s % TILE)))
            return g.spread(lo, lim, toks[:m], taken) + (g.spread(lim, hi, toks[m:], taken) if toks[m:] and hi - lim > 200
                                                         else [])
        return g.spread(lo, hi, toks, taken)

    if layout == 1:
        host = b"Macintosh.Firefox/1.example" if v % 3 == 1 else None
        ip = o["true"][0].replace(b" ", b"")
        if own == "tok":
            ip = b"ab=token"
        pl = others_spread(r.randrange(5, 13), hl, n, [])
        return g.build(1, v, klass, own, n, pl, ip=ip, host=host)
    if layout == 2:
        t = _own_tok(g, own, v)
        p = n - len(t) - r.randrange(0, 16 - len(t) + 1)
        k = max(5, (s % TILE + n) // TILE + 1)
        pl = others_spread(min(k + r.randrange(0, 3), 12 if klass != "cap" else 6), hl, p - 2, [])
        return g.build(2, v, klass, own, n, pl + [(p, t)])
    if layout == 3:
        t = _own_tok(g, own, v)
        p = r.randrange(hl, (100 if klass == "cap" else CERTAIN_GAP) - len(t))
        lo = 600 if n > 1200 else p + len(t) + 2
        pl = others_spread(r.randrange(5, 10) if klass != "cap" else 5, lo, n, [(p, t)])
        return g.build(3, v, klass, own, n, pl + [(p, t)])
    if layout == 4:
        t = _own_tok(g, own, v).replace(b" ", b"_")
        m = r.randrange(300, max(301, min(701, n - 380)))
        fld = bytearray(g.fill(m).replace(b" ", b"_"))
        q = r.randrange(CERTAIN_GAP, m - len(t))  # >= 256 into the field, so into the line
        fld[q:q + len(t)] = t
        fld = bytes(fld)
        kw = dict(ip=fld) if v % 2 else dict(host=fld)
        extra = []
        if v % 4 == 1 and own not in ("site", "needle"):  # the site's rules on some of the long-header lines
            kw["host"] = b"h.com"
            extra = [[b"sitelit", b"needle4"][v // 4 % 2]]
        lo = len(b"%d " % T0) + m + 80
        pl = others_spread(r.randrange(5, 10), lo, n, [], extra=extra)
        return g.build(4, v, klass, own, n, pl, **kw)
    if layout == 5:
        # the token crosses boundary B by len - k bytes: k bytes before it
        o_t = o["true"] + o["near"] if v % 2 else o["true"]
        t = o_t[(v // 2) % len(o_t)]
        k = 1 + (v // 4) % (len(t) - 1)
        tile_next = (s // TILE + 1) * TILE
        if klass in ("cap", "halo", "edge"):
            B = tile_next  # these lines end before the halo does
            if not (s + hl + 16 < B and B + len(t) < s + n):
                B = None
        else:
            B = tile_next + (HALO if v % 4 >= 2 else 0)
            if B - k < s + hl + 8:
                B += TILE
        taken, strad = [], None
        if B is not None:
            taken = [(B - k - s, t)]
            strad = (B, k, t)
        else:
            taken = [(r.randrange(hl, n - len(t)), t)]
        pl = others_spread(r.randrange(5, 10) if klass != "cap" else 5, hl, n, taken)
        return g.build(5, v, klass, own, n, pl + taken, straddle=strad)
    if layout == 6:
        near = (o["near"] + o["half"])[v % len(o["near"] + o["half"])]
        true = o["true"][v % len(o["true"])]
        second = true if v % 3 else o["near"][0]  # every third line: no true one at all
        if klass == "cap":
            a = (r.randrange(hl, hl + 12), near)
            b = (r.randrange(270, n - len(second) + 1), second)
        else:
            a = (r.randrange(hl, hl + (n - hl) // 3 - 20), near)
            b = (r.randrange(n - (n - hl) // 3, n - len(second) + 1), second)
        if klass == "cap":
            pl = others_spread(5, a[0] + len(near) + 2, b[0] - 2, [])
        else:
            pl = others_spread(r.randrange(5, 10), hl, n, [a, b])
        return g.build(6, v, klass, own, n, pl + [a, b])
    if layout == 7:
        own = ("scr", "tok", "mech")[v % 3]
        o = OWN[own]
        lit = o["lit"] if own != "scr" else b"crapy"
        pre = [b"\xc3\xa9", b"\xc5\xbf", b"\xe2\x84\xaa", b"\xff", b"s", b"S", b"ab", b" ", b"abcde"][(v // 3) % 9]
        sub = (v // 3) % 3
        method, taken = b"GET", []
        if sub == 0:  # the bounded piece crosses the start of rest: rest begins with the token
            method = [b"Scrapy", b"crapy", b"xscrapy", b"ab=token", b"=token", b"abcd=token", b"Mechanize", b"echanize"][(v // 9) % 8]
        tile_next = (s // TILE + 1) * TILE
        if sub == 1 and klass not in ("cap", "halo", "edge"):
            # the literal starts on a tile edge, its bounded piece ends the tile before
            B = tile_next if tile_next - len(pre) > s + hl + 24 else tile_next + TILE
            taken = [(B - len(pre) - s, pre + lit)]
        else:
            taken = [(r.randrange(hl + 40, n - 16), pre + lit)]
        pl = others_spread(r.randrange(5, 10) if klass != "cap" else 5, hl + (24 if sub == 0 else 0), n, taken)
        return g.build(7, v, klass, own, n, pl + taken, method=method)
    if layout == 8:
        own = "ff"
        dense = b"Firefox/ " * 300
        tile_next = (s // TILE + 1) * TILE
        if tile_next - s < 100:
            tile_next += TILE
        a = tile_next + r.randrange(0, TILE - len(dense)) - s
        pl = [(a, dense)]
        if v % 2:
            pl.append((r.randrange(a + len(dense) + 2, n - 9), b"Firefox/9"))
        if v % 4 >= 2:
            pl.append((r.randrange(hl, a - 12), b"Macintosh"))
        return g.build(8, v, klass, own, n, pl)
    if layout == 9:
        # one token in each of k distinct tiles of the line
        spans = []
        for ti in range(s // TILE, (s + n - 1) // TILE + 1):
            a, b = max(ti * TILE - s, hl), min((ti + 1) * TILE - s, n) - 12
            if b - a >= 40:
                spans.append((a, b))
        k = min(3 + v % 2, len(spans))
        toks = g.others(own, k - 1, True) + [o["true"][0] if own in ("ahrefs", "ff", "scr", "mac", "mech") else b"Scrapy"]
        r.shuffle(toks)
        pl = [(r.randrange(a, b), t) for (a, b), t in zip(sorted(r.sample(spans, k)), toks)]
        return g.build(9, v, klass, own, n, pl, expect_hits=k)
    if layout == 10:
        k = 4 + v % 2
        rep = [b"Firefox/x", b"AhrefsBot", b"Scrapy", b"Macintosh", b"Firefox/3"][(v // 2) % 5]
        toks = [rep] * (2 + v % 3) + g.others("hay", 5, True)
        toks = toks[:k]
        r.shuffle(toks)
        pl = g.spread(hl, n, toks, [])
        return g.build(10, v, klass, "ff" if b"Firefox" in rep else own, n, pl, expect_hits=k)
    raise ValueError(layout)


_cache = {}


def batch(seed: int) -> Batch:
    """The batch of this seed (built once; treat it as read-only)."""
    if seed not in _cache:
        g = _Gen(seed)
        order = [(layout, v) for v in range(LINES_PER_LAYOUT) for layout in LAYOUTS]
        for layout, v in order:
            _layout_line(g, layout, v)
        g.filler_line(100)
        _cache[seed] = Batch(bytes(g.out), g.lines, g.n_lines)
    return _cache[seed]


def tile_start_batch(seed: int, n_lines: int = 96) -> Batch:
    """Lines of the "edge" class only, every token a true literal of every
    ruleset and clear of the tile edges, so the scan records exactly
    count_hits(data) hits: half the lines with 1-3 hits past the tile's end and
    none or one before (no overflow, so a slot that took a later hit for an
    earlier one shows), half with 5-9 hits."""
    g = _Gen(seed)
    for v in range(n_lines):
        n = g.place("edge")
        toks_in = [g.rnd.choice(OTHERS_A) for _ in range(g.rnd.randrange(4, 8) if v % 2 else v % 4 // 2)]
        toks_out = [g.rnd.choice(OTHERS_A) for _ in range(g.rnd.randrange(1, 4))]
        pl = g.spread(64, TILE - 16, toks_in, []) if toks_in else []
        pl += g.spread(TILE + 8, n, toks_out, []) if n - TILE - 8 >= 16 * len(toks_out) + 16 else []
        g.build(0, v, "edge", None, n, pl, expect_hits=len(pl))  # layout 0, own None: no layout's line
    g.filler_line(100)
    return Batch(bytes(g.out), g.lines, g.n_lines)


# Lines of workload cfg4 (workloads.CFG4, the batch that starts at line 0) whose
# offset is a multiple of the scan tile and whose length is 4,096-4,607 bytes:
# each starts a tile and ends in its halo (found by walking the workload's
# first 650k lines on the host).  tests/golden/make_golden.py puts them,
# verbatim, on tile starts again in the fixture long_line_hits.
CFG4_TILE_START_LINES = [69741, 74545, 121633, 149726, 180774, 207030, 275111, 416762, 511199, 545791, 582522, 627669]


def cfg4_tile_start_log() -> bytes:
    import workloads
    g = _Gen(0)
    for idx in CFG4_TILE_START_LINES:
        g.pad_to(0)
        g.emit(workloads.CFG4.host_lines(idx, 1)[:-1])
    g.filler_line(100)
    return bytes(g.out)


def golden_batch() -> Batch:
    """The batch of tests/golden/long_line_hits.json.gz; Batch.lines are its
    cfg4 lines (the fillers between them are not listed)."""
    import base64
    import gzip
    import json
    import os
    with gzip.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "long_line_hits.json.gz"), "rt") as f:
        fx = json.load(f)
    data = base64.b64decode(fx["batches"][0]["log_b64"])
    lines, s = [], 0
    for k, text in enumerate(data.split(b"\n")[:-1]):
        if s % TILE == 0 and len(text) >= TILE:
            # layout 0, own None: these lines come from the workload, not from a layout
            lines.append(Line(0, len(lines), "edge", None, s, text, len(text) - len(text.split(b" ", 2)[2]), k))
        s += len(text) + 1
    return Batch(data, lines, data.count(b"\n"), fx["batches"][0]["now_ns"])
