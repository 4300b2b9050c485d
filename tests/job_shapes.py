"""Exact shapes for the DFA job stage: emit_job -> radix sort by job key ->
k_dfa / k_dfa_legacy / k_nfa<WT> / k_nfa_wide, with k_rule_bounds giving the NFA
launches their ranges.

The sorted job array is rule-major: the windowed keys r (k_dfa's), then the
legacy keys n_rules + r (k_dfa_legacy's and the NFA kernels').  Every kernel
cuts it into blocks of 256 lanes, and what a block does depends on where the
rule boundaries fall in it (`uniform` from its first and last key), on the
rule's table sizes against the LDS staging limits, and on which key kinds
share it.  This module plans batches whose sorted array has a chosen
composition, lane by lane: every line carries the literal of exactly one rule
(the rules are unanchored prefilter rules with a literal no other rule and no
filler byte can spell, not equivalent to it, so a hit always becomes a job and
no inline table of k_lines2 decides it), and Engine.debug_job_counts() then
proves on the GPU that the planned array is the one the kernels saw.

Rule classes, found at import time by a search over the repetition count k of
`<lit>.{k}y` (the counts differ with the literal's bytes) and confirmed from
Ruleset.rule_info by tests/test_job_shapes_cpu.py:
  S  ncls * n_states <= 8192 and n_states <= 2048: transitions and accel words staged
  T  ncls * n_states > 8192, n_states <= 2048: never staged
  A  n_states > 2048 under the 4,096 cap, still a DFA: never staged either
  L  `(?s)aaaa.{15}a`: two byte classes, so 2 * 2185 transitions are staged while
     the 2,185 accel words stay in HBM.  This is the class "LDS transitions with
     n_states > 2048"; it needs ncls <= 3, which a one-byte literal and (?s) reach.
  N  per-lane bit-parallel NFA (`.{60}y`, `.{900}y`: 2 and 16 state words)
  W  wide block-cooperative NFA (`.{600}y.{600}w`)

Rulesets:
  MAIN  41 per-site rules on five hosts (scopes of ten or less), every class;
        small enough for k_lines2's 20 KB of tables.  Rules 0-31 have literal
        ids below 32 (windowed jobs unless NFA), rules 32-34 are DFA rules
        with literal ids past 32 (legacy jobs), rule 0 and rule 40 are NFA rules
        (the lowest and the highest index), 35 and 36 adjacent NFA rules.
  BIG   320 class-S rules on five hosts.  One block of 256 different rules
        needs 256 rules, and the rows k_lines2 keeps per literal and host class
        (32 B each) pass its 20 KB long before that, so this ruleset always
        runs on k_lines with legacy jobs; its cases run under BJX_NO_LINES2.
  EDGE  13 rules of one host for the text edges, and on a host of its own
        `^GET .*<lit>.{k}y` with 256 states or more (no inline table): every
        line of that host is a job that starts past the anchored `GET `, in
        the rule's skip state (kJobSkipState).
  GROW  32 class-S rules of one host for the job-buffer growth path.

Legacy DFA jobs come from an engine under BJX_NO_LINES2 (every job), from the
rules with literal ids past 32, and from lead rules on lines with more than four
literal hits (Item.overflow: the own literal five times).

Text edges (edge_specs): the job of a lead rule starts at the first hit of its
literal, that of `x+<lit>.*d` (no lead) at the start of rest.  Every start
offset modulo 16 is crossed with every text length from the literal alone to
past the second 16-byte chunk, so the '\\n' falls on every byte of the first
chunk it can (the literal has to fit before it) and on every byte of the
second; see EDGE_KINDS for the rest.
"""
from __future__ import annotations

import functools
import random
from dataclasses import dataclass, field

from banjax_amd import Config, Ruleset

T0 = 1700000000
BLOCK = 256
# no filler byte is part of a literal, an escape byte or a deciding byte of any rule
FILL = b"befgijkmnoprstuv"
IPS = ["10.3.%d.%d" % (k // 8, k % 8) for k in range(24)]
LDS_ENTRIES, LDS_ACCEL, STATE_CAP = 8192, 2048, 4096
_rnd = random.Random(7)
_BLOCK_BYTES = bytes(_rnd.choices(FILL, k=1 << 16))


def fill(n: int, salt: int = 0) -> bytes:
    o = (salt * 7919) % (len(_BLOCK_BYTES) - n - 1) if n < len(_BLOCK_BYTES) - 1 else 0
    return _BLOCK_BYTES[o:o + n]


@dataclass
class Rule:
    name: str
    host: str
    lit: bytes
    kind: str            # dotk, dollar, star, xstar, L, wide, anchored
    k: int
    cls: str             # S, T, A, L, N, W
    hits: int = 1000000
    regex: str = ""

    def __post_init__(self):
        lit = self.lit.decode()
        self.regex = {"dotk": "%s.{%d}y" % (lit, self.k), "dollar": "%s.{%d}y$" % (lit, self.k), "star": "%s.*d" % lit,
                      "xstar": "x+%s.*d" % lit, "anchored": "^GET .*%s.{%d}y" % (lit, self.k), "L": "(?s)%s.{%d}a" % (lit, self.k),
                      "wide": "%s.{%d}y.{%d}w" % (lit, self.k, self.k)}[self.kind]

    @property
    def nfa(self):
        return self.cls in "NW"

    # ---- texts from the literal on (the literal included)
    def hit(self, salt=0) -> bytes:
        f = fill(self.k, salt)
        if self.kind in ("dotk", "dollar", "anchored"):
            return self.lit + f + b"y"
        if self.kind in ("star", "xstar"):
            return (b"x" if self.kind == "xstar" else b"") + self.lit + fill(salt % 40, salt) + b"d"
        if self.kind == "L":
            return self.lit + f + b"a"
        return self.lit + f + b"y" + fill(self.k, salt + 1) + b"w"

    def miss(self, salt=0) -> bytes:
        if self.kind in ("dotk", "dollar", "anchored"):
            v = salt % 3
            if v == 0 or self.k < 2:
                return self.lit + fill(self.k, salt) + b"f"                    # the wrong byte where y belongs
            if v == 1:
                return self.lit + fill(self.k - 1, salt) + b"y" + b"ee"        # y one byte early
            return self.lit + fill(min(self.k, 1 + salt % max(1, self.k)), salt)  # the line ends inside .{k}
        if self.kind in ("star", "xstar"):
            return (b"x" if self.kind == "xstar" else b"") + self.lit + fill(salt % 40, salt)
        if self.kind == "L":
            return self.lit + fill(self.k, salt) + b"e"
        return self.lit + fill(20 + salt % 30, salt) + b"y" + fill(10, salt)

    @property
    def after_ok(self):
        """May text follow a hit() without changing the outcome?"""
        return self.kind != "dollar"


def _info(regex: str):
    y = ("per_site_regexes_with_rates:\n  p.example:\n    - rule: 'p'\n      regex: '%s'\n      interval: 1\n"
         "      hits_per_interval: 1\n      decision: challenge\n" % regex)
    return Ruleset(Config.from_yaml(y)).rule_info(0)


def class_of(states: int, ncls: int, flags: int) -> str:
    if flags & 8:
        return "W"
    if flags & 4:
        return "N"
    if states > LDS_ACCEL:
        return "L" if ncls * states <= LDS_ENTRIES else "A"
    return "S" if ncls * states <= LDS_ENTRIES else "T"


@functools.lru_cache(maxsize=None)
def _find_k(lit: bytes, kind: str, cls: str) -> int:
    """The smallest repetition count that puts `<lit>.{k}y` (or its `$` form) into the class."""
    for k in range(3, 40):
        r = Rule("p", "p", lit, kind, k, cls)
        if class_of(*_info(r.regex)) == cls:
            return k
    raise AssertionError("no repetition count puts %r (%s) into class %s" % (lit, kind, cls))


def _mk(name, host, lit, cls, kind="dotk", hits=1000000):
    if cls == "N":
        return Rule(name, host, lit, "dollar" if kind == "dollar" else "dotk", 900 if kind == "n900" else 60, "N", hits)
    if cls == "L":
        return Rule(name, host, lit, "L", 15, "L", hits)
    if cls == "W":
        return Rule(name, host, lit, "wide", 600, "W", hits)
    if kind == "anchored":
        # 256 states or more: no inline table of k_lines2 (u8 next states), so every line of the host is a job
        for k in range(8, 24):
            r = Rule(name, host, lit, kind, k, cls, hits)
            st, ncls, fl = _info(r.regex)
            if st >= 256 and class_of(st, ncls, fl) == cls:
                return r
        raise AssertionError("no anchored rule of class %s with 256 states" % cls)
    if cls == "S":
        return Rule(name, host, lit, kind, 3 if kind in ("dotk", "dollar") else 0, "S", hits)
    return Rule(name, host, lit, kind, _find_k(lit, kind, cls), cls, hits)


def _lit(tag: str, i: int) -> bytes:
    return b"q%s%02dz" % (tag.encode(), i)


@functools.lru_cache(maxsize=None)
def rules(ruleset: str):
    """The rules of a ruleset in index order (the hosts in YAML order)."""
    out = []
    if ruleset == "MAIN":
        spec = {0: ("N", "n60"), 3: ("T", "dotk"), 5: ("A", "dotk"), 7: ("L", "L"), 8: ("S", "star"), 9: ("S", "dollar"),
                18: ("T", "dotk"), 33: ("T", "dotk"), 34: ("A", "dotk"), 35: ("N", "n60"), 36: ("N", "n900"),
                37: ("W", "wide"), 38: ("W", "wide"), 40: ("N", "n60")}
        hosts = [0] * 10 + [1] * 10 + [2] * 10 + [3] * 6 + [4] * 5
        for i, h in enumerate(hosts):
            cls, kind = spec.get(i, ("S", "dotk"))
            lit = b"aaaa" if cls == "L" else _lit("m", i)
            out.append(_mk("m%d" % i, "h%d.example" % h, lit, cls, kind, hits=3 if i % 4 == 1 else 1000000))
    elif ruleset == "BIG":
        for i in range(320):
            out.append(_mk("b%d" % i, "h%d.example" % (i // 64), b"q%03dz" % i, "S", "dotk", hits=3 if i % 16 == 1 else 1000000))
    elif ruleset == "EDGE":
        spec = [("S", "dotk"), ("S", "dotk"), ("S", "dollar"), ("S", "star"), ("S", "xstar"), ("T", "dotk"), ("T", "dollar"),
                ("A", "dotk"), ("A", "dollar"), ("L", "L"), ("N", "n60"), ("N", "dollar"), ("S", "dotk"), ("S", "anchored")]
        for i, (cls, kind) in enumerate(spec):
            lit = b"aaaa" if cls == "L" else _lit("e", i)
            out.append(_mk("e%d" % i, "e1.example" if kind == "anchored" else "e0.example", lit, cls, kind,
                           hits=3 if i in (1, 5) else 1000000))
    elif ruleset == "GROW":
        for i in range(32):
            out.append(Rule("g%d" % i, "g.example", _lit("g", i), "dotk", 1, "S", 4 if i == 5 else 1000000))
    else:
        raise ValueError(ruleset)
    return tuple(out)


def rules_yaml(ruleset: str) -> str:
    y, host = ["per_site_regexes_with_rates:"], None
    for r in rules(ruleset):
        if r.host != host:
            host = r.host
            y.append("  %s:" % host)
        y.append("    - rule: '%s'\n      regex: '%s'\n      interval: 5\n      hits_per_interval: %d\n      decision: %s"
                 % (r.name, r.regex, r.hits, "challenge" if r.hits > 100 else "nginx_block"))
    return "\n".join(y) + "\nexpiring_decision_ttl_seconds: 10\n"


# ---- batches ---------------------------------------------------------------------------------

@dataclass
class Item:
    rule: int
    n: int
    overflow: bool = False   # the own literal five times: more hits than the line has slots


@dataclass
class Line:
    rule: int            # -1: no literal
    start: int           # batch offset of the line's first byte
    text: bytes
    job: int = -1        # batch offset of the job's first byte, as planned
    kind: str = ""       # edge lines: which edge


class Batch:
    def __init__(self, ruleset: str):
        self.ruleset = ruleset
        self.rules = rules(ruleset)
        self.out = bytearray()
        self.lines = []
        self.k = 0

    def head(self, host: str) -> bytes:
        self.k += 1
        return b"%d %s GET %s GET /" % (T0, IPS[self.k % len(IPS)].encode(), host.encode())

    def emit(self, rule, text, job_rel=-1, kind=""):
        assert b"\n" not in text
        ln = Line(rule, len(self.out), text, len(self.out) + job_rel if job_rel >= 0 else -1, kind)
        self.lines.append(ln)
        self.out += text + b"\n"
        return ln

    def pad_line(self, n=0):
        """A line of host f.org (no rules) of n bytes, '\\n' included (its minimum if shorter)."""
        h = self.head("f.org")
        return self.emit(-1, h + fill(max(0, n - 1 - len(h)), self.k))

    def quiet_line(self, host):
        """A line of a host with rules that spells no literal."""
        return self.emit(-1, self.head(host) + fill(12 + self.k % 30, self.k))

    def job_line(self, r: int, salt: int, overflow=False, pre=None, body=None, tail=None, kind=""):
        """One line with rule r's literal: `<head><pre><body><tail>`; the job starts at the literal's first byte
        (xstar: at the start of rest).  body defaults to a hit or a miss by salt."""
        R = self.rules[r]
        h = self.head(R.host)
        pre = fill(3 + salt % 9, salt) if pre is None else pre
        want = salt % 2 == 0
        if body is None:
            body = R.hit(salt) if want else R.miss(salt)
        if tail is None:
            tail = fill(salt % 23, salt + 5) if (R.after_ok or not want) and R.kind != "dollar" else b""
            if R.kind == "dollar" and not want and salt % 3 == 0:
                body, tail = R.hit(salt), b"e"      # the y is there, but not at the line's end
        if overflow:
            tail += b"".join(b" " + R.lit for _ in range(4))
        text = h + pre + body + tail
        rest_off = len(b"%d %s " % (T0, IPS[self.k % len(IPS)].encode()))
        job_rel = rest_off if R.kind == "xstar" else rest_off + 4 if R.kind == "anchored" else len(h) + pre.index(R.lit) if R.lit in pre else len(h) + len(pre) + body.index(R.lit)
        return self.emit(r, text, job_rel, kind)

    @property
    def data(self) -> bytes:
        return bytes(self.out)


def interleave(items):
    """The lines of the items in a fixed shuffled order, so the sort has work to do: (rule, salt, overflow)."""
    seq = [(it.rule, s, it.overflow) for it in items for s in range(it.n)]
    random.Random(len(seq)).shuffle(seq)
    return seq


def build(ruleset: str, items, quiet=0) -> Batch:
    b = Batch(ruleset)
    for i, (r, s, ov) in enumerate(interleave(items)):
        b.job_line(r, s + r, ov)
        if quiet and i % quiet == 0:
            b.quiet_line(b.rules[r].host)
    if not items:
        for i in range(50):
            b.quiet_line(b.rules[i % len(b.rules)].host)
    return b


def counts(ruleset: str, items, no_lines2=False):
    """(windowed, legacy) planned jobs per rule."""
    rs = rules(ruleset)
    w, g = [0] * len(rs), [0] * len(rs)
    windowed_ok = ruleset != "BIG" and not no_lines2
    for it in items:
        if windowed_ok and it.rule < 32 and not rs[it.rule].nfa and not it.overflow:
            w[it.rule] += it.n
        else:
            g[it.rule] += it.n
    return w, g


@dataclass
class Run:
    legacy: bool
    rule: int
    cls: str
    start: int
    n: int


def runs_of(cnt, classes):
    w, g = cnt
    out, at = [], 0
    for legacy, arr in ((False, w), (True, g)):
        for r, n in enumerate(arr):
            if n:
                out.append(Run(legacy, r, classes[r], at, n))
                at += n
    return out


@dataclass
class Block:
    kind: str        # uniform, mixed, windowed+legacy, legacy+nfa, nfa
    cls: str         # the class of its first rule
    legacy: bool     # its first key is a legacy one
    lanes: int
    parts: list = field(default_factory=list)   # (legacy, rule, cls, lanes) in lane order


def classify_blocks(cnt, classes):
    """Cut the planned sorted job array (windowed keys by rule, then legacy keys by rule) into blocks of 256 lanes."""
    runs = runs_of(cnt, classes)
    total = sum(r.n for r in runs)
    out = []
    for b0 in range(0, total, BLOCK):
        b1 = min(total, b0 + BLOCK)
        parts = [(r.legacy, r.rule, r.cls, min(b1, r.start + r.n) - max(b0, r.start)) for r in runs if r.start < b1 and r.start + r.n > b0]
        nfa = [p for p in parts if p[2] in "NW"]
        win = [p for p in parts if not p[0]]
        leg_dfa = [p for p in parts if p[0] and p[2] not in "NW"]
        if win and len(win) < len(parts):
            kind = "windowed+legacy"
        elif nfa and len(nfa) == len(parts):
            kind = "nfa"
        elif nfa:
            kind = "legacy+nfa"
        elif len(parts) == 1:
            kind = "uniform"
        else:
            kind = "mixed"
        assert win or leg_dfa or nfa
        out.append(Block(kind, parts[0][2], parts[0][0], b1 - b0, parts))
    return out


class Seq:
    """Items in sorted-key order with the lane each run starts at."""

    def __init__(self, ruleset, no_lines2=False):
        self.ruleset, self.no_lines2 = ruleset, no_lines2
        self.items, self.at, self.key = [], 0, (-1, -1)

    def add(self, rule, n, overflow=False):
        if n <= 0:
            return self
        w, g = counts(self.ruleset, [Item(rule, n, overflow)], self.no_lines2)
        key = (1 if g[rule] else 0, rule)
        assert key > self.key, ("items must come in key order", key, self.key)
        self.key = key
        self.items.append(Item(rule, n, overflow))
        self.at += n
        return self

    def pad_to(self, lane, rule, overflow=False):
        return self.add(rule, (lane - self.at) % BLOCK, overflow)


SIZES = (1, 255, 256, 257, 511, 512, 513)


@dataclass
class Case:
    name: str
    ruleset: str
    items: list
    no_lines2: bool = False

    @property
    def counts(self):
        return counts(self.ruleset, self.items, self.no_lines2)

    @property
    def classes(self):
        return [r.cls for r in rules(self.ruleset)]

    def blocks(self):
        return classify_blocks(self.counts, self.classes)

    def runs(self):
        return runs_of(self.counts, self.classes)

    def batch(self) -> Batch:
        return build(self.ruleset, self.items, quiet=7)


def _kinds(no_lines2):
    """Every key kind in one array: windowed S / A / L / T, legacy S (overflow lines and a literal id past 32), T, A,
    the NFA rules and the wide ones."""
    s = Seq("MAIN", no_lines2)
    if no_lines2:
        s.add(0, 30)
    s.add(1, 256).add(5, 300).add(7, 212 + 256).add(18, 100)
    if not no_lines2:
        s.add(0, 30)
        s.add(1, 50, overflow=True)
    s.add(32, (-s.at) % BLOCK + 256)    # to the block's end, then a uniform legacy block of a DFA rule
    s.add(33, 300).add(34, 100)
    s.add(35, 256).add(36, 257).add(37, 1).add(38, 257).add(39, 10).add(40, 1)
    return s.items


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for k in SIZES:
        out.append(Case("aligned%d" % k, "MAIN", Seq("MAIN").add(1, k).pad_to(0, 2).add(3, k).items))
    out.append(Case("lanes", "MAIN", Seq("MAIN").add(1, 1).add(2, 257).pad_to(128, 4).add(6, 257).pad_to(255, 8).add(9, 257).items))
    out.append(Case("single", "MAIN", [Item(1, 1)]))
    out.append(Case("single_nfa", "MAIN", [Item(40, 1)]))
    out.append(Case("kinds", "MAIN", _kinds(False)))
    out.append(Case("nojobs", "MAIN", []))
    out.append(Case("kinds_nl2", "MAIN", _kinds(True), True))
    out.append(Case("aligned257_nl2", "MAIN", Seq("MAIN", True).add(1, 257).pad_to(0, 2).add(3, 257).items, True))
    out.append(Case("rules256_nl2", "BIG", Seq("BIG", True).add(3, 5).pad_to(0, 4).items + [Item(r, 1) for r in range(10, 266)]
                    + [Item(300, 3)], True))
    return {c.name: c for c in out}


# ---- text edges ------------------------------------------------------------------------------

EDGE_KINDS = {
    "len": "start offset mod 16 x text length: the '\\n' on every byte of the first two chunks; at length "
           "len(lit) + k + 1 the match completes on the last byte before the '\\n' (a `$` rule: accepted only there)",
    "dollar_late": "a `$` rule's y followed by one more byte",
    "nonascii": "a two-byte rune at every chunk position after the literal; .{k} counts runes",
    "rune_cut": "a rune cut short by the line's end, or by an ASCII byte",
    "esc_before": "`.*d`: a d before the job's start in its chunk, none after",
    "esc_next_line": "`.*d`: no d in the line, the next line (an error line) begins with d",
    "esc_in_skip": "`.*d`: the d, or a q, 1 / 16 / 17 bytes into a skipped stretch of 64 bytes or more",
}
EDGE_RULES = {"S": (1, 2, 3, 4, 13), "T": (5, 6), "A": (7, 8), "L": (9,), "N": (10, 11)}
EDGE_PADS = (0, 12)


@dataclass
class Spec:
    rule: int
    s: int               # the job's batch offset modulo 16
    body: bytes          # from the literal (xstar: from its x) to the line's end
    kind: str
    d_before: bool = False   # a d directly before the literal (star), at the start of the path (xstar)
    follow: bytes = None     # a line of its own after this one


def place(b: Batch, sp: Spec) -> Line:
    """The job line of a spec appended to b with its job at batch offset = sp.s modulo 16."""
    R = b.rules[sp.rule]
    if R.kind in ("xstar", "anchored"):
        # the job starts where rest does, after `<ts> <ip> ` (anchored: past its `GET `, in the skip state): a pad
        # line before moves the whole line
        hl = len(b"%d %s " % (T0, IPS[0].encode())) + (4 if R.kind == "anchored" else 0)
        want = (sp.s - hl) % 16
        b.pad_line(48 + (want - len(b.out)) % 16)
        assert len(b.out) % 16 == want
        pre = (b"d" if sp.d_before else b"") + fill(5, sp.s)
    else:
        hl = len(b.head(R.host))
        b.k -= 1
        p = (sp.s - (len(b.out) + hl)) % 16
        p += 16 if p < 2 else 0
        pre = fill(p - 1, sp.s) + (b"d" if sp.d_before else fill(1, p))
    ln = b.job_line(sp.rule, 0, pre=pre, body=sp.body, tail=b"", kind=sp.kind)
    assert ln.job % 16 == sp.s, (ln, sp)
    if sp.follow is not None:
        b.emit(-1, sp.follow, kind=sp.kind)
    return ln


@functools.lru_cache(maxsize=None)
def edge_specs(r: int):
    """Every text edge of EDGE rule r."""
    R = rules("EDGE")[r]
    L, k = len(R.lit), R.k
    x = b"x" if R.kind == "xstar" else b""
    out = []
    if R.kind == "anchored":
        for s in range(16):
            for n in range(L, L + k + 9):
                body = bytearray(R.lit + fill(n - L, s + n))
                if n >= L + k + 1 and (n == L + k + 1 or (s + n) % 2):
                    body[L + k] = ord("y")
                out.append(Spec(r, s, bytes(body), "len"))
            f = fill(k - 1, s)
            for j in (s % k, (s + 1) % k):
                out.append(Spec(r, s, R.lit + f[:j] + b"\xc3\xa9" + f[j:] + (b"y" if j == s % k else b"e"), "nonascii"))
        return tuple(out)
    if R.kind in ("dotk", "dollar", "L"):
        y = b"a" if R.kind == "L" else b"y"
        for s in range(16):
            for n in range(L, max(40, L + k + 6)):
                # n bytes from the literal to the '\n': y where it decides when the text is long enough, else filler
                body = bytearray(R.lit + fill(n - L, s + n))
                if n >= L + k + 1 and (n == L + k + 1 or (s + n) % 2):
                    body[L + k] = y[0]
                out.append(Spec(r, s, bytes(body), "len"))
        if R.kind == "dollar":
            for s in range(16):
                out.append(Spec(r, s, R.hit(s) + b"e", "dollar_late"))
        for s in (range(16) if k < 16 else (0, 5, 11)):
            for j in range(min(16, k)):
                # k runes (one of them two bytes) then y; or y after k bytes, one rune early
                f = fill(k - 1, s + j)
                body = R.lit + f[:j] + b"\xc3\xa9" + f[j:]
                out.append(Spec(r, s, body + y, "nonascii"))
                out.append(Spec(r, s, body[:L + k] + y + b"ee", "nonascii"))
        for s in (0, 7, 13, 15):
            out.append(Spec(r, s, R.lit + fill(max(0, k - 2), s) + b"\xe2\x84", "rune_cut"))
            out.append(Spec(r, s, R.lit + fill(max(0, k - 1), s) + b"\xc3", "rune_cut"))
            out.append(Spec(r, s, R.lit + fill(max(0, k - 2), s) + b"\xe2\x84" + y, "rune_cut"))
        return tuple(out)
    for s in range(16):
        for n in range(0, 36):
            out.append(Spec(r, s, x + R.lit + fill(n, s + n) + b"d", "len"))
            out.append(Spec(r, s, x + R.lit + fill(n, s + n), "len"))
    for s in range(16):
        out.append(Spec(r, s, x + R.lit + fill(20, s), "esc_before", d_before=True))
    for s in (0, 3, 9, 15):
        for n in (0, 5, 11, 12, 27):
            out.append(Spec(r, s, x + R.lit + fill(n, s + n), "esc_next_line", follow=b"d" + fill(9, n)))
    for s in range(16):
        for at in (1, 16, 17):
            for esc in (b"d", b"q", b"qd"):
                stretch = bytearray(fill(64 + 2 * s, s + at))
                stretch[at:at + 1] = esc[:1]
                out.append(Spec(r, s, x + R.lit + bytes(stretch) + esc[1:], "esc_in_skip"))
    for s in (0, 5, 11):
        for j in range(16):
            out.append(Spec(r, s, x + R.lit + fill(j, s) + b"\xc3\xa9" + fill(7, j) + b"d", "nonascii"))
            out.append(Spec(r, s, x + R.lit + fill(j, s) + b"\xc3\xa9" + fill(7, j), "nonascii"))
    for s in (0, 7, 15):
        out.append(Spec(r, s, x + R.lit + fill(6, s) + b"\xe2\x84", "rune_cut"))
        out.append(Spec(r, s, x + R.lit + fill(6, s) + b"\xe2\x84d", "rune_cut"))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def edge_uniform(r: int) -> Batch:
    """Rule r's edges alone: every block of the sorted array is r's."""
    b = Batch("EDGE")
    for sp in edge_specs(r):
        place(b, sp)
    return b


MIXED_PARTS = 8


@functools.lru_cache(maxsize=None)
def edge_mixed():
    """Every edge rule's specs dealt round-robin over MIXED_PARTS batches, with a few jobs of the two pad rules
    (the lowest and the highest index): no block of the sorted array is uniform."""
    out = []
    for part in range(MIXED_PARTS):
        b = Batch("EDGE")
        for i in range(3):
            b.job_line(EDGE_PADS[0], i)
            b.job_line(EDGE_PADS[1], i)
        for rs in EDGE_RULES.values():
            for r in rs:
                for sp in edge_specs(r)[part::MIXED_PARTS]:
                    place(b, sp)
        out.append(b)
    return tuple(out)


def edge_counts(b: Batch, no_lines2=False):
    n = len(b.rules)
    w, g = [0] * n, [0] * n
    for ln in b.lines:
        if ln.rule >= 0:
            (g if no_lines2 or b.rules[ln.rule].nfa else w)[ln.rule] += 1
    return w, g


def last_line_batches(r: int, mixed: bool):
    """16 batches whose last line is a job of EDGE rule r (a match in every other one), the batch's length modulo 16
    taking every value."""
    out = []
    for v in range(16):
        for match in (v % 2 == 0,):
            b = Batch("EDGE")
            b.pad_line(40)
            if mixed:
                b.job_line(EDGE_PADS[0], v)
            R = b.rules[r]
            body = R.hit(v) if match else R.miss(v)
            hl = len(b.head(R.host))
            b.k -= 1
            p = (v - 1 - (len(b.out) + hl + len(body))) % 16
            p += 16 if p < 2 else 0
            b.job_line(r, 0, pre=fill(p, v), body=body, tail=b"", kind="last")
            assert len(b.out) % 16 == v and b.lines[-1].rule == r
            out.append(b)
    return out


# ---- job-buffer growth -----------------------------------------------------------------------

GROW_LINES = 44_000
JOB_SLACK = 1 << 20


def grow_batch() -> Batch:
    """Every line carries the literals of all 32 GROW rules (two of them match): 32 jobs a line, more than the job
    buffers of a fresh engine hold: max(n, lines + 2^20) elements asked for, plus a quarter (DevBuf::ensure)."""
    b = Batch("GROW")
    assert GROW_LINES * 32 > (GROW_LINES + JOB_SLACK) * 5 // 4
    for i in range(GROW_LINES):
        hit = (i % 32, (7 * i + 3) % 32)
        b.k = i
        h = b"%d 10.4.%d.%d GET g.example GET /" % (T0, (i // 8) % 8, i % 8)
        b.emit(0, h + b"".join(R.lit + b"e" + (b"y" if k in hit else b"f") for k, R in enumerate(b.rules)))
    return b
