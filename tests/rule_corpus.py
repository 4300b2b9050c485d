"""A generated corpus of literal-bearing rules for the rule planner's tests
(tests/test_rule_plans_cpu.py on the host tables, tests/test_gpu_rule_plans.py
on the device): a pattern generator over a small AST that prints Go syntax, a
sampler that writes strings a pattern is built to match, the texts a rule is
judged on, and the one parser of the plan hooks' text.

Everything here is deterministic from a seed and knows nothing of the engine:
the tests hand in the library and the ruleset handle where a hook is read, and
the oracle alone says whether a text matches."""
from __future__ import annotations

import random
import re
from dataclasses import dataclass, field

# RuleMode of banjax_amd/csrc/regex_compiler.h
MODE_ALWAYS, MODE_NEVER, MODE_ANCHORED, MODE_PREFILTER, MODE_SCAN = range(5)

KELVIN, LONG_S = "K", "ſ"  # the non-ASCII members of the fold orbits of k and s

# ------------------------------------------------------------------ plan reader


@dataclass(frozen=True)
class Literal:
    s: bytes
    ci: tuple          # per byte: compared ASCII-case-insensitively
    gram_off: int = 0  # pref rows only

    @property
    def any_ci(self):
        return any(self.ci)


@dataclass
class Plan:
    mode: int
    equiv: bool                 # pref_equivalent
    pref: list = field(default_factory=list)
    anchor: list = field(default_factory=list)
    anchor_equiv: bool = False  # ^= rows (False with ^~ rows, and with none)
    lead: int = -1              # bjx_debug_rule_lead: -1 or the lead distance

    @property
    def literals(self):
        return self.pref + self.anchor


def parse_plan(text: bytes, lead: int = -1) -> Plan:
    """bjx_debug_rule_literal's text: row 0 is `<mode> <pref_equivalent>`, a
    pref row `<gram_off> <ci mask> <bytes>`, an anchor row `^=` or `^~`, then
    `<ci mask> <bytes>`.  Rows are separated by '\\n', so the text cannot hold
    a literal with '\\n' in it; no pattern of the corpus (nor of the rulesets
    of tests/long_lines.py and tests/wide_scopes.py) has one."""
    rows = text.split(b"\n")
    mode, equiv = (int(x) for x in rows[0].split())
    p = Plan(mode, bool(equiv), lead=lead)
    for row in rows[1:]:
        head, ci, s = row.split(b" ", 2)
        assert len(ci) == len(s) and set(ci) <= set(b"01"), row
        mask = tuple(c == 0x31 for c in ci)
        if head in (b"^=", b"^~"):
            p.anchor.append(Literal(s, mask))
            p.anchor_equiv = head == b"^="
        else:
            p.pref.append(Literal(s, mask, int(head)))
    return p


def read_plan(L, handle, i) -> Plan:
    """The plan record of rule i of a compiled ruleset (L: the loaded library)."""
    n = L.bjx_debug_rule_literal(handle, i, None, 0)
    buf = bytes(n)
    L.bjx_debug_rule_literal(handle, i, buf, n)
    return parse_plan(buf, L.bjx_debug_rule_lead(handle, i))


def _letter(b):
    return 0x41 <= (b & 0xDF) <= 0x5A


def lit_at(text: bytes, i: int, lit: Literal) -> bool:
    """The literal occurs at text[i:]: byte for byte where ci is 0; where it is 1
    the text byte is an ASCII letter equal under | 0x20."""
    if i < 0 or i + len(lit.s) > len(text):
        return False
    for k, c in enumerate(lit.s):
        t = text[i + k]
        if lit.ci[k]:
            if not (_letter(t) and (t | 0x20) == (c | 0x20)):
                return False
        elif t != c:
            return False
    return True


_find_cache = {}


def lit_find(text: bytes, lit: Literal) -> int:
    """First occurrence (lit_at) of the literal in text, or -1."""
    if not lit.any_ci:
        return text.find(lit.s)
    rx = _find_cache.get(lit)
    if rx is None:
        parts = []
        for k, c in enumerate(lit.s):
            one = bytes([c])
            parts.append(b"[" + bytes([c & 0xDF, c | 0x20]) + b"]" if lit.ci[k] and _letter(c) else re.escape(one))
        rx = _find_cache[lit] = re.compile(b"".join(parts), re.S)
    m = rx.search(text)
    return m.start() if m else -1


def first_hit(text: bytes, lits) -> int:
    """First occurrence of any of the literals, or -1."""
    best = -1
    for l in lits:
        i = lit_find(text, l)
        if i >= 0 and (best < 0 or i < best):
            best = i
    return best


# ------------------------------------------------------------------------- AST

_SPECIAL = set("\\.+*?()|[]{}^$")


def _esc(w):
    return "".join("\\" + c if c in _SPECIAL else c for c in w)


class Node:
    atomic = False  # prints as one repeatable unit


@dataclass
class Lit(Node):
    word: str
    fold: bool = False  # (?i:word)

    def go(self):
        return "(?i:%s)" % _esc(self.word) if self.fold else _esc(self.word)

    @property
    def atomic(self):
        return self.fold or len(self.word) == 1


@dataclass
class Cls(Node):
    src: str
    members: tuple  # strings the sampler picks from
    atomic = True

    def go(self):
        return self.src


@dataclass
class Rep(Node):
    sub: Node
    min: int
    max: int | None  # None: unbounded
    atomic = False

    def go(self):
        s = self.sub.go() if self.sub.atomic else "(?:%s)" % self.sub.go()
        if (self.min, self.max) == (0, None):
            return s + "*"
        if (self.min, self.max) == (1, None):
            return s + "+"
        if (self.min, self.max) == (0, 1):
            return s + "?"
        if self.max is None:
            return s + "{%d,}" % self.min
        if self.min == self.max:
            return s + "{%d}" % self.min
        return s + "{%d,%d}" % (self.min, self.max)


@dataclass
class Alt(Node):
    subs: list  # an empty Cat is the empty branch
    capture: bool = False
    atomic = True

    def go(self):
        return ("(%s)" if self.capture else "(?:%s)") % "|".join(s.go() for s in self.subs)


@dataclass
class Cat(Node):
    subs: list

    def go(self):
        return "".join(s.go() for s in self.subs)


@dataclass
class Cap(Node):
    sub: Node
    atomic = True

    def go(self):
        return "(%s)" % self.sub.go()


@dataclass
class Fold(Node):
    """(?i) over the whole of `sub`: printed as a leading (?i) at the top of a
    pattern, as (?i:...) inside one."""
    sub: Node
    top: bool = True
    atomic = True

    def go(self):
        return ("(?i)%s" if self.top else "(?i:%s)") % self.sub.go()


@dataclass
class DotStar(Node):
    atomic = False

    def go(self):
        return ".*"


@dataclass
class Assert(Node):
    src: str  # \b \B ^ $ (?m:^) (?m:$)
    atomic = True

    def go(self):
        return self.src


EMPTY = Cat([])

# ---------------------------------------------------------------------- sampler

_MULTI = ("é", "\U0001F600")  # a 2-byte and a 4-byte rune
_FILL_STR = (" ", "a", "Z", "9", "_", "-", "/", "q7", "é", KELVIN, "\U0001F600")


def _fold_str(s, rnd, ks):
    """Random case; k and s become U+212A and U+017F at rate ks."""
    out = []
    for c in s:
        if c.isascii() and c.isalpha():
            r = rnd.random()
            if c in "kK" and r < ks:
                c = KELVIN
            elif c in "sS" and r < ks:
                c = LONG_S
            else:
                c = c.upper() if rnd.random() < 0.5 else c.lower()
        out.append(c)
    return "".join(out)


def _far_run(rnd):
    """70-200 bytes for an unbounded piece, a non-ASCII byte among the first 64."""
    head = "".join(rnd.choice(_FILL_STR[:8]) for _ in range(rnd.randint(5, 40))) + rnd.choice(("é", KELVIN))
    n = rnd.randint(70, 200)
    while len(head.encode()) < n:
        head += rnd.choice(_FILL_STR[:9])
    return head


def _sample(n, rnd, fold, far, ks):
    if isinstance(n, Lit):
        return _fold_str(n.word, rnd, ks) if (fold or n.fold) else n.word
    if isinstance(n, Cls):
        m = rnd.choice(n.members)
        return _fold_str(m, rnd, ks) if fold else m
    if isinstance(n, Rep):
        hi = n.max if n.max is not None else n.min + 3
        k = rnd.choice((n.min, hi, rnd.randint(n.min, hi)))
        if far and n.max is None:
            k = rnd.randint(70, 100)
        return "".join(_sample(n.sub, rnd, fold, far and n.max is not None, ks) for _ in range(k))
    if isinstance(n, Alt):
        return _sample(rnd.choice(n.subs), rnd, fold, far, ks)
    if isinstance(n, Cat):
        return "".join(_sample(s, rnd, fold, far, ks) for s in n.subs)
    if isinstance(n, Cap):
        return _sample(n.sub, rnd, fold, far, ks)
    if isinstance(n, Fold):
        return _sample(n.sub, rnd, True, far, ks)
    if isinstance(n, DotStar):
        if far:
            return _far_run(rnd)
        return "".join(rnd.choice(_FILL_STR) for _ in range(rnd.choice((0, 0, 1, 3, 9))))
    if isinstance(n, Assert):
        return ""
    raise TypeError(n)


def sample(ast, rnd, far=False) -> bytes:
    """A string the pattern is built to match, assertions ignored.  far: every
    unbounded piece runs for 70 bytes or more, so that what decides the rule lies
    far behind where its automaton starts."""
    # now and then every folded k and s of a sample leaves ASCII: the longest a folded literal gets
    return _sample(ast, rnd, False, far, rnd.choice((0.15, 0.15, 0.15, 0.6, 1.0))).encode()


# -------------------------------------------------------------------- generator

LONG = ["abcd", "wxyz", "token", "=token", "kiosk", "mask", "scrapy", "GET ", "HTTP/1.1", ".php", "wp-login", "/admin",
        "ahrefs", "semrush", "mj12", "python-requests", "curl/7.", "Mozilla/5.0", "Firefox/", "Macintosh", "sqlmap",
        "/etc/passwd", "UNION", "Select", "efgh", "xmlrpc", "nikto", "MASK", "Kiosk", "index.", "?id=1", "/.env",
        "POST /", "sitemap", "Basket", "zgrab", "qwer7", "HeadlessChrome", ".asp", "bot/"]
SHORT = ["K", "s", "k", "S", "ab", "cd", "xy", "x", "y", "bot", "/", "=", "id", "no", "1", "-", "Sk", "ok"]
SK_WORDS = ["scrapy", "kiosk-token", "sqlmap", "semrush", "mask=on", "kiosk", "mask", "basket", "nikto", "zgrabs",
            "wxyzs", "abcdk", "tokens", "kkabcd", "skkwxyz", "ssk-token", "ksadmin"]

C_DIGIT = Cls("[0-9]", tuple("0123456789"))
C_LOWER = Cls("[a-z]", tuple("abkmsz"))
C_HEX = Cls("[a-f0-9]", tuple("af09c"))
C_PD = Cls("\\d", tuple("0369"))
C_PW = Cls("\\w", tuple("aZ_5ks"))
C_PS = Cls("\\s", (" ", "\t"))
C_E = Cls("é", ("é",))
C_DOT = Cls(".", ("a", " ", "/", "K") + _MULTI + (KELVIN,))
C_NS = Cls("\\S", ("a", "-", "7") + _MULTI)
C_NSLASH = Cls("[^/]", ("a", " ", "?") + _MULTI)
C_AA = Cls("[aA]", ("a", "A"))
C_KK = Cls("[kK]", ("k", "K"))
C_EE = Cls("[eE]", ("e", "E"))
C_SS = Cls("[sS]", ("s", "S"))
CLASSES = [C_DIGIT, C_LOWER, C_HEX, C_PD, C_PW, C_PS, C_E, C_DOT, C_NS, C_NSLASH, C_AA, C_KK, C_EE]
BOUNDED = [C_DIGIT, C_LOWER, C_HEX, C_PD, C_PW, C_E, C_DOT, C_NS, C_NSLASH, C_AA, C_KK]


def _wordc(c):
    return c.isascii() and (c.isalnum() or c == "_")


def _long(rnd):
    return rnd.choice(LONG)


def _word(rnd):
    return rnd.choice(LONG if rnd.random() < 0.6 else SHORT)


def _lit(rnd, w=None, fold_p=0.25):
    return Lit(w if w is not None else _long(rnd), rnd.random() < fold_p)


def _maybe_fold(rnd, n, p=0.3):
    return Fold(n) if rnd.random() < p else n


def _tail(rnd):
    k = rnd.randrange(6)
    if k == 0:
        return []
    if k == 1:
        return [DotStar()]
    if k == 2:
        return [rnd.choice(CLASSES)]
    if k == 3:
        return [Rep(rnd.choice(CLASSES), rnd.randrange(0, 2), rnd.choice((None, 3)))]
    if k == 4:
        return [DotStar(), _lit(rnd, _word(rnd), 0.1)]
    return [Assert("$")]


def s_pure(rnd):
    ws = [_long(rnd)] + [_word(rnd) for _ in range(rnd.choice((0, 0, 1)))]
    rnd.shuffle(ws)
    n = Cat([Lit(w) for w in ws]) if len(ws) > 1 else Lit(ws[0])
    if rnd.random() < 0.2:
        return Lit(ws[0], True)
    if rnd.random() < 0.2:
        return Cap(n)
    return _maybe_fold(rnd, n, 0.25)


def s_alt_suffix(rnd):
    ws = rnd.sample(LONG + SHORT, rnd.randint(2, 5))
    alt = Alt([Lit(w) for w in ws], capture=rnd.random() < 0.6)
    k = rnd.randrange(4)
    suf = Lit(rnd.choice(["bot", "bot/", "-agent", "/1.", "k", "s", "xy"]))
    if k == 0:
        n = Cat([alt, suf])
    elif k == 1:
        n = Cat([Lit(rnd.choice(["/", "ua=", "x", "GET /"])), alt])
    elif k == 2:
        n = Cat([Lit(rnd.choice(["/", "ua=", "k"])), alt, suf])
    else:
        n = alt
    return _maybe_fold(rnd, n, 0.4)


def s_dotstar(rnd):
    x, y = _lit(rnd), _lit(rnd, _word(rnd))
    if rnd.random() < 0.25:
        x = Alt([_lit(rnd, fold_p=0), _lit(rnd, fold_p=0)])
    k = rnd.randrange(6)
    subs = [[DotStar(), x, DotStar()], [x, DotStar(), y], [DotStar(), x], [x, DotStar()],
            [x, DotStar(), y, DotStar(), _lit(rnd, _word(rnd))], [DotStar(), x, DotStar(), y, DotStar()]][k]
    return _maybe_fold(rnd, Cat(subs), 0.15)


def _piece(rnd):
    c = rnd.choice(BOUNDED)
    k = rnd.randrange(5)
    if k == 0:
        return c
    if k == 1:
        m = rnd.randint(1, 3)
        return Rep(c, m, m)
    if k == 2:
        return Rep(c, rnd.randint(0, 1), rnd.randint(1, 4))
    if k == 3:
        return Cat([Lit(rnd.choice(SHORT)), Rep(c, 1, 2)])
    return Rep(Alt([Lit(rnd.choice(SHORT)), c]), 1, 2)


def s_bounded(rnd):
    if rnd.random() < 0.35:  # (?i) over a literal whose k / s break it
        w = rnd.choice(SK_WORDS)
        n = Lit(w)
        if rnd.random() < 0.4:
            n = Cat([n] + _tail(rnd))
        return Fold(n)
    n = Cat([_piece(rnd), _lit(rnd, fold_p=0.15)] + _tail(rnd))
    if rnd.random() < 0.2:
        n = Cat([DotStar(), n])
    return n


def s_caret(rnd):
    k = rnd.randrange(10)
    w = Lit(_word(rnd), rnd.random() < 0.2)
    if k < 3:
        n = [w] + rnd.choice(([], [DotStar()], [DotStar(), DotStar()]))
    elif k < 6:
        n = [w] + rnd.choice(([rnd.choice(CLASSES)], [Assert("$")], [Rep(rnd.choice(CLASSES), 1, None)],
                              [DotStar(), _lit(rnd)], [Rep(rnd.choice(CLASSES), 0, 3), Lit("/")]))
    elif k == 6:
        n = [Alt([Lit(a) for a in rnd.sample(["GET", "POST", "HEAD", "k", "PUT /"], 2)], capture=rnd.random() < 0.5),
             Lit(rnd.choice([" /", " ", "/x"]))] + _tail(rnd)
    elif k == 7:
        n = [Rep(rnd.choice(CLASSES), 1, rnd.choice((None, 3))), _lit(rnd)]
    elif k == 8:
        n = [rnd.choice((Assert("\\b"), DotStar(), Rep(Lit("x"), 0, 1))), _lit(rnd, rnd.choice(["abcd", "token", "kiosk"]))]
    else:
        n = [rnd.choice(CLASSES), w]
    n = Cat([Assert("^")] + n)
    if k == 9 and rnd.random() < 0.5:
        n = Cap(n)
    return _maybe_fold(rnd, n, 0.15)


def _inner_assert(w, i):
    return "\\b" if _wordc(w[i - 1]) != _wordc(w[i]) else "\\B"


def s_assert(rnd):
    w = _long(rnd)
    k = rnd.randrange(8)
    if k == 0:
        n = [Assert("\\b" if _wordc(w[0]) else "\\B"), Lit(w)]
    elif k == 1:
        n = [Lit(w), Assert("\\b" if _wordc(w[-1]) else "\\B")]
    elif k == 2:
        n = [Alt([Lit("x"), Cat([Assert("^"), Lit("y")])]), Lit(w)]
    elif k == 3:
        n = [Lit(w), Assert(rnd.choice(("$", "(?m:$)")))]
    elif k == 4:
        n = [Assert("(?m:^)"), Lit(w)] + _tail(rnd)
    elif k == 5:
        i = rnd.randrange(1, len(w))
        n = [Lit(w[:i]), Assert(_inner_assert(w, i)), Lit(w[i:])]
    elif k == 6:
        n = [DotStar(), Assert("\\b" if _wordc(w[0]) else "\\B"), Lit(w), DotStar()]
    else:
        n = [Alt([Assert("^"), Lit(" ")]), Lit(w), Alt([Assert("$"), Lit(" ")])]
    return _maybe_fold(rnd, Cat(n), 0.15)


def s_optional(rnd):
    w = _long(rnd) + rnd.choice(LONG + SHORT)
    i = rnd.randrange(1, len(w) - 2)
    j = rnd.randrange(i + 1, min(len(w), i + 4))
    a, b, c = w[:i], w[i:j], w[j:]
    k = rnd.randrange(4)
    if k == 0:
        mid = Alt([Lit(b), EMPTY], capture=True)
    elif k == 1:
        mid = Rep(Lit(b), 0, 1)
    elif k == 2:
        mid = Alt([EMPTY, Lit(b), Lit(rnd.choice(SHORT))])
    else:
        mid = Rep(Lit(b[0]), 0, 1)
        c = b[1:] + c
    return _maybe_fold(rnd, Cat([Lit(a), mid, Lit(c)]), 0.2)


def s_exact_rep(rnd):
    k = rnd.randrange(5)
    if k == 0:
        n = Rep(Cap(Lit(_long(rnd))), 2, 2)
    elif k == 1:
        n = Cat([Rep(Alt([Lit(a) for a in rnd.sample(SHORT, 2)], capture=True), 2, 2), Lit(_word(rnd))])
    elif k == 2:
        n = Rep(Alt([Lit(a) for a in rnd.sample(["ab", "cd", "ks", "xy", "01"], 2)]), 3, 3)
    elif k == 3:
        n = Cat([Rep(rnd.choice((C_AA, C_KK, C_EE, C_SS)), 2, 2), Lit(_word(rnd))])
    else:
        n = Cat([Lit(_word(rnd)), Rep(Lit(rnd.choice(SHORT)), 2, 3), Lit(_word(rnd))])
    return _maybe_fold(rnd, n, 0.2)


def s_product(rnd):
    """Exact sets near cross()'s limits: 32 strings, 96 bytes."""
    k = rnd.randrange(6)
    tag = rnd.choice(["q", "zz", "k", "ua", "s-"])
    if k == 0:  # 31, 32, 33 alternatives
        n = Alt([Lit("%s%02dxy" % (tag, i)) for i in range(rnd.choice((31, 32, 33)))])
    elif k == 1:  # 2^4, 2^5, 2^6 strings
        m = rnd.choice((4, 5, 6))
        n = Cat([Rep(Alt([Lit(a) for a in rnd.sample(["ab", "cd", "xy", "01", "k-"], 2)]), m, m), Lit(tag)])
    elif k == 2:  # a literal of 94..98 bytes
        w = (tag + "0123456789abcdefghij-") * 6
        n = Lit(w[:rnd.choice((94, 95, 96, 97, 98))])
    elif k == 3:  # 4 x 8 = 32, 3 x 11 = 33, 5 x 7 = 35 strings
        a, b = rnd.choice(((4, 8), (3, 11), (5, 7), (2, 16)))
        n = Cat([Alt([Lit("%s%d" % (tag, i)) for i in range(a)]), Lit("-"), Alt([Lit("v%02d" % i) for i in range(b)])])
    elif k == 4:  # two strings of 47..49 bytes, twice: 94..98 bytes
        m = rnd.choice((47, 48, 49))
        n = Rep(Alt([Lit(("ab" + tag + "0123456789" * 5)[:m]), Lit(("cd" + tag + "9876543210" * 5)[:m])]), 2, 2)
    else:  # 32 / 33 strings behind a bounded piece
        n = Cat([Rep(C_DIGIT, 1, 2), Alt([Lit("%s%02dxy" % (tag, i)) for i in range(rnd.choice((30, 32, 33)))])])
    return _maybe_fold(rnd, n, 0.15)


def s_class_lit(rnd):
    """Letters written as two-range classes: [aA] becomes a ci byte, [kK] must not."""
    w = rnd.choice(["abcd", "token", "kiosk", "mask", "admin", "select", "wxyz"])
    subs = []
    for c in w:
        if c.isalpha() and rnd.random() < 0.5:
            subs.append(Cls("[%s%s]" % ((c, c.upper()) if rnd.random() < 0.5 else (c.upper(), c)), (c, c.upper())))
        else:
            subs.append(Lit(c))
    if rnd.random() < 0.4:
        subs = [_piece(rnd)] + subs
    return Cat(subs + _tail(rnd))


def s_always(rnd):
    w = Lit(_word(rnd))
    return rnd.choice([Cat([DotStar()]), Assert("^"), Assert("$"), Rep(w, 0, None), Alt([w, EMPTY], capture=True),
                       Rep(w, 0, 1), Cat([Rep(w, 0, 1), Rep(rnd.choice(CLASSES), 0, None)]), Cat([DotStar(), Assert("$")]),
                       Cat([Assert("^"), DotStar()]), Cat([DotStar(), Rep(w, 0, 3)]), Alt([w, DotStar()]),
                       Cat([Assert("^"), Rep(w, 0, None)]), Rep(Alt([w, rnd.choice(CLASSES)]), 0, 2)])


def s_never(rnd):
    a, b = Lit(_word(rnd)), Lit(_word(rnd))
    wa = rnd.choice(["abcd", "token", "xy", "k"])
    return rnd.choice([Cat([a, Assert("^"), b]), Cat([a, Assert("$"), b]), Cat([Assert("$"), b]), Cat([a, Assert("^")]),
                       Cat([Lit(wa), Assert("\\b"), Lit(wa)]), Cat([Lit("-"), Assert("\\B"), Lit(wa)]),
                       Cat([DotStar(), a, Assert("$"), rnd.choice(CLASSES)]), Cls("[^\\x00-\\x{10FFFF}]", ("",)),
                       Cat([a, Cls("[^\\x00-\\x{10FFFF}]", ("",))])])


def s_scan(rnd):
    c = rnd.choice(CLASSES)
    s = Lit(rnd.choice(SHORT))
    return rnd.choice([
        Cat([Rep(C_DIGIT, 1, 3), Lit("."), Rep(C_DIGIT, 1, 3)]), Cat([Rep(C_PD, 1, None), s]), Cat([s, c, s]),
        Fold(Lit(rnd.choice(["kiosk", "mask", "sks", "Sk", "ask"]))), Cat([Lit("id="), Rep(C_PD, 1, None)]),
        Cat([s, Rep(c, 1, 3)]), Cat([Assert("\\b"), s, Assert("\\b")]), Cat([c, Rep(C_LOWER, 2, 2), Assert("$")]),
        Alt([s, Lit(_long(rnd))]), Cat([C_E, Rep(c, 0, None), s]), Cat([s, DotStar(), Lit(rnd.choice(SHORT))])])


def _rand_node(rnd, depth):
    k = rnd.randrange(10 if depth > 0 else 5)
    if k < 3:
        return _lit(rnd, _word(rnd))
    if k == 3:
        return rnd.choice(CLASSES)
    if k == 4:
        return rnd.choice([DotStar(), Assert("\\b"), Assert("\\B"), Assert("(?m:$)"), Assert("(?m:^)")])
    if k < 7:
        return Cat([_rand_node(rnd, depth - 1) for _ in range(rnd.randint(2, 3))])
    if k == 7:
        subs = [_rand_node(rnd, depth - 1) for _ in range(rnd.randint(2, 3))]
        if rnd.random() < 0.25:
            subs.append(EMPTY)
        return Alt(subs, capture=rnd.random() < 0.5)
    if k == 8:
        lo = rnd.randint(0, 2)
        return Rep(_rand_node(rnd, depth - 1), lo, rnd.choice((None, lo, lo + 2)))
    return Fold(_rand_node(rnd, depth - 1), top=False)


def s_random(rnd):
    n = Cat([_rand_node(rnd, 2) for _ in range(rnd.randint(1, 3))])
    if rnd.random() < 0.15:
        n = Cat([Assert("^"), n])
    return n


SHAPES = [("pure", s_pure, 8), ("alt_suffix", s_alt_suffix, 10), ("dotstar", s_dotstar, 9), ("bounded", s_bounded, 16),
          ("caret", s_caret, 14), ("assert", s_assert, 9), ("optional", s_optional, 7), ("exact_rep", s_exact_rep, 6),
          ("product", s_product, 6), ("class_lit", s_class_lit, 6), ("always", s_always, 3), ("never", s_never, 3),
          ("scan", s_scan, 5), ("random", s_random, 10)]


@dataclass
class Rule:
    pattern: str
    ast: Node
    shape: str


def patterns(seed: int, n: int, compiles=None):
    """n distinct generated rules; `compiles(pattern)` keeps a pattern (the
    tests pass the oracle's compile check)."""
    rnd = random.Random(seed)
    names, fns, weights = zip(*SHAPES)
    out, seen = [], set()
    while len(out) < n:
        k = rnd.choices(range(len(fns)), weights)[0]
        ast = fns[k](rnd)
        pat = ast.go()
        if pat in seen or "'" in pat or "\n" in pat or (compiles and not compiles(pat)):
            continue
        seen.add(pat)
        out.append(Rule(pat, ast, names[k]))
    return out


# ------------------------------------------------------------------------ texts

FILLER = (b" ", b"a", b"Zq", b"w_9", b"-", b"/", b"\xc3\xa9", KELVIN.encode(), b"\xff", b"\xc3", b"\xf0\x9f\x98",
          b"GET h.com GET /", b"7", b"=")
NONASCII_FILLER = (b"\xc3\xa9", KELVIN.encode(), b"\xff", b"\xc3", b"\xf0\x9f\x98")
# P5 of tests/test_rule_plans_cpu.py: put in front of a text an anchored rule matches
PREFIXES = (b" ", b"x", b"\xc3\xa9", b"\xff", b"\xf0\x9f\x98", b"GET h.com GET /", b"K")

NEAR_MISS = ("lit_flip", "lit_repl", "lit_nofirst", "lit_nolast")  # text kinds a literal is one byte off in


def filler(rnd, lo=0, hi=6):
    return b"".join(rnd.choice(FILLER) for _ in range(rnd.randint(lo, hi)))


def _flip(b):
    return b ^ 0x20 if _letter(b) else b


def _mutations(s, rnd):
    if not s:
        return []
    i, j, k = (rnd.randrange(len(s)) for _ in range(3))
    letters = [q for q in range(len(s)) if _letter(s[q])]
    out = [("del", s[:i] + s[i + 1:]), ("repl", s[:k] + rnd.choice((b"#", b"0", b"\xc3\xa9", b"K")) + s[k + 1:])]
    if letters:
        j = rnd.choice(letters)
        out.append(("flip", s[:j] + bytes([_flip(s[j])]) + s[j + 1:]))
    return out


def literal_texts(lit: Literal, rnd):
    """The texts every claimed literal adds."""
    s = lit.s
    out = [("lit", s), ("lit_upper", s.upper()), ("lit_lower", s.lower()), ("lit_nofirst", s[1:]), ("lit_nolast", s[:-1]),
           ("lit_wrap", rnd.choice((b" ", b"a", b"\xc3\xa9", b"\xff")) + s + rnd.choice((b" ", b"a", b"\xc3", b"/")))]
    letters = [q for q in range(len(s)) if _letter(s[q])]
    if letters:
        j = rnd.choice(letters)
        # a flip on a byte the plan compares exactly is a near miss; on a ci byte it is another hit
        out.append(("lit_flip" if not lit.ci[j] else "lit_ciflip", s[:j] + bytes([_flip(s[j])]) + s[j + 1:]))
        strict = [q for q in letters if not lit.ci[q]]
        if strict and lit.ci[j]:
            j = rnd.choice(strict)
            out.append(("lit_flip", s[:j] + bytes([_flip(s[j])]) + s[j + 1:]))
    j = rnd.randrange(len(s))
    out.append(("lit_repl", s[:j] + (b"#" if s[j] != 0x23 else b"%") + s[j + 1:]))
    return out


def rule_texts(rule: Rule, plan: Plan, seed: int, n_samples=16):
    """[(kind, text)] a rule is judged on; no text holds '\\n'."""
    rnd = random.Random(seed)
    out = [("empty", b"")]
    samples = [sample(rule.ast, rnd) for _ in range(n_samples)]
    for q, s in enumerate(samples):
        out.append(("sample", s))
        out.append(("wrapped", filler(rnd, 1) + s + filler(rnd)))
        # a non-ASCII byte or a cut rune right in front of the sample
        out.append(("wrapped", filler(rnd, 0, 3) + rnd.choice(NONASCII_FILLER) + s + filler(rnd, 0, 3)))
        out.extend(_mutations(s, rnd))
        other = samples[(q + 1) % len(samples)]
        out.append(("front", other[:rnd.randint(1, 4)] + s))
    for lit in plan.literals:
        out.extend(literal_texts(lit, rnd))
    seen, uniq = set(), []
    for kind, t in out:
        t = t.replace(b"\n", b" ")
        if (kind, t) not in seen:
            seen.add((kind, t))
            uniq.append((kind, t))
    return uniq


def plan_classes(pattern: str, plan: Plan):
    """The plan classes a rule counts for (the floors of tests/test_rule_plans_cpu.py)."""
    c = []
    if plan.mode == MODE_ALWAYS:
        c.append("always")
    elif plan.mode == MODE_NEVER:
        c.append("never")
    elif plan.mode == MODE_SCAN:
        c.append("scan")
    elif plan.mode == MODE_ANCHORED:
        c.append("anchored_none" if not plan.anchor else "anchored_eq" if plan.anchor_equiv else "anchored_ne")
    else:
        if plan.equiv:
            c.append("pref_equiv")
        elif plan.lead < 0:
            c.append("pref_nolead")
        if plan.lead == 0:
            c.append("pref_lead0")
        if plan.lead > 0:
            c.append("pref_lead")
        if any(l.any_ci for l in plan.pref):
            c.append("pref_ci")
        if len(plan.pref) >= 2:
            c.append("pref_multi")
        if has_fold_ks(pattern):
            c.append("pref_fold_ks")
    return c


PLAN_CLASSES = ("always", "never", "anchored_eq", "anchored_ne", "anchored_none", "pref_equiv", "pref_nolead", "pref_lead0",
                "pref_lead", "pref_ci", "pref_multi", "pref_fold_ks", "scan")


def has_fold_ks(pattern: str) -> bool:
    """The pattern holds (?i) over a letter k or s."""
    if pattern.startswith("(?i)"):
        return bool(re.search(r"[kKsS]", re.sub(r"\\.", "", pattern[4:])))
    return any(re.search(r"[kKsS]", re.sub(r"\\.", "", g)) for g in re.findall(r"\(\?i:([^()]*)\)", pattern))


# ---------------------------------------------------------------- log lines
#
# A text T of a rule as access-log lines `<ts> <ip> <rest>`; the rules match on
# rest.  A line whose rest has fewer than two spaces is an error line, so every
# layout writes two.
#   start     rest = T + " - -": T at rest[0], where anchored rules look
#   end       rest = "GET hN.com " + T: T ends the line ($, \b at the end, accept at end)
#   window    end, padded so that the rule's first literal in T starts at line byte
#             WIN - len + 1 .. WIN: it straddles the end of k_lines2's window
#   far       end, with 70-200 bytes before T and, in a matching T, inside every
#             unbounded piece: the decision lies past the inline automata's 64 steps
#   overflow  end, with five or more literal occurrences before T: more than the
#             scan pass has hit slots for a line
LAYOUTS = ("start", "end", "window", "far", "overflow")
TS = 1700000000
WIN = 112  # lines2.h kL2Win
_PAD = b"mn o-p/1"


@dataclass
class Line:
    layout: str
    owner: int  # index in the ruleset of the rule whose text this is
    data: bytes


def _head(j):
    return b"%d 9.9.%d.%d " % (TS, j % 4, j % 61)


def _frame(j):
    return _head(j) + b"GET h%d.com " % (j % 7)


def _cased(lit: Literal, rnd):
    return bytes((c ^ 0x20) if ci and rnd.random() < 0.5 else c for c, ci in zip(lit.s, lit.ci))


def _near(lit: Literal, rnd):
    j = rnd.randrange(len(lit.s))
    return lit.s[:j] + (b"#" if lit.s[j] != 0x23 else b"%") + lit.s[j + 1:]


def text_lines(owner, rule, plan, t, m, k, rnd, n_win, pool):
    """The lines of text t (the oracle's answer on it alone: m; the k-th text of
    its rule).  pool: literals of the other rules of the ruleset."""
    out = []
    j = rnd.randrange(1 << 20)
    out.append(Line("start", owner, _head(j) + t + b" - -"))
    out.append(Line("end", owner, _frame(j) + t))
    # window: the first pref literal in t, or t itself where the rule claims none
    f, ln = 0, max(1, min(len(t), 24))
    if plan.pref:
        h = first_hit(t, plan.pref)
        if h >= 0:
            f, ln = h, len(next(l for l in plan.pref if lit_at(t, h, l)).s)
    fr = _frame(j)
    offs = [b for b in range(WIN - ln + 1, WIN + 1) if b - f - len(fr) >= 0]
    if len(offs) > n_win:
        offs = [offs[(len(offs) - 1) * q // (n_win - 1)] for q in range(n_win)] if n_win > 1 else [offs[len(offs) // 2]]
    for b in offs or [len(fr) + f]:
        pad = (_PAD * 16)[:b - f - len(fr)]
        out.append(Line("window", owner, fr + pad + t))
    far = sample(rule.ast, rnd, far=True) if m else t
    out.append(Line("far", owner, _frame(j + 1) + _far_run(rnd).encode() + b" " + far))
    own = plan.pref or plan.anchor
    items = []
    for q in range(rnd.randint(5, 7)):
        if own and (m or (k % 2 == 1 and not plan.equiv)):
            items.append(_cased(rnd.choice(own), rnd) if rnd.random() < 0.8 else _near(rnd.choice(own), rnd))
        elif own and q % 3 == 0:
            items.append(_near(rnd.choice(own), rnd))
        elif pool:
            items.append(_cased(rnd.choice(pool), rnd))
        else:
            items.append(b"qq")
    out.append(Line("overflow", owner, _frame(j + 2) + b" ".join(items) + b" " + t))
    return out


def rule_lines(owner, rule, plan, texts, want, seed, n_match, n_non, n_win, pool):
    """Lines for n_match texts the oracle matches and n_non it does not (near
    misses of the literals first), in every layout.  The lines of a text depend
    on the seed and the text's rank alone, so a larger budget only adds lines."""
    rnd = random.Random(seed)
    yes = [t for (_, t), m in zip(texts, want) if m and len(t) < 160]
    near = [t for (kind, t), m in zip(texts, want) if not m and kind in NEAR_MISS]
    no = [t for (kind, t), m in zip(texts, want) if not m and kind not in NEAR_MISS and t and len(t) < 160]
    rnd.shuffle(yes), rnd.shuffle(near), rnd.shuffle(no)
    # a short hit offset leaves room for the window layout's padding
    yes.sort(key=lambda t: max(0, first_hit(t, plan.pref)) > 60 if plan.pref else len(t) > 60)
    non = [x for pair in zip(near, no) for x in pair] + near[len(no):] + no[len(near):]
    out = []
    for k, t in enumerate(yes[:n_match]):
        out += text_lines(owner, rule, plan, t, True, k, random.Random(seed * 7919 + 2 * k + 1), n_win, pool)
    for k, t in enumerate(non[:n_non]):
        out += text_lines(owner, rule, plan, t, False, k, random.Random(seed * 7919 + 2 * k), n_win, pool)
    return out


def batch(lines):
    return b"".join(l.data + b"\n" for l in lines)
