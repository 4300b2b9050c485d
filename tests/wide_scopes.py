"""Rulesets and batches for scopes of more than 128 positions.

A line's scope is its host's site rules followed by the global rules.  Past
128 positions the line kernels hand the line to the per-line fallback
(k_parse_match<SLOW>), which decides it in decide_wide: not every rule of the
scope by its automaton, as the reference does (regex_rate_limiter.go:175-211),
but the rules the line's literal hits name, its anchored / no-literal rules and
its ALWAYS rules.  rules_yaml(kind) builds the rulesets that reach the branches
of that walk, batch(kind, seed) the lines (checked on the host by
tests/test_wide_scopes_cpu.py, fed to the engine by
tests/test_gpu_wide_scopes.py).

Hosts: big, mid and tiny.example.com have site rules; other.example.org has
none.  Kinds (global rules / site rules):
  MIX     100 / big 60, mid 20, tiny 2: only big's scope (160 positions, three
          mask words) is wide, so k_lines decides the other hosts' lines and
          lists big's for the fallback
  ALL     140 / the same: every scope wide, no line pass (k_parse_match), or
          k_lines listing every line with BJX_LINES=1
  SITE    20 / big 150, mid 5: site positions past 128, global ones from 150
  NOLIT   130 / big 3, no rule with a prefilter literal: the every-rule loop
          of the fallback writing three mask words
  NARROW  60 / as many as MIX: no scope past 128, the same lines through k_lines2 (few
          literals under many tails: its tables must fit k_lines2's LDS)
  WNFA    130 one-literal fillers and wide-NFA rules / big 4

Rule kinds (Rule.letter), each placed among big's site rules in every 64-position
band the ruleset has and among the global rules where big sees it past
position 128 (NARROW: past 64):
  a  equivalent one-literal rule            tok017x
  b  literal with a regex tail              \\/p017\\/[a-z]+  .*Fox017\\/\\d+  Mac017.*Fox017\\/\\d+
  c  case-insensitive alternation           (?i)scr017py|mec017ize
  d  ALWAYS                                 .*
  e  anchored, with an anchor literal       ^GET \\S+ GET \\/q17\\/
  f  anchored and equivalent                ^POST
  g  no literal, anchored or not            ^[A-Z]+ \\S+ [A-Z]+ \\/7\\d   \\d{3}z
  h  a, b, d or e with hosts_to_skip: big
  i  host-split site rules (the literal spells the rule's own host), the
     identical pair on big, mid and tiny:   POST <host> POST \\/xmlrpc\\.php (equivalent)
                                            GET <host> GET \\/wp-login\\.php HTTP\\/[0-2.]+ .*
     and two global rules whose literals are exactly the host-free pieces
  j  30 literals shr00_ .. shr29_, each in a global rule and in site rules of big
     and (half of them; SITE: three) mid, with another regex tail in each
"""
from __future__ import annotations

import random
from dataclasses import dataclass, field

from tests.long_lines import FILL, filler_literal

T0 = 1700000000
BIG, MID, TINY, OTHER = "big.example.com", "mid.example.com", "tiny.example.com", "other.example.org"
HOSTS = (BIG, MID, TINY, OTHER)
KINDS = ("MIX", "ALL", "SITE", "NOLIT", "NARROW", "WNFA")
SEEDS = (1, 2)
N_LINES = {"MIX": 4000, "ALL": 4000, "SITE": 4000, "NARROW": 4000, "NOLIT": 1500, "WNFA": 400}
IPS = ["10.9.%d.%d" % (k // 8, k % 8) for k in range(60)] + ["2001:db8::%x" % k for k in range(1, 5)]
ALLOWED_IP = IPS[59]
FAR_OFFSETS = (65534, 65535, 65536, 70001)
MODE_ALWAYS, MODE_ANCHORED, MODE_PREFILTER, MODE_SCAN = 0, 2, 3, 4
F_METHODS = ("POST", "PUT", "HEAD", "PATCH")
G2_LETTERS = "zwvu"
DECISIONS = ("challenge", "nginx_block", "iptables_block")


@dataclass
class Rule:
    name: str
    regex: str
    letter: str               # a-j, "p" (the split pieces' global rules), "w" (wide NFA), "-" (fillers)
    sub: str
    site: str = None
    skip: bool = False
    mode: int = MODE_PREFILTER
    equiv: bool = False       # pref_equivalent, or the anchor literal's for mode 2
    lits: list = field(default_factory=list)   # (bytes, case-insensitive), as bjx_debug_rule_literal lists them
    hit: list = field(default_factory=list)    # URI tokens that make the rule match
    miss: list = field(default_factory=list)   # tokens that hold its literal without a match, or a near miss of it
    key: int = 0              # e: the q number; g1: the digit; f: the method's index; g2: the letter's index
    interval: int = 5
    hits: int = 1
    decision: str = "challenge"
    wide: bool = False        # kRuleNfaWide expected


def piece_of(lit: bytes, host: str) -> bytes:
    """The longest piece of lit left when the host is cut out (engine.hip split_at_host)."""
    parts = lit.split(host.encode())
    if len(parts) == 1:
        return lit
    best = max(parts, key=len)
    return best if len(best) >= 4 else lit


def _mk(sub, k, site=None, skip=False):
    """Rule of sub-kind sub, numbered k (unique per ruleset)."""
    tag = ("s" + site[0] if site else "g") + sub + "%03d" % k + ("k" if skip else "")
    R = dict(name=tag, sub=sub, site=site, skip=skip, interval=(3, 5, 20, 60)[k % 4], hits=k % 4, decision=DECISIONS[k % 3])
    letter = "h" if skip else {"bl": "b", "bn": "b", "bm": "b", "g1": "g", "g2": "g", "i1": "i", "i2": "i"}.get(sub, sub)
    n = b"%03d" % k
    if sub == "a":
        return Rule(regex="tok%03dx" % k, letter=letter, equiv=True, lits=[(b"tok" + n + b"x", False)], hit=[b"tok" + n + b"x"],
                    miss=[b"tok" + n + b"y"], **R)
    if sub == "bl":
        return Rule(regex=r"\/p%03d\/[a-z]+" % k, letter=letter, lits=[(b"/p" + n + b"/", False)], hit=[b"/p" + n + b"/ab"],
                    miss=[b"/p" + n + b"/9", b"/p" + n + b"."], **R)
    if sub == "bn":
        return Rule(regex=r".*Fox%03d\/\d+" % k, letter=letter, lits=[(b"Fox" + n + b"/", False)], hit=[b"Fox" + n + b"/5"],
                    miss=[b"Fox" + n + b"/x", b"Fox" + n + b"-5"], **R)
    if sub == "bm":
        return Rule(regex=r"Mac%03d.*Fox%03d\/\d+" % (k, k), letter=letter, lits=[(b"Mac" + n, False)],
                    hit=[b"Mac" + n + b"_Fox" + n + b"/42"], miss=[b"Mac" + n, b"Fox" + n + b"/4", b"Mac" + n + b"-Fox" + n + b"/x"], **R)
    if sub == "c":
        return Rule(regex="(?i)scr%03dpy|mec%03dize" % (k, k), letter=letter, lits=[(b"cr" + n + b"py", True), (b"mec" + n + b"ize", True)],
                    hit=[b"SCR" + n + b"PY", b"mec" + n + b"IZE", b"Scr" + n + b"py"], miss=[b"scr" + n + b"pz", b"nec" + n + b"ize"], **R)
    if sub == "d":
        return Rule(regex=".*", letter=letter, mode=MODE_ALWAYS, **R)
    if sub == "e":
        return Rule(regex=r"^GET \S+ GET \/q%d\/" % k, letter=letter, mode=MODE_ANCHORED, lits=[(b"GET ", False)], key=k, **R)
    if sub == "f":
        return Rule(regex="^%s " % F_METHODS[k % 4], letter=letter, mode=MODE_ANCHORED, equiv=True,
                    lits=[(F_METHODS[k % 4].encode() + b" ", False)], key=k % 4, **R)
    if sub == "g1":
        return Rule(regex=r"^[A-Z]+ \S+ [A-Z]+ \/%d\d" % (k % 10), letter=letter, mode=MODE_ANCHORED, key=k % 10, **R)
    if sub == "g2":
        return Rule(regex=r"\d{3}%s" % G2_LETTERS[k % 4], letter=letter, mode=MODE_SCAN, key=k % 4,
                    hit=[b"%03d%s" % (k, G2_LETTERS[k % 4].encode())], miss=[b"%02d%s" % (k % 100, G2_LETTERS[k % 4].encode())], **R)
    if sub == "i1":
        h = site.encode()
        return Rule(regex=r"POST %s POST \/xmlrpc\.php" % site.replace(".", r"\."), letter=letter, equiv=True,
                    lits=[(b"POST " + h + b" POST /xmlrpc.php", False)], **R)
    if sub == "i2":
        h = site.encode()
        return Rule(regex=r"GET %s GET \/wp-login\.php HTTP\/[0-2.]+ .*" % site.replace(".", r"\."), letter=letter,
                    lits=[(b"GET " + h + b" GET /wp-login.php HTTP/", False)], **R)
    raise ValueError(sub)


J_TAILS = {"g": (("[a-c]", b"a"), ("[d-f]", b"d"), ("[g-i]", b"g"), ("[j-l]", b"j"), ("[m-o]", b"m")),
           "b": ((r"\d", b"5"), (r"[p-r]\d", b"p5"), (r"[s-u]\d", b"s5"), (r"[v-x]\d", b"v5"), (r"[y-z]\d", b"y5")),
           "m": (("[x-z]{2}", b"xy"), ("[A-C]", b"A"), ("[D-F]", b"D"))}


def _shared(k, where, t=0):
    """The rule of shared literal k (kind j) in the global rules, on big or on mid: one literal,
    another tail in each (t: further rules of the same literal in one list)."""
    lit = b"shr%02d_" % k
    tail, hit = J_TAILS[where][t]
    return Rule(name="%sj%02d%s" % (where, k, "t%d" % t if t else ""), regex="shr%02d_%s" % (k, tail), letter="j", sub="j",
                lits=[(lit, False)], site={"g": None, "b": BIG, "m": MID}[where], hit=[lit + hit], miss=[lit + b"-", b"shr%02d-" % k],
                interval=(3, 5, 20)[(k + t) % 3], hits=(k + t) % 3, decision=DECISIONS[k % 3])


def _filler(k, site=None):
    lit = filler_literal(k) if site is None else b"zs%03dzs" % k
    return Rule(name=("fs%s%d" % (site[0], k)) if site else "fill%d" % k, regex=lit.decode(), letter="-", sub="fill", site=site, equiv=True,
                lits=[(lit, False)], hit=[lit], miss=[lit[:-1] + b"r"], interval=5, hits=1 + k % 3)


BLOCK = (("a", False), ("bl", False), ("bn", False), ("bm", False), ("c", False), ("d", False), ("e", False), ("f", False),
         ("g1", False), ("g2", False), ("a", True), ("bl", True), ("d", True), ("e", True))


class _Num:
    def __init__(self):
        self.k = 10

    def __call__(self):
        self.k += 1
        return self.k


def _block(num, site=None):
    return [_mk(sub, num(), site, skip) for sub, skip in BLOCK]


def _pad(rules, n, site, start):
    """Site fillers up to n rules."""
    return rules + [_filler(start + i, site) for i in range(n - len(rules))]


def _split_pair(site):
    return [_mk("i1", 1, site), _mk("i2", 2, site)]


def _pieces():
    return [Rule(name="gp1", regex=r" POST \/xmlrpc\.php", letter="p", sub="p1", equiv=True, lits=[(b" POST /xmlrpc.php", False)],
                 interval=5, hits=2),
            Rule(name="gp2", regex=r" GET \/wp-login\.php HTTP\/", letter="p", sub="p2", equiv=True,
                 lits=[(b" GET /wp-login.php HTTP/", False)], interval=5, hits=2)]


def _wide(name, regex, lit, site=None, skip=False):
    return Rule(name=name, regex=regex, letter="w", sub="w", site=site, skip=skip, wide=True, mode=MODE_PREFILTER if lit else MODE_SCAN,
                lits=[(lit, False)] if lit else [], interval=5, hits=1, decision="nginx_block")


WIDE_GAP = 1500  # .{750}.{750}
# (head, tail): the pattern is head.{750}.{750}tail
WIDE_PATS = {"lit": (b"tokwide", b"end"), "nolit": (b"a", b"b"), "one": (b"tokshare", b"one"), "two": (b"tokshare", b"two"),
             "site": (b"toksite", b"fin")}

_rules_cache = {}


def rules(kind: str):
    """(global rules, {host: site rules}) of the ruleset, as Rule records."""
    if kind in _rules_cache:
        return _rules_cache[kind]
    num = _Num()
    if kind == "NARROW":
        # k_lines2 keeps a table row per literal and host class in 20 KB of LDS: the counts of MIX's
        # site rules and 60 global rules, but 8 shared literals under several tails in place of
        # one-literal fillers (36 literals in all)
        nj = 8
        plain = lambda site: [_mk(sub, num(), site) for sub in ("d", "e", "g1", "g2")]
        glob = plain(None) + _block(num) + _pieces() + [_shared(k, "g", t) for t in range(5) for k in range(nj)]
        big = _block(num, BIG) + _split_pair(BIG) + [_shared(k, "b", t) for t in range(5) for k in range(nj)] + plain(BIG)
        mid = _split_pair(MID) + [_mk("a", num(), MID), _mk("d", num(), MID)] + [_shared(k, "m", t) for t in range(2) for k in range(nj)]
        assert (len(glob), len(big), len(mid)) == (60, 60, 20)
        sites = {BIG: big, MID: mid, TINY: _split_pair(TINY)}
    elif kind in ("MIX", "ALL"):
        n_glob = {"MIX": 100, "ALL": 140}[kind]
        # big: the block, the split pair, the 30 shared literals, fillers: 60 rules, positions 0-59
        big = _pad([_filler(0, BIG), _filler(1, BIG)] + _block(num, BIG) + _split_pair(BIG) + [_shared(k, "b") for k in range(30)], 60, BIG, 2)
        mid = _pad(_split_pair(MID) + [_shared(k, "m") for k in range(0, 30, 2)] + [_mk("a", num(), MID), _mk("d", num(), MID)], 20, MID, 0)
        tiny = _split_pair(TINY)
        # global: an early block (narrow hosts see it in mask words 0 and 1), then, from where
        # big sees position 128, the block, the pieces and the shared literals
        n_late_j = 16 if kind == "MIX" else 30  # MIX: 32 positions are left past big's 128th
        late = _block(num) + _pieces() + [_shared(k, "g") for k in range(n_late_j)]
        early = [_filler(k) for k in range(4)] + _block(num) + [_shared(k, "g") for k in range(n_late_j, 30)]
        first_late = 128 - 60
        glob = early + [_filler(4 + k) for k in range(first_late - len(early))] + late
        glob += [_filler(200 + k) for k in range(n_glob - len(glob))]
        assert len(glob) == n_glob, (kind, len(glob))
        sites = {BIG: big, MID: mid, TINY: tiny}
    elif kind == "SITE":
        j = [_shared(k, "b") for k in range(30)]
        big = [_filler(0, BIG), _filler(1, BIG)] + _block(num, BIG) + _split_pair(BIG) + j[:10]            # 0-27
        big = _pad(big, 66, BIG, 2) + _block(num, BIG) + j[10:20]                                            # 66-89
        # a second split pair past position 128 (another path, big only)
        x1, x2 = _mk("i1", 3, BIG), _mk("i2", 4, BIG)
        x1.regex, x1.lits = x1.regex.replace("xmlrpc", "xmlrpcB"), [(x1.lits[0][0].replace(b"xmlrpc", b"xmlrpcB"), False)]
        x2.regex, x2.lits = x2.regex.replace("wp-login", "wp-loginB"), [(x2.lits[0][0].replace(b"wp-login", b"wp-loginB"), False)]
        big = _pad(big, 130, BIG, 50) + _block(num, BIG) + [x1, x2] + j[20:24]                               # 130-149
        assert len(big) == 150
        mid = _split_pair(MID) + [_shared(k, "m") for k in (0, 12, 23)]
        glob = _block(num) + _pieces() + [_shared(k, "g") for k in (0, 12, 23, 5)]
        assert len(glob) == 20
        sites = {BIG: big, MID: mid}
    elif kind == "NOLIT":
        glob = []
        for k in range(130):
            a, b = "defghjklmn"[k % 10], "opqrstuvwxyz"[k // 10 % 12]
            if k % 2:
                glob.append(Rule(name="n%d" % k, regex=r"\d{2}%s%s" % (a, b), letter="g", sub="n", mode=MODE_SCAN,
                                 hit=[b"47" + (a + b).encode()], miss=[b"4" + (a + b).encode()], interval=5, hits=k % 3,
                                 skip=k % 20 == 1))
            else:
                glob.append(Rule(name="n%d" % k, regex=r"[a-c]{2}\d%s" % b, letter="g", sub="n", mode=MODE_SCAN,
                                 hit=[b"ca7" + b.encode()], miss=[b"cd7" + b.encode()], interval=5, hits=k % 3))
        sites = {BIG: [_mk("g2", 0, BIG), _mk("g1", 7, BIG), _mk("f", 0, BIG)]}
    elif kind == "WNFA":
        def pat(nm):
            h, t = WIDE_PATS[nm]
            return "%s.{750}.{750}%s" % (h.decode(), t.decode())
        glob = [_filler(k) for k in range(130)]
        # one pattern, three rules: the first without hosts_to_skip, a later one with it, a site rule of big;
        # then the same with the order of the two global rules reversed
        glob += [_wide("w_lit", pat("lit"), b"tokwide"), _wide("w_nolit", pat("nolit"), None),
                 _wide("w_one_plain", pat("one"), b"tokshare"), _wide("w_two_skip", pat("two"), b"tokshare", skip=True),
                 _filler(130), _wide("w_one_skip", pat("one"), b"tokshare", skip=True), _wide("w_two_plain", pat("two"), b"tokshare")]
        sites = {BIG: [_wide("w_one_big", pat("one"), b"tokshare", BIG), _mk("a", 900, BIG), _wide("w_two_big", pat("two"), b"tokshare", BIG),
                       _wide("w_site_skip", pat("site"), b"toksite", BIG, skip=True)]}
    else:
        raise ValueError(kind)
    _rules_cache[kind] = (glob, sites)
    return _rules_cache[kind]


def rules_yaml(kind: str) -> str:
    glob, sites = rules(kind)

    def one(r, ind):
        skip = "\n%s  hosts_to_skip:\n%s    %s: true" % (ind, ind, BIG) if r.skip else ""
        return ("%s- rule: '%s'\n%s  regex: '%s'\n%s  interval: %d\n%s  hits_per_interval: %d\n%s  decision: %s%s\n"
                % (ind, r.name, ind, r.regex.replace("'", "''"), ind, r.interval, ind, r.hits, ind, r.decision, skip))
    y = "regexes_with_rates:\n" + "".join(one(r, "  ") for r in glob) + "per_site_regexes_with_rates:\n"
    for h, rs in sites.items():
        y += "  %s:\n" % h + "".join(one(r, "    ") for r in rs)
    if kind != "NOLIT":
        y += "global_decision_lists:\n  allow:\n    - %s\n" % ALLOWED_IP
    return y + "expiring_decision_ttl_seconds: 10\n"


def all_rules(kind: str):
    """Ruleset index order (Config.all_rules): the global rules, then each site's."""
    glob, sites = rules(kind)
    return glob + [r for h in sites for r in sites[h]]


def scope(kind: str, host: str):
    glob, sites = rules(kind)
    return sites.get(host, []) + glob


def wide_hosts(kind: str):
    return [h for h in HOSTS if len(scope(kind, h)) > 128]


def scan_literals(kind: str):
    """The literals the scan pass looks for: every prefilter literal, a host-split one as its piece."""
    out = set()
    for r in all_rules(kind):
        if r.mode == MODE_PREFILTER:
            for s, ci in r.lits:
                out.add((piece_of(s, r.site) if r.site else s, ci))
    return sorted(out)


# ---------------------------------------------------------------- batches

@dataclass
class Line:
    cls: str
    host: str
    index: int
    text: bytes
    spaces4: bool = True
    exotic: bool = False
    targets: set = field(default_factory=set)   # names of the rules a token of the line aims at (hit or miss)
    expect: dict = field(default_factory=dict)  # far lines: rule name -> the oracle's verdict


@dataclass
class Batch:
    kind: str
    data: bytes
    now_ns: int
    lines: list
    n_lines: int

    def fallback_lines(self):
        """Lines k_lines hands to the per-line fallback: four spaces and a host whose scope
        is past 128 positions, or an exotic timestamp (on any host)."""
        wide = set(wide_hosts(self.kind))
        return sum(1 for ln in self.lines if ln.spaces4 and (ln.host in wide or ln.exotic))


CLASSES = ("zero", "hits", "hits", "twice", "ovf_site", "ovf_glob", "shared", "near", "split", "exotic", "hits", "old", "ovf_site",
           "short", "allow", "split", "shared", "twice", "ovf_glob", "hits", "near", "split", "zero")


class _Gen:
    def __init__(self, kind, seed):
        self.kind, self.seed = kind, seed
        self.r = random.Random(1000 * seed + KINDS.index(kind))
        self.alpha = bytes(c for c in FILL if c not in b"ab ") if kind == "WNFA" else FILL.replace(b" ", b"")
        self.clock = T0 + 3 * (seed - 1)
        self.lines = []
        self.glob, self.sites = rules(kind)
        self.everything = all_rules(kind)
        self.tok_rules = [r for r in self.everything if r.hit and r.mode == MODE_PREFILTER]
        self.e_rules = [r for r in self.everything if r.sub == "e"]
        self.g1_rules = [r for r in self.everything if r.sub == "g1"]
        self.g2_rules = [r for r in self.everything if r.sub in ("g2", "n")]

    def fill(self, n):
        return bytes(self.r.choices(self.alpha, k=n))

    def ts(self, old=False):
        d = self.r.randrange(11000, 20000) if old else self.r.randrange(0, 8500)
        ms = self.clock * 1000 - d
        return b"%d.%03d" % (ms // 1000, ms % 1000)

    def exotic_ts(self):
        """Go's ParseFloat takes it, the kernels' fast parsers decline it (as in tests/test_gpu_nfa.py)."""
        return b"17.0000000%d%03de8" % (self.clock - T0, self.r.randrange(1000))

    def emit(self, cls, host, m1, m2, uri, targets=(), ts=None, ip=None, exotic=False, expect=None, raw=None):
        ip = ip or self.r.choice(IPS[:59] + IPS[60:]).encode()
        text = raw if raw is not None else b"%s %s %s %s %s /%s" % (ts or self.ts(), ip, m1, host.encode(), m2, uri)
        assert b"\n" not in text
        self.lines.append(Line(cls, host, len(self.lines), text, text.count(b" ") >= 4, exotic, set(targets), expect or {}))

    # ---- the parts every ordinary line has: methods, the URI's first bytes, a no-literal token
    def dress(self, host):
        r = self.r
        tg = set()
        m = b"GET"
        head = b""
        x = r.random()
        if x < 0.18 and self.e_rules:
            e = r.choice(self.e_rules)
            tg.add(e.name)
            head = b"q%d/" % e.key if r.random() < 0.7 else b"q%d." % e.key
            if r.random() < 0.2:
                m = b"POST"
        elif x < 0.30 and self.g1_rules:
            g = r.choice(self.g1_rules)
            tg.add(g.name)
            head = b"%d%d" % (g.key, r.randrange(10)) if r.random() < 0.7 else b"%dx" % g.key
        if m == b"GET" and r.random() < 0.3:
            m = r.choice(F_METHODS + ("DELETE",)).encode()
        if m != b"GET":
            tg |= {f.name for f in self.everything if f.sub == "f"}
        tail = b""
        if r.random() < 0.2 and self.g2_rules:
            g = r.choice(self.g2_rules)
            tg.add(g.name)
            tail = self.fill(3) + (g.hit[0] if r.random() < 0.6 else g.miss[0])
        return m, head, tail, tg

    def join(self, toks):
        out = b""
        for t in toks:
            out += self.fill(self.r.randrange(2, 24)) + t
        return out + self.fill(self.r.randrange(0, 12))

    def pick(self, host, n, site_bias=0.5, only_global=False, distinct=True):
        """n literal rules: of the host's site rules, of the global rules, now and then of another host's."""
        r = self.r
        site = [x for x in self.sites.get(host, []) if x.hit and x.mode == MODE_PREFILTER]
        glob = [x for x in self.glob if x.hit and x.mode == MODE_PREFILTER]
        out = []
        while len(out) < n:
            u = r.random()
            if only_global or not site:
                pool = glob if (only_global or u < 0.85) else self.tok_rules
            else:
                pool = site if u < site_bias else (glob if u < 0.92 else self.tok_rules)
            if r.random() < 0.7:  # mostly the rule kinds under test, not the fillers and the shared literals
                pool = [y for y in pool if y.letter in "abch"] or pool
            x = r.choice(pool)
            if distinct and any(x.lits[0] == y.lits[0] for y in out):
                continue
            out.append(x)
        return out

    def token(self, rule, p_hit=0.7):
        return self.r.choice(rule.hit) if self.r.random() < p_hit else self.r.choice(rule.miss)

    def ordinary(self, cls, host):
        r = self.r
        m, head, tail, tg = self.dress(host)
        toks = []
        if cls in ("hits", "exotic", "old", "allow"):
            for x in self.pick(host, r.randrange(1, 5)):
                toks.append(self.token(x))
                tg.add(x.name)
        elif cls == "twice":
            x = self.pick(host, 1)[0]
            order = r.choice([(0, 1), (1, 0), (1, 1), (0, 0)])  # miss then hit: the second occurrence decides
            toks = [r.choice(x.hit) if o else r.choice(x.miss) for o in order]
            tg.add(x.name)
            if r.random() < 0.5:
                y = self.pick(host, 1)[0]
                toks.insert(r.randrange(3), self.token(y))
                tg.add(y.name)
        elif cls in ("ovf_site", "ovf_glob"):
            n = r.randrange(5, 10)
            xs = self.pick(host, n, site_bias=0.4, only_global=cls == "ovf_glob", distinct=False)
            own = [x for x in self.sites.get(host, []) if x.hit and x.mode == MODE_PREFILTER]
            if cls == "ovf_site" and own and not any(x.site == host for x in xs):
                xs[r.randrange(n)] = r.choice(own)
            for x in xs:
                toks.append(self.token(x, 0.75))
                tg.add(x.name)
        elif cls == "shared":
            js = [x for x in self.everything if x.letter == "j"]
            if js:
                for _ in range(r.randrange(1, 4)):
                    x = r.choice(js)
                    same = [y for y in js if y.lits == x.lits]
                    toks.append(self.token(r.choice(same), 0.8))
                    tg |= {y.name for y in same}
        elif cls == "near":
            for x in self.pick(host, r.randrange(1, 4)):
                toks.append(x.miss[-1])
                tg.add(x.name)
        uri = head + self.join(toks) + tail
        kw = {}
        if cls == "exotic":
            # the general ParseFloat: the line kernels hand the line to the per-line fallback
            kw = dict(ts=self.exotic_ts(), exotic=True)
        if cls == "old":
            kw = dict(ts=self.ts(old=True))
        if cls == "allow":
            kw = dict(ip=ALLOWED_IP.encode())
        self.emit(cls, host, m, m, uri, tg, **kw)

    def short(self, host):
        v = self.r.randrange(3)
        raw = [b"%s %s GET %s" % (self.ts(), self.r.choice(IPS).encode(), host.encode()), b"x", b"%s tok017x" % self.ts()][v]
        self.emit("short", host, b"", b"", b"", raw=raw)

    def split(self, host, v):
        """The split rules' lines (kind i).  v: bit 0 which rule, bit 1 deep (after a long path) or within
        the first 100 bytes, bits 2-3 the variant: the true line, the wrong method, another host's name,
        the piece twice with only the second surrounded by the full literal."""
        r = self.r
        which, deep, var = v & 1, (v >> 1) & 1, (v >> 2) & 3
        sfx = b"B" if (self.kind == "SITE" and host == BIG and (v >> 4) & 1) else b""
        if which == 0:
            ok_m, bad_m, path = b"POST", b"GET", b"/xmlrpc" + sfx + b".php"
        else:
            ok_m, bad_m, path = b"GET", b"POST", b"/wp-login" + sfx + b".php HTTP/1.1 UA" + self.fill(6)
        h = host.encode()
        h2 = r.choice([x for x in (BIG, MID, TINY) if x != host]).encode()
        tg = {x.name for x in self.everything if x.letter in "ip"}
        if not deep:
            if var == 0:
                self.emit("split", host, ok_m, ok_m, path[1:], tg)
            elif var == 1:
                self.emit("split", host, bad_m, ok_m, path[1:], tg)
            elif var == 2:
                self.emit("split", host, ok_m, ok_m, self.fill(5) + b" " + ok_m + b" " + h2 + b" " + ok_m + b" " + path, tg)
            else:
                self.emit("split", host, bad_m, ok_m, path[1:] + self.fill(8) + b" " + ok_m + b" " + h + b" " + ok_m + b" " + path, tg)
            return
        pad = self.fill(r.randrange(300, 3000))
        emb = {0: ok_m + b" " + h + b" " + ok_m + b" " + path,
               1: bad_m + b" " + h + b" " + ok_m + b" " + path,
               2: ok_m + b" " + h2 + b" " + ok_m + b" " + path,
               3: bad_m + b" " + h + b" " + ok_m + b" " + path + self.fill(9) + b" " + ok_m + b" " + h + b" " + ok_m + b" " + path}[var]
        self.emit("split", host, b"GET", b"GET", pad + b" " + emb, tg)

    def far(self, k):
        """Far lines: the line's only literal hit lies FAR_OFFSETS[k % 4] bytes into rest (65,535 and up: the
        offset no longer fits the 16 bits the kernels keep, so the split rule goes to its automaton)."""
        off = FAR_OFFSETS[k % 4]
        var = k // 4  # 0 split, true; 1 split, wrong method; 2 plain literal
        oi = k % 4
        big_sites = self.sites.get(BIG, [])
        i1 = [x for x in big_sites if x.sub == "i1"][:1]
        plain_site = [x for x in big_sites if x.sub == "a" and not x.skip][:1]
        plain_glob = [x for x in self.glob if x.sub == "a" and not x.skip][-1:]
        if var < 2:
            host = BIG if (var == 0 or self.seed == 1) else OTHER  # the wrong method: on big in one batch, on other in the next
            h = host.encode()
            head = b"POST " + h + b" POST /"
            emb = (b"POST " if var == 0 else b"GET ") + BIG.encode() + b" POST /xmlrpc.php"
            at = len(emb) - len(b" POST /xmlrpc.php")           # the piece's offset in emb
            rest = head + self.fill(off - at - len(head) - 1) + b" " + emb
            assert rest.index(b" POST /xmlrpc.php") == off
            expect = {"gp1": True}
            if i1 and host == BIG:
                expect[i1[0].name] = var == 0
        else:
            # per offset: a true token and a near miss, one on big and one on other, over the two batches
            host = BIG if (oi < 2) == (self.seed == 1) else OTHER
            rule = (plain_glob if (host == OTHER or not plain_site) else plain_site)[0]
            good = (oi % 2 == 0) == (self.seed == 1)
            tok = rule.hit[0] if good else rule.miss[0]
            head = b"GET " + host.encode() + b" GET /"
            rest = head + self.fill(off - len(head)) + tok
            assert len(rest) - len(tok) == off
            expect = {rule.name: good}
        self.emit("far", host, b"", b"", b"", set(expect), raw=self.ts() + b" " + self.r.choice(IPS[:50]).encode() + b" " + rest,
                  expect=expect)

    def wnfa(self, j, host):
        """WNFA: 1.6 KB lines that match a wide rule, or miss it by one byte; short lines between."""
        r = self.r
        if j % 3 == 2:
            self.emit("zero", host, b"GET", b"GET", self.join([self.token(x) for x in self.pick(host, r.randrange(0, 3))]))
            return
        nm = ("lit", "nolit", "one", "two", "site", "one", "two")[j // 3 % 7]
        head, tail = WIDE_PATS[nm]
        gap = WIDE_GAP + (0 if r.random() < 0.6 else r.choice([-1, 1]))
        body = self.fill(r.randrange(3, 40)) + head + self.fill(gap) + tail + self.fill(r.randrange(0, 30))
        tg = {x.name for x in self.everything if x.wide}
        self.emit("wide_hit" if gap == WIDE_GAP else "wide_miss", host, b"GET", b"GET", body, tg)


_cache = {}


def batch(kind: str, seed: int) -> Batch:
    """The batch of this kind and seed (built once; read-only).  Its clock is 3 s later per seed."""
    if (kind, seed) in _cache:
        return _cache[(kind, seed)]
    g = _Gen(kind, seed)
    hosts = HOSTS[seed % 4:] + HOSTS[:seed % 4]  # another host at every line index than in the other seed's batch
    n = N_LINES[kind]
    n_split = n_far = 0
    far_at = {n // 13 * (k + 1) for k in range(12)} if kind != "WNFA" else set()
    for j in range(n):
        host = hosts[(j + j // 92) % 4] if kind != "WNFA" else (BIG, OTHER, BIG, MID)[(j + seed) % 4]
        if kind == "WNFA":
            g.wnfa(j, host)
            continue
        if j in far_at and kind != "NOLIT":
            g.far(n_far)
            n_far += 1
            continue
        cls = CLASSES[j % len(CLASSES)]
        if cls == "split":
            if kind == "NOLIT":
                cls = "hits"
            else:
                g.split(host, n_split // 4)  # every variant on each of the four hosts in turn
                n_split += 1
                continue
        if cls == "short":
            g.short(host)
        elif kind == "NOLIT":
            m, head, tail, tg = g.dress(host)
            toks = []
            for _ in range(g.r.randrange(0, 4)):
                x = g.r.choice(g.g2_rules)
                toks.append(g.token(x))
                tg.add(x.name)
            kw = dict(ts=g.ts(old=True)) if cls == "old" else {}
            if cls == "exotic":
                kw = dict(ts=g.exotic_ts(), exotic=True)
            g.emit(cls, host, m, m, head + g.join(toks) + tail, tg, **kw)
        else:
            g.ordinary(cls, host)
    data = b"".join(ln.text + b"\n" for ln in g.lines)
    _cache[(kind, seed)] = Batch(kind, data, g.clock * 1_000_000_000, g.lines, len(g.lines))
    return _cache[(kind, seed)]
