"""k_scan's pair filter and tile framing at every position class of the probe.

Small batches (one to three 4 KB wave tiles) with literals placed at chosen
byte offsets, so that each path of the probe sees a true occurrence: both
parities and all four word alignments at a tile start, the last positions of
a lane's 64-byte slice (the next lane's first word, and across the tile end
the halo's), the halo part of the tile's last line, the batch end (edge
tiles), an interior tile, and a line longer than the window (flush_long).

Every batch is checked bit-exactly against the oracle (tests/parity.py), and
the scan's recorded literal hits against a count made here: the data holds
the two plain literals only where they are placed, each literal has one gram
window in the table, so every occurrence inside a consumed line is recorded
exactly once.  Each case runs on the default line pass and with BJX_LINES=1.
"""
import pytest

from banjax_amd import Engine
from tests.parity import Pair

pytestmark = pytest.mark.gpu
S = 1_000_000_000
T0 = 1700000000
WT, HALO = 4096, 512  # engine.hip kWT, kHalo

CFG = r"""
regexes_with_rates:
  - rule: "env"
    regex: '\/\.env'
    interval: 5
    hits_per_interval: 2
    decision: nginx_block
  - rule: "wp"
    regex: 'wp-login'
    interval: 5
    hits_per_interval: 3
    decision: challenge
  - rule: "bots"
    regex: '(?i)(ahrefs|semrush|mj12)bot'
    interval: 5
    hits_per_interval: 1
    decision: challenge
"""
ENV, WP = b"/.env", b"wp-login"
IPS = ["10.0.0.%d" % i for i in range(4)]


@pytest.fixture(scope="module")
def engine():
    e = Engine()
    yield e
    e.close()


@pytest.fixture(params=[False, True], ids=["default", "lines"])
def pair(request, engine, monkeypatch):
    if request.param:
        monkeypatch.setenv("BJX_LINES", "1")
    return Pair(CFG, engine)


def batch(n, ends, lits):
    """n bytes of log lines: a '\\n' at every offset of `ends` (the rest after
    the last one is an unterminated line), each line a valid header then 'a'
    filler, and literal `lit` at offset `off` for (off, lit) in `lits`."""
    buf = bytearray(b"a" * n)
    start, k = 0, 0
    for e in list(ends) + [n]:
        head = b"%d %s GET h.com GET /" % (T0, IPS[k % len(IPS)].encode())
        k += 1
        if e - start >= len(head):
            buf[start:start + len(head)] = head
        else:
            assert e == n  # only the unterminated rest may be shorter than a header
        if e < n:
            buf[e] = 0x0A
        start = e + 1
    clean = bytes(buf)
    for off, lit in lits:
        assert 0 <= off and off + len(lit) <= n
        assert clean[off:off + len(lit)] == b"a" * len(lit), (off, lit)  # filler only: no header, no '\n'
        buf[off:off + len(lit)] = lit
    data = bytes(buf)
    assert len(data) == n and data.count(ENV) + data.count(WP) == len(lits)
    return data


def check(pair, data):
    out = pair.feed(data, T0 * S)
    consumed = data.rfind(b"\n") + 1
    assert out.consumed_bytes == consumed
    want = data[:consumed].count(ENV) + data[:consumed].count(WP)
    assert pair.engine.scan_stats()["literal_hits"] == want
    return out


def two_tiles(lits, n=2 * WT + 700):
    # the line across the first tile's end starts at 3801 and ends past the halo
    return batch(n, [900, 2000, 3800, WT + HALO + 88, n - 1], lits)


def test_tile_start_offsets(pair):
    """A literal starting at each of offsets 0..7 of the second tile."""
    for i in range(8):
        check(pair, two_tiles([(WT + i, (ENV, WP)[i & 1]), (1000, WP)]))
    pair.compare_state(IPS)


def test_lane_slice_end(pair):
    """A literal starting at bytes 57..63 of a lane's 64-byte slice: its last
    pairs take the next lane's first word, in the tile and (lane 63, the
    literal straddling the tile end) in the halo."""
    for j in range(57, 64):
        lit = (WP, ENV)[j & 1]
        check(pair, two_tiles([(64 * 10 + j, lit), (64 * 63 + j, lit), (WT + 64 * 5 + j, ENV)]))
    pair.compare_state(IPS)


def test_halo_of_last_line(pair):
    """Literals wholly inside the halo, on a line that started in the tile
    and ends in the halo: the halo pairs, with the end of the line cutting them."""
    for end in (WT + 300, WT + 301, WT + 306, WT + HALO - 1):
        data = batch(2 * WT + 700, [900, 3800, end, 2 * WT + 699],
                     [(WT + 7, ENV), (WT + 130, WP), (end - len(WP), WP), (end + 60, ENV)])
        check(pair, data)
    pair.compare_state(IPS)


def test_batch_end(pair):
    """The last tile: a literal ending at the batch's last byte (in a line with
    no '\\n': not consumed, not counted), one ending just before the final
    '\\n', and bytes past the batch end that must read as nothing."""
    n = WT + 1000
    check(pair, batch(n, [900, WT + 100], [(n - len(WP), WP), (WT + 50, ENV), (WT + 500, ENV)]))
    check(pair, batch(n, [900, WT + 100, n - 1], [(n - 1 - len(ENV), ENV), (WT + 50, ENV)]))
    # the batch ends inside the first tile's halo, and inside a lane's slice
    for n in (WT + 20, WT + 300, WT + HALO + 37):
        check(pair, batch(n, [900, 3800, n - 1], [(n - 1 - len(WP), WP), (3900, ENV), (WT - 3, ENV)]))
    pair.compare_state(IPS)


def test_one_tile(pair):
    """Exactly one tile, and one tile plus one byte (the first tile is the
    last, and the second tile holds a single byte)."""
    check(pair, batch(WT, [900, 2000, WT - 1], [(WT - 1 - len(WP), WP), (64 * 7 + 62, ENV), (1500, WP)]))
    check(pair, batch(WT + 1, [900, 2000, WT], [(WT - len(WP), WP), (WT - 40, ENV), (1500, WP)]))
    check(pair, batch(WT + 1, [900, 2000, WT - 1], [(WT - 1 - len(ENV), ENV), (1500, WP)]))
    pair.compare_state(IPS)


def test_interior_tile(pair):
    """Three tiles: the middle one has its whole window inside the batch and a
    next tile (the interior path).  Literals at its start, across its lanes,
    across its end and in its halo; the last line of the batch unterminated
    and started in the middle tile."""
    n = 3 * WT
    lits = [(WT + 1, ENV), (WT + 64 * 20 + 61, WP), (WT + 64 * 40 + 2, ENV), (2 * WT - 4, WP), (2 * WT + 100, ENV),
            (2 * WT + 400, WP), (300, ENV), (n - 20, WP)]
    check(pair, batch(n, [900, 3800, WT + 600, WT + 3000, 2 * WT + 450, n - 1], lits))
    # no '\n' after the middle tile: the line it starts runs to the batch end unconsumed
    check(pair, batch(n, [900, 3800, WT + 600, WT + 3000], lits))
    pair.compare_state(IPS)


def test_long_line(pair):
    """A line longer than a tile plus its halo, hits inside the first window
    and past it (listed for the end of the round: flush_long)."""
    n = 3 * WT + 100
    lits = [(200, ENV), (WT + 5, WP), (WT + HALO + 300, ENV), (2 * WT + 3, WP), (2 * WT + 64 * 9 + 59, ENV),
            (3 * WT - 2, ENV), (n - 30, WP)]
    check(pair, batch(n, [80, 3 * WT + 30, n - 1], lits))
    # more hits on the long line than it has slots
    lits = [(1000 + 700 * i, (ENV, WP)[i & 1]) for i in range(14)]
    check(pair, batch(n, [80, 3 * WT + 30, n - 1], lits))
    pair.compare_state(IPS)


def test_bot_words_among_literals(pair):
    """The case-insensitive alternation's literals beside the plain ones
    (parity only: its hits are not part of the count above)."""
    data = bytearray(two_tiles([(WT + 40, ENV), (64 * 30 + 60, WP)]))
    for off, word in ((1200, b"AhRefsBot"), (WT - 5, b"semrushBOT"), (WT + 64 * 3 + 58, b"MJ12bot"), (2100, b"mj12bo")):
        data[off:off + len(word)] = word
    pair.feed(bytes(data), T0 * S)
    pair.compare_state(IPS)
