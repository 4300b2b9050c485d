"""The state tables' sizing rule without a GPU: table_cap_for, arena_cap_for and
clamp_cap (banjax_amd/csrc/bjx_common.h), the one rule growth, expiry and
import size their tables by, built for the host from tests/cpu/state_caps.cpp,
a program with its own main."""
import functools
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu", "state_caps.cpp")
U64 = (1 << 64) - 1


def _next_pow2(x):
    p = 1
    while p < x:
        p <<= 1
    return p


def _sizes():
    """0, 1, either side of every power of two up to 2^33, 2^31 - 1, and either
    side of every n at which n*4/3 + 1024 reaches a power of two"""
    ns = {0, 1, (1 << 31) - 1}
    for k in range(1, 34):
        ns.update(((1 << k) - 1, 1 << k, (1 << k) + 1))
    for k in range(11, 36):
        edge = ((1 << k) - 1024) * 3 // 4
        ns.update(n for n in (edge - 1, edge, edge + 1, edge + 2) if 0 <= n <= (1 << 33) + 1)
    return sorted(ns)


# (want, floor, ceiling) -> the floor, the ceiling or the rule's value
CLAMPS = [
    ((1 << 10), (1 << 22), (1 << 24), 1 << 22),   # below the floor
    ((1 << 23), (1 << 22), (1 << 24), 1 << 23),   # between
    ((1 << 26), (1 << 22), (1 << 24), 1 << 24),   # above the ceiling
    ((1 << 22), (1 << 22), (1 << 22), 1 << 22),   # all equal
    ((1 << 10), (1 << 24), (1 << 22), 1 << 22),   # floor > ceiling: the ceiling wins
    ((1 << 26), (1 << 24), (1 << 22), 1 << 22),
    ((1 << 34), (1 << 22), U64, 1 << 34),         # no ceiling (import), past 32 bits
    (0, 0, U64, 0),
    (100 << 20, 64 << 20, 200 << 20, 100 << 20),  # an arena floor that is no power of two
    (4096, 64 << 20, 200 << 20, 64 << 20),
]


@functools.lru_cache(maxsize=None)
def _run():
    d = tempfile.mkdtemp(prefix="bjx_caps_")
    exe = os.path.join(d, "state_caps")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, SRC], check=True)
    args = [str(n) for n in _sizes()] + ["%d:%d:%d" % c[:3] for c in CLAMPS]
    out = subprocess.run([exe] + args, check=True, capture_output=True, text=True).stdout.split("\n")
    rows = [tuple(int(x) for x in line.split()) for line in out if line and not line.startswith("clamp")]
    clamps = [int(line.split()[1]) for line in out if line.startswith("clamp")]
    assert [r[0] for r in rows] == _sizes() and len(clamps) == len(CLAMPS)
    return rows, clamps


def test_table_rule_is_a_power_of_two_under_three_quarters_load():
    for n, cap, _ in _run()[0]:
        assert cap & (cap - 1) == 0 and cap >= 1024, (n, cap)
        assert n * 4 <= cap * 3, (n, cap)              # the n it was sized for fits under 3/4
        assert cap >= n * 4 // 3 + 1024 > cap // 2, (n, cap)  # with the spare, and no larger than needed
        assert cap == _next_pow2(n * 4 // 3 + 1024), (n, cap)


def test_arena_rule():
    for b, _, cap in _run()[0]:
        assert cap & (cap - 1) == 0, (b, cap)
        assert cap >= 2 * b + 4096 > cap // 2, (b, cap)
        assert cap == _next_pow2(2 * b + 4096), (b, cap)


def test_sizes_reach_past_32_bits():
    rows = {n: (t, a) for n, t, a in _run()[0]}
    assert rows[(1 << 31) - 1] == (1 << 32, 1 << 33)  # n * 4 does not fit 32 bits
    assert rows[1 << 33] == (1 << 34, 1 << 35)
    assert rows[0] == (1024, 4096)


def test_clamp():
    for (want, floor, ceiling, expect), got in zip(CLAMPS, _run()[1]):
        assert got == expect, (want, floor, ceiling, got)
