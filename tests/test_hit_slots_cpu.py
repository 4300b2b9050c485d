"""What a DFA job concludes from a line's literal-hit slots and overflow
summary (`slot_lead_start`, `slot_certain`, `lead_bound` in bjx_common.h: the
one copy `l2_job_rec` in lines2.h and `lead_start` / `eq_certain` in engine.hip
call), on the host build of the same functions, exhaustively.

A long line's hits take their four slots in the order several waves reach an
atomic counter, so tests/cpu/hit_slots.cpp enumerates, for every set of hits
over a grid, every choice and order of the hits that get slots, folds the rest
into the summary as CandMeta documents, and checks: the start bound never
passes the first own hit at or past rest (less the bounded lead), and is the
no-match value only when there is none; certainty implies a verified own hit
in rest; without overflow every order gives the same, exact, answer.

The grid: rest starts at 1042 (not a multiple of 8, and the summary keeps
position >> 3), positions 3 before it, 1 and 6 and 20 past it (the first
rounds down to before rest), and 236 and 241 past it (256 bytes into a line
whose header is 20 bytes); literal own, another, and own + 32 (the aliased
summary bit, rulesets of more than 32 literals only); unverified, verified,
verified and far (only where the hit lies 256 bytes into the line).  Sets of up
to 4 hits over the whole grid, sets of 5 to 7 over a reduced one (three
positions; the other literals in one state each), for a header of 20 and of
300 bytes, with and without a bounded lead, with and without aliased bits."""
import ctypes
import os
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
RS = 1042
FULL = [RS - 3, RS + 1, RS + 6, RS + 20, RS + 236, RS + 241]
REDUCED = [RS - 3, RS + 1, RS + 236]


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="bjx_hs_")
    so = os.path.join(d, "libhs.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so,
                    os.path.join(HERE, "cpu", "hit_slots.cpp")], check=True)
    L = ctypes.CDLL(so)
    u32 = ctypes.c_uint32
    L.bjx_test_hit_slots.restype = ctypes.c_uint64
    L.bjx_test_hit_slots.argtypes = [ctypes.POINTER(u32), u32, u32, u32, u32, u32, u32, u32,
                                     ctypes.POINTER(ctypes.c_uint64), ctypes.c_char_p, u32]
    L.bjx_test_hit_slots_eval.restype = u32
    L.bjx_test_hit_slots_eval.argtypes = [ctypes.POINTER(u32), u32, u32, u32, u32, u32, ctypes.POINTER(u32)]
    return L


def run(lib, positions, n_lo, n_hi, rest_off, back, lits_small, reduced):
    pos = (ctypes.c_uint32 * len(positions))(*positions)
    out = (ctypes.c_uint64 * 3)()
    msg = ctypes.create_string_buffer(512)
    bad = lib.bjx_test_hit_slots(pos, len(positions), n_lo, n_hi, rest_off, back, 1 if lits_small else 0,
                                 1 if reduced else 0, out, msg, 512)
    return bad, out[0], out[1], msg.value.decode()


# header bytes, bounded lead + 3 (0: none), at most 32 literals
ENVS = [(20, 7, True), (300, 7, True), (20, 7, False), (20, 0, True), (300, 0, False)]


@pytest.mark.parametrize("rest_off,back,lits_small", ENVS)
def test_up_to_four_hits_full_grid(lib, rest_off, back, lits_small):
    bad, sets, evals, msg = run(lib, FULL, 0, 4, rest_off, back, lits_small, False)
    assert bad == 0, msg
    assert sets > 30_000 and evals > 500_000  # the enumeration ran: 28 or more hit kinds


@pytest.mark.parametrize("rest_off,back,lits_small", ENVS[:4])
def test_five_to_seven_hits_every_slot_choice(lib, rest_off, back, lits_small):
    bad, sets, evals, msg = run(lib, REDUCED, 5, 7, rest_off, back, lits_small, True)
    assert bad == 0, msg
    assert sets > 10_000 and evals > 5_000_000


def _eval(lib, hits, ns, rest_off=20, back=7, lits_small=True):
    q = (ctypes.c_uint32 * (4 * len(hits)))(*[x for h in hits for x in h])
    c = ctypes.c_uint32()
    s = lib.bjx_test_hit_slots_eval(q, len(hits), ns, rest_off, back, 1 if lits_small else 0, ctypes.byref(c))
    return s, bool(c.value)


def test_named_cases(lib):
    """The cases the slot consumers branch on, one by one (own literal id 5, another 9)."""
    own, oth = 5, 9
    far = RS + 240
    others = [(RS + 50 + 10 * k, oth, 1, 0) for k in range(4)]
    # the own hit only in the header: kept in a slot and skipped, or summarised (mf < rs): start 0 then
    assert _eval(lib, [(RS - 3, own, 1, 0)] + others[:3], 4) == (400, False)
    assert _eval(lib, others + [(RS - 3, own, 1, 0)], 4) == (0, False)
    # a verified own hit in rest, less than 256 bytes into the line, past the slots: not certain
    assert _eval(lib, others + [(RS + 100, own, 1, 0)], 4) == (50 - 7, False)
    # ... and far: certain, unless the header is longer than 256 bytes or the bits alias
    assert _eval(lib, others + [(far, own, 1, 1)], 4) == (50 - 7, True)
    assert _eval(lib, others + [(far, own, 1, 1)], 4, rest_off=300)[1] is False
    assert _eval(lib, others + [(far, own + 32, 1, 1)], 4, lits_small=False)[1] is False
    # an unverified own slot hit bounds the start and proves nothing
    assert _eval(lib, [(RS + 30, own, 0, 0)], 1) == (30 - 7, False)
    # a hit just past rs whose position >> 3 rounds to before it
    assert _eval(lib, others + [(RS + 1, own, 1, 0)], 4) == (0, False)
    # no hit of the rule at all
    assert _eval(lib, others[:2], 2) == (400, False)
