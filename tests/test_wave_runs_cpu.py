"""The wave-per-run path of `k_bucket_apply` (`bucket_wave_run` in engine.hip):
a run of one (ip, rule name) state taken in chunks of 64 events, each chunk in
closed form (`bjx::window_past`, `bjx::window_hits`) from the state the chunk
before it left, against the event-by-event walk of Apply (reference
internal/rate_limit.go:37-78), on the host build of the same helpers
(tests/cpu/wave_runs.cpp).  Outcomes and the final state must be identical."""
import ctypes
import os
import random
import subprocess
import tempfile

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu", "wave_runs.cpp")
T0 = 1_700_000_000_000_000_000
MS = 1_000_000
LIMITS = (-1, 0, 1, 5, 800)


@pytest.fixture(scope="module")
def lib():
    d = tempfile.mkdtemp(prefix="bjx_wr_")
    so = os.path.join(d, "libwr.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC], check=True)
    L = ctypes.CDLL(so)
    p64, p8 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint8)
    L.bjx_test_wave_run.restype = ctypes.c_uint32
    L.bjx_test_wave_run.argtypes = [ctypes.c_uint32, p64, p64, p64, p64, p64, p8, p8]
    return L


def run(lib, ts, iv, lim, state):
    """state = (valid, hits, start); returns the number of closed-form chunks
    after asserting that both walks agree."""
    n = len(ts)
    A = ctypes.c_int64 * n
    s0, s1 = (ctypes.c_int64 * 3)(*state), (ctypes.c_int64 * 3)(*state)
    o0, o1 = (ctypes.c_uint8 * n)(), (ctypes.c_uint8 * n)()
    closed = lib.bjx_test_wave_run(n, A(*ts), A(*iv), A(*lim), s0, s1, o0, o1)
    a, b = list(o0), list(o1)
    if a != b:
        k = next(i for i in range(n) if a[i] != b[i])
        raise AssertionError("event %d of %d: walk %d, chunked %d (state %s, limit %s, interval %s)"
                             % (k, n, a[k], b[k], state, lim[k], iv[k]))
    assert list(s0) == list(s1), (list(s0), list(s1), state)
    return closed


def uniform(lib, ts, interval, limit, state):
    n = len(ts)
    closed = run(lib, ts, [interval] * n, [limit] * n, state)
    assert closed == (n + 63) // 64  # every chunk took the closed form
    return closed


def states(interval, limit, first_ts):
    """Stored states: none, a window the head continues (with room, at the
    limit, and with more hits than the limit, as after a reload), one that
    ends exactly at the head, and ones the head does not continue."""
    yield (0, 0, 0)
    for hits in (0, 1, max(limit, 0), max(limit, 0) + 3, 900):
        yield (1, hits, first_ts - interval // 2)
        yield (1, hits, first_ts - interval)        # exactly at start + interval: still inside
        yield (1, hits, first_ts - interval - 1)    # 1 ns past it: a new window
        yield (1, hits, first_ts - 10 * interval)


@pytest.mark.parametrize("limit", LIMITS)
def test_every_length(lib, limit):
    """Lengths 1 to 300 at 1 ms spacing with a 0.1 s interval: a window every
    101 events, so chunks with one boundary, with none, and a last chunk of
    every size."""
    interval = 100 * MS
    for n in range(1, 301):
        ts = [T0 + k * MS for k in range(n)]
        for st in states(interval, limit, ts[0]):
            uniform(lib, ts, interval, limit, st)


@pytest.mark.parametrize("limit", LIMITS)
def test_windows_inside_a_chunk_and_on_its_edges(lib, limit):
    """A 5 ms interval at 1 ms spacing opens a window every 6 events (ten in a
    chunk); shifting the run's first timestamp against the stored window
    moves the boundaries over every lane, the last lane of a chunk and the
    first lane of the next included.  Events exactly at start + interval
    stay inside, events 1 ns later do not."""
    interval = 5 * MS
    for n in (63, 64, 65, 127, 128, 129, 200):
        for shift in range(0, 8):
            for eps in (0, 1):
                ts = [T0 + k * MS + eps * (k % 6 == 5) for k in range(n)]
                for hits in (0, 3, 900):
                    uniform(lib, ts, interval, limit, (1, hits, T0 - shift * MS))
                uniform(lib, ts, interval, limit, (0, 0, 0))


def test_window_opens_on_a_chunk_edge(lib):
    """One boundary placed on lane 63 of the first chunk, then on lane 0 of the second."""
    interval = 1000 * MS
    for edge in (63, 64, 127, 128):
        for n in (edge + 1, edge + 2, 200):
            ts = [T0 + k * MS + (2 * interval if k >= edge else 0) for k in range(n)]
            for limit in LIMITS:
                for st in states(interval, limit, ts[0]):
                    uniform(lib, ts, interval, limit, st)


@pytest.mark.parametrize("limit", LIMITS)
def test_decreasing_timestamps(lib, limit):
    """The first event in event order that lies past the window opens the next
    one, whatever the timestamps' order: every 97th (and every 5th) event 5 s
    back, and fully reversed runs."""
    interval = 250 * MS
    for n in (9, 64, 65, 130, 300):
        for every in (97, 5):
            ts = [T0 + k * MS * 7 - (5_000 * MS if k % every == 0 else 0) for k in range(n)]
            for st in states(interval, limit, ts[0]):
                uniform(lib, ts, interval, limit, st)
        ts = [T0 - k * MS * 7 for k in range(n)]
        for st in states(interval, limit, ts[0]):
            uniform(lib, ts, interval, limit, st)


def test_rules_sharing_a_name(lib):
    """Two rules with different limits share the state: a chunk that holds
    both is walked event by event, the run's other chunks take the closed
    form, and the state passes between the two kinds."""
    interval = 50 * MS
    for la, lb in ((37, 5), (5, 37), (0, 1), (-1, 5), (800, 1)):
        for n in (8, 64, 100, 200, 300):
            ts = [T0 + k * MS for k in range(n)]
            for where in (range(0, n, 7), range(70, min(n, 75)), range(0, min(n, 3)), range(max(n - 2, 0), n)):
                lim = [la] * n
                for k in where:
                    lim[k] = lb
                # a chunk takes the closed form when all its events have the head's limit
                want = sum(1 for c in range(0, n, 64) if set(lim[c:c + 64]) == {lim[0]})
                for st in states(interval, la, ts[0]):
                    assert run(lib, ts, [interval] * n, lim, st) == want
    # same limit, different interval
    n = 150
    ts = [T0 + k * MS for k in range(n)]
    iv = [interval if k % 9 else 3 * MS for k in range(n)]
    for st in states(interval, 5, ts[0]):
        assert run(lib, ts, iv, [5] * n, st) == 0


def test_random_runs(lib):
    rng = random.Random(64)
    closed = 0
    for _ in range(6000):
        n = rng.randint(1, 300)
        interval = rng.choice((3, 60, 250, 1000)) * MS
        limit = rng.choice(LIMITS)
        other = rng.choice(LIMITS)
        p_other = rng.choice((0, 0, 0.01, 0.2))
        t, ts = T0, []
        for _k in range(n):
            t += rng.choice((0, 1, 1, 1, 2, 40, interval // MS, interval // MS + 1)) * MS + rng.choice((0, 0, 1))
            ts.append(t - 5_000 * MS if rng.random() < 0.02 else t)
        lim = [other if rng.random() < p_other else limit for _k in range(n)]
        st = rng.choice(list(states(interval, limit, ts[0])))
        closed += run(lib, ts, [interval] * n, lim, st)
    assert closed > 6000


def test_standalone_sanitized():
    """The same file with its own main under AddressSanitizer and UBSan."""
    d = tempfile.mkdtemp(prefix="bjx_wr_san_")
    exe = os.path.join(d, "wave_runs")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-DWAVE_RUNS_MAIN", "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert " 0 mismatches" in r.stdout
