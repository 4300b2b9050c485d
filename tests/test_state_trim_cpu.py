"""The budgeted trim without a GPU: the C symbols, their NULL handling and the
struct sizes; the pure-Python model (banjax_amd/state_trim.py) against brute
force, the removal's model and the query's model; that the inputs of the GPU
tests are telling (computed with the oracle and the models alone); and the host
parts of the call -- the select's digit step, the biased key, the saturating
+ 1, the bound's priority, the node's max and sum (banjax_amd/csrc/state_trim.h)
-- built for the host from tests/cpu/trim_host.cpp, a program with its own main."""
import ctypes
import os
import random
import subprocess
import tempfile

from banjax_amd import _lib, snapshot, state_query, state_remove, state_trim
from tests import state_trim as H
from tests.state_trim import INT64_MAX, INT64_MIN

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu", "trim_host.cpp")


def test_symbols_structs_and_null_arguments():
    L = _lib.lib()
    for name in ("bjx_state_trim", "bjx_node_state_trim"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert ctypes.sizeof(_lib.TrimBudget) == 32 and ctypes.sizeof(_lib.TrimStats) == 104
    assert [k for k, _ in _lib.TrimBudget._fields_] == ["max_states", "max_ips", "floor_cutoff_ns", "flags", "_pad"]
    assert [k for k, _ in _lib.TrimStats._fields_] == [
        "cutoff_ns", "bound", "budget_met", "states_before", "states_dropped", "states_dropped_live", "ips_before",
        "ips_dropped", "arena_bytes_before", "arena_bytes_after", "device_bytes_before", "device_bytes_after",
        "select_ms", "device_ms"]
    assert (_lib.TRIM_DRY_RUN, _lib.TRIM_BY_NONE, _lib.TRIM_BY_FLOOR, _lib.TRIM_BY_STATES, _lib.TRIM_BY_IPS) == (1, 0, 1, 2, 3)
    assert (state_trim.DRY_RUN, state_trim.BY_NONE, state_trim.BY_FLOOR, state_trim.BY_STATES, state_trim.BY_IPS) == (1, 0, 1, 2, 3)
    b, out = _lib.TrimBudget(5, 5, INT64_MIN, 0, 0), _lib.TrimStats()
    for fn in (L.bjx_state_trim, L.bjx_node_state_trim):
        # a NULL handle is refused whatever else is passed; nothing is followed
        assert fn(None, ctypes.byref(b), ctypes.byref(out)) == _lib.ERR_ARG
        assert fn(None, None, None) == _lib.ERR_ARG
        assert fn(None, ctypes.byref(b), None) == _lib.ERR_ARG
    assert L.bjx_debug_set_trim_grid(None, 1) == _lib.ERR_ARG


def _small(seed, n_ips=25):
    rng = random.Random(seed)
    ips = ["10.%d.0.%d" % (seed, k) for k in range(n_ips)]
    rng.shuffle(ips)
    pool = [rng.randrange(-5, 12) * 10 for _ in range(8)] + [INT64_MIN, INT64_MAX, INT64_MAX - 1, -1, 0]
    states = {ip: {n: (rng.randrange(4), rng.choice(pool)) for n in rng.sample(H.NAMES, rng.randrange(1, 4))} for ip in ips}
    return ips, states


def _brute_cut(values, k):
    """the smallest C among the candidates (INT64_MIN, each distinct value and its + 1) with #{v >= C} <= k"""
    if k == 0:
        return INT64_MIN
    cands = {INT64_MIN} | set(values) | {min(v + 1, INT64_MAX) for v in values}
    ok = [c for c in cands if sum(1 for v in values if v >= c) <= k]
    return min(ok) if ok else INT64_MAX


def test_model_against_brute_force_remove_and_query():
    bounds, saturated = set(), 0
    for seed in range(8):
        ips, states = _small(seed)
        rng = random.Random(50 + seed)
        n_st = len(H.all_starts(states))
        newest = [max(s[1] for s in d.values()) for d in states.values()]
        for _ in range(60):
            ms = rng.choice((0, rng.randrange(1, n_st + 3)))
            mi = rng.choice((0, rng.randrange(1, len(ips) + 3)))
            floor = rng.choice((INT64_MIN, INT64_MIN, rng.choice(H.all_starts(states)), INT64_MAX))
            kept_ips, kept, st = state_trim.trim(ips, states, ms, mi, floor)
            c = st["cutoff_ns"]
            assert c == max(floor, _brute_cut(H.all_starts(states), ms), _brute_cut(newest, mi))
            # the trim is the expiry at C: the removal's and the query's models agree
            if c > INT64_MIN:
                w_ips, w_kept, w = state_remove.remove(ips, states, max_start_ns=c - 1)
                assert st["states_dropped"] == state_query.select(ips, states, max_start_ns=c - 1)[0]
            else:
                w_ips, w_kept, w = state_remove.remove(ips, states, ips=["nobody"])
                assert st["states_dropped"] == 0
            assert (kept_ips, kept) == (w_ips, w_kept)
            assert snapshot.parse(snapshot.build(kept_ips, kept)) == (kept_ips, kept)
            for k in ("states_before", "states_dropped", "ips_before", "ips_dropped", "arena_bytes_before", "arena_bytes_after"):
                assert st[k] == w[k]
            assert st["states_dropped_live"] == sum(1 for v in H.all_starts(states) if floor <= v < c)
            left, left_ips = len(H.all_starts(kept)), len(kept_ips)
            if st["budget_met"]:
                assert (not ms or left <= ms) and (not mi or left_ips <= mi)
            else:
                assert c == INT64_MAX and all(v == INT64_MAX for v in H.all_starts(kept))
                assert (ms and left > ms) or (mi and left_ips > mi)
                saturated += 1
            bounds.add(st["bound"])
    assert bounds == {0, 1, 2, 3} and saturated > 0


def test_model_node_is_one_cutoff():
    ips, states = H.sample(seed=2, n_ips=90)
    parts = [(ips[k::3], {ip: states[ip] for ip in ips[k::3]}) for k in range(3)]
    out, total = state_trim.node_trim(parts, max_states=40, max_ips=25, floor_cutoff_ns=H.T0)
    own = [state_trim.pick(i, s, 40, 25, H.T0) for i, s in parts]
    assert total["cutoff_ns"] == max(p[0] for p in own)
    assert total["bound"] == next(p[1] for p in own if p[0] == total["cutoff_ns"])
    for (kept_ips, kept), (i, s) in zip(out, parts):
        assert len(H.all_starts(kept)) <= 40 and len(kept_ips) <= 25
        assert (kept_ips, kept) == state_trim.apply(i, s, total["cutoff_ns"], H.T0)[:2]
    assert total["states_dropped"] == sum(len(H.all_starts(s)) for _, s in parts) - sum(len(H.all_starts(k)) for _, k in out)


def test_gpu_test_inputs_are_telling():
    """Conditions on the inputs of tests/test_gpu_state_trim.py, from the models alone."""
    ips, states = H.sample()
    starts = H.all_starts(states)
    assert 550 <= len(ips) <= 650 and 1300 <= len(starts) <= 1700
    assert INT64_MIN in starts and INT64_MAX - 1 in starts and min(s for s in starts if s > INT64_MIN + 1) < -(1 << 60)
    by_bound, tie_cuts, noops, partial = {0: 0, 1: 0, 2: 0, 3: 0}, 0, 0, 0
    for bud in H.budgets(states):
        kept_ips, kept, st = state_trim.trim(ips, states, **bud)
        by_bound[st["bound"]] += 1
        noops += st["states_dropped"] == 0
        left, left_ips = len(H.all_starts(kept)), len(kept_ips)
        # a tie group was cut: the bound that set the cutoff leaves room
        if st["bound"] == state_trim.BY_STATES and left < bud["max_states"] and len(starts) > bud["max_states"]:
            tie_cuts += 1
        elif st["bound"] == state_trim.BY_IPS and left_ips < bud["max_ips"] and len(ips) > bud["max_ips"]:
            tie_cuts += 1
        partial += any(0 < len(kept[state_query._b(ip)]) < len(states[ip]) for ip in ips if state_query._b(ip) in kept)
    assert min(by_bound[1], by_bound[2], by_bound[3]) >= 20, by_bound
    assert tie_cuts >= 20 and noops >= 3 and partial >= 1, (tie_cuts, noops, partial)
    # the real trims cover every bound
    expected = [state_trim.trim(ips, states, **b)[2] for b in H.budgets(states)]
    sub = H.real_subset(expected)
    assert {expected[k]["bound"] for k in sub} == {0, 1, 2, 3} and 15 <= len(sub) <= 25
    # the digit cases cut in the middle
    for d in range(8):
        vals = H.byte_starts(d)
        assert len(set(vals)) > 100 and all((a ^ b) & ~(0xFF << (8 * d)) & ((1 << 64) - 1) == 0 for a, b in zip(vals, vals[1:]))
        assert d != 7 or (min(vals) < 0 < max(vals))
        st = state_trim.trim(*H.flat_state(vals), max_states=150)[2]
        assert 100 < st["states_dropped"] < 200 and st["bound"] == state_trim.BY_STATES


def test_stream_shows_both_effects():
    """The across-batches run of the GPU test, the models alone: the trims drop
    live states, and later events show both effects -- FirstTime with seen_ip 1
    (a dropped rule of a known IP) and seen_ip 0 (an IP that lost everything)."""
    run, done = H.stream_run(None)
    assert len(done) == 3
    assert {st["bound"] for st in done} == {state_trim.BY_STATES, state_trim.BY_IPS}
    for st in done:
        assert st["states_dropped_live"] > 0 and 0 < st["states_dropped"] < st["states_before"], st
    assert run.diff_first > 0 and run.diff_seen > 0


# ---- the host header, through tests/cpu/trim_host.cpp

def _script():
    """-> (command lines, the expected output lines)"""
    cmds, want = [], []

    def add(line, answer):
        cmds.append(line)
        want.append(answer)

    add("check NULL", "check no budget")
    add("check 0", "check ok")
    add("check 1", "check ok")
    add("check 2", "check budget: unknown flag bits")
    add("check 4294967295", "check budget: unknown flag bits")
    add("geom", "geom 51:8192 38:8192 25:8192 12:8192 0:4096")

    def sel(vals, k):
        if k == 0 or len(vals) <= k:
            answer = "sel none"
        else:
            v = sorted(vals, reverse=True)[k]
            answer = "sel %d %d %d" % (v, min(v + 1, INT64_MAX), v == INT64_MAX)
            assert state_trim.cut(vals, k) == (min(v + 1, INT64_MAX), v == INT64_MAX)  # the Python model says the same
        add("sel %d %s" % (k, " ".join(map(str, vals))), answer)

    rng = random.Random(11)
    edge = [INT64_MIN, -1, 0, INT64_MAX]
    for n in (1, 2, 255, 256, 257):
        arrays = [[rng.randrange(INT64_MIN, INT64_MAX + 1) for _ in range(n)],
                  [rng.randrange(-1000, 1000) for _ in range(n)],
                  [H.T0 + rng.randrange(64) * H.S for _ in range(n)],
                  [rng.choice(edge) for _ in range(n)],
                  [rng.choice(edge + [rng.randrange(INT64_MIN, INT64_MAX + 1)]) for _ in range(n)]]
        arrays += [[v] * n for v in edge + [H.T0]]
        for vals in arrays:
            for k in sorted({0, 1, max(n - 1, 1), n, n + 1}):
                sel(vals, k)
    for d in range(8):
        vals = H.byte_starts(d, n=257)
        for k in (1, 100, 128, 256, 257):
            sel(vals, k)
        # two values that differ in one bit of byte d
        for bit in (8 * d, 8 * d + 7):
            lo = 0x0102030405060708 & ~(1 << bit)
            pair = [u - (1 << 64) if u >= 1 << 63 else u for u in (lo, lo | (1 << bit), lo)]
            for k in (1, 2, 3):
                sel(pair, k)
    sel([INT64_MAX, INT64_MAX, 5], 1)
    sel([INT64_MAX, INT64_MAX - 1, 5], 1)

    for v in (INT64_MIN, -1, 0, INT64_MAX - 1, INT64_MAX):
        add("plus %d" % v, "plus %d %d" % (min(v + 1, INT64_MAX), v == INT64_MAX))

    def pick(floor, cs, ss, ci, si):
        c = max(floor, cs, ci)
        bound = 3 if ci == c and ci > INT64_MIN else 2 if cs == c and cs > INT64_MIN else 1 if floor > INT64_MIN else 0
        add("pick %d %d %d %d %d" % (floor, cs, ss, ci, si), "pick %d %d %d" % (c, bound, not (ss or si)))

    vals = [INT64_MIN, -7, 0, 7, INT64_MAX]
    for floor in vals:
        for cs in vals:
            for ci in vals:
                pick(floor, cs, cs == INT64_MAX and floor < 0, ci, ci == INT64_MAX and floor > 0)

    engines = [(rng.choice(vals), rng.randrange(4), rng.randrange(2), rng.randrange(1, 100) / 4) for _ in range(6)]
    for n in (1, 2, 6):
        cmds.append("node %d" % n)
        cmds += ["p %d %d %d %g" % e for e in engines[:n]]
        c = max(e[0] for e in engines[:n])
        want.append("node %d %d %d %g" % (c, next(e[1] for e in engines[:n] if e[0] == c),
                                          all(e[2] for e in engines[:n]), max(e[3] for e in engines[:n])))
    cmds += ["node 3", "p 5 1 1 1", "p 5 2 1 1", "p 5 3 1 1"]  # several engines gave C: the lowest index wins
    want.append("node 5 1 1 1")
    shards = [[rng.randrange(1 << 40) for _ in range(9)] + [rng.randrange(1, 100) / 4, rng.randrange(1, 100) / 4]
              for _ in range(5)]
    for n in (0, 1, 5):
        cmds.append("sum %d" % n)
        cmds += ["s " + " ".join("%d" % v for v in s[:9]) + " %g %g" % (s[9], s[10]) for s in shards[:n]]
        want.append("sum " + " ".join("%d" % sum(s[k] for s in shards[:n]) for k in range(9)) +
                    " %g %g" % (max([s[9] for s in shards[:n]] + [0]), max([s[10] for s in shards[:n]] + [0])))
    return cmds, want


def _run_and_check(exe):
    cmds, want = _script()
    with tempfile.NamedTemporaryFile("w", suffix=".txt", delete=False) as f:
        f.write("\n".join(cmds) + "\n")
    try:
        r = subprocess.run([exe, f.name], capture_output=True, text=True, timeout=120)
    finally:
        os.unlink(f.name)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = r.stdout.splitlines()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w
    return len(want)


def test_host_header_select_cut_bound_and_node():
    d = tempfile.mkdtemp(prefix="bjx_trim_")
    exe = os.path.join(d, "trim_host")
    subprocess.run(["g++", "-O2", "-std=c++17", "-o", exe, SRC], check=True)
    assert _run_and_check(exe) > 400


def test_standalone_program_under_sanitizers():
    """The same program built with ASan + UBSan and run once as a child process
    over the same script (nothing loaded into Python runs under a sanitizer)."""
    d = tempfile.mkdtemp(prefix="bjx_trim_san_")
    exe = os.path.join(d, "trim_host")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-o", exe, SRC], check=True)
    _run_and_check(exe)
