"""bjx_state_merge without a GPU: the C symbols, their NULL handling and the
struct sizes, the header's declarations, and the pure-Python model
(banjax_amd/state_merge.py): the algebra of NEWER (idempotent, commutative,
associative), KEEP and REPLACE against hand-written cases, the ties, the
counts, the min_start_ns and owner filters."""
import ctypes
import random
import re

import pytest

from banjax_amd import _lib, snapshot, state_merge
from banjax_amd.state_merge import KEEP, NEWER, REPLACE

INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
NAMES = ["fast", "mid", "slow"]
COUNTS = ("states_added", "states_replaced", "states_kept", "states_skipped")


def test_symbols_structs_and_null_arguments():
    L = _lib.lib()
    for name in ("bjx_state_merge", "bjx_node_state_merge"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    assert ctypes.sizeof(_lib.MergeOptions) == 24 and ctypes.sizeof(_lib.MergeStats) == 136
    assert [k for k, _ in _lib.MergeOptions._fields_] == ["min_start_ns", "part", "n_parts", "policy", "flags"]
    assert [k for k, _ in _lib.MergeStats._fields_] == [
        "snap_ips", "snap_states", "snap_names", "snap_bytes", "ips_before", "ips_added", "ips_skipped", "states_before",
        "states_added", "states_replaced", "states_kept", "states_skipped", "arena_bytes_before", "arena_bytes_after",
        "device_bytes_before", "device_bytes_after", "device_ms"]
    assert (_lib.MERGE_NEWER, _lib.MERGE_KEEP, _lib.MERGE_REPLACE, _lib.MERGE_DRY_RUN) == (0, 1, 2, 1)
    assert (NEWER, KEEP, REPLACE) == (0, 1, 2)
    blob = snapshot.build([], {})
    o, out = _lib.MergeOptions(INT64_MIN, 0, 1, 0, 0), _lib.MergeStats()
    for fn in (L.bjx_state_merge, L.bjx_node_state_merge):
        # a NULL handle is refused whatever else is passed; nothing is followed
        assert fn(None, blob, len(blob), ctypes.byref(o), ctypes.byref(out)) == _lib.ERR_ARG
        assert fn(None, None, 0, None, None) == _lib.ERR_ARG
        assert fn(None, blob, len(blob), None, None) == _lib.ERR_ARG


def test_header_declares_both_calls():
    text = open("include/banjax_gpu.h").read()
    for pre, handle in (("bjx_state_merge", "bjx_engine *e"), ("bjx_node_state_merge", "bjx_node *n")):
        assert re.search(r"^int %s\(%s, const uint8_t \*snap, uint64_t len, const bjx_merge_options \*o,\s*"
                         r"bjx_merge_stats \*out\);" % (pre, re.escape(handle)), text, re.M), pre
    assert "enum bjx_merge_policy { BJX_MERGE_NEWER = 0, BJX_MERGE_KEEP = 1, BJX_MERGE_REPLACE = 2 };" in text
    assert "enum bjx_merge_flags { BJX_MERGE_DRY_RUN = 1 };" in text
    assert re.search(r"#define BJX_ABI_VERSION 5\b", text)


def test_check_abi_passes():
    import __graft_entry__ as G
    assert G.check_abi() == 5


def _small(seed, n_ips=12, lo=0):
    """a random small state over a pool of IPs that overlaps its neighbours' and a few start values, so keys tie"""
    rng = random.Random(seed)
    ips = ["10.0.0.%d" % k for k in rng.sample(range(lo, lo + 20), n_ips)]
    pool = [10, 20, 20, 30, INT64_MIN, INT64_MAX, -1, 0]
    states = {ip: {n: (rng.randrange(-2, 4), rng.choice(pool)) for n in rng.sample(NAMES, rng.randrange(1, 4))} for ip in ips}
    return snapshot.build(ips, states)


def _as_dict(blob):
    return snapshot.parse(blob)[1]


def test_newer_is_idempotent_commutative_associative():
    for seed in range(20):
        a, b, c = _small(3 * seed), _small(3 * seed + 1, lo=5), _small(3 * seed + 2, lo=10)
        aa, s = state_merge.merge(a, a)
        assert aa == a
        assert (s["ips_added"], s["states_added"], s["states_replaced"], s["states_skipped"]) == (0, 0, 0, 0)
        assert s["states_kept"] == s["snap_states"] == s["states_before"]
        ab, ba = state_merge.merge(a, b)[0], state_merge.merge(b, a)[0]
        assert _as_dict(ab) == _as_dict(ba)  # (the IP order differs: whose IPs were there first)
        assert set(_as_dict(ab)) == set(_as_dict(a)) | set(_as_dict(b))
        left = state_merge.merge(state_merge.merge(a, b)[0], c)[0]
        right = state_merge.merge(a, state_merge.merge(b, c)[0])[0]
        assert left == right  # a's IPs, then b's, then c's, either way
        # merging a second time changes nothing
        assert state_merge.merge(ab, b)[0] == ab and state_merge.merge(ab, a)[0] == ab


def _one(mine, theirs, policy):
    """one key on both sides -> (the record left, (added, replaced, kept, skipped))"""
    a = snapshot.build(["1.1.1.1"], {"1.1.1.1": {"r": mine}})
    b = snapshot.build(["1.1.1.1"], {"1.1.1.1": {"r": theirs}})
    m, s = state_merge.merge(a, b, policy)
    assert sum(s[k] for k in COUNTS) == s["snap_states"] == 1
    return _as_dict(m)[b"1.1.1.1"][b"r"], tuple(s[k] for k in COUNTS)


TIES = [
    # (engine (hits, start), snapshot (hits, start), NEWER's record, NEWER's counts)
    ((3, 100), (1, 200), (1, 200), (0, 1, 0, 0)),            # the later start wins whatever the hits
    ((1, 200), (3, 100), (1, 200), (0, 0, 1, 0)),
    ((3, 100), (5, 100), (5, 100), (0, 1, 0, 0)),            # equal start: the larger hits
    ((5, 100), (3, 100), (5, 100), (0, 0, 1, 0)),
    ((4, 100), (4, 100), (4, 100), (0, 0, 1, 0)),            # equal in both: kept
    ((0, 100), (7, 100), (7, 100), (0, 1, 0, 0)),            # hits 0 after a trip lose to the pre-trip count of the window
    ((7, 100), (0, 100), (7, 100), (0, 0, 1, 0)),
    ((1, INT64_MIN), (1, INT64_MAX), (1, INT64_MAX), (0, 1, 0, 0)),
    ((9, INT64_MAX), (1, INT64_MIN), (9, INT64_MAX), (0, 0, 1, 0)),
    ((1, INT64_MIN), (2, INT64_MIN), (2, INT64_MIN), (0, 1, 0, 0)),
    ((-1, 50), (-2, 50), (-1, 50), (0, 0, 1, 0)),            # hits compare signed
    ((-2, 50), (-1, 50), (-1, 50), (0, 1, 0, 0)),
    ((-1, 50), (0, 50), (0, 50), (0, 1, 0, 0)),
    ((5, -1), (1, 0), (1, 0), (0, 1, 0, 0)),                 # starts compare signed
]


@pytest.mark.parametrize("mine,theirs,rec,counts", TIES)
def test_ties(mine, theirs, rec, counts):
    assert _one(mine, theirs, NEWER) == (rec, counts)
    # KEEP: the engine's record whatever the snapshot's; REPLACE: the snapshot's, counted only when it differs
    assert _one(mine, theirs, KEEP) == (mine, (0, 0, 1, 0))
    assert _one(mine, theirs, REPLACE) == (theirs, (0, 0, 1, 0) if mine == theirs else (0, 1, 0, 0))


def test_keep_and_replace_by_hand():
    eng = snapshot.build(["a", "b", "c"], {"a": {"fast": (1, 10), "mid": (2, 20)}, "b": {"fast": (3, 30)}, "c": {"slow": (4, 40)}})
    snp = snapshot.build(["d", "b", "a"], {"d": {"mid": (9, 5)}, "b": {"fast": (0, 99), "slow": (7, 7)},
                                           "a": {"fast": (1, 10), "mid": (1, 21)}})
    m, s = state_merge.merge(eng, snp, KEEP)
    assert snapshot.parse(m) == ([b"a", b"b", b"c", b"d"], {
        b"a": {b"fast": (1, 10), b"mid": (2, 20)}, b"b": {b"fast": (3, 30), b"slow": (7, 7)}, b"c": {b"slow": (4, 40)},
        b"d": {b"mid": (9, 5)}})
    assert [s[k] for k in COUNTS] == [2, 0, 3, 0] and (s["ips_before"], s["ips_added"], s["ips_skipped"]) == (3, 1, 0)
    assert (s["arena_bytes_before"], s["arena_bytes_after"], s["states_before"]) == (3, 4, 4)
    m, s = state_merge.merge(eng, snp, REPLACE)
    assert snapshot.parse(m) == ([b"a", b"b", b"c", b"d"], {
        b"a": {b"fast": (1, 10), b"mid": (1, 21)}, b"b": {b"fast": (0, 99), b"slow": (7, 7)}, b"c": {b"slow": (4, 40)},
        b"d": {b"mid": (9, 5)}})
    assert [s[k] for k in COUNTS] == [2, 2, 1, 0]  # a/fast is equal on both sides: kept
    m, s = state_merge.merge(eng, snp, NEWER)
    assert _as_dict(m)[b"a"] == {b"fast": (1, 10), b"mid": (1, 21)} and _as_dict(m)[b"b"][b"fast"] == (0, 99)
    assert [s[k] for k in COUNTS] == [2, 2, 1, 0]
    assert (s["snap_ips"], s["snap_states"], s["snap_names"], s["snap_bytes"]) == (3, 5, 3, len(snp))
    with pytest.raises(ValueError):
        state_merge.merge(eng, snp, 3)
    with pytest.raises(ValueError):
        state_merge.merge(eng, snp, NEWER, INT64_MIN, 2, 2)


def test_counts_sum_and_min_start():
    for seed in range(20):
        a, b = _small(100 + seed), _small(200 + seed, lo=4)
        for policy in (NEWER, KEEP, REPLACE):
            for cut in (INT64_MIN, 0, 20, 21, INT64_MAX):
                m, s = state_merge.merge(a, b, policy, cut)
                assert sum(s[k] for k in COUNTS) == s["snap_states"]
                assert s["states_skipped"] == sum(1 for d in _as_dict(b).values() for r in d.values() if r[1] < cut)
                ips, st = snapshot.parse(m)
                assert len(ips) == s["ips_before"] + s["ips_added"]
                assert sum(len(d) for d in st.values()) == s["states_before"] + s["states_added"]
                assert sum(len(ip) for ip in ips) == s["arena_bytes_after"]
    # an IP all of whose records fall below min_start_ns is not added
    eng = snapshot.build(["a"], {"a": {"fast": (1, 10)}})
    snp = snapshot.build(["old", "a", "half"], {"old": {"fast": (1, 5), "mid": (2, 9)}, "a": {"fast": (2, 9)},
                                                "half": {"fast": (1, 9), "mid": (1, 10)}})
    m, s = state_merge.merge(eng, snp, NEWER, 10)
    assert snapshot.parse(m) == ([b"a", b"half"], {b"a": {b"fast": (1, 10)}, b"half": {b"mid": (1, 10)}})
    assert (s["ips_added"], s["ips_skipped"], s["states_skipped"], s["states_added"]) == (1, 2, 4, 1)


def test_parts_cover_the_snapshot_once():
    for seed in range(10):
        a, b = _small(300 + seed), _small(400 + seed, n_ips=18, lo=2)
        whole, s = state_merge.merge(a, b)
        step, tot = a, dict.fromkeys(COUNTS + ("ips_added",), 0)
        for k in range(3):
            step, sk = state_merge.merge(step, b, NEWER, INT64_MIN, k, 3)
            for f in tot:
                tot[f] += sk[f]
        assert _as_dict(step) == _as_dict(whole)
        assert tot["ips_added"] == s["ips_added"] and tot["states_added"] == s["states_added"]
        assert tot["states_replaced"] == s["states_replaced"] and tot["states_kept"] == s["states_kept"]
        assert tot["states_skipped"] == 2 * s["snap_states"]  # each record skipped by the two parts that do not own it
    # the owner function is the node's: hash_bytes of known inputs (tests/test_gpu_state_snapshot.py restates it too)
    assert state_merge.hash_bytes(b"") != 0 and state_merge.owner(b"10.1.0.1", 1) == 0
    assert {state_merge.owner(b"10.1.0.%d" % k, 3) for k in range(40)} == {0, 1, 2}
