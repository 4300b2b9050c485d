"""Per-rule-name totals on the device (bjx_state_query_names and its node
form, include/banjax_gpu.h).

Expected values (tests/state_names.py): the answers of the pure-Python model
banjax_amd/state_names.py over the model state of tests/state_remove.Run or
over the snapshot that was imported; tests/test_state_names_cpu.py holds that
model against a brute-force aggregation and shows the worlds are telling.
Every returned row is also checked against bjx_state_query and
bjx_state_remove, the calls a row's name is meant for."""
import ctypes as C

import pytest

from banjax_amd import Engine, Node, _lib, snapshot, state_names
from banjax_amd._lib import BanjaxGpuError
from tests import state_names as M
from tests import state_nets as N
from tests import state_remove as H
from tests.state_names import INT64_MAX, INT64_MIN, check_names, check_rows_against_query

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def wengine():
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def world(wengine):
    """an engine of its own holding the nets world, and (ips, states) of its model; the tests that use it only query"""
    run = N.build_world(wengine)
    return run.model.snapshot_args()


@pytest.fixture(scope="module")
def sengine():
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def shape(sengine):
    """an engine of its own that imported the shape world; the tests that use it only query"""
    ips, states = M.shape_world()
    sengine.state_import(snapshot.build(ips, states))
    return ips, states


def imported(ips, states):
    e = Engine()
    e.state_import(snapshot.build(ips, states))
    return e


def all_rows(target, **kw):
    out = []
    for order in M.ORDERS:
        a = target.state_query_names(order=order, limit=65536, **kw)
        out.append(({k: a[k] for k in M.COUNTS}, a["rows"]))
    return out


@pytest.mark.parametrize("which", ["nets", "shape"])
def test_model_parity_every_order_limit_and_floor(wengine, world, sengine, shape, which):
    eng, (ips, states) = (wengine, world) if which == "nets" else (sengine, shape)
    full = check_names(eng, ips, states, limit=65536)
    n = full["n_names"]
    assert n >= 3 and len(full["rows"]) == n and eng.debug_names_info()[0] == "lds"
    top = max(r.n_states for r in full["rows"])
    for order in M.ORDERS:
        for limit in (0, 1, n - 1, n, 65536):
            for min_states in (0, 2, top + 1):
                got = check_names(eng, ips, states, order=order, limit=limit, min_states=min_states)
                assert got["n_names"] == n and (min_states != top + 1 or got["n_names_min"] == 0)
    check_names(eng, ips, states, order="newest", limit=2)
    plain = eng.state_query(limit=0)
    assert (plain["n_matched"], plain["n_ips_matched"]) == (full["n_matched"], full["n_ips_matched"])


def test_filters_and_cross_checks_on_the_nets_world(wengine, world):
    ips, states = world
    for filt in ({}, {"min_hits": 2}, {"min_hits": 3}, {"min_start_ns": N.NOW + 50_000_000},
                 {"min_start_ns": N.NOW + 20_000_000, "max_start_ns": N.NOW + 90_000_000, "min_hits": 1}):
        for order in M.ORDERS:
            got = check_names(wengine, ips, states, order=order, limit=65536, **filt)
        check_rows_against_query(wengine, got["rows"], **filt)            # (the orders return the same rows)
        plain = wengine.state_query(limit=0, **filt)
        assert (plain["n_matched"], plain["n_ips_matched"]) == (got["n_matched"], got["n_ips_matched"])
    for filt in ({"name": "slow"}, {"name": "mid", "min_hits": 2}):
        got = check_names(wengine, ips, states, limit=65536, **filt)
        assert [r.name for r in got["rows"]] == [filt["name"].encode()]
    # a held IP, a held text that is no address, and IPs not held
    for ip in ("170.85.195.60", "::ffff:170.85.195.60", "01.2.3.4", ""):
        for filt in ({}, {"name": "mid"}, {"min_hits": 2}):
            got = check_names(wengine, ips, states, ip=ip, limit=10, **filt)
            assert got["n_ips_matched"] <= 1
        assert check_names(wengine, ips, states, ip=ip)["n_ips_matched"] == 1
    for ip in ("170.85.195.77", "2001:db8:85a3::77", "not-an-ip"):
        got = check_names(wengine, ips, states, ip=ip)
        assert got["rows"] == [] and all(got[k] == 0 for k in M.COUNTS)
    for empty in (wengine.state_query_names(name="never-interned"), wengine.state_query_names(min_start_ns=5, max_start_ns=4)):
        assert empty["rows"] == [] and all(empty[k] == 0 for k in M.COUNTS)
    fresh = Engine()
    try:
        empty = fresh.state_query_names()
        assert empty["rows"] == [] and all(empty[k] == 0 for k in M.COUNTS) and fresh.debug_names_info()[0] == "none"
    finally:
        fresh.close()


def test_shape_world_filters_name_shapes_and_cross_checks(sengine, shape):
    ips, states = shape
    got = check_names(sengine, ips, states, order="name", limit=65536)
    names = [r.name for r in got["rows"]]
    assert names[0] == b"" and names.index(b"a") + 1 == names.index(b"ab") and names[-1] == M.HIGH and M.LONG in names
    check_rows_against_query(sengine, got["rows"])
    for filt in ({"min_hits": 1}, {"min_hits": 1 << 14}, {"max_start_ns": M.T0}, {"ip": ips[0]}, {"ip": ips[39], "min_hits": 2}):
        for order in M.ORDERS:
            got = check_names(sengine, ips, states, order=order, limit=65536, **filt)
    check_rows_against_query(sengine, check_names(sengine, ips, states, limit=65536, min_hits=1)["rows"], min_hits=1)
    for name in (b"", b"a", b"ab", M.HIGH, M.LONG, b"zero", b"hist"):
        got = check_names(sengine, ips, states, name=name, limit=5)
        assert [r.name for r in got["rows"]] == [name]
    rows = {r.name: r for r in sengine.state_query_names(limit=65536)["rows"]}
    assert all(c > 0 for c in rows[b"hist"].hist) and rows[b"zero"].hist == (6,) + (0,) * 15
    assert state_names.orphans(list(rows.values()), [n for n in rows if n != b"ab"]) == [rows[b"ab"]]


def test_paths_at_the_real_lds_limit():
    """L - 1, L and L + 1 interned names: LDS, LDS, global, and the same answers as the model"""
    probe = Engine()
    try:
        path, L = probe.debug_names_info()
        assert path == "none" and L == (128 * 1024) // 96
    finally:
        probe.close()
    for n, want_path in ((L - 1, "lds"), (L, "lds"), (L + 1, "global")):
        ips, states = M.count_world(n)
        eng = imported(ips, states)
        try:
            got = check_names(eng, ips, states, order="name", limit=65536)
            assert got["n_names"] == n and eng.debug_names_info() == (want_path, L)
            check_names(eng, ips, states, order="hits", limit=7, min_states=2)
            check_names(eng, ips, states, limit=65536, min_hits=20)
            check_rows_against_query(eng, got["rows"][::211])
        finally:
            eng.close()


def test_hooked_limits_grid_of_one_and_the_skewed_world():
    ips, states = M.count_world(8)
    eng = imported(ips, states)
    try:
        for cap, want_path in ((7, "global"), (8, "lds"), (9, "lds"), (0, "lds"), (1 << 30, "lds")):
            eng.debug_set_names(cap, 0)
            check_names(eng, ips, states, limit=65536)
            assert eng.debug_names_info()[0] == want_path, cap
        for cap, want_path in ((0, "lds"), (1, "global")):                 # one block walks the whole table
            eng.debug_set_names(cap, 1)
            for order in M.ORDERS:
                check_names(eng, ips, states, order=order, limit=65536)
            check_names(eng, ips, states, ip=ips[2], limit=65536)
            assert eng.debug_names_info()[0] == want_path
        eng.debug_set_names(0, 0)
    finally:
        eng.close()
    ips, states = M.skewed_world()
    eng = imported(ips, states)
    try:
        want = all_rows(eng)
        assert eng.debug_names_info()[0] == "lds" and want[0][1][0].name == b"big" and want[0][1][0].n_states == M.N_SKEW
        check_names(eng, ips, states, limit=65536)
        for lds_names, blocks in ((1, 0), (1, 1), (0, 1), (0, 3)):
            eng.debug_set_names(lds_names, blocks)
            assert all_rows(eng) == want
            assert eng.debug_names_info()[0] == ("global" if lds_names else "lds")
        check_names(eng, ips, states, limit=65536, min_hits=33)
        check_rows_against_query(eng, want[0][1])
    finally:
        eng.close()


def test_extremes_wrap_and_remove_agrees():
    ips, states = M.extreme_world()
    eng = imported(ips, states)
    try:
        for lds_names in (0, 1):
            eng.debug_set_names(lds_names, 0)
            for order in M.ORDERS:
                got = check_names(eng, ips, states, order=order, limit=10)
            rows = {r.name: r for r in got["rows"]}
            assert rows[b"up"].hits_sum == 10 and rows[b"down"].hits_sum == -1 and rows[b"ends"].hits_sum == -1
            assert (rows[b"ends"].max_hits, rows[b"ends"].newest_start_ns, rows[b"ends"].oldest_start_ns) == (INT64_MAX, INT64_MAX, INT64_MIN)
            assert rows[b"neg"].max_hits == -1 and rows[b"zero"].hist == (2,) + (0,) * 15 and rows[b"down"].max_hits == -1
            check_names(eng, ips, states, limit=10, min_start_ns=INT64_MIN + 1)
            check_names(eng, ips, states, limit=10, min_hits=INT64_MAX)
            check_names(eng, ips, states, limit=10, max_start_ns=INT64_MIN)
        eng.debug_set_names(0, 0)
        check_rows_against_query(eng, got["rows"])
        # bjx_state_remove with the same filter and the row's name drops exactly the row's states
        filt = {"min_start_ns": INT64_MIN + 1}
        for r in eng.state_query_names(limit=10, **filt)["rows"]:
            assert eng.state_remove(name=r.name, **filt)["states_dropped"] == r.n_states, r
        left = eng.state_query_names(limit=10)
        assert left["n_matched"] == sum(1 for d in states.values() for h, s in d.values() if s == INT64_MIN) > 0
        assert eng.state_query_names(limit=10, **filt)["n_matched"] == 0
    finally:
        eng.close()


def test_layout_and_history_do_not_show():
    """The same logical state under the debug hash mask, after a removal, after an expiry, after a
    re-import of the export, and merged in two pieces (names interned in another order):
    identical rows; a removed name has no row."""
    ips, states = M.shape_world()
    blob = snapshot.build(ips, states)
    eng, masked, pieces = Engine(), Engine(), Engine()
    try:
        masked.debug_set_ip_hash_mask(0x6)
        eng.state_import(blob)
        masked.state_import(blob)
        want = all_rows(eng)
        assert all_rows(masked) == want and eng.state_export() == blob
        # the later names first, then the rest merged in: other name ids
        names = sorted({n for d in states.values() for n in d})
        late = set(names[len(names) // 2:])
        first = {ip: {n: v for n, v in d.items() if n in late} for ip, d in states.items()}
        rest = {ip: {n: v for n, v in d.items() if n not in late} for ip, d in states.items()}
        pieces.state_import(snapshot.build(ips[::-1], first))
        pieces.state_merge(snapshot.build(ips, rest))
        assert all_rows(pieces) == want
        # a removal by name: no row, although the name stays interned; survivors get new slots
        assert eng.state_remove(name=b"all")["states_dropped"] == len(ips)
        kept = {ip: {n: v for n, v in d.items() if n != b"all"} for ip, d in states.items()}
        got = check_names(eng, ips, kept, limit=65536)
        assert b"all" not in {r.name for r in got["rows"]} and eng.state_query_names(name=b"all")["n_names"] == 0
        masked.state_remove(name=b"all")
        assert all_rows(masked) == all_rows(eng)
        cut = M.T0 + 3
        pre = all_rows(eng, min_start_ns=cut)
        assert eng.state_expire(cut)["states_dropped"] > 0
        assert all_rows(eng) == pre
        fresh = Engine()
        try:
            fresh.state_import(eng.state_export())
            assert all_rows(fresh) == pre
        finally:
            fresh.close()
    finally:
        masked.debug_set_ip_hash_mask(0)
        for e in (eng, masked, pieces):
            e.close()


def test_after_real_batches_unbound_rules_and_rolled_back_claims():
    eng = Engine()
    try:
        run, _ = H.parity_run(eng, H.stream()[:3], compare_dump=False)
        ips, states = run.model.snapshot_args()
        blob = eng.state_export()
        for order in M.ORDERS:
            got = check_names(eng, ips, states, order=order, limit=65536)
        check_names(eng, ips, states, limit=65536, min_hits=2)
        check_rows_against_query(eng, got["rows"])
        assert eng.state_export() == blob
        data, now = H.stream()[3]
        run.feed(data, now)                                                # the RuleResults equal the oracle's model
        check_names(eng, *run.model.snapshot_args(), limit=65536)
        # a ruleset's rule that never matched is interned and has no row
        quiet = H.Run(H.one_rule().replace("expiring", "  - {rule: \"never\", regex: 'ZZZZ', interval: 5, hits_per_interval: 1, "
                                                       "decision: challenge}\nexpiring"), eng)
        quiet.feed(H.lines([(k, "10.3.0.%d" % (k % 9)) for k in range(50)]), H.T0_MS * 1_000_000)
        got = check_names(eng, *quiet.model.snapshot_args(), limit=65536)
        assert [r.name for r in got["rows"]] == [b"r"] and eng.state_query_names(name="never")["n_matched"] == 0
        # a claim pass that was rolled back and run again leaves nothing that counts
        run = H.Run(H.one_rule(60, 100), eng)
        many = ["192.168.%d.%d" % (k >> 8, k & 255) for k in range(3000)]
        eng.debug_set_claim_budget(64)
        try:
            run.feed(H.lines([(k // 7, ip) for k, ip in enumerate(many)]), H.T0_MS * 1_000_000)
        finally:
            eng.debug_set_claim_budget(0)
        got = check_names(eng, *run.model.snapshot_args(), limit=65536)
        assert (got["n_matched"], got["n_ips_matched"], got["rows"][0].hist[1]) == (3000, 3000, 3000)
    finally:
        eng.close()


def test_bad_arguments_and_open_batch(wengine, world):
    import torch
    before = wengine.state_export()
    for kw, word in (({"order": 5}, "order"), ({"order": 0xFFFFFFFF}, "order"), ({"limit": 65537}, "limit")):
        with pytest.raises(BanjaxGpuError) as ei:
            wengine.state_query_names(**kw)
        assert ei.value.code == -2 and word in str(ei.value), (kw, str(ei.value))
    L = _lib.lib()
    f = _lib.StateFilter(_lib.Str(None, 0), _lib.Str(None, 0), INT64_MIN, INT64_MIN, INT64_MAX, 0, 0)
    s = _lib.NamesSpec(0, 2, 0)
    out = _lib.StateNames()
    assert L.bjx_state_query_names(wengine._h, C.byref(f), C.byref(s), C.byref(out)) == _lib.OK and out.n_rows == 2 and out.n_names == 3
    first = (out.n_matched, out.n_ips_matched, out.n_names, out.n_rows)
    assert first[0] > first[1] > 0
    for args in ((None, C.byref(s), C.byref(out)), (C.byref(f), None, C.byref(out)), (C.byref(f), C.byref(s), None)):
        assert L.bjx_state_query_names(wengine._h, *args) == _lib.ERR_ARG
    for bad in (_lib.StateFilter(_lib.Str(None, 0), _lib.Str(None, 0), 0, 0, 0, 2, 0),          # what bjx_state_query refuses
                _lib.StateFilter(_lib.Str(None, 0), _lib.Str(None, 0), 0, 0, 0, 0, 65537),
                _lib.StateFilter(_lib.Str(None, 3), _lib.Str(None, 0), 0, 0, 0, 0, 0),
                _lib.StateFilter(_lib.Str(None, 0), _lib.Str(None, 3), 0, 0, 0, 0, 0)):
        assert L.bjx_state_query_names(wengine._h, C.byref(bad), C.byref(s), C.byref(out)) == _lib.ERR_ARG
    # f->order and f->limit that bjx_state_query takes change nothing
    g = _lib.StateFilter(_lib.Str(None, 0), _lib.Str(None, 0), INT64_MIN, INT64_MIN, INT64_MAX, 1, 7)
    out2 = _lib.StateNames()
    assert L.bjx_state_query_names(wengine._h, C.byref(g), C.byref(s), C.byref(out2)) == _lib.OK
    assert (out2.n_matched, out2.n_ips_matched, out2.n_names, out2.n_rows) == first == first[:2] + (3, 2)
    assert wengine.state_export() == before
    # an open batch on an engine of its own
    eng = Engine()
    try:
        run = H.Run(H.CFG, eng)
        data, now = H.stream()[0]
        run.feed(data, now)
        dump = eng.state_dump()
        buf = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
        eng.match(run.rs, now, buf.data_ptr(), len(data))
        with pytest.raises(BanjaxGpuError) as ei:
            eng.state_query_names()
        assert ei.value.code == -2 and "bjx_finish_batch" in str(ei.value)
        assert eng.state_dump() == dump
    finally:
        eng.close()


@pytest.mark.parametrize("n_engines", [2, 3])
def test_node_equals_the_model_of_the_union(n_engines):
    """A name's states are spread over the engines of a node: a name on one shard, a name on
    all, and the limit and the floor applied only after the merge."""
    ips, states = M.shape_world()
    node = Node([0] * n_engines)
    try:
        node.state_import(snapshot.build(ips, states))
        for order in M.ORDERS:
            for kw in ({"limit": 65536}, {"limit": 3}, {"limit": 65536, "min_states": 7}, {"limit": 0}, {"limit": 20, "name": b"hist"},
                       {"limit": 5, "ip": ips[0]}, {"limit": 5, "ip": "1.2.3"}, {"limit": 4, "min_hits": 5}):
                check_names(node, ips, states, order=order, **kw)
        parts = [{r.name: r for r in node.engine(k).state_query_names(limit=65536)["rows"]} for k in range(n_engines)]
        assert sum(1 for p in parts if b"solo" in p) == 1 and all(b"all" in p and b"hist" in p for p in parts)
        whole = {r.name: r for r in node.state_query_names(limit=65536)["rows"]}
        assert whole[b"all"].n_states == sum(p[b"all"].n_states for p in parts) == len(ips)
        assert whole[b"hist"].hist == tuple(sum(p[b"hist"].hist[b] for p in parts) for b in range(16))
        # a name below the floor on every shard reaches it in total; the shards' own top 3 are not the node's
        floor = max(p[b"all"].n_states for p in parts) + 1
        assert b"all" in {r.name for r in node.state_query_names(limit=65536, min_states=floor)["rows"]}
        with pytest.raises(BanjaxGpuError) as ei:
            node.state_query_names(order=5)
        assert ei.value.code == -2
    finally:
        node.close()
