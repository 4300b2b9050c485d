"""Top networks by prefix on the device (bjx_state_query_groups and its node
form, include/banjax_gpu.h).

Expected values (tests/state_groups.py): the answers of the pure-Python model
banjax_amd/state_groups.py over the model state of tests/state_remove.Run or
over the snapshot that was imported; tests/test_state_groups_cpu.py holds that
model against a brute-force grouping and shows the worlds are telling.  Every
returned row is also checked against bjx_state_query_nets, the call the row's
.net is meant for."""
import pytest

from banjax_amd import Engine, Node, snapshot, state_groups, state_nets
from banjax_amd._lib import BanjaxGpuError
from tests import state_groups as G
from tests import state_nets as N
from tests import state_remove as H
from tests.state_groups import B, INT64_MAX, INT64_MIN, check_groups

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
    assert H.dump_ips(wengine.state_dump()) == N.world_ips()
    return run.model.snapshot_args()


@pytest.fixture(scope="module")
def sengine():
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def shape(sengine):
    """an engine of its own that imported the shape world; the tests that use it only query"""
    ips, states = G.shape_world()
    sengine.state_import(snapshot.build(ips, states))
    return ips, states


def check_rows_against_nets(target, rows, **filt):
    """for every row, the nets query of its .net alone counts the row's states and IPs;
    and all the rows' nets at once count each row's IPs"""
    for r in rows:
        fam, bits, v = state_nets.parse_entry(r.net)
        assert (fam, bits) == (r.family, r.bits) and v == int.from_bytes(r.addr[:4] if fam == 4 else r.addr, "big"), r
        a = target.state_query(nets=[r.net], limit=0, **filt)
        assert (a["n_matched"], a["net_ips"]) == (r.n_states, [r.n_ips]), (r, a)
    if rows:
        a = target.state_query(nets=[r.net for r in rows], limit=0, **filt)
        assert a["net_ips"] == [r.n_ips for r in rows] and a["n_matched"] == sum(r.n_states for r in rows)


@pytest.mark.parametrize("v4_bits", G.LEN4)
def test_model_parity_every_prefix_pair_order_limit_and_floor(wengine, world, v4_bits):
    """Every (v4_bits, v6_bits) of LEN4 x LEN6 on the nets world, every order; limits 0, 1,
    n_groups - 1, n_groups and the most; min_ips 0, 2 and above every group."""
    ips, states = world
    for v6_bits in G.LEN6:
        full = check_groups(wengine, ips, states, v4_bits=v4_bits, v6_bits=v6_bits, limit=65536)
        n = full["n_groups"]
        assert n >= 2 and full["n_ips_unparsed"] >= len(N.NOT_ADDRESSES) - 1 and len(full["rows"]) == n
        check_rows_against_nets(wengine, full["rows"])
        top = max(r.n_ips for r in full["rows"])
        for order in G.ORDERS:
            for limit in (0, 1, n - 1, n, 65536):
                for min_ips in (0, 2, top + 1):
                    got = check_groups(wengine, ips, states, v4_bits=v4_bits, v6_bits=v6_bits, order=order, limit=limit,
                                       min_ips=min_ips)
                    assert got["n_groups"] == n and (min_ips != top + 1 or got["n_groups_min"] == 0)


def test_filters_select_parts_of_ips_and_windows(wengine, world):
    ips, states = world
    for filt in ({"name": "slow"}, {"name": "mid", "min_hits": 2}, {"min_hits": 3}, {"min_start_ns": N.NOW + 50_000_000},
                 {"min_start_ns": N.NOW + 20_000_000, "max_start_ns": N.NOW + 90_000_000, "min_hits": 1},
                 {"name": "never-interned"}, {"min_start_ns": 5, "max_start_ns": 4}):
        for v4_bits, v6_bits in ((24, 64), (0, 0), (32, 128), (8, 1)):
            for order in G.ORDERS:
                got = check_groups(wengine, ips, states, v4_bits=v4_bits, v6_bits=v6_bits, order=order, limit=65536, **filt)
            check_rows_against_nets(wengine, got["rows"], **filt)      # (the orders return the same rows)
    everything = wengine.state_query_groups(limit=0)
    part = wengine.state_query_groups(limit=0, name="slow")
    assert 0 < part["n_ips_matched"] < everything["n_ips_matched"] and part["n_matched"] == part["n_ips_matched"]
    plain = wengine.state_query(limit=0, name="slow")
    assert (plain["n_matched"], plain["n_ips_matched"]) == (part["n_matched"], part["n_ips_matched"])
    for empty in (wengine.state_query_groups(name="never-interned"), wengine.state_query_groups(min_start_ns=5, max_start_ns=4)):
        assert empty["rows"] == [] and all(empty[k] == 0 for k in G.COUNTS)


def test_ip_filter_inside_and_outside(wengine, world):
    ips, states = world
    for ip in ("170.85.195.60", "::ffff:170.85.195.60", "2001:db8:85a3:c55a:aa55:c33c:ff1:ce5a", "::170.85.195.60",   # held
               "01.2.3.4", "",                                                                                     # held, no address
               "170.85.195.77", "2001:db8:85a3::77", "not-an-ip"):                                                 # not held
        for filt in ({}, {"name": "mid"}, {"min_hits": 3}):
            for order in G.ORDERS:
                got = check_groups(wengine, ips, states, ip=ip, limit=5, **filt)
                assert got["n_ips_matched"] <= 1 and len(got["rows"]) <= 1
    a = wengine.state_query_groups(ip="::ffff:170.85.195.60")
    assert [r.net for r in a["rows"]] == ["170.85.195.0/24"] and a["rows"][0].n_ips == 1
    a = wengine.state_query_groups(ip="::170.85.195.60")
    assert [r.family for r in a["rows"]] == [6]
    a = wengine.state_query_groups(ip="01.2.3.4")
    assert (a["n_ips_matched"], a["n_ips_unparsed"], a["n_groups"], a["rows"]) == (1, 1, 0, [])
    assert wengine.state_query_groups(ip="170.85.195.77")["n_matched"] == 0


def test_run_shapes_of_the_reduction(sengine, shape):
    """B = 1024 sorted keys a block of k_grp_runs: /16 groups of exactly 1, B - 1, B and B + 1 IPs,
    the B-sized one exactly one block (the groups before it hold B keys together), one group over
    three blocks and more; next to them 2000 IPv6 singletons, one key a group."""
    ips, states = shape
    sizes = G.shape_sizes()
    from banjax_amd import _lib
    assert B == _lib.lib().bjx_debug_groups_tile()
    assert sizes[:4] == [1, B - 1, B, B + 1] and sizes[0] + sizes[1] == B and sum(sizes[:4]) % B + sizes[4] > 2 * B
    for order in G.ORDERS:
        got = check_groups(sengine, ips, states, v4_bits=16, v6_bits=64, order=order, limit=65536)
        assert got["n_groups"] == len(sizes) + G.N_V6_SINGLES
    by_net = {r.net: r.n_ips for r in got["rows"]}
    assert [by_net["10.%d.0.0/16" % k] for k in range(len(sizes))] == sizes
    check_rows_against_nets(sengine, got["rows"])
    for filt in ({"name": "s"}, {"min_hits": 4}):                                          # other sizes, other boundaries
        check_groups(sengine, ips, states, v4_bits=16, v6_bits=64, limit=65536, **filt)
    check_groups(sengine, ips, states, v4_bits=16, v6_bits=64, limit=3, min_ips=B)
    check_groups(sengine, ips, states, v4_bits=24, v6_bits=128, order=state_groups.BY_HITS, limit=50)


def test_one_group_of_every_ipv4_next_to_singletons(sengine, shape):
    """/0: every IPv4 IP in one group, five and a half blocks long; the IPv6 IPs one each; and ::/0 too."""
    ips, states = shape
    n4 = sum(G.shape_sizes())
    got = check_groups(sengine, ips, states, v4_bits=0, v6_bits=64, limit=65536)
    assert got["n_groups"] == 1 + G.N_V6_SINGLES and got["rows"][0].net == "0.0.0.0/0" and got["rows"][0].n_ips == n4
    check_rows_against_nets(sengine, got["rows"])
    got = check_groups(sengine, ips, states, v4_bits=0, v6_bits=0, order=state_groups.BY_STATES, limit=65536)
    assert [(r.net, r.n_ips) for r in got["rows"]] == [("0.0.0.0/0", n4), ("::/0", G.N_V6_SINGLES)]
    check_rows_against_nets(sengine, got["rows"])
    got = check_groups(sengine, ips, states, v4_bits=32, v6_bits=0, limit=10, min_ips=2)
    assert [r.net for r in got["rows"]] == ["::/0"] and got["n_groups"] == n4 + 1


def test_sums_that_wrap_and_starts_at_both_ends():
    ips, states = G.extreme_world()
    eng = Engine()
    try:
        eng.state_import(snapshot.build(ips, states))
        for order in G.ORDERS:
            got = check_groups(eng, ips, states, v4_bits=24, v6_bits=64, order=order, limit=10)
        rows = {r.net: r for r in got["rows"]}
        a, b, c = rows["192.0.2.0/24"], rows["198.51.100.0/24"], rows["2001:db8::/64"]
        assert a.hits_sum == state_groups.wrap64(2 * INT64_MAX + 12) == 10 and a.newest_start_ns == INT64_MIN
        assert b.hits_sum == state_groups.wrap64(2 * INT64_MIN - 1) == -1 and b.newest_start_ns == INT64_MAX
        assert c.hits_sum == INT64_MIN and got["rows"][-1] == c and c.newest_start_ns == INT64_MIN
        assert (got["n_ips_unparsed"], got["n_states_unparsed"]) == (1, 1)
        check_rows_against_nets(eng, got["rows"])
        check_groups(eng, ips, states, v4_bits=0, v6_bits=0, order=state_groups.BY_HITS, limit=10, min_start_ns=INT64_MIN + 1)
    finally:
        eng.close()


def _rows_of(target, **kw):
    out = []
    for v4_bits, v6_bits in ((24, 64), (0, 0), (32, 128)):
        for order in G.ORDERS:
            a = target.state_query_groups(v4_bits=v4_bits, v6_bits=v6_bits, order=order, limit=65536, **kw)
            out.append(({k: a[k] for k in G.COUNTS}, a["rows"]))
    return out


def test_layout_independence_and_unchanged_engine():
    """The same logical state under the debug hash mask, after a removal of part of it and after
    an expiry (dense ids again): identical rows.  The export is byte-identical around the
    queries and a following batch answers as the oracle does."""
    eng, masked = Engine(), Engine()
    try:
        masked.debug_set_ip_hash_mask(0x6)
        run = N.build_world(eng)
        other = N.build_world(masked)
        blob = eng.state_export()
        want = _rows_of(eng)
        assert _rows_of(masked) == want and eng.state_export() == blob
        ips, states = run.model.snapshot_args()
        check_groups(eng, ips, states, limit=65536)
        # part of the state goes on both sides: the survivors get new ids and slots
        run.remove(nets=["170.85.0.0/16", "2001:db8:85a3::/48"])
        other.remove(name="mid", nets=["0.0.0.0/1"])
        ips, states = run.model.snapshot_args()
        after = check_groups(eng, ips, states, limit=65536)
        assert after["n_groups"] < want[0][0]["n_groups"]
        check_groups(masked, *other.model.snapshot_args(), limit=65536, order="states")
        fresh = Engine()
        try:
            fresh.state_import(eng.state_export())
            assert _rows_of(fresh) == _rows_of(eng)
        finally:
            fresh.close()
        cut = N.NOW + 60_000_000
        pre = _rows_of(eng, min_start_ns=cut)
        assert eng.state_expire(cut)["states_dropped"] > 0
        assert _rows_of(eng) == pre
        kept_ips = H.dump_ips(eng.state_dump())
        kept = {ip: {n: v for n, v in d.items() if v[1] >= cut} for ip, d in states.items()}
        check_groups(eng, kept_ips, kept, limit=65536)
        # the engine goes on as the model says (the expiry was transparent: every window had run out)
        blob = masked.state_export()
        _rows_of(masked)
        assert masked.state_export() == blob
        other.feed(N.world_lines(N.world_ips()[::3], N.T0_MS + 500), N.NOW + 500_000_000)
        other.compare_states(dump=False)
        check_groups(masked, *other.model.snapshot_args(), limit=65536)
    finally:
        masked.debug_set_ip_hash_mask(0)
        eng.close()
        masked.close()


def test_bad_arguments_and_open_batch(wengine, world):
    import ctypes as C

    import torch
    from banjax_amd import _lib
    before = wengine.state_export()
    for kw, word in (({"v4_bits": 33}, "v4_bits"), ({"v6_bits": 129}, "v6_bits"), ({"order": 3}, "order"),
                     ({"limit": 65537}, "limit")):
        with pytest.raises(BanjaxGpuError) as ei:
            wengine.state_query_groups(**kw)
        assert ei.value.code == -2 and word in str(ei.value), (kw, str(ei.value))
    L = _lib.lib()
    f = _lib.StateFilter(_lib.Str(None, 0), _lib.Str(None, 0), INT64_MIN, INT64_MIN, INT64_MAX, 0, 0)
    g = _lib.GroupSpec(24, 64, 0, 10, 0)
    out = _lib.StateGroups()
    assert L.bjx_state_query_groups(wengine._h, C.byref(f), C.byref(g), C.byref(out)) == _lib.OK and out.n_rows == 10
    for args in ((None, C.byref(g), C.byref(out)), (C.byref(f), None, C.byref(out)), (C.byref(f), C.byref(g), None)):
        assert L.bjx_state_query_groups(wengine._h, *args) == _lib.ERR_ARG
    for bad in (_lib.StateFilter(_lib.Str(None, 0), _lib.Str(None, 0), 0, 0, 0, 2, 0),          # what bjx_state_query refuses
                _lib.StateFilter(_lib.Str(None, 0), _lib.Str(None, 0), 0, 0, 0, 0, 65537),
                _lib.StateFilter(_lib.Str(None, 3), _lib.Str(None, 0), 0, 0, 0, 0, 0),
                _lib.StateFilter(_lib.Str(None, 0), _lib.Str(None, 3), 0, 0, 0, 0, 0)):
        assert L.bjx_state_query_groups(wengine._h, C.byref(bad), C.byref(g), C.byref(out)) == _lib.ERR_ARG
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
            eng.state_query_groups()
        assert ei.value.code == -2 and "bjx_finish_batch" in str(ei.value)
        assert eng.state_dump() == dump
    finally:
        eng.close()


@pytest.mark.parametrize("n_engines", [2, 3])
def test_node_equals_single_engine(wengine, world, n_engines):
    """Groups span the engines of a node: rows and every count equal the single engine on the
    same lines, and a group reaches min_ips only in total."""
    ips, states = world
    node = Node([0] * n_engines)
    try:
        sharded = N.build_world(node)
        assert sorted(H.dump_ips(node.state_dump())) == sorted(ips)
        split = 0
        for v4_bits, v6_bits in ((24, 64), (0, 0), (32, 128), (8, 65), (31, 1)):
            for order in G.ORDERS:
                for kw in ({"limit": 65536}, {"limit": 3}, {"limit": 65536, "min_ips": 3}, {"limit": 0}, {"limit": 20, "name": "slow"},
                           {"limit": 5, "ip": "170.85.195.60"}, {"limit": 5, "ip": "1.2.3"}):
                    a = wengine.state_query_groups(v4_bits=v4_bits, v6_bits=v6_bits, order=order, **kw)
                    b = check_groups(node, ips, states, v4_bits=v4_bits, v6_bits=v6_bits, order=order, **kw)
                    assert a["rows"] == b["rows"] and {k: a[k] for k in G.COUNTS} == {k: b[k] for k in G.COUNTS}
        for v4_bits in range(1, 32):
            parts = [node.engine(k).state_query_groups(v4_bits=v4_bits, v6_bits=64, limit=65536)["rows"] for k in range(n_engines)]
            for r in node.state_query_groups(v4_bits=v4_bits, v6_bits=64, limit=65536, min_ips=3)["rows"]:
                split += all(p.n_ips < 3 for rows in parts for p in rows if p.net == r.net)
        assert split > 0      # a group below min_ips on every shard that reaches it in total
        with pytest.raises(BanjaxGpuError) as ei:
            node.state_query_groups(v6_bits=129)
        assert ei.value.code == -2
    finally:
        node.close()
