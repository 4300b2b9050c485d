"""CPU-side checks of the state expiry surface (no GPU): the trip-transparent
cutoff (expire_cutoff_ns: now - 10 s - the longest interval of the config,
saturating) and the two C-ABI entry points (exported, NULL handles refused
before any device call)."""
import ctypes as C

from banjax_amd import Config, _lib, expire_cutoff_ns
from banjax_amd.config import RegexWithRate

S = 1_000_000_000
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
NOW = 1_700_000_000 * S


def _rule(name, interval_ns):
    return RegexWithRate(rule=name, regex="x", interval=interval_ns, hits_per_interval=1, decision=2)


def _cfg(global_ivs=(), site_ivs=None):
    c = Config()
    c.regexes_with_rates = [_rule("g%d" % k, iv) for k, iv in enumerate(global_ivs)]
    for host, ivs in (site_ivs or {}).items():
        c.per_site_regexes_with_rates[host] = [_rule("%s%d" % (host, k), iv) for k, iv in enumerate(ivs)]
    return c


def test_cutoff_takes_the_longest_interval_over_global_and_site_rules():
    assert expire_cutoff_ns(NOW, _cfg([1 * S, 60 * S, 5 * S])) == NOW - 10 * S - 60 * S
    # the longest interval belongs to a per-site rule
    assert expire_cutoff_ns(NOW, _cfg([1 * S, 60 * S], {"a.com": [5 * S], "b.com": [300 * S, 2 * S]})) == NOW - 310 * S
    # ... or to a global one while sites have shorter ones
    assert expire_cutoff_ns(NOW, _cfg([600 * S], {"a.com": [5 * S]})) == NOW - 610 * S


def test_cutoff_from_yaml_config():
    cfg = Config.from_yaml("""
regexes_with_rates:
  - {rule: a, regex: 'GET', interval: 1.5, hits_per_interval: 0, decision: challenge}
per_site_regexes_with_rates:
  s.com:
    - {rule: a, regex: 'POST', interval: 45, hits_per_interval: 3, decision: nginx_block}
""")
    assert expire_cutoff_ns(NOW, cfg) == NOW - 55 * S


def test_cutoff_without_rules_is_the_old_line_horizon():
    assert expire_cutoff_ns(NOW, _cfg()) == NOW - 10 * S
    assert expire_cutoff_ns(NOW, Config()) == NOW - 10 * S


def test_zero_and_negative_intervals_count_as_zero():
    # every later event of such a rule is OutsideInterval whatever the state's start
    assert expire_cutoff_ns(NOW, _cfg([0])) == NOW - 10 * S
    assert expire_cutoff_ns(NOW, _cfg([-5 * S], {"a.com": [INT64_MIN]})) == NOW - 10 * S
    assert expire_cutoff_ns(NOW, _cfg([-5 * S, 3 * S])) == NOW - 13 * S


def test_cutoff_saturates_at_int64_min():
    assert expire_cutoff_ns(5 * S, _cfg([INT64_MAX])) == INT64_MIN      # a huge interval, an early clock
    assert expire_cutoff_ns(0, _cfg([INT64_MAX - 5 * S])) == INT64_MIN
    assert expire_cutoff_ns(NOW, _cfg([INT64_MAX])) == NOW - 10 * S - INT64_MAX  # fits: no saturation
    assert expire_cutoff_ns(INT64_MIN + 3 * S, _cfg([1 * S])) == INT64_MIN  # a small now_ns
    assert expire_cutoff_ns(INT64_MIN + 11 * S, _cfg([1 * S])) == INT64_MIN
    assert expire_cutoff_ns(INT64_MIN + 12 * S, _cfg([1 * S])) == INT64_MIN + 1 * S  # the first value that fits
    for now, ivs in ((NOW, [INT64_MAX]), (INT64_MIN, []), (INT64_MAX, [0]), (5, [7 * S])):
        assert INT64_MIN <= expire_cutoff_ns(now, _cfg(ivs)) <= INT64_MAX


def test_library_exports_and_refuses_null_handles():
    L = _lib.lib()
    for name in ("bjx_state_expire", "bjx_node_state_expire"):
        assert name in _lib.EXPORTS and hasattr(L, name), name
    st = _lib.ExpireStats()
    assert C.sizeof(st) == 9 * 8
    assert L.bjx_state_expire(None, 0, C.byref(st)) == _lib.ERR_ARG
    assert L.bjx_state_expire(None, INT64_MAX, None) == _lib.ERR_ARG
    assert L.bjx_node_state_expire(None, 0, C.byref(st)) == _lib.ERR_ARG
    assert L.bjx_node_state_expire(None, INT64_MIN, None) == _lib.ERR_ARG
