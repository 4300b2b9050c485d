"""The per-rule statistics without a GPU: the model (banjax_amd/rule_stats.py)
on hand-written RuleResults and on every golden fixture that records them, and
the boundary -- the header's declarations against the library and the ctypes
binding."""
import base64
import ctypes as C
import glob
import gzip
import json
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

from banjax_amd import Config, _lib
from banjax_amd import rule_stats as RS

HEADER = "include/banjax_gpu.h"
GOLDEN = sorted(glob.glob(os.path.join(os.path.dirname(__file__), "golden", "*.json.gz")))
NAMES = ("bjx_batch_rule_stats", "bjx_rule_stats_total", "bjx_rule_stats_reset",
         "bjx_node_batch_rule_stats", "bjx_node_rule_stats_total", "bjx_node_rule_stats_reset")


def test_count_by_hand():
    """Objects with rule_idx (the engine's records), objects with rule_id (the oracle's) and
    dicts count alike; a SkipHost result is a match and never a trip."""
    res = [SimpleNamespace(rule_idx=2, skip_host=0, exceeded=0),
           SimpleNamespace(rule_id=2, skip_host=1, exceeded=0),
           {"rule_idx": 0, "skip_host": 0, "exceeded": 1},
           {"rule_id": 2, "skip_host": False, "exceeded": True},
           SimpleNamespace(rule_idx=3, skip_host=1, exceeded=0)]
    m, s, t = RS.count(res, 5)
    assert m.dtype == s.dtype == t.dtype == np.uint64
    assert m.tolist() == [1, 0, 3, 1, 0] and s.tolist() == [0, 0, 1, 1, 0] and t.tolist() == [1, 0, 1, 0, 0]
    rows = RS.as_rows(m, s, t)
    assert rows.dtype == RS.DTYPE == np.dtype(_lib.RuleStat) and rows.itemsize == 24
    assert rows[2].tolist() == (3, 1, 1)
    assert all(x.tolist() == [0, 0] for x in RS.count([], 2))
    assert all(len(x) == 0 for x in RS.count([], 0))
    with pytest.raises(IndexError):
        RS.count(res, 3)
    with pytest.raises(AttributeError):
        RS.count([SimpleNamespace(rule=1, skip_host=0, exceeded=0)], 3)


def test_by_name_merges_rules_of_one_name():
    """State is keyed by rule name: a global rule and a site rule of one name are one line of
    the metrics; names keep the order their first rule has in the ruleset."""
    cfg = Config.from_yaml(r"""
regexes_with_rates:
  - {rule: shared, regex: 'a', interval: 1, hits_per_interval: 1, decision: challenge}
  - {rule: alone, regex: 'b', interval: 1, hits_per_interval: 1, decision: challenge}
per_site_regexes_with_rates:
  one.example.com:
    - {rule: shared, regex: 'c', interval: 1, hits_per_interval: 1, decision: challenge}
    - {rule: site only, regex: 'd', interval: 1, hits_per_interval: 1, decision: challenge}
""")
    assert [r.rule for r in cfg.all_rules()] == ["shared", "alone", "shared", "site only"]
    triple = (np.array([5, 2, 7, 0], np.uint64), np.array([1, 0, 3, 0], np.uint64), np.array([2, 1, 0, 0], np.uint64))
    want = {"shared": {"matches": 12, "skip_host": 4, "events": 8, "trips": 2},
            "alone": {"matches": 2, "skip_host": 0, "events": 2, "trips": 1},
            "site only": {"matches": 0, "skip_host": 0, "events": 0, "trips": 0}}
    assert RS.by_name(cfg, triple) == want
    assert list(RS.by_name(cfg, triple)) == ["shared", "alone", "site only"]
    assert RS.by_name(cfg, RS.as_rows(*triple)) == want
    assert RS.by_name(cfg, {"rules": RS.as_rows(*triple), "n_batches": 1}) == want
    with pytest.raises(ValueError):
        RS.by_name(cfg, RS.as_rows(*RS.count([], 3)))


@pytest.mark.parametrize("path", GOLDEN, ids=[os.path.basename(p)[:-len(".json.gz")] for p in GOLDEN])
def test_model_sums_on_golden(path):
    """Per batch of every fixture: the three arrays add up to the fixture's RuleResults, the
    ones that reached Apply, and its trips; every trip is counted under its rule."""
    with gzip.open(path, "rt", encoding="utf-8") as f:
        fx = json.load(f)
    cfg = Config.from_yaml(fx["config_yaml"])
    seen = 0
    for b in fx["batches"]:
        if "sighup_yaml" in b:
            cfg = Config.from_yaml(b["sighup_yaml"])
        if "results" not in b:
            continue
        n_rules = len(cfg.all_rules())
        res = [{"rule_id": r[1], "skip_host": r[3], "exceeded": r[6]} for r in b["results"]]
        m, s, t = RS.count(res, n_rules)
        assert int(m.sum()) == len(b["results"])
        assert int(m.sum() - s.sum()) == sum(1 for r in b["results"] if not r[3])
        assert int(t.sum()) == len(b["trips"])
        assert t.tolist() == np.bincount([tr[1] for tr in b["trips"]], minlength=n_rules).tolist()
        assert (s <= m).all() and (t <= m - s).all()
        named = RS.by_name(cfg, (m, s, t))
        assert sum(d["matches"] for d in named.values()) == len(b["results"])
        assert base64.b64decode(b["log_b64"]).count(b"\n") >= len({r[0] for r in b["results"]})
        seen += 1
    assert seen > 0, "the fixture records no RuleResults"


def test_header_library_and_binding_agree():
    text = open(HEADER).read()
    L = _lib.lib()
    for name in NAMES:
        assert re.search(r"^int %s\(bjx_(engine|node) \*\w+(, bjx_rule_stats \*out)?\);" % name, text, re.M), name
        assert name in _lib.EXPORTS and hasattr(L, name)
    assert re.search(r"\bBJX_RULE_STATS = 32\b", text) and _lib.RULE_STATS == 32
    assert re.search(r"#define BJX_ABI_VERSION 5\b", text) and L.bjx_abi_version() == 5
    # bjx_rule_stat: three uint64 in the header's order, 24 B; bjx_rule_stats: 40 B
    body = re.search(r"typedef struct bjx_rule_stat \{(.*?)\} bjx_rule_stat;", text, re.S).group(1)
    assert re.findall(r"uint64_t (\w+);", body) == ["matches", "skip_host", "trips"]
    assert [f for f, _ in _lib.RuleStat._fields_] == ["matches", "skip_host", "trips"]
    assert C.sizeof(_lib.RuleStat) == 24
    body = re.sub(r"/\*.*?\*/", "", re.search(r"typedef struct bjx_rule_stats \{(.*?)\} bjx_rule_stats;", text, re.S).group(1),
                  flags=re.S)
    assert re.findall(r"(\w+)[;,]", body) == [f for f, _ in _lib.RuleStats._fields_]
    assert C.sizeof(_lib.RuleStats) == 40
    dbg = open("include/banjax_gpu_debug.h").read()
    assert "int bjx_debug_set_rule_stats_lds(bjx_engine *e, uint32_t max_rules);" in dbg
    assert hasattr(L, "bjx_debug_set_rule_stats_lds")
    # a NULL handle or out pointer is an argument error, not a crash (no GPU needed)
    out = _lib.RuleStats()
    for pre in ("bjx_", "bjx_node_"):
        assert getattr(L, pre + "batch_rule_stats")(None, C.byref(out)) == _lib.ERR_ARG
        assert getattr(L, pre + "rule_stats_total")(None, C.byref(out)) == _lib.ERR_ARG
        assert getattr(L, pre + "rule_stats_reset")(None) == _lib.ERR_ARG
