#!/usr/bin/env python3
"""Time bjx_state_query_names on the cfg3 state next to its two yardsticks.

    python tools/names_bench.py [--lines N] [--runs 3] [--out profiles/state_names/names_cfg3.json]

One child process under `timeout` (a failure stops the run; nothing is tried
again).  It fills an engine with one cfg3 batch, exports the state and imports
it into the cleared engine, as tools/groups_bench.py does before its cases;
every call after that only reads the state.  The yardsticks are calls the
parent commit has, in the same process on the same state:

  query_plain        a counts-only bjx_state_query, every state open: the same
                     one read of the state table (k_qry_scan)
  groups_24_64       bjx_state_query_groups at (24, 64), limit 100: the other
                     scan with atomics per state (k_grp_scan)

and beside them:

  names_all          every name by states, limit 65536 (the LDS path at cfg3's
                     1,006 names)
  names_one          one name through f->name (the name with the most states)
  names_min_hits     a min_hits filter (min_hits = 2)
  names_all_global   names_all with the global path forced through
                     bjx_debug_set_names(1, 0)
  names_all_g2048    names_all on the LDS path with the grid cap raised to 2048
                     blocks (the default is one block per CU)

Every case runs once unrecorded (the warm-up) and then --runs times; all runs
are kept, and the summary gives the lowest, the median and the highest
device_ms and the ratio of the medians to both yardsticks.  device_ms is the
call's own (HIP events, copies excluded), wall_ms the call as Python sees it.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def child(lines, runs):
    import torch
    import workloads as W
    from banjax_amd import Config, Engine, Ruleset
    w = W.scaled(W.CFG3, lines, n_ips=W.CFG3.n_ips) if lines != W.CFG3.n_lines else W.CFG3
    data, nbytes = w.device_lines(0, 0, lines)
    torch.cuda.synchronize()
    cfg = Config.from_yaml(w.rules_yaml)
    rs = Ruleset(cfg)
    eng = Engine(0, ip_arena_bytes=256 << 20)
    eng.set_decision_lists(cfg.decision_entries)
    now = w.now_ns(0, lines)
    eng.process(rs, None, now, device_ptr=data.data_ptr(), nbytes=nbytes, compact_trips=True)
    torch.cuda.synchronize()
    del data
    blob = eng.state_export()
    eng.state_clear()
    eng.state_import(blob)
    del blob
    out = {"lines": lines, "runs": runs, "held": eng.state_stats(), "lds_names_max": eng.debug_names_info()[1], "cases": {}}

    def case(label, call):
        call()                                    # the warm-up, not recorded
        res = []
        for _ in range(runs):
            t0 = time.perf_counter()
            s = call()
            wall = (time.perf_counter() - t0) * 1000.0
            top = [(r.name.decode("latin-1"), r.n_states, r.hits_sum, r.max_hits) for r in s["rows"][:3]] \
                if s.get("rows") and hasattr(s["rows"][0], "hist") else []
            s = {k: v for k, v in s.items() if k != "rows"}
            res.append(dict(s, wall_ms=round(wall, 3), top=top))
        if label.startswith("names"):
            res[0]["path"] = eng.debug_names_info()[0]
        out["cases"][label] = res
        print("%s: device_ms %s wall_ms %s" % (label, [round(r["device_ms"], 3) for r in res], [r["wall_ms"] for r in res]), flush=True)

    case("query_plain", lambda: eng.state_query(limit=0))
    case("groups_24_64", lambda: eng.state_query_groups(v4_bits=24, v6_bits=64, order="ips", limit=100))
    case("names_all", lambda: eng.state_query_names(order="states", limit=65536))
    biggest = eng.state_query_names(order="states", limit=1)["rows"][0].name
    case("names_one", lambda: eng.state_query_names(name=biggest, limit=65536))
    case("names_min_hits", lambda: eng.state_query_names(min_hits=2, limit=65536))
    eng.debug_set_names(1, 0)
    case("names_all_global", lambda: eng.state_query_names(order="states", limit=65536))
    eng.debug_set_names(0, 2048)
    case("names_all_g2048", lambda: eng.state_query_names(order="states", limit=65536))
    eng.debug_set_names(0, 0)
    plain = out["cases"]["query_plain"][0]
    for label in ("groups_24_64", "names_all", "names_all_global", "names_all_g2048"):
        res = out["cases"][label]
        assert (res[0]["n_matched"], res[0]["n_ips_matched"]) == (plain["n_matched"], plain["n_ips_matched"]), label
    assert out["cases"]["names_all_global"][0]["path"] == "global" and out["cases"]["names_all"][0]["path"] == "lds"
    summary = {}
    for label, res in out["cases"].items():
        ms = sorted(r["device_ms"] for r in res)
        summary[label] = {"min": ms[0], "median": statistics.median(ms), "max": ms[-1]}
    for label, s in summary.items():
        s["ratio_to_query_plain"] = s["median"] / summary["query_plain"]["median"]
        s["ratio_to_groups_24_64"] = s["median"] / summary["groups_24_64"]["median"]
    out["device_ms"] = summary
    print("median device_ms, its ratio to query_plain and to groups_24_64: %s"
          % {k: (round(v["median"], 3), round(v["ratio_to_query_plain"], 2), round(v["ratio_to_groups_24_64"], 2))
             for k, v in summary.items()}, flush=True)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=0, help="lines of the fill batch (default: cfg3's)")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=420, help="seconds for the child")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        import workloads as W
        r = child(args.lines or W.CFG3.n_lines, args.runs)
        print("__RESULT__ " + json.dumps(r), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--lines",
           str(args.lines), "--runs", str(args.runs)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    line = next((l for l in p.stdout.splitlines() if l.startswith("__RESULT__ ")), None)
    for l in p.stdout.splitlines():
        if not l.startswith("__RESULT__ "):
            print(l, flush=True)
    if p.returncode != 0 or line is None:
        print("names_bench: the child ended with status %d; stopping" % p.returncode, file=sys.stderr)
        return p.returncode or 1
    result = dict(json.loads(line[len("__RESULT__ "):]), workload="cfg3")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
