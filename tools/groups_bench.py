#!/usr/bin/env python3
"""Time bjx_state_query_groups on the cfg3 state next to the counts-only query.

    python tools/groups_bench.py [--lines N] [--runs 3] [--out profiles/<dir>/groups_cfg3.json]

One child process under `timeout` (a failure stops the run; nothing is tried
again).  It fills an engine with one cfg3 batch, exports the state and imports
it into the cleared engine, as tools/nets_bench.py does before its cases; every
call after that only reads the state.  The yardstick is a call the
parent commit has, in the same process on the same state:

  query_plain            a counts-only bjx_state_query, every state open

and beside it, for (v4_bits, v6_bits) = (0, 0), (24, 64) and (32, 128), the
first 100 rows by IPs and by hits:

  groups_<v4>_<v6>_ips   bjx_state_query_groups, order BJX_GROUPS_BY_IPS
  groups_<v4>_<v6>_hits  bjx_state_query_groups, order BJX_GROUPS_BY_HITS

Every case runs once unrecorded (the warm-up: hipcub's temporary buffer grows
on first use) and then --runs times; all runs are kept, and the summary gives
the lowest, the median and the highest device_ms and the ratio of the medians
to the yardstick's.  device_ms is the call's own (HIP events, copies
excluded), wall_ms the call as Python sees it.

For the per-kernel split run the child itself under the profiler:

    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/groups_bench.py --child --runs 1
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

PAIRS = ((0, 0), (24, 64), (32, 128))
ORDERS = ("ips", "hits")


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
    blob = eng.state_export()            # the state as tools/nets_bench.py times it: the snapshot imported into a cleared engine
    eng.state_clear()
    eng.state_import(blob)
    del blob
    out = {"lines": lines, "runs": runs, "held": eng.state_stats(), "cases": {}}

    def case(label, call):
        call()                                    # the warm-up, not recorded
        res = []
        for _ in range(runs):
            t0 = time.perf_counter()
            s = call()
            wall = (time.perf_counter() - t0) * 1000.0
            top = [(r.net, r.n_ips, r.n_states, r.hits_sum) for r in s["rows"][:3]] if s.get("rows") and hasattr(s["rows"][0], "net") else []
            s = {k: v for k, v in s.items() if k != "rows"}
            res.append(dict(s, wall_ms=round(wall, 3), top=top))
        out["cases"][label] = res
        print("%s: device_ms %s wall_ms %s" % (label, [round(r["device_ms"], 3) for r in res], [r["wall_ms"] for r in res]), flush=True)

    case("query_plain", lambda: eng.state_query(limit=0))
    for v4, v6 in PAIRS:
        for order in ORDERS:
            case("groups_%d_%d_%s" % (v4, v6, order),
                 lambda v4=v4, v6=v6, order=order: eng.state_query_groups(v4_bits=v4, v6_bits=v6, order=order, limit=100))
    plain = out["cases"]["query_plain"][0]
    for label, res in out["cases"].items():
        assert (res[0]["n_matched"], res[0]["n_ips_matched"]) == (plain["n_matched"], plain["n_ips_matched"]), label
    summary = {}
    for label, res in out["cases"].items():
        ms = sorted(r["device_ms"] for r in res)
        summary[label] = {"min": ms[0], "median": statistics.median(ms), "max": ms[-1]}
    for label, s in summary.items():
        s["ratio_to_query_plain"] = s["median"] / summary["query_plain"]["median"]
    out["device_ms"] = summary
    print("median device_ms and its ratio to query_plain: %s"
          % {k: (round(v["median"], 3), round(v["ratio_to_query_plain"], 2)) for k, v in summary.items()}, flush=True)
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
        print("groups_bench: the child ended with status %d; stopping" % p.returncode, file=sys.stderr)
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
