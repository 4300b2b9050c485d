#!/usr/bin/env python3
"""Time bjx_state_query on the cfg3 state (55M states, 1.9M IPs), next to its
yardsticks measured in the same process: bjx_state_export(INT64_MIN), the
other read-only pass over the same tables, and one k_exp_mark pass (an export
with min_start_ns = INT64_MAX: the mark and the id scans, nothing kept).

    python tools/query_bench.py [--lines N] [--out profiles/<dir>/query_cfg3.json]

One child process under its own `timeout` (nothing is tried again): fills an
engine with one cfg3 batch, then times, `--reps` times each,
  - Get(ip) as one query against the loop of bjx_state_get over the ruleset's
    names (wall: the loop has no device time of its own),
  - top-100 by hits for one rule name, top-100 and top-65536 over all names,
    top-100 by start, and a counts-only query.
device_ms are the library's HIP-event times (copies excluded), wall_ms the C
call as the host sees it.  The state table read is state_slots * 32 B; the
candidates a scan appends are 16 B per matched state.
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
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1


def child(lines, reps):
    import ctypes as C
    import torch
    import workloads as W
    from banjax_amd import Config, Engine, Ruleset, _lib
    w = W.scaled(W.CFG3, lines, n_ips=W.CFG3.n_ips) if lines != W.CFG3.n_lines else W.CFG3
    data, nbytes = w.device_lines(0, 0, lines)
    torch.cuda.synchronize()
    cfg = Config.from_yaml(w.rules_yaml)
    rs = Ruleset(cfg)
    a = Engine(0, ip_arena_bytes=256 << 20)
    a.set_decision_lists(cfg.decision_entries)
    a.process(rs, None, w.now_ns(0, lines), device_ptr=data.data_ptr(), nbytes=nbytes, compact_trips=True)
    torch.cuda.synchronize()
    del data
    torch.cuda.empty_cache()
    tables = a.state_stats()
    names = sorted(set(r.rule for r in cfg.all_rules()))

    def timed(**q):
        dev, wall, ans = [], [], None
        for _ in range(reps):
            t = time.perf_counter()
            ans = a.state_query(**q)
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(ans["device_ms"])
        return {"device_ms": round(statistics.median(dev), 3), "device_ms_all": [round(x, 3) for x in dev],
                "wall_ms": round(statistics.median(wall), 3), "n_matched": ans["n_matched"],
                "n_ips_matched": ans["n_ips_matched"], "rows": len(ans["rows"])}, ans

    out = {}
    out["top100_all_names"], top = timed(limit=100)
    busiest_ip, top_name = top["rows"][0][0], top["rows"][0][1]
    out["top100_one_name"], _ = timed(name=top_name, limit=100)
    out["top100_one_name"]["name"] = top_name.decode(errors="replace")
    out["top65536_all_names"], _ = timed(limit=65536)
    out["top100_by_start"], _ = timed(limit=100, order=_lib.QUERY_BY_START)
    out["counts_only"], _ = timed(limit=0)
    out["get_ip_query"], got = timed(ip=busiest_ip, limit=65536)
    # the loop RegexRateLimitStates.get runs: one bjx_state_get per name of the ruleset
    loop = []
    for _ in range(reps):
        t = time.perf_counter()
        found = {n: a.state_get(busiest_ip, n) for n in names}
        loop.append((time.perf_counter() - t) * 1e3)
    found = {n: v for n, v in found.items() if v is not None}
    out["get_ip_loop"] = {"wall_ms": round(statistics.median(loop), 3), "calls": len(names), "found": len(found)}
    # (every interned name is in the ruleset here, so the two must agree)
    out["get_ip_loop"]["equals_query"] = {n.decode(errors="replace"): (h, s) for _, n, h, s in got["rows"]} == found

    # yardsticks: the whole export, and the mark pass alone (nothing kept)
    L = _lib.lib()
    cap = L.bjx_state_export_bound(a._h)
    buf = (C.c_uint8 * cap)()
    yard = {}
    for key, cutoff in (("export_everything", INT64_MIN), ("mark_pass_only", INT64_MAX)):
        n, st = C.c_uint64(0), _lib.SnapshotStats()
        t = time.perf_counter()
        rc = L.bjx_state_export(a._h, cutoff, C.cast(buf, C.c_void_p), cap, C.byref(n), C.byref(st))
        wall = (time.perf_counter() - t) * 1e3
        assert rc == 0, rc
        yard[key] = {"device_ms": round(st.device_ms, 3), "wall_ms": round(wall, 3), "states": st.states, "bytes": n.value}
    del buf
    return {"lines": lines, "reps": reps, "tables": tables, "interned_names": len(names),
            "state_table_bytes": tables["state_slots"] * 32, "candidate_buffer_bytes": tables["states"] * 16,
            "queries": out, "yardsticks": yard,
            "top100_below_export": out["top100_all_names"]["device_ms"] < yard["export_everything"]["device_ms"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=0, help="lines of the fill batch (default: cfg3's 125M)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=420, help="seconds for the child")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        import workloads as W
        print("__RESULT__ " + json.dumps(child(args.lines or W.CFG3.n_lines, args.reps)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--lines",
           str(args.lines), "--reps", str(args.reps)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    line = next((l for l in p.stdout.splitlines() if l.startswith("__RESULT__ ")), None)
    if p.returncode != 0 or line is None:
        print("query_bench: the child ended with status %d" % p.returncode, file=sys.stderr)
        return p.returncode or 1
    r = json.loads(line[len("__RESULT__ "):])
    r["workload"] = "cfg3"
    print(json.dumps(r), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
