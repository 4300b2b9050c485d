#!/usr/bin/env python3
"""Time bjx_state_remove on the cfg3 state next to bjx_state_expire.

    python tools/remove_bench.py [--lines N] [--runs 3] [--out profiles/<dir>/remove_cfg3.json]

One child process under `timeout` (a failure stops the run; nothing is tried
again).  It fills an engine with one cfg3 batch, exports the state once and
then, for every measurement, clears the engine, imports that snapshot and runs
one call, so every call sees the same state in the same tables (the import's:
the growth rule on what it holds).  The yardstick is the existing code in the
same process on the same state: bjx_state_expire at the cutoff that drops the
same states, alternating with the removal, `--runs` times each.

  window half / few   state_expire(cutoff) and state_remove(max_start_ns =
                      cutoff - 1) at half the batch's time span and at a cutoff
                      that drops only a handful of states
  list 1 / 100000     that many held IPs, taken at stride through the ids
  name                every state of the rule name that holds the most
  noop                one IP the engine does not hold: nothing is rebuilt
  ips_only 1 / 100000 the same lists with an empty start window: no state can
                      pass, so only the list is looked up (k_rm_ips, the clear
                      of sel[] and the sum behind ips_found) -- that part of a
                      list removal's device time on its own

device_ms is the call's own (HIP events, copies excluded), wall_ms the call as
Python sees it, the list's marshalling included.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
INT64_MIN = -(1 << 63)


def _snapshot_ips(blob, stride_count):
    """`stride_count` IPs of the snapshot at stride through its ids (numpy over the offsets alone)"""
    import numpy as np
    from banjax_amd import snapshot
    _, _, _, total, n_names, names_bytes, n_ips, ip_bytes, n_states = snapshot._HDR.unpack_from(blob)
    _, _, o_ip_off, o_ips, _, _ = snapshot.layout(n_names, names_bytes, n_ips, ip_bytes, n_states)
    off = np.frombuffer(blob, dtype="<u8", count=n_ips + 1, offset=o_ip_off)
    step = max(1, n_ips // stride_count)
    ids = range(1, n_ips, step)[:stride_count]
    return [bytes(blob[o_ips + int(off[i]):o_ips + int(off[i + 1])]) for i in ids]


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
    filled = eng.state_stats()
    blob = eng.state_export()
    span_ns = int(lines * w.us_per_line) * 1000
    cut_half = now + span_ns // 2
    # a handful: the states started in the batch's first 20 microseconds' worth of lines
    cut_few = now + max(1, int(20 * w.us_per_line)) * 1000
    ips_1 = _snapshot_ips(blob, 1)
    ips_100k = _snapshot_ips(blob, 100_000)
    names = sorted(set(r.rule for r in cfg.all_rules()))

    def restore():
        eng.state_clear()
        eng.state_import(blob)

    restore()
    imported = eng.state_stats()
    by_name = {n: eng.state_query(name=n, limit=0)["n_matched"] for n in names}
    name = max(by_name, key=by_name.get)

    def timed(call):
        restore()
        t0 = time.perf_counter()
        s = call()
        wall = (time.perf_counter() - t0) * 1000.0
        s = dict(s, wall_ms=round(wall, 3), state_slots_after=eng.state_stats()["state_slots"])
        return s

    out = {"lines": lines, "runs": runs, "filled": filled, "imported": imported, "snapshot_bytes": len(blob),
           "states_by_name": by_name, "name": name, "cutoff_half_ns": cut_half, "cutoff_few_ns": cut_few, "cases": {}}

    def case(label, calls):
        """calls: {side: callable}; the sides alternate, `runs` times each"""
        res = {k: [] for k in calls}
        for _ in range(runs):
            for k, c in calls.items():
                res[k].append(timed(c))
        out["cases"][label] = res
        print("%s: %s" % (label, {k: [round(r["device_ms"], 3) for r in v] for k, v in res.items()}), flush=True)

    case("window_half", {"expire": lambda: eng.state_expire(cut_half), "remove": lambda: eng.state_remove(max_start_ns=cut_half - 1)})
    case("window_few", {"expire": lambda: eng.state_expire(cut_few), "remove": lambda: eng.state_remove(max_start_ns=cut_few - 1)})
    case("list_1", {"remove": lambda: eng.state_remove(ips=ips_1)})
    case("list_100000", {"remove": lambda: eng.state_remove(ips=ips_100k)})
    case("name", {"remove": lambda: eng.state_remove(name=name)})
    case("noop", {"remove": lambda: eng.state_remove(ips=[b"203.0.113.254"])})
    case("ips_only_1", {"remove": lambda: eng.state_remove(ips=ips_1, min_start_ns=1, max_start_ns=0)})
    case("ips_only_100000", {"remove": lambda: eng.state_remove(ips=ips_100k, min_start_ns=1, max_start_ns=0)})
    for label in ("window_half", "window_few"):
        a, b = out["cases"][label]["expire"][0], out["cases"][label]["remove"][0]
        for k in ("states_before", "states_dropped", "ips_before", "ips_dropped", "arena_bytes_after", "device_bytes_after"):
            assert a[k] == b[k], (label, k, a, b)
    eng.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=0, help="lines of the fill batch (default: cfg3's 125M)")
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
        print("remove_bench: the child ended with status %d; stopping" % p.returncode, file=sys.stderr)
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
