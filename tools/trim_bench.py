#!/usr/bin/env python3
"""Time bjx_state_trim on the cfg3 state next to bjx_state_expire.

    python tools/trim_bench.py [--lines N] [--runs 3] [--out profiles/<dir>/trim_cfg3.json]

One child process under `timeout` (a failure stops the run; nothing is tried
again).  It fills an engine with one cfg3 batch and exports the state once.
Dry runs leave the state alone, so they repeat on the same tables; before every
call that rebuilds, the engine is cleared and imports that snapshot, so every
such call sees the same state in the same tables.  The yardstick is the
existing code in the same process on the same state: bjx_state_expire at the
cutoff the trim found, alternating with the trim, `--runs` times each.

  select_states / _ips / _both   dry runs with max_states / max_ips at half of
                                 what is held, and both: select_ms is the search
                                 for the cutoff, device_ms adds the mark and scans
  trim / expire                  the real trim with max_states at half, and
                                 state_expire at its cutoff
  noop                           a budget the counters meet: no pass at all

select_temp_bytes is the selection's temporary device memory for this state
(8 bytes and one bit per IP with max_ips, 128 KiB of digit counters), from the
allocation sizes in trim_select_locked.
"""
import argparse
import json
import os
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
    eng.process(rs, None, w.now_ns(0, lines), device_ptr=data.data_ptr(), nbytes=nbytes, compact_trips=True)
    torch.cuda.synchronize()
    del data
    blob = eng.state_export()

    def restore():
        eng.state_clear()
        eng.state_import(blob)

    restore()
    held = eng.state_stats()
    half_st, half_ip = held["states"] // 2, held["ips"] // 2
    out = {"lines": lines, "runs": runs, "held": held, "max_states": half_st, "max_ips": half_ip, "cases": {},
           "select_temp_bytes": {"max_states": 2 * 8192 * 8,
                                 "max_ips": 8 * (held["ips"] + 1) + 4 * (held["ips"] // 32 + 1) + 2 * 8192 * 8}}

    def timed(call, fresh):
        if fresh:
            restore()
        t0 = time.perf_counter()
        s = call()
        return dict(s, wall_ms=round((time.perf_counter() - t0) * 1000.0, 3))

    def case(label, call, fresh=False):
        res = [timed(call, fresh) for _ in range(runs)]
        out["cases"][label] = res
        print("%s: device_ms %s select_ms %s dropped %d" % (label, [round(r["device_ms"], 3) for r in res],
                                                          [round(r.get("select_ms", 0), 3) for r in res],
                                                          res[0]["states_dropped"]), flush=True)
        return res

    eng.state_trim(max_states=half_st, max_ips=half_ip, dry_run=True)  # warm: code objects, the pinned ring
    case("select_states", lambda: eng.state_trim(max_states=half_st, dry_run=True))
    case("select_ips", lambda: eng.state_trim(max_ips=half_ip, dry_run=True))
    case("select_both", lambda: eng.state_trim(max_states=half_st, max_ips=half_ip, dry_run=True))
    case("noop", lambda: eng.state_trim(max_states=held["states"], max_ips=held["ips"]))
    cutoff = out["cases"]["select_states"][0]["cutoff_ns"]
    trims, expires = [], []
    for _ in range(runs):  # alternating
        trims.append(timed(lambda: eng.state_trim(max_states=half_st), True))
        expires.append(timed(lambda: eng.state_expire(cutoff), True))
    out["cases"]["trim"], out["cases"]["expire"] = trims, expires
    print("trim: device_ms %s select_ms %s" % ([round(r["device_ms"], 3) for r in trims], [round(r["select_ms"], 3) for r in trims]))
    print("expire: device_ms %s" % [round(r["device_ms"], 3) for r in expires], flush=True)
    for k in ("states_dropped", "ips_dropped", "arena_bytes_after", "device_bytes_after"):
        assert trims[0][k] == expires[0][k], (k, trims[0], expires[0])
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
        print("trim_bench: the child ended with status %d; stopping" % p.returncode, file=sys.stderr)
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
