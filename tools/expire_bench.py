#!/usr/bin/env python3
"""Time bjx_state_expire on the cfg3 state next to the table rehash of growth.

    python tools/expire_bench.py [--lines N] [--out profiles/<dir>/expire_cfg3.json]

Runs four children, each a fresh process under its own `timeout`, one after
the other; the first that fails stops the run (nothing is tried again):

  rehash       fills an engine with one cfg3 batch, feeds the same batch again
               (the capacity prediction takes the first batch's new entries
               as the next one's, so grow_ip + grow_st rehash the full tables
               before the second batch claims anything) and once more (no
               growth).  ip_rehash_ms = the second batch's "capacity" phase
               minus the third's: the rehash at the filled occupancy of the
               tables that grew (at cfg3 the IP table only: the first batch
               sized the state table for its worst case), allocation and
               frees included.
               Then an expiry that keeps everything shrinks the state table
               to the growth rule's size for its states, and the batch after
               it grows both tables: st_rehash_ms is that batch's "capacity"
               phase minus the IP table's rehash measured before, i.e.
               grow_st alone, the same states moved by k_rehash_st.
  expire 0 / 0.5 / 0.99
               fills the same way and expires with the cutoff that far into
               the time the batch spans (0: INT64_MIN, nothing dropped; most
               states are started once, so the fraction dropped follows the
               fraction of time).  The fraction really dropped is what the
               stats say.

The bytes each pass moves are worked out from the counts (slot sizes: state
32 B, IP 32 B + 4 B first + 4 B slot cache, id arrays 8 + 4 B per IP).
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


def _fill(lines, shared=None):
    import torch
    import workloads as W
    from banjax_amd import Config, Engine, Ruleset
    w = W.scaled(W.CFG3, lines, n_ips=W.CFG3.n_ips) if lines != W.CFG3.n_lines else W.CFG3
    if shared is None:
        shared = w.device_lines(0, 0, lines)
        torch.cuda.synchronize()
    data, nbytes = shared
    cfg = Config.from_yaml(w.rules_yaml)
    rs = Ruleset(cfg)
    eng = Engine(0, ip_arena_bytes=256 << 20)
    eng.set_decision_lists(cfg.decision_entries)
    now = w.now_ns(0, lines)

    def step():
        o = eng.process(rs, None, now, device_ptr=data.data_ptr(), nbytes=nbytes, compact_trips=True)
        torch.cuda.synchronize()
        return o
    step()
    step.shared = shared
    return w, cfg, eng, step


def child_rehash(lines):
    w, cfg, eng, step = _fill(lines)
    s1 = eng.state_stats()
    step()
    grow_ms, s2 = eng.phase_ms()["capacity"], eng.state_stats()
    step()
    base_ms, s3 = eng.phase_ms()["capacity"], eng.state_stats()
    eng.close()
    # a second engine: filled, shrunk by an expiry that keeps everything, and
    # grown by the batch after it (both tables this time)
    _, _, eng, step2 = _fill(lines, step.shared)
    eng.state_expire(INT64_MIN)
    s4 = eng.state_stats()
    step2()
    st_ms, s5 = eng.phase_ms()["capacity"], eng.state_stats()
    return {"st_rehash_ms": round(st_ms - grow_ms, 3), "both_tables_rehash_ms": st_ms, "st_rehash_from_slots": s4["state_slots"],
            "st_rehash_to_slots": s5["state_slots"], "st_rehash_ip_slots": [s4["ip_slots"], s5["ip_slots"]],
            "st_rehash_bytes_read": s4["state_slots"] * 32,
            "st_rehash_bytes_written": s5["state_slots"] * 32 + s4["states"] * 32,
            "lines": lines, "filled": s1, "after_growth": s2, "tables_rehashed": s2["rehashes"] - s1["rehashes"],
            "grew_again": s3["rehashes"] - s2["rehashes"], "capacity_ms_growing": grow_ms, "capacity_ms_steady": base_ms,
            "ip_rehash_ms": round(grow_ms - base_ms, 3),
            # the table read once, every live slot written once, the new table and its side arrays cleared / copied
            "ip_rehash_bytes_read": s1["ip_slots"] * 32 + s1["ips"] * 12,
            "ip_rehash_bytes_written": s1["ips"] * 44 + s2["ip_slots"] * 40}


def child_expire(lines, q):
    w, cfg, eng, _ = _fill(lines)
    before = eng.state_stats()
    cutoff = INT64_MIN
    if q > 0:  # that far into the time the batch spans
        cutoff = w.now_ns(0, lines) + int(q * lines * w.us_per_line) * 1000
    t0 = time.perf_counter()
    s = eng.state_expire(cutoff)
    wall_ms = (time.perf_counter() - t0) * 1000.0
    after = eng.state_stats()
    kept_st, kept_ips = s["states_before"] - s["states_dropped"], s["ips_before"] - s["ips_dropped"]
    n_ips = s["ips_before"]
    passes = {
        "mark": {"read": before["state_slots"] * 32, "written": n_ips * 4},
        "lengths_and_scans": {"read": n_ips * (4 + 4) + n_ips * (4 + 8), "written": n_ips * 8 + n_ips * (4 + 8)},
        "arena": {"read": n_ips * 8 + kept_ips * 20 + s["arena_bytes_after"], "written": s["arena_bytes_after"] + kept_ips * 12},
        "state_rehash": {"read": before["state_slots"] * 32 + kept_st * 4, "written": after["state_slots"] * 32 + kept_st * 32},
        "ip_rehash": {"read": before["ip_slots"] * 32 + kept_ips * 8, "written": after["ip_slots"] * 40 + kept_ips * 32},
    }
    return {"lines": lines, "time_fraction": q, "cutoff_ns": cutoff, "stats": s, "wall_ms": round(wall_ms, 3),
            "dropped_fraction": round(s["states_dropped"] / max(1, s["states_before"]), 4),
            "tables_before": before, "tables_after": after, "pass_bytes": passes,
            "bytes_read": sum(p["read"] for p in passes.values()), "bytes_written": sum(p["written"] for p in passes.values())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=0, help="lines of the fill batch (default: cfg3's 125M)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--child", default=None)
    ap.add_argument("--fraction", type=float, default=0.0)
    args = ap.parse_args()
    if args.child:
        import workloads as W
        lines = args.lines or W.CFG3.n_lines
        r = child_rehash(lines) if args.child == "rehash" else child_expire(lines, args.fraction)
        print("__RESULT__ " + json.dumps(r), flush=True)
        return 0
    result = {"workload": "cfg3", "expire": []}
    for child, q in (("rehash", 0.0), ("expire", 0.0), ("expire", 0.5), ("expire", 0.99)):
        cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", child,
               "--fraction", str(q), "--lines", str(args.lines)]
        p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = next((l for l in p.stdout.splitlines() if l.startswith("__RESULT__ ")), None)
        if p.returncode != 0 or line is None:
            print("expire_bench: %s %.2f ended with status %d; stopping" % (child, q, p.returncode), file=sys.stderr)
            return p.returncode or 1
        r = json.loads(line[len("__RESULT__ "):])
        print("%s %.2f: %s" % (child, q, json.dumps(r)), flush=True)
        if child == "rehash":
            result["rehash"] = r
        else:
            result["expire"].append(r)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
