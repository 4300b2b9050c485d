#!/usr/bin/env python3
"""Time the per-rule counting of BJX_RULE_STATS batches next to its yardstick,
the emit phase of the same batches.

    python tools/rule_stats_bench.py [--out profiles/rule_stats] [--parent-root DIR] [--shapes cfg3:20000000,...]

Per shape two child processes, each under its own `timeout` (nothing is tried
again): one runs the batch `--reps` times with the flag and records the stats
call's device_ms (HIP events around the counting alone) and the batch's
device_ms; the other runs the same batches without the flag and records
phase_ms()["emit"] (k_emit walks the same masks and also writes 8-12 B per
event) and the batch's device_ms.  --parent-root: a checkout of the parent
commit, with its own library, for the second child (k_emit is the same code in
both; without it the child runs this tree).  Every step repeats the same batch
with the same clock, as bench.py does; the first `--warmup` steps are dropped
(the first fills empty tables).  Medians are reported.

Writes <out>/rule_stats.json and <out>/summary.md.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = "cfg3:20000000,cfg3:125000000,cfg2:20000000,cfg2k:5000000,cfg5:20000000,cfg5:100000000"


def child(root, config, lines, reps, warmup, flag):
    sys.path.insert(0, root)
    import torch
    import workloads as W
    from banjax_amd import Config, Engine, Ruleset
    w0 = W.ALL[config]
    w = W.scaled(w0, lines, n_ips=w0.n_ips) if lines != w0.n_lines else w0
    data, nbytes = w.device_lines(0, 0, lines)
    torch.cuda.synchronize()
    cfg = Config.from_yaml(w.rules_yaml)
    rs = Ruleset(cfg)
    eng = Engine(0, ip_arena_bytes=256 << 20)
    eng.set_decision_lists(cfg.decision_entries)
    eng.set_ban_options(cfg.expiring_decision_ttl_seconds, [h for h, v in cfg.disable_logging.items() if v])
    now = w.now_ns(0, lines)
    kw = {"rule_stats": True} if flag else {}
    steps = []
    for k in range(warmup + reps):
        out = eng.process(rs, None, now, device_ptr=data.data_ptr(), nbytes=nbytes, compact_trips=True, **kw)
        ph = eng.phase_ms()
        rec = {"batch_device_ms": out.device_ms, "emit_ms": ph["emit"], "trips_phase_ms": ph["trips"], "n_trips": out.n_trips,
               "n_results": out.n_results, "n_events": out.n_events, "n_lines": out.n_lines}
        if flag:
            st = eng.rule_stats()
            rec["stats_ms"] = st["device_ms"]
            rows = st["rules"]
            rec["rules"] = len(rows)
            rec["rules_matched"] = int((rows["matches"] != 0).sum())
            rec["busiest_rule_matches"] = int(rows["matches"].max()) if len(rows) else 0
            rec["busiest_rule_trips"] = int(rows["trips"].max()) if len(rows) else 0
        if k >= warmup:
            steps.append(rec)
    med = lambda key: round(statistics.median(s[key] for s in steps), 3)  # noqa: E731
    r = {"config": config, "lines": lines, "reps": reps, "warmup": warmup, "flag": flag, "root": os.path.basename(root),
         "line_kernel": eng.line_kernel()[0], "batch_device_ms": med("batch_device_ms"), "emit_ms": med("emit_ms"),
         "trips_phase_ms": med("trips_phase_ms"), "last": steps[-1]}
    if flag:
        r["stats_ms"] = med("stats_ms")
        r["stats_ms_all"] = [round(s["stats_ms"], 3) for s in steps]
    else:
        r["emit_ms_all"] = [round(s["emit_ms"], 3) for s in steps]
    return r


def run_child(args, root, config, lines, flag):
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--root", root,
           "--config", config, "--lines", str(lines), "--reps", str(args.reps), "--warmup", str(args.warmup)]
    if flag:
        cmd.append("--flag")
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    line = next((ln for ln in p.stdout.splitlines() if ln.startswith("__RESULT__ ")), None)
    if p.returncode != 0 or line is None:
        print("rule_stats_bench: the child for %s:%d (flag %s) ended with status %d" % (config, lines, flag, p.returncode),
              file=sys.stderr)
        return None, p.returncode or 1
    return json.loads(line[len("__RESULT__ "):]), 0


def summary(rows, parent):
    out = ["# Per-rule statistics: the cost of a `BJX_RULE_STATS` batch", "",
           "One MI355X, `tools/rule_stats_bench.py` (`rule_stats.json`): per shape the same batch repeated, medians of the",
           "steps after the warm-up.  `stats` is `bjx_batch_rule_stats`' `device_ms` (HIP events around the zeroing, `k_rule_hist`",
           "and `k_rule_hist_trips`); the yardstick `emit` is `phase_ms()[\"emit\"]` of the same batches run without the flag on",
           ("the parent commit's library" if parent else "this tree's library (k_emit is unchanged)") + ".", "",
           "| shape | lines | line kernel | rules (matched) | results | trips | stats ms | emit ms | stats / emit | "
           "batch ms with flag | batch ms without |", "|---|---|---|---|---|---|---|---|---|---|---|"]
    for on, off in rows:
        last = on["last"]
        out.append("| %s | %s | %s | %d (%d) | %s | %s | %.3f | %.3f | %.2f | %.3f | %.3f |" % (
            on["config"], format(on["lines"], ","), on["line_kernel"], last["rules"], last["rules_matched"],
            format(last["n_results"], ","), format(last["n_trips"], ","), on["stats_ms"], off["emit_ms"],
            on["stats_ms"] / off["emit_ms"] if off["emit_ms"] else float("nan"), on["batch_device_ms"], off["batch_device_ms"]))
    return "\n".join(out) + "\n"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rule_stats"))
    ap.add_argument("--parent-root", default=None, help="checkout of the parent commit with its own library")
    ap.add_argument("--shapes", default=SHAPES, help="config:lines,...")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per child")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--config", default="cfg3")
    ap.add_argument("--lines", type=int, default=0)
    ap.add_argument("--flag", action="store_true")
    args = ap.parse_args()
    if args.child:
        print("__RESULT__ " + json.dumps(child(os.path.abspath(args.root), args.config, args.lines, args.reps, args.warmup,
                                                 args.flag)), flush=True)
        return 0
    rows = []
    for shape in args.shapes.split(","):
        config, lines = shape.split(":")
        on, rc = run_child(args, ROOT, config, int(lines), True)
        if rc:
            return rc  # a child that failed or hung: nothing more is started
        off, rc = run_child(args, os.path.abspath(args.parent_root) if args.parent_root else ROOT, config, int(lines), False)
        if rc:
            return rc
        rows.append((on, off))
        print(json.dumps({"shape": shape, "stats_ms": on["stats_ms"], "emit_ms": off["emit_ms"]}), flush=True)
        os.makedirs(args.out, exist_ok=True)
        with open(os.path.join(args.out, "rule_stats.json"), "w") as f:
            json.dump({"parent_library": bool(args.parent_root), "shapes": [{"with_flag": a, "without_flag": b} for a, b in rows]},
                      f, indent=1)
            f.write("\n")
        with open(os.path.join(args.out, "summary.md"), "w") as f:
            f.write(summary(rows, bool(args.parent_root)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
