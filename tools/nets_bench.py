#!/usr/bin/env python3
"""Time bjx_state_query_nets and bjx_state_remove_nets on the cfg3 state next
to the calls without nets.

    python tools/nets_bench.py [--lines N] [--runs 3] [--out profiles/<dir>/nets_cfg3.json]

One child process under `timeout` (a failure stops the run; nothing is tried
again).  It fills an engine with one cfg3 batch and exports the state once.
The queries run on that state as it is (they only read); before every removal
the engine is cleared and the snapshot imported, so every removal sees the same
state in the same tables.  The yardsticks are the calls the parent commit has,
in the same process on the same state:

  query_plain        a counts-only bjx_state_query, every state open
  remove_window      bjx_state_remove(max_start_ns = half the batch's span)

and beside them, with 1, 1,000 and 65,536 entries of mixed lengths:

  query_nets_<n>     a counts-only bjx_state_query_nets
  remove_nets_<n>    bjx_state_remove_nets, every state of the selected IPs

The entries are made from held IPs taken at stride through the ids: each
becomes a network of a length that cycles through /12 .. /32 (IPv4) and
/32 .. /128 (IPv6), so a list holds single addresses next to wide networks and
nests.  device_ms is the call's own (HIP events, copies excluded), wall_ms the
call as Python sees it, parsing and upload of the net table included.
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIZES = (1, 1000, 65536)
LEN4 = (24, 32, 16, 28, 20, 32, 12, 30)
LEN6 = (64, 128, 48, 96, 32, 128, 56, 112)


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


def make_nets(ips, n):
    """n entries from held IP texts (bytes): ip/len, the length by position"""
    from banjax_amd import state_nets
    out = []
    for k, ip in enumerate(ips):
        p = state_nets.parse_ip(ip)
        if p is None:
            continue
        out.append(ip + b"/%d" % (LEN4 if p[1] else LEN6)[k % 8])
        if len(out) == n:
            break
    return out


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
    cut_half = now + int(lines * w.us_per_line) * 1000 // 2
    pool = _snapshot_ips(blob, 3 * SIZES[-1])
    nets = {n: make_nets(pool[::max(1, len(pool) // (2 * n))], n) for n in SIZES}
    assert all(len(nets[n]) == n for n in SIZES), {n: len(v) for n, v in nets.items()}

    def restore():
        eng.state_clear()
        eng.state_import(blob)

    restore()
    out = {"lines": lines, "runs": runs, "imported": eng.state_stats(), "snapshot_bytes": len(blob), "cutoff_half_ns": cut_half,
           "cases": {}}

    def case(label, call, rebuild):
        res = []
        for _ in range(runs):
            if rebuild:
                restore()
            t0 = time.perf_counter()
            s = call()
            wall = (time.perf_counter() - t0) * 1000.0
            s = {k: v for k, v in s.items() if k not in ("rows", "net_ips")}
            res.append(dict(s, wall_ms=round(wall, 3)))
        out["cases"][label] = res
        print("%s: device_ms %s wall_ms %s" % (label, [round(r["device_ms"], 3) for r in res], [r["wall_ms"] for r in res]), flush=True)

    case("query_plain", lambda: eng.state_query(limit=0), False)
    for n in SIZES:
        case("query_nets_%d" % n, lambda n=n: eng.state_query(nets=nets[n], limit=0), False)
    case("remove_window", lambda: eng.state_remove(max_start_ns=cut_half - 1), True)
    for n in SIZES:
        case("remove_nets_%d" % n, lambda n=n: eng.state_remove(nets=nets[n]), True)
    for n in SIZES:  # the counts-only query previews the removal
        assert out["cases"]["query_nets_%d" % n][0]["n_matched"] == out["cases"]["remove_nets_%d" % n][0]["states_dropped"]
    best = {k: min(r["device_ms"] for r in v) for k, v in out["cases"].items()}
    out["best_device_ms"] = best
    out["ratio"] = dict({"query_nets_%d" % n: best["query_nets_%d" % n] / best["query_plain"] for n in SIZES},
                        **{"remove_nets_%d" % n: best["remove_nets_%d" % n] / best["remove_window"] for n in SIZES})
    print("ratio to the call without nets: %s" % {k: round(v, 3) for k, v in out["ratio"].items()}, flush=True)
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
        print("nets_bench: the child ended with status %d; stopping" % p.returncode, file=sys.stderr)
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
