#!/usr/bin/env python3
"""Time bjx_state_export / bjx_state_import on the cfg3 state, next to their
two yardsticks measured in the same process: bjx_state_expire(INT64_MIN), a
rebuild of the same tables, and the snapshot's bytes at the pinned D2H rate.

    python tools/snapshot_bench.py [--lines N] [--out profiles/<dir>/snapshot_cfg3.json]

One child process under its own `timeout` (nothing is tried again):
fills an engine with one cfg3 batch, exports everything, imports the blob into
a second default engine, exports that again (the bytes must be equal), then
runs the keep-everything expiry on the first engine and times pinned D2H copies
of 256 MB.  device_ms are the library's HIP-event times (copies excluded),
wall_ms the C call as the host sees it (the export's other host steps -- the
bound, the caller's buffer, the copy into a Python bytes -- are timed apart).

The bytes each call moves are worked out from the counts (slot sizes: state
32 B, IP 32 B + 4 B first + 4 B slot cache, id arrays 8 + 4 B per IP, sort
pairs 8 + 4 B, payload 16 B, record 24 B).
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


def _d2h_gbs():
    import torch
    n = 256 << 20
    d = torch.empty(n, dtype=torch.uint8, device="cuda")
    h = torch.empty(n, dtype=torch.uint8, pin_memory=True)
    h.copy_(d, non_blocking=True)
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(5):
        h.copy_(d, non_blocking=True)
    torch.cuda.synchronize()
    return n / ((time.perf_counter() - t) / 5) / 1e9


def child(lines):
    import torch
    import workloads as W
    from banjax_amd import Config, Engine, Ruleset
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
    before = a.state_stats()

    # the export through the C ABI, its host-side steps timed apart: the bound,
    # the caller's buffer (allocated and touched), the call, the copy into bytes
    import ctypes as C
    from banjax_amd import _lib
    L = _lib.lib()
    t0 = time.perf_counter()
    cap = L.bjx_state_export_bound(a._h)
    t1 = time.perf_counter()
    buf = (C.c_uint8 * cap)()
    t2 = time.perf_counter()
    n, st = C.c_uint64(0), _lib.SnapshotStats()
    rc = L.bjx_state_export(a._h, INT64_MIN, C.cast(buf, C.c_void_p), cap, C.byref(n), C.byref(st))
    t3 = time.perf_counter()
    assert rc == 0, rc
    blob = bytes(memoryview(buf)[:n.value])
    t4 = time.perf_counter()
    del buf
    export_wall = (t3 - t2) * 1e3
    export_parts = {"bound_ms": round((t1 - t0) * 1e3, 3), "caller_buffer_ms": round((t2 - t1) * 1e3, 3),
                    "call_ms": round(export_wall, 3), "copy_to_bytes_ms": round((t4 - t3) * 1e3, 3)}
    ex = {k: getattr(st, k) for k, _ in _lib.SnapshotStats._fields_}
    b = Engine(0)
    t0 = time.perf_counter()
    im = b.state_import(blob)
    import_wall = (time.perf_counter() - t0) * 1e3
    after = b.state_stats()
    same = b.state_export() == blob
    b.close()
    t0 = time.perf_counter()
    xp = a.state_expire(INT64_MIN)
    expire_wall = (time.perf_counter() - t0) * 1e3
    gbs = _d2h_gbs()

    n_ips, n_st = ex["ips"], ex["states"]
    ip_bytes = before["arena_bytes"]
    body = 8 * (n_ips + 1) + ip_bytes + 24 * n_st
    sort_passes = (24 + max(1, n_ips.bit_length()) + 7) // 8
    export_bytes = {
        "mark": {"read": before["state_slots"] * 32, "written": n_ips * 4},
        "lengths_and_scans": {"read": n_ips * 8 + n_ips * 12, "written": n_ips * 8 + n_ips * 12},
        "compact": {"read": before["state_slots"] * 32 + n_st * 4, "written": n_st * (8 + 4 + 16)},
        "remap": {"read": n_st * 8, "written": n_st * 8},
        # the radix sort's passes of 8 bits over the key bits in use (24 + bits(n_ips))
        "sort": {"read": n_st * 12 * sort_passes, "written": n_st * 12 * sort_passes},
        "gather": {"read": n_st * (12 + 16), "written": n_st * 24},
        "ips": {"read": n_ips * 20 + ip_bytes, "written": n_ips * 8 + ip_bytes},
    }
    import_bytes = {
        "check": {"read": n_ips * 8 + n_st * 8, "written": 0},
        "hash_and_scans": {"read": n_ips * 8 + ip_bytes + n_ips * 24, "written": n_ips * 20 + n_ips * 12},
        "count": {"read": n_st * 12, "written": 0},
        "clear": {"read": 0, "written": after["ip_slots"] * 40 + after["state_slots"] * 32},
        "place": {"read": n_ips * 28 + ip_bytes, "written": ip_bytes + n_ips * (12 + 32)},
        "states": {"read": n_st * (24 + 8), "written": n_st * 32},
        "verify": {"read": n_ips * (28 + 32) + ip_bytes, "written": 0},
    }
    tot = lambda p: (sum(x["read"] for x in p.values()), sum(x["written"] for x in p.values()))  # noqa: E731
    return {"lines": lines, "tables": before, "tables_after_import": after, "round_trip_equal": same,
            "snapshot_bytes": len(blob), "body_bytes": body,
            "export": {"device_ms": ex["device_ms"], "wall_ms": round(export_wall, 3), "host_steps": export_parts, "stats": ex,
                       "sort_passes": sort_passes, "pass_bytes": export_bytes,
                       "bytes_read": tot(export_bytes)[0], "bytes_written": tot(export_bytes)[1]},
            "import": {"device_ms": im["device_ms"], "wall_ms": round(import_wall, 3), "stats": im, "pass_bytes": import_bytes,
                       "bytes_read": tot(import_bytes)[0], "bytes_written": tot(import_bytes)[1]},
            "expire_keep_all": {"device_ms": xp["device_ms"], "wall_ms": round(expire_wall, 3)},
            "pinned_d2h_gb_per_s": round(gbs, 2), "snapshot_at_d2h_rate_ms": round(len(blob) / gbs / 1e6, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lines", type=int, default=0, help="lines of the fill batch (default: cfg3's 125M)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=420, help="seconds for the child")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        import workloads as W
        print("__RESULT__ " + json.dumps(child(args.lines or W.CFG3.n_lines)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--lines",
           str(args.lines)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    line = next((l for l in p.stdout.splitlines() if l.startswith("__RESULT__ ")), None)
    if p.returncode != 0 or line is None:
        print("snapshot_bench: the child ended with status %d" % p.returncode, file=sys.stderr)
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
