#!/usr/bin/env python3
"""Time bjx_state_merge next to bjx_state_import of the same snapshot, in one
process on one build.

    python tools/merge_bench.py [--ips N] [--reps R] [--out profiles/<dir>/merge.json]

The engine holds N IPs with three states each; the snapshot holds N IPs with
three states each, half of them the engine's (every other shared IP with a
later window, so NEWER replaces half of the shared keys and keeps the rest).
Each repetition, on fresh default engines: import the engine's state, merge the
snapshot (device_ms, wall), export and compare with the expected bytes, then a
dry run and a repeat of the merge on the merged engine (nothing to change);
and import the snapshot into an empty engine (device_ms, wall).  The first
repetition is the warm-up and is reported apart.  device_ms are the library's
HIP-event times (copies excluded), wall_ms the call as the host sees it.

One child process under its own `timeout` (nothing is tried again).
"""
import argparse
import json
import os
import struct
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
NAMES = [b"flood", b"login", b"scan"]
T0 = 1_700_000_000 * 10 ** 9


def blob_of(ids, hits, starts):
    """The snapshot of IPs "a.b.c.d" of the ids given, each with the three
    names; hits / starts: arrays of shape (len(ids), 3)."""
    import numpy as np
    from banjax_amd import snapshot
    ips = [b"%d.%d.%d.%d" % (10 + (k >> 24), (k >> 16) & 255, (k >> 8) & 255, k & 255) for k in ids.tolist()]
    n = len(ips)
    off = np.zeros(n + 1, dtype="<u8")
    off[1:] = np.cumsum(np.fromiter((len(x) for x in ips), dtype=np.uint64, count=n))
    ipb = b"".join(ips)
    recs = np.zeros(3 * n, dtype=np.dtype([("ip", "<u4"), ("name", "<u4"), ("hits", "<i8"), ("start", "<i8")]))
    recs["ip"], recs["name"] = np.repeat(np.arange(n), 3), np.tile(np.arange(3), n)
    recs["hits"], recs["start"] = hits.reshape(-1), starts.reshape(-1)
    nb = b"".join(NAMES)
    total = snapshot.layout(3, len(nb), n, len(ipb), 3 * n)[-1]
    noff = [0]
    for x in NAMES:
        noff.append(noff[-1] + len(x))
    blob = struct.pack("<8sII6Q", snapshot.MAGIC, 1, 64, total, 3, len(nb), n, len(ipb), 3 * n) + \
        struct.pack("<4Q", *noff) + nb + b"\0" * (-len(nb) % 8) + off.tobytes() + ipb + b"\0" * (-len(ipb) % 8) + recs.tobytes()
    assert len(blob) == total
    return blob


def merged_blob(e, s, m):
    """NEWER in numpy: e, s = (ids, hits, starts); the last m IPs of e are the
    first m of s.  A shared key goes to the larger (start, hits)."""
    import numpy as np
    (e_ids, e_hits, e_starts), (s_ids, s_hits, s_starts) = e, s
    sh = slice(len(e_ids) - m, len(e_ids))
    assert (e_ids[sh] == s_ids[:m]).all()
    wins = (s_starts[:m] > e_starts[sh]) | ((s_starts[:m] == e_starts[sh]) & (s_hits[:m] > e_hits[sh]))
    hits, starts = e_hits.copy(), e_starts.copy()
    hits[sh], starts[sh] = np.where(wins, s_hits[:m], e_hits[sh]), np.where(wins, s_starts[:m], e_starts[sh])
    return blob_of(np.concatenate([e_ids, s_ids[m:]]), np.concatenate([hits, s_hits[m:]]), np.concatenate([starts, s_starts[m:]]))


def inputs(n):
    """-> (the engine's state, the snapshot, the expected export after the merge) for n IPs a side, n / 2 shared"""
    import numpy as np
    e_ids, s_ids = np.arange(n), np.arange(n // 2, n // 2 + n)
    col = np.arange(3)
    e = (e_ids, (e_ids[:, None] + col) % 7, T0 + (e_ids[:, None] % 50) * 10 ** 8 + col)
    # the snapshot's window of a shared IP: odd ids a second later (wins), even ids a second earlier (loses)
    s = (s_ids, (s_ids[:, None] + col) % 5,
         T0 + (s_ids[:, None] % 50) * 10 ** 8 + col + np.where(s_ids[:, None] % 2 == 1, 10 ** 9, -10 ** 9))
    return blob_of(*e), blob_of(*s), merged_blob(e, s, n // 2)


def child(n, reps):
    from banjax_amd import Engine, state_merge
    # the numpy restatement of the rule against the model, at a size the model takes
    small = inputs(4000)
    assert state_merge.merge(small[0], small[1])[0] == small[2]
    engine_blob, snap, want = inputs(n)

    runs = []
    for _ in range(reps + 1):
        a, b = Engine(0), Engine(0)
        try:
            a.state_import(engine_blob)
            before = a.state_stats()
            t0 = time.perf_counter()
            mg = a.state_merge(snap)
            merge_wall = (time.perf_counter() - t0) * 1e3
            assert a.state_export() == want
            assert (mg["ips_added"], mg["states_added"], mg["states_replaced"], mg["states_kept"]) == \
                (n // 2, 3 * (n // 2), 3 * (n // 4), 3 * (n // 2) - 3 * (n // 4)), mg
            dry = a.state_merge(snap, dry_run=True)
            t0 = time.perf_counter()
            again = a.state_merge(snap)
            again_wall = (time.perf_counter() - t0) * 1e3
            assert again["states_added"] == again["states_replaced"] == dry["states_added"] == 0
            t0 = time.perf_counter()
            im = b.state_import(snap)
            import_wall = (time.perf_counter() - t0) * 1e3
            runs.append({"merge_device_ms": mg["device_ms"], "merge_wall_ms": round(merge_wall, 3),
                         "merge_nothing_to_change_device_ms": again["device_ms"],
                         "merge_nothing_to_change_wall_ms": round(again_wall, 3),
                         "import_device_ms": im["device_ms"], "import_wall_ms": round(import_wall, 3),
                         "tables_before": before, "tables_after": a.state_stats(), "tables_after_import": b.state_stats()})
        finally:
            a.close()
            b.close()
    med = lambda k: sorted(r[k] for r in runs[1:])[len(runs[1:]) // 2]  # noqa: E731
    return {"engine_ips": n, "engine_states": 3 * n, "snapshot_ips": n, "snapshot_states": 3 * n, "shared_ips": n // 2,
            "snapshot_bytes": len(snap), "merge_stats": {k: v for k, v in mg.items() if k != "device_ms"},
            "median": {k: med(k) for k in ("merge_device_ms", "merge_wall_ms", "merge_nothing_to_change_device_ms",
                                           "import_device_ms", "import_wall_ms")},
            "warm_up": runs[0], "runs": runs[1:]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ips", type=int, default=1_000_000, help="IPs on each side (half of them shared)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--timeout", type=int, default=420, help="seconds for the child")
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        print("__RESULT__ " + json.dumps(child(args.ips, args.reps)), flush=True)
        return 0
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, os.path.abspath(__file__), "--child", "--ips",
           str(args.ips), "--reps", str(args.reps)]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
    line = next((l for l in p.stdout.splitlines() if l.startswith("__RESULT__ ")), None)
    if p.returncode != 0 or line is None:
        print("merge_bench: the child ended with status %d" % p.returncode, file=sys.stderr)
        return p.returncode or 1
    r = json.loads(line[len("__RESULT__ "):])
    print(json.dumps({k: r[k] for k in ("engine_ips", "snapshot_states", "median")}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
