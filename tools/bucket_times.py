"""The rate-limit stage's two-level path under several settings in one process (GPU).

    python tools/bucket_times.py [workload] [lines] [reps] [setting ...]

A setting is `default` or `NAME=VALUE[,NAME=VALUE]` (BJX_WAVE_RUNS=0, BJX_WAVE_RUNS=16, ...:
the hooks the stage reads per batch).  The bench's steady state is reproduced -- the
same batch again and again into the state the step before left -- and after three
warm-up steps every setting runs `reps` steps; one JSON line per step.  Under
`rocprofv3 --kernel-trace` the k-th `k_bucket_apply` dispatch belongs to the k-th
line (tools/bucket_trace.py joins them).  Load another build of the library with
BJX_LIB_PATH (tools/build_variant.sh).
"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import workloads as W  # noqa: E402
from banjax_amd import Config, Engine, Ruleset  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "cfg3"
n = int(sys.argv[2]) if len(sys.argv) > 2 else 0
reps = int(sys.argv[3]) if len(sys.argv) > 3 else 3
settings = sys.argv[4:] or ["default"]
HOOKS = ("BJX_WAVE_RUNS", "BJX_SORT2")

w0 = W.ALL[name]
w = W.scaled(w0, n, n_ips=w0.n_ips) if n else w0
n = n or w0.n_lines
data, nbytes = w.device_lines(0, 0, n)
torch.cuda.synchronize()
cfg = Config.from_yaml(w.rules_yaml)
rs = Ruleset(cfg)
e = Engine(0, ip_arena_bytes=256 << 20)
e.set_decision_lists(cfg.decision_entries)
e.set_ban_options(cfg.expiring_decision_ttl_seconds, [h for h, v in cfg.disable_logging.items() if v])
now = w.now_ns(0, n)
for s in ["warmup"] + settings:
    for h in HOOKS:
        os.environ.pop(h, None)
    if s not in ("warmup", "default"):
        for kv in s.split(","):
            k, v = kv.split("=")
            os.environ[k] = v
    for r in range(3 if s == "warmup" else reps):
        o = e.process(rs, None, now, device_ptr=data.data_ptr(), nbytes=nbytes, compact_trips=True)
        torch.cuda.synchronize()
        print(json.dumps({"setting": s, "rep": r, "workload": name, "lines": o.n_lines, "events": o.n_events,
                          "trips": o.n_trips, "device_ms": round(o.device_ms, 3), "phases": e.phase_ms(),
                          "grouping": e.scan_stats()["grouping"]}), flush=True)
