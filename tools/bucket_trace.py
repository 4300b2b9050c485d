"""Join tools/bucket_times.py's JSON lines with the rocprofv3 kernel trace of the same run.

    python tools/bucket_trace.py times.jsonl tr_kernel_trace.csv

Every step dispatches k_bucket_apply and k_bucket_bounds once, in order, so the
k-th dispatch belongs to the k-th line.  Prints, per setting, each step's
k_bucket_apply and k_bucket_bounds kernel ms, the sort_apply phase and the step's device ms.
"""
import csv
import json
import sys
from collections import OrderedDict


def main():
    steps = [json.loads(ln) for ln in open(sys.argv[1]) if ln.startswith("{")]
    rows = sorted(csv.DictReader(open(sys.argv[2])), key=lambda r: int(r["Start_Timestamp"]))
    ms = {"k_bucket_apply": [], "k_bucket_bounds": []}
    for r in rows:
        for k in ms:
            if k in r["Kernel_Name"]:
                ms[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6)
    for k, v in ms.items():
        if len(v) != len(steps):
            sys.exit("%d dispatches of %s for %d steps" % (len(v), k, len(steps)))
    per = OrderedDict()
    for i, s in enumerate(steps):
        per.setdefault(s["setting"], []).append((ms["k_bucket_apply"][i], ms["k_bucket_bounds"][i],
                                                 s["phases"].get("sort_apply", 0.0), s["device_ms"]))
    print("%-24s %-30s %-24s %-26s %s" % ("setting", "k_bucket_apply ms", "k_bucket_bounds ms", "sort_apply ms", "device ms"))
    for name, v in per.items():
        cols = [" ".join("%.3f" % x[c] for x in v) for c in range(4)]
        print("%-24s %-30s %-24s %-26s %s" % (name, cols[0], cols[1], cols[2], cols[3]))


if __name__ == "__main__":
    main()
