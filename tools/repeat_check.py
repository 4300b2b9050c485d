"""Is a workload's result list repeatable?

    python tools/repeat_check.py [--config cfg4] [--lines N] [--slice 200000]

Processes the workload in slices, each slice twice on one engine (the state
cleared before each pass) with the RuleResults copied back, and compares the
(line, rule) pairs of the two passes.  For every pair only one pass reported,
it prints the line's length, where it starts in its 4,096-byte scan tile,
where each literal of the ruleset occurs in it (line offset, offset in its
tile, distance from the start of rest) and what the oracle says of the rule on
that line alone.  Exit status 1 when any pair differs.

One pass over the workload is one bounded run; it is not meant to be looped
until something differs.
"""
import argparse
import ctypes as C
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
TILE = 4096


def result_pairs(out):
    """(line_idx << 20 | rule_idx) of every RuleResult of a batch, as a numpy array (copied)."""
    import numpy as np
    from banjax_amd import _lib
    if not out.n_results:
        return np.zeros(0, dtype=np.uint64)
    size = C.sizeof(_lib.RuleResult)
    dt = np.dtype({"names": ["line_idx", "rule_idx"], "formats": ["<u8", "<u4"],
                   "offsets": [_lib.RuleResult.line_idx.offset, _lib.RuleResult.rule_idx.offset], "itemsize": size})
    buf = (C.c_char * (size * out.n_results)).from_address(C.addressof(out._res.results.contents))
    a = np.frombuffer(buf, dtype=dt)
    return (a["line_idx"] << np.uint64(20)) | a["rule_idx"].astype(np.uint64)


def rule_literals(rs, i):
    from banjax_amd import _lib
    L = _lib.lib()
    n = L.bjx_debug_rule_literal(rs.handle, i, None, 0)
    buf = bytes(n)
    L.bjx_debug_rule_literal(rs.handle, i, buf, n)
    out = []
    for row in buf.split(b"\n")[1:]:
        _, ci, s = row.split(b" ", 2)
        out.append((s, b"1" in ci))
    return out


def explain(line, start, r, rule, lits, only_in):
    from oracle import oracle as O
    parts = line.split(b" ", 2)
    rest_off = len(line) - len(parts[2]) if len(parts) == 3 else len(line)
    print("  line of %d bytes at batch offset %d (%d into its tile), rest at %d; rule %d %r reported by pass %d only"
          % (len(line), start, start % TILE, rest_off, r, rule.rule, only_in))
    low = line.lower()
    for s, ci in lits:
        hay, needle = (low, s.lower()) if ci else (line, s)
        i = hay.find(needle)
        while i >= 0:
            print("    literal %r at %d: %d into its tile, %d from a tile's end, %+d from rest"
                  % (s, i, (start + i) % TILE, TILE - (start + i) % TILE, i - rest_off))
            i = hay.find(needle, i + 1)
    print("    oracle on this line alone: %s" % ("match" if O.Regex(rule.regex).match(line[rest_off:]) else "no match"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg4")
    ap.add_argument("--lines", type=int, default=0)
    ap.add_argument("--slice", type=int, default=200_000)
    args = ap.parse_args()
    import numpy as np
    import torch
    import workloads as W
    from banjax_amd import Config, Engine, Ruleset

    w0 = W.ALL[args.config]
    n_lines = args.lines or w0.n_lines
    w = W.scaled(w0, n_lines, n_ips=w0.n_ips)
    cfg = Config.from_yaml(w.rules_yaml)
    rules = cfg.all_rules()
    rs = Ruleset(cfg)
    lits = sorted({l for i in range(len(rules)) for l in rule_literals(rs, i)})
    eng = Engine(0)
    eng.set_decision_lists(cfg.decision_entries)
    n_diff = n_pairs = 0
    for first in range(0, n_lines, args.slice):
        cnt = min(args.slice, n_lines - first)
        t, nb = w.device_lines(0, first, cnt)
        torch.cuda.synchronize()
        now = w.now_ns(first, cnt)
        seen, hits = [], []
        for _ in range(2):
            eng.state_clear()
            out = eng.process(rs, None, now, copy_results=True, device_ptr=t.data_ptr(), nbytes=nb)
            seen.append(np.sort(result_pairs(out)))
            hits.append(eng.scan_stats()["literal_hits"])
        n_pairs += len(seen[0])
        diff = np.setxor1d(seen[0], seen[1])
        print("lines %d..%d: %d bytes, %d / %d results, %d / %d recorded hits, %d pairs differ"
              % (first, first + cnt, nb, len(seen[0]), len(seen[1]), hits[0], hits[1], len(diff)), flush=True)
        if len(diff):
            n_diff += len(diff)
            host = t[:nb].cpu().numpy().tobytes()
            nl = np.flatnonzero(np.frombuffer(host, dtype=np.uint8) == 10)
            for key in diff[:20]:
                j, r = int(key) >> 20, int(key) & 0xFFFFF
                s = int(nl[j - 1]) + 1 if j else 0
                explain(host[s:int(nl[j])], s, r, rules[r], lits, 1 if key in seen[0] else 2)
        del t
    print("%d of %d (line, rule) pairs differ between the two passes" % (n_diff, n_pairs))
    eng.close()
    return 1 if n_diff else 0


if __name__ == "__main__":
    sys.exit(main())
