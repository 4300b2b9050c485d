#!/usr/bin/env python3
"""Static figures of a kernel (default k_lines2<1>) from the device assembly of engine.hip.

  hipcc <build flags> --cuda-device-only -S -o engine.s banjax_amd/csrc/engine.hip
  tools/klines2_isa.py engine.s [kernel ...]

A kernel is named as the source names it (k_lines2<1>, k_scan<true>, k_dfa).
Prints per kernel: code bytes (the compiler's "codeLenInByte" comment after the
kernel's code, which is the symbol's size); registers, spills, LDS and scratch
from the metadata; static counts of vector, scalar, LDS
and vector-memory instructions; and for the main loop (the longest span between
a label and a backward branch to it): its instructions, its v_readlane /
v_writelane and s_nop counts, and the distinct (register, lane) spill slots its
lane operations use.  The assembly is read for counts only.
"""
import collections
import re
import sys


def mangled_pattern(name):
    m = re.match(r"^(\w+)(?:<(\w+)>)?$", name)
    if not m:
        sys.exit("kernel name not understood: " + name)
    base, arg = m.group(1), m.group(2)
    pat = r"_Z\w*?%d%s" % (len(base), base)
    if arg is not None:
        if arg in ("true", "false"):
            pat += r"ILb%dE" % (arg == "true")
        else:
            pat += r"ILi%sE" % arg
    return re.compile(r"^(%s\w*):" % pat)


def kernel_lines(path, name):
    pat = mangled_pattern(name)
    sym, out = None, []
    for line in open(path, errors="replace"):
        if sym is None:
            m = pat.match(line)
            if m:
                sym = m.group(1)
            continue
        if line.startswith(".Lfunc_end"):
            break
        out.append(line.rstrip("\n"))
    return sym, out


def meta(txt, sym):
    i = txt.find(".name:           " + sym + "\n")
    if i < 0:
        return {}
    a = txt.rfind("  - .agpr_count", 0, i)
    b = txt.find("  - .agpr_count", i)
    blk = txt[a:b if b > 0 else len(txt)]
    keys = ("vgpr_count", "vgpr_spill_count", "sgpr_count", "sgpr_spill_count", "group_segment_fixed_size",
            "private_segment_fixed_size")
    out = {}
    for k in keys:
        m = re.search(r"\.%s:\s+(\d+)" % k, blk)
        if m:
            out[k] = int(m.group(1))
    return out


def code_bytes(txt, sym):
    # the compiler's own resource comment block: "; codeLenInByte = N" follows the kernel's code
    i = txt.find("\n" + sym + ":")
    m = re.compile(r"; codeLenInByte = (\d+)").search(txt, i) if i >= 0 else None
    return int(m.group(1)) if m else None


def instructions(lines):
    """(index, label or None, opcode, operands) of every instruction and label."""
    out = []
    for ln in lines:
        s = ln.split(";")[0].strip()
        if not s:
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", s)
        if m:
            out.append((m.group(1), None, None))
            continue
        if s.startswith("."):
            continue
        parts = s.split(None, 1)
        out.append((None, parts[0], parts[1] if len(parts) > 1 else ""))
    return out


def main_loop(ins):
    """The longest label .. backward-branch span."""
    at = {lab: i for i, (lab, _, _) in enumerate(ins) if lab}
    best = (0, 0)
    for i, (lab, op, args) in enumerate(ins):
        if op and (op.startswith("s_cbranch") or op == "s_branch"):
            t = args.strip()
            if t in at and at[t] < i and i - at[t] > best[1] - best[0]:
                best = (at[t], i)
    return best


def counts(ins):
    ops = collections.Counter(op for _, op, _ in ins if op)
    return {
        "vector": sum(n for o, n in ops.items() if o.startswith("v_")),
        "scalar": sum(n for o, n in ops.items() if o.startswith("s_")),
        "LDS": sum(n for o, n in ops.items() if o.startswith("ds_")),
        "vector-memory": sum(n for o, n in ops.items() if o.startswith(("global_", "flat_", "buffer_", "scratch_"))),
        "v_readlane": ops["v_readlane_b32"],
        "v_writelane": ops["v_writelane_b32"],
        "s_nop": ops["s_nop"],
    }


def spill_lanes(ins):
    slots = set()
    for _, op, args in ins:
        a = [x.strip() for x in (args or "").split(",")]
        if op == "v_writelane_b32" and len(a) == 3:
            slots.add((a[0], a[2]))
        elif op == "v_readlane_b32" and len(a) == 3:
            slots.add((a[1], a[2]))
    return slots


def main():
    path = sys.argv[1]
    names = sys.argv[2:] or ["k_lines2<1>"]
    txt = open(path, errors="replace").read()
    for name in names:
        sym, lines = kernel_lines(path, name)
        if sym is None:
            sys.exit("no kernel %s in %s" % (name, path))
        ins = instructions(lines)
        c = counts(ins)
        cb = code_bytes(txt, sym)
        print("%s  code %s bytes  %s" % (name, cb if cb is not None else "?", meta(txt, sym)))
        print("  static: %(vector)d vector, %(scalar)d scalar, %(LDS)d LDS, %(vector-memory)d vector-memory instructions; "
              "%(v_readlane)d v_readlane, %(v_writelane)d v_writelane, %(s_nop)d s_nop" % c)
        a, b = main_loop(ins)
        loop = ins[a:b + 1]
        lc = counts(loop)
        print("  main loop (%d instructions): %d vector, %d scalar, %d LDS, %d vector-memory; %d v_readlane, %d v_writelane, %d s_nop"
              % (sum(1 for x in loop if x[1]), lc["vector"], lc["scalar"], lc["LDS"], lc["vector-memory"], lc["v_readlane"],
                 lc["v_writelane"], lc["s_nop"]))
        print("  distinct spill lanes: %d in the kernel, %d used in the main loop; v_writelane before the loop: %d"
              % (len(spill_lanes(ins)), len(spill_lanes(loop)), counts(ins[:a])["v_writelane"]))


if __name__ == "__main__":
    main()
