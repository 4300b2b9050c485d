#!/usr/bin/env python3
"""Static figures of k_scan from the device assembly of engine.hip.

  hipcc <build flags> --cuda-device-only -S -o engine.s banjax_amd/csrc/engine.hip
  tools/kscan_isa.py engine.s [--dump kscan.s]

Prints, for k_scan<true> and k_scan<false>: registers, LDS and scratch from
the kernel's metadata, the static count of vector, scalar and LDS instructions,
the opcodes the pair probe must not contain (a 32-bit multiply; an add of a
literal 0, which is how an LDS base of 0 shows), and the straight-line block
that holds the filter's hash multiplies with its vector-instruction count:
that block is the pair filter of the main positions (64 positions per lane).
"""
import collections
import re
import sys


syms = {}


def kernels(path):
    cur, out = None, {}
    syms.clear()
    for line in open(path, errors="replace"):
        m = re.match(r"^(_Z\w*6k_scanILb([01])E\w*):", line)
        if m:
            cur = "k_scan<%s>" % ("true" if m.group(2) == "1" else "false")
            out[cur] = []
            syms[cur] = m.group(1)
            continue
        if cur:
            if line.startswith(".Lfunc_end"):
                cur = None
                continue
            out[cur].append(line.rstrip("\n"))
    return out


def meta(path, sym):
    txt = open(path, errors="replace").read()
    i = txt.find(".name:           " + sym)
    if i < 0:
        return {}
    a = txt.rfind("  - .agpr_count", 0, i)
    b = txt.find("  - .agpr_count", i)
    blk = txt[a:b if b > 0 else len(txt)]
    keys = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count")
    return {k: int(re.search(r"\.%s:\s+(\d+)" % k, blk).group(1)) for k in keys if re.search(r"\.%s:\s+(\d+)" % k, blk)}


def main():
    path = sys.argv[1]
    ks = kernels(path)
    if "--dump" in sys.argv:
        with open(sys.argv[sys.argv.index("--dump") + 1], "w") as f:
            for name, lines in ks.items():
                f.write("; ==== %s\n" % name)
                f.write("\n".join(lines) + "\n")
    for name, lines in ks.items():
        sym = syms[name]
        ops = collections.Counter()
        blocks, cur = [], []
        for ln in lines:
            s = ln.strip()
            if not s or s.startswith(";") or s.startswith("."):
                if re.match(r"^\.LBB\d+_\d+:", s) and cur:
                    blocks.append(cur)
                    cur = []
                continue
            op = s.split()[0]
            ops[op] += 1
            cur.append(s)
            if op.startswith("s_cbranch") or op == "s_branch":
                blocks.append(cur)
                cur = []
        if cur:
            blocks.append(cur)
        valu = sum(n for o, n in ops.items() if o.startswith("v_"))
        salu = sum(n for o, n in ops.items() if o.startswith("s_"))
        lds = sum(n for o, n in ops.items() if o.startswith("ds_"))
        vmem = sum(n for o, n in ops.items() if o.startswith(("global_", "flat_", "buffer_", "scratch_")))
        add0 = sum(1 for ln in lines if re.match(r"\s*v_add_u32(_e32)?\s+v\d+,\s*0,\s*v\d+\s*$", ln))
        # the pair filter of the main positions: the block with its 32 hash multiplies
        big = max(blocks, key=lambda b: sum(1 for s in b if s.startswith("v_mul_")))
        bv = sum(1 for s in big if s.startswith("v_"))
        bl = sum(1 for s in big if s.startswith("ds_"))
        print(name, meta(path, sym))
        print("  static: %d vector, %d scalar, %d LDS, %d vector-memory instructions" % (valu, salu, lds, vmem))
        print("  v_mul_lo_u32 %d, v_mul_u32_u24 %d, v_add_u32 of literal 0: %d" % (ops["v_mul_lo_u32"], ops["v_mul_u32_u24"] + ops["v_mul_u32_u24_e32"], add0))
        print("  pair-filter block: %d instructions, %d vector, %d LDS" % (len(big), bv, bl))
        bo = collections.Counter(s.split()[0] for s in big)
        print("   ", ", ".join("%s %d" % kv for kv in bo.most_common(14)))


if __name__ == "__main__":
    main()
