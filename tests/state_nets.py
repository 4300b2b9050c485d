"""Shared by tests/test_state_nets_cpu.py and tests/test_gpu_state_nets.py (not
collected): the held IPs, the net lists and the expected values of
bjx_state_query_nets / bjx_state_remove_nets.

State is built by feeding lines whose second field is the IP text, through
tests/state_remove.Run (the oracle says which (line, rule) pairs are events, a
restatement of Apply replays them).  Expected answers come from the pure-Python
models: banjax_amd.state_query.select and banjax_amd.state_remove.remove with
nets=, which read entries and membership from banjax_amd.state_nets.

Every net list a test uses is registered in LISTS with the world of held IPs it
is used on; tests/test_state_nets_cpu.py shows with the models alone that each
selects some held IPs and not all, whole IPs, and parts of IPs under a name
filter."""
import struct

from tests import header_fields as HF
from tests import state_remove as H

T0_MS = H.T0_MS
NOW = T0_MS * 1_000_000
NETS_MAX = 65536

BASE4 = bytes([170, 85, 195, 60])
BASE6 = bytes.fromhex("20010db885a3c55aaa55c33c0ff1ce5a")
LEN4 = (0, 1, 7, 8, 9, 31, 32)
LEN6 = (0, 1, 63, 64, 65, 127, 128)


def t4(b4: bytes) -> str:
    return "%d.%d.%d.%d" % tuple(b4)


def t6(b16: bytes) -> str:
    return HF._compress(struct.unpack(">8H", b16))


def around(raw: bytes, n: int):
    """Addresses at the edges of raw/n: the address, the first and last inside,
    the ones just below and above the network, and the address with its last
    masked bit (outside) and its first unmasked bit (inside) flipped."""
    w = len(raw) * 8
    host = (1 << (w - n)) - 1
    lo = int.from_bytes(raw, "big") & ~host
    hi = lo | host
    out = [raw, lo.to_bytes(len(raw), "big"), HF._last_inside(raw, n)]
    if n > 0:
        out.append(HF._flip(raw, n - 1))
    if n < w:
        out.append(HF._flip(raw, n))
    if lo > 0:
        out.append((lo - 1).to_bytes(len(raw), "big"))
    if hi < (1 << w) - 1:
        out.append((hi + 1).to_bytes(len(raw), "big"))
    return out


# texts that net.ParseIP refuses: members of no network
NOT_ADDRESSES = ["01.2.3.4", "1.2.3", "1.2.3.4%eth0", "", "fe80::1%eth0", "x" * 16, ("1:2:3:4:5:6:7:8:9:a:b:c:d:e:f:" * 2)[:46],
                 "170.85.195.60." + "1" * 50, ("abcd:" * 60)[:300], "170.85.195.060", "170.85.195.60/32"]
assert [len(x) for x in NOT_ADDRESSES[5:9]] == [16, 46, 64, 300]

# one /24 per index: 20.0.0.0 + (2 i + 1) * 256, so the even /24s lie between neighbours
SIZE_N = (1, 2, 3, 255, 256, 257)
SIZE_AT = (0, 1, 2, 127, 254, 255, 256)


def size_net(i: int) -> str:
    return t4((0x14000000 + ((2 * i + 1) << 8)).to_bytes(4, "big")) + "/24"


def size_ips():
    out = ["20.0.0.255"]                                   # below the first network
    for i in SIZE_AT:
        v = 0x14000000 + ((2 * i + 1) << 8)
        out += [t4((v + 9).to_bytes(4, "big")), t4((v + 256 + 9).to_bytes(4, "big"))]  # inside i; between i and i + 1
    return out


def world_ips():
    """The held IPs of the query tests, every text once."""
    out = []
    for n in LEN4:
        for k, b in enumerate(around(BASE4, n)):
            out.append(t4(b) if k % 3 else "::ffff:" + t4(b))      # v4-mapped text of the same address among them
            out.append(t4(b))
    for n in LEN6:
        out += [t6(b) for b in around(BASE6, n)]
    out += HF.spellings(BASE6) + HF.spellings(HF.V4_PREFIX + BASE4)
    out += HF.spellings(b"\0" * 12 + BASE4)                        # ::170.85.195.60: IPv6, not v4-mapped
    out += NOT_ADDRESSES + size_ips() + ["2001:db8::1", "9.9.9.9", "::", "0.0.0.0", "::ffff:0:0", "255.255.255.255"]
    return list(dict.fromkeys(out))


def world_lines(ips, t0_ms=T0_MS):
    """Every IP gets "fast" (GET) and "mid" (POST, 1..4 times); every third "slow" (/login) too."""
    out, k = [], 0

    def line(ip, m, path):
        nonlocal k
        t = t0_ms + k
        k += 1
        out.append("%d.%03d %s %s h.com %s %s HTTP/1.1 ua" % (t // 1000, t % 1000, ip, m, m, path))

    for j, ip in enumerate(ips):
        line(ip, "GET", "/x")
        for _ in range(1 + j % 4):
            line(ip, "POST", "/login" if j % 3 == 0 else "/x")
    return ("\n".join(out) + "\n").encode()


def count_ips(n):
    """n IPs, IPv4 and IPv6 mixed, a third of them inside COUNT_NETS"""
    return ["10.%d.%d.%d" % (k % 24, (k >> 8) & 255, k & 255) if k % 4 else "2001:db8:%x::%x" % (0x70 + k % 16, k) for k in range(n)]


COUNTS_HELD = (1, 255, 257, 3001)
COUNT_NETS = ["10.0.0.0/13", "2001:db8:70::/46", "10.16.0.0/14", "10.9.9.9"]


# k_net_count counts a block's networks in an LDS table of 2048 slots before it adds them to the
# global counters: one block walks up to 4096 held IPs, so with 3001 IPs held one block meets this
# many distinct single-address networks -- below, at and past the table's size -- and a wide one
SINGLES_N = (2047, 2048, 2049, 2600)


def singles(n):
    return count_ips(COUNTS_HELD[-1])[:n] + ["10.0.0.0/8"]


def max_list():
    """BJX_NETS_MAX entries of mixed lengths; a handful hold IPs of the world"""
    out = ["170.85.195.0/24", t6(BASE6) + "/64", "20.0.1.0/24", "::ffff:170.85.195.61"]
    k = 0
    while len(out) < NETS_MAX:
        m = k % 4
        if m == 0:
            out.append("30.%d.%d.%d" % ((k >> 18) & 255, (k >> 10) & 255, (k >> 2) & 255))
        elif m == 1:
            out.append("31.%d.%d.0/24" % ((k >> 10) & 255, (k >> 2) & 255))
        elif m == 2:
            out.append("2001:db9:%x:%x::/64" % ((k >> 18) & 0xffff, (k >> 2) & 0xffff))
        else:
            out.append("2001:dba::%x:%x/%d" % ((k >> 18) & 0xffff, (k >> 2) & 0xffff, 113 + (k >> 2) % 16))
        k += 1
    return out


def all_lengths():
    return [t4(BASE4) + "/%d" % n for n in range(33)] + [t6(BASE6) + "/%d" % n for n in range(129)]


def lists():
    """{name: (world, [entry])}; world: "world" (world_ips), "count" (count_ips(3001)), "pool" (H.POOL)"""
    out = {}
    for n in LEN4:
        out["v4/%d" % n] = ("world", [t4(BASE4) + "/%d" % n])
    for n in LEN6:
        out["v6/%d" % n] = ("world", [t6(BASE6) + "/%d" % n])
    out["mapped/104"] = ("world", ["::ffff:%s/104" % t4(BASE4)])
    out["mapped/96"] = ("world", ["::ffff:0:0/96"])
    out["mapped/128"] = ("world", ["::FFFF:%s/128" % t4(BASE4)])
    out["mapped"] = ("world", ["0:0:0:0:0:ffff:aa55:c33c"])
    out["all_lengths"] = ("world", all_lengths())
    for n in SIZE_N:
        out["size_%d" % n] = ("world", [size_net(i) for i in reversed(range(n))])
    out["nested_dup"] = ("world", ["170.85.0.0/16", "170.85.195.0/24", "170.85.195.60", "170.85.0.0/16", "2001:db8:85a3::/48",
                                    "203.0.113.0/24", "170.85.195.61/24", "2001:0DB8:85A3:C55A::/64"])
    out["spell4"] = ("world", [t4(BASE4)])
    out["spell6"] = ("world", [":".join("%04X" % x for x in struct.unpack(">8H", BASE6)) + "/128"])
    out["max"] = ("world", max_list())
    out["count"] = ("count", COUNT_NETS)
    for n in SINGLES_N:
        out["singles_%d" % n] = ("count", singles(n))
    for b in range(3):
        out["pool_%d" % b] = ("pool", pool_selection(b, 0)["nets"])
    out["pool_node"] = ("pool", ["10.1.0.64/26", "2001:db8:85a3:20::/59"])
    return out


def pool_selection(b, now_ns):
    """The removal after batch b of H.stream() (H.POOL: 10.1.0.0 .. 10.1.0.199 and
    2001:db8:85a3:k:0:8a2e:370:7000+k, k < 100).
    0: nested, duplicate and empty networks of both families, a single address
    1: one rule name inside an IPv4 network given as v4-mapped text
    2: min_hits and a start window inside a /25 and most of the IPv6 block"""
    if b == 0:
        return {"nets": ["10.1.0.0/26", "10.1.0.128/25", "2001:db8:85a3::/61", "10.1.0.77", "10.1.0.0/27", "10.1.0.0/26",
                         "192.0.2.0/24", "2001:db8:85a3:10::/60", "10.1.0.200/29"]}
    if b == 1:
        return {"name": "mid", "nets": ["::ffff:10.1.0.64/122", "2001:db8:85a3:40::/58"]}
    return {"min_hits": 2, "min_start_ns": now_ns + 20 * H.S, "max_start_ns": now_ns + 95 * H.S,
            "nets": ["10.1.0.0/25", "2001:db8:85a3::/57"]}


def world_of(name):
    return {"world": world_ips, "count": lambda: count_ips(COUNTS_HELD[-1]), "pool": lambda: list(H.POOL)}[name]()


def build_world(target, ips=None):
    """-> the Run after one batch that makes every IP of the world held"""
    run = H.Run(H.CFG, target)
    run.feed(world_lines(world_ips() if ips is None else ips), NOW)
    return run


def parity_run(target, batches, compare_dump=True):
    """H.parity_run with the removals of pool_selection"""
    run = H.Run(H.CFG, target)
    done = []
    for b, (data, now) in enumerate(batches):
        run.feed(data, now)
        if b < H.N_BATCH - 1:
            done.append(run.remove(**pool_selection(b, now)))
            if target is not None:
                run.compare_states(dump=compare_dump)
    if target is not None:
        run.compare_states(dump=compare_dump)
    return run, done
