"""State snapshots without a GPU: the C symbols and their NULL handling, the
pure-Python format code (banjax_amd/snapshot.py), and the host part of the
importer -- header / section / name validation and the node's merge of shard
snapshots (banjax_amd/csrc/snapshot.h) -- built for the host from
tests/cpu/snapshot_host.cpp.  Expected bytes come from snapshot.build."""
import ctypes
import os
import random
import struct
import subprocess
import tempfile

import pytest

from banjax_amd import _lib, snapshot

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpu", "snapshot_host.cpp")
T0 = 1_700_000_000_000_000_000
NEW = ["bjx_state_export_bound", "bjx_state_export", "bjx_state_import", "bjx_node_state_export_bound",
       "bjx_node_state_export", "bjx_node_state_import"]


def test_symbols_and_null_arguments():
    L = _lib.lib()
    for name in NEW:
        assert name in _lib.EXPORTS and hasattr(L, name), name
    st, n = _lib.SnapshotStats(), ctypes.c_uint64(7)
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.bjx_state_export(None, 0, p, 64, ctypes.byref(n), ctypes.byref(st)) == _lib.ERR_ARG
    assert L.bjx_state_import(None, bytes(64), 64, 0, 1, ctypes.byref(st)) == _lib.ERR_ARG
    assert L.bjx_node_state_export(None, 0, p, 64, ctypes.byref(n), ctypes.byref(st)) == _lib.ERR_ARG
    assert L.bjx_node_state_import(None, bytes(64), 64, ctypes.byref(st)) == _lib.ERR_ARG
    assert L.bjx_state_export_bound(None) == 0 and L.bjx_node_state_export_bound(None) == 0
    assert ctypes.sizeof(_lib.SnapshotStats) == 56


def _sample(seed=1, n_ips=40, names=("mid", "fast", "slow", "a", "ab", "")):
    rng = random.Random(seed)
    ips = ["10.%d.%d.%d" % (seed, k >> 8, k & 255) if k % 3 else "2001:db8::%x:%x" % (seed, k) for k in range(n_ips)]
    rng.shuffle(ips)
    states = {}
    for ip in ips:
        use = rng.sample(list(names), rng.randrange(1, len(names) + 1))
        states[ip] = {n: (rng.randrange(0, 50), T0 + rng.randrange(-10**12, 10**12)) for n in use}
    return ips, states


def test_python_format_round_trip_and_canonical_form():
    ips, states = _sample()
    blob = snapshot.build(ips, states)
    got_ips, got = snapshot.parse(blob)
    assert got_ips == [ip.encode() for ip in ips]
    assert got == {ip.encode(): {n.encode(): v for n, v in d.items()} for ip, d in states.items()}
    # insertion order of the names (per IP and overall) does not reach the bytes
    rng = random.Random(2)
    shuffled = {}
    for ip in reversed(ips):
        items = list(states[ip].items())
        rng.shuffle(items)
        shuffled[ip] = dict(items)
    assert snapshot.build(ips, shuffled) == blob
    # the IP order does
    assert snapshot.build(ips[::-1], states) != blob
    # the header says what the doc says
    magic, ver, hb, total, n_names, names_bytes, n_ips, ip_bytes, n_states = struct.unpack_from("<8sII6Q", blob)
    assert (magic, ver, hb, total, n_ips) == (b"BJXSTATE", 1, 64, len(blob), len(ips))
    assert n_states == sum(len(d) for d in states.values()) and ip_bytes == sum(len(ip) for ip in ips)
    # an IP without a state is left out; an empty snapshot is header + two offsets
    assert snapshot.build(ips + ["9.9.9.9"], dict(states, **{"9.9.9.9": {}})) == blob
    empty = snapshot.build([], {})
    assert len(empty) == 80 and snapshot.parse(empty) == ([], {})


@pytest.fixture(scope="module")
def host():
    d = tempfile.mkdtemp(prefix="bjx_snap_")
    so = os.path.join(d, "libsnap.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-o", so, SRC], check=True)
    L = ctypes.CDLL(so)
    L.bjx_test_snap_validate.restype = ctypes.c_int
    L.bjx_test_snap_validate.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_char_p, ctypes.c_uint64]
    L.bjx_test_snap_merge.restype = ctypes.c_int
    L.bjx_test_snap_merge.argtypes = [ctypes.c_uint32, ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint64),
                                      ctypes.c_char_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_uint64), ctypes.c_char_p,
                                      ctypes.c_uint64]
    return L


def _validate(host, blob):
    msg = ctypes.create_string_buffer(256)
    rc = host.bjx_test_snap_validate(bytes(blob), len(blob), msg, 256)
    return rc, msg.value.decode()


def _with_header(blob, **kw):
    """blob with header fields replaced"""
    f = list(struct.unpack_from("<8sII6Q", blob))
    keys = ["magic", "version", "header_bytes", "total_bytes", "n_names", "names_bytes", "n_ips", "ip_bytes", "n_states"]
    for k, v in kw.items():
        f[keys.index(k)] = v
    return struct.pack("<8sII6Q", *f) + blob[64:]


def _names_blob(names):
    """a snapshot-shaped blob with the given name table as it is (one IP, one record per name)"""
    blob = snapshot.build(["1.1.1.1"], {"1.1.1.1": {"n%03d" % k: (1, T0) for k in range(len(names))}})
    nb = b"".join(names)
    off, t = [0], 0
    for x in names:
        t += len(x)
        off.append(t)
    _, o_names, o_ip_off, _, _, _ = snapshot.layout(len(names), 4 * len(names), 1, 7, len(names))
    tail = blob[o_ip_off:]
    body = struct.pack("<%dQ" % len(off), *off) + nb + b"\0" * (-len(nb) % 8) + tail
    return _with_header(blob[:64] + body, names_bytes=len(nb), total_bytes=64 + len(body))


def corrupt_corpus():
    """(blob, accept, keyword the rejection's message must contain)"""
    ips, states = _sample(3)
    good = snapshot.build(ips, states)
    magic, ver, hb, total, n_names, names_bytes, n_ips, ip_bytes, n_states = struct.unpack_from("<8sII6Q", good)
    bounds = snapshot.layout(n_names, names_bytes, n_ips, ip_bytes, n_states)
    cases = [(good, 1, ""), (snapshot.build([], {}), 1, ""), (snapshot.build(*_sample(4, 1, ("x",))), 1, "")]
    # truncation: inside the header, at every section boundary, one byte short
    for cut in (0, 8, 63):
        cases.append((good[:cut], 0, "header"))
    for cut in sorted(set(bounds[:5])) + [total - 1]:
        cases.append((good[:cut], 0, "total_bytes"))
    cases.append((good + b"\0" * 8, 0, "total_bytes"))
    cases.append((_with_header(good, magic=b"BJXSTATF"), 0, "magic"))
    cases.append((_with_header(good, version=2), 0, "version"))
    cases.append((_with_header(good, header_bytes=72), 0, "header_bytes"))
    for d in (8, -8):
        cases.append((_with_header(good, total_bytes=total + d), 0, "total_bytes"))
    # a section length that overflows u64 when the sections are summed
    cases.append((_with_header(good, names_bytes=(1 << 64) - 8), 0, "overflow"))
    cases.append((_with_header(good, ip_bytes=(1 << 64) - names_bytes - 64), 0, "overflow"))
    # section sizes that are plausible alone but do not add up
    cases.append((_with_header(good, ip_bytes=ip_bytes + 8), 0, "add up"))
    cases.append((_with_header(good, n_names=1 << 24), 0, "n_names"))
    cases.append((_with_header(good, n_ips=1 << 31), 0, "n_ips"))
    cases.append((_with_header(good, n_states=1 << 31), 0, "n_states"))
    cases.append((_names_blob([b"a", b"b", b"c"]), 1, ""))
    cases.append((_names_blob([b"b", b"a", b"c"]), 0, "not sorted"))
    cases.append((_names_blob([b"a", b"ab", b"aa"]), 0, "not sorted"))
    cases.append((_names_blob([b"a", b"b", b"b"]), 0, "duplicate"))
    cases.append((_names_blob([b"", b""]), 0, "duplicate"))
    # what the device checks of the importer catch, in their host form
    o_ip_off, o_recs = bounds[2], bounds[4]

    def poke(off, fmt, v):
        b = bytearray(good)
        struct.pack_into(fmt, b, off, v)
        return bytes(b)

    cases.append((poke(o_recs + 24 * 5, "<I", n_ips), 0, "records"))
    cases.append((poke(o_recs + 24 * 5 + 4, "<I", n_names), 0, "records"))
    r = [good[o_recs + 24 * k:o_recs + 24 * (k + 1)] for k in (7, 8)]
    cases.append((good[:o_recs + 24 * 7] + r[1] + r[0] + good[o_recs + 24 * 9:], 0, "records"))
    cases.append((poke(o_ip_off + 8 * 3, "<Q", ip_bytes + 1), 0, "ip_off"))
    cases.append((poke(o_ip_off + 8 * n_ips, "<Q", ip_bytes - 1), 0, "ip_off"))
    return cases


def test_host_validation_accepts_build_and_names_each_failed_check(host):
    for k, (blob, accept, kw) in enumerate(corrupt_corpus()):
        rc, msg = _validate(host, blob)
        if accept:
            assert rc == 0, (k, msg)
        else:
            assert rc == 1 and kw in msg, (k, kw, msg)


def _merge(host, blobs):
    n = len(blobs)
    ptrs = (ctypes.c_char_p * n)(*blobs)
    lens = (ctypes.c_uint64 * n)(*[len(b) for b in blobs])
    cap = sum(len(b) for b in blobs)
    out, got, msg = ctypes.create_string_buffer(cap), ctypes.c_uint64(0), ctypes.create_string_buffer(256)
    rc = host.bjx_test_snap_merge(n, ptrs, lens, out, cap, ctypes.byref(got), msg, 256)
    assert rc == 0, msg.value
    return out.raw[:got.value]


def test_merge_of_three_shards_is_build_of_the_union(host):
    """Shards with different name sets (one empty shard among them): the merge
    is build() over the IPs engine-major and the union of the states."""
    a = _sample(11, 30, ("mid", "fast", "zz"))
    b = _sample(12, 17, ("slow", "", "mid"))
    c = _sample(13, 25, ("b", "a", "fast", "slow"))
    blobs = [snapshot.build(*s) for s in (a, b, c)]
    union = {}
    for s in (a, b, c):
        union.update(s[1])
    assert _merge(host, blobs) == snapshot.build(a[0] + b[0] + c[0], union)
    assert _merge(host, [blobs[0], snapshot.build([], {}), blobs[2]]) == \
        snapshot.build(a[0] + c[0], {**a[1], **c[1]})
    assert _merge(host, [blobs[1]]) == blobs[1]
    msg = ctypes.create_string_buffer(256)
    bad = blobs[1][:-1]
    ptrs, lens = (ctypes.c_char_p * 2)(blobs[0], bad), (ctypes.c_uint64 * 2)(len(blobs[0]), len(bad))
    out, got = ctypes.create_string_buffer(1 << 16), ctypes.c_uint64(0)
    assert host.bjx_test_snap_merge(2, ptrs, lens, out, 1 << 16, ctypes.byref(got), msg, 256) == 1
    assert b"total_bytes" in msg.value


def test_standalone_program_under_sanitizers():
    """The same source with its own main, built with ASan + UBSan and run once
    as a subprocess over the corrupt corpus (never loaded into Python)."""
    d = tempfile.mkdtemp(prefix="bjx_snap_san_")
    exe = os.path.join(d, "snapshot_host")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-DBJX_SNAPSHOT_MAIN", "-o", exe, SRC]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.skip("the compiler cannot build with -fsanitize=address,undefined here: " + r.stderr.strip()[-300:])
    corpus = os.path.join(d, "corpus.bin")
    with open(corpus, "wb") as f:
        for blob, accept, kw in corrupt_corpus():
            k = kw.encode()
            f.write(struct.pack("<II", accept, len(k)) + k + struct.pack("<Q", len(blob)) + blob)
    r = subprocess.run([exe, corpus], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "%d cases, 0 wrong" % len(corrupt_corpus()) in r.stdout
