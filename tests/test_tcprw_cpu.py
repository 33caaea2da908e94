"""TCP-header rewrites of NAT'd packets (VPCSUM_NAT_TCP_REWRITES), the parts that need no GPU: the
Python restatement of the reference's setters against the hand-checked crafted vectors, the
per-packet rewrite the kernel's lanes run (vproxy_amd/csrc/tcp_rewrite.h) in a stand-alone program
under ASan / UBSan against that restatement, and the new kernel's scratch budget."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import tcprwvec as T
from oracle import oracle as O
from test_kernel_resources import kernels

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vecs(orc):
    return T.crafted(orc)


def test_restatement_on_crafted_vectors(vecs):
    """java_tcp_rewrite writes exactly the hand-listed bytes of each crafted vector and reports the
    hand-listed dirty / absent; the vector list covers the branches the spec names."""
    names = [v["name"] for v in vecs]
    assert len(set(names)) == len(names) >= 45
    for v in vecs:
        if v["name"] in ("ttl_expired", "outside_arena"):   # refused before the TCP setters: the GPU tests' matter
            continue
        rsv = bytes(v["rw"]["rsv"])
        before = bytearray(v["l3"])
        l3 = bytearray(before)
        dirty, absent = T.java_tcp_rewrite(l3, v["ver"], v["proto"], len(l3), v["l4_off"], v["rw"])
        t = v["l4_off"]
        want = bytearray(before)
        for at, b in v["writes"].items():
            if b is None and at == 13:     # the flags byte: its two high bits stay
                b = bytes([(before[t + 13] & 0xC0) | (rsv[1] & 0x3F)])
            elif b is None and at == 4:    # seq + addend mod 2^32
                s = int.from_bytes(before[t + 4:t + 8], "big") + int.from_bytes(rsv[4:8], "big")
                b = (s & 0xFFFFFFFF).to_bytes(4, "big")
            want[t + at:t + at + len(b)] = b
        assert (dirty, absent) == (v["dirty"], v["absent"]), v["name"]
        assert l3 == want, v["name"]
        if v["name"].startswith(("bad_", "udp", "icmp", "tcp_19", "clamp_without", "mss_equal", "max_mss_0_equal",
                                 "max_mss_ffff")):
            assert l3 == before and not dirty and not absent, v["name"]


def test_checksum_edge_vectors(vecs, orc):
    """The two checksum-edge vectors are what they claim: a stored TCP sum of 0x0000 before the
    rewrite, and one after it."""
    by = {v["name"]: v for v in vecs}
    v = by["sum_was_0000"]
    assert v["l3"][v["l4_off"] + 16:v["l4_off"] + 18] == b"\x00\x00"
    for name, zero_after in (("sum_becomes_0000", True), ("sum_was_0000", False)):
        v = by[name]
        arena, desc, rw = T.pack([v], 0)
        got, st = T.expected(orc, arena, desc, rw)
        o = int(desc[0]["l3_off"]) + v["l4_off"] + 16
        assert st[0] == O.S_DONE
        assert (got[o:o + 2].tobytes() == b"\x00\x00") == zero_after, name
        # and the incoming sum is valid: a full recompute of the untouched packet changes nothing
        assert O.l4_csum(v["l3"], len(v["l3"]), v["l4_off"], v["ver"], v["proto"]) == \
            int.from_bytes(v["l3"][v["l4_off"] + 16:v["l4_off"] + 18], "big")


def test_received_frames_cover_every_branch():
    """hsumvec.received(11, 512), the batch tests' frames: SYNs above and at most maxMss, SYNs
    without the option, other TCP and UDP frames, corrupted ones, L4 offsets 20..60."""
    fs = T.H.received(11, 512)
    syn = [f for f in fs if f["proto"] == 6 and f["syn"]]
    assert len([f for f in syn if f["mss"] is not None and f["mss"] > T.MAX_MSS]) == 147
    assert len([f for f in syn if f["mss"] is not None and f["mss"] <= T.MAX_MSS]) == 83
    assert len([f for f in syn if f["mss"] is None]) == 64
    assert len([f for f in fs if f["proto"] == 6 and not f["syn"]]) == 144
    assert len([f for f in fs if f["proto"] == 17]) == 74
    assert len([f for f in fs if f["corrupt"] and f["proto"] == 6]) == 25   # and 14 UDP ones
    assert len([f for f in fs if f["corrupt"]]) == 39
    l4 = {T.H.frame_l3(f["frame"]).l4_off for f in fs}
    assert min(l4) == 20 and max(l4) == 60


def _vector_file(orc, path, batches):
    """Every packet of `batches` the address / port rewrite does not refuse, as
    tests/cpp/tcp_rewrite_test.cpp reads them."""
    recs = []
    for arena, desc, rw in batches:
        pre = arena.copy()
        st = orc.nat_java(pre, desc, rw)
        for i, d in enumerate(desc):
            if st[i] & O.S_BAD_DESC:
                continue
            o, n, l4 = int(d["l3_off"]), int(d["l3_len"]), int(d["l4_off"])
            ver, proto = int(d["l3_ver"]), int(d["l4_proto"])
            a = pre[o:o + n].tobytes()
            l3 = bytearray(a)
            dirty, absent = T.java_tcp_rewrite(l3, ver, proto, n, l4, rw[i])
            setters = bytes(l3)
            if dirty:
                l3[l4 + 16:l4 + 18] = O.l4_csum(bytes(l3), n, l4, ver, proto).to_bytes(2, "big")
            recs.append(struct.pack("<IIBBBB", n, l4, ver, proto, dirty, absent) + rw[i].tobytes() + a + setters +
                        bytes(l3))
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(recs)) + b"".join(recs))
    return len(recs)


def test_tcp_rewrite_header_under_sanitizers(vecs, orc, tmp_path):
    """tcp_rewrite.h (what each k_nat_tcp lane runs) equals the restatement on every crafted vector
    and on 257 received frames with random ops, in the strict form (setters, dirty, absent) and the
    RFC 1624 form (the updated sum equals the full recompute: the inputs' sums are valid), each
    packet at its exact size under ASan / UBSan; nat_tcp_header_end's extents.  Nothing of the
    library is linked."""
    arena, desc, rw, bad = T.received_batch(257)
    keep = ~bad   # RFC 1624 equals the recompute on valid input only
    vf = tmp_path / "vectors.bin"
    n = _vector_file(orc, vf, [T.pack(vecs, None), T.pack(vecs, 1), (arena, desc[keep], rw[keep])])
    assert n > 300
    exe = tmp_path / "tcp_rewrite_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-Wall", "-Werror", "-I", os.path.join(REPO, "include"),
                           "-I", os.path.join(REPO, "vproxy_amd", "csrc"),
                           os.path.join(REPO, "tests", "cpp", "tcp_rewrite_test.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), str(vf)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tcp_rewrite ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    m = re.search(r"vectors (\d+) applied (\d+) dirty (\d+) absent (\d+)", r.stdout)
    assert m and int(m.group(1)) == n and int(m.group(2)) > 200 and int(m.group(3)) > 100 and int(m.group(4)) > 20


def test_binding_fills_the_same_bytes():
    """vpcsum.nat_tcp_fill writes the entry bytes include/vpcsum.h lays out (tcprwvec.fill)."""
    from vproxy_amd import vpcsum as V
    assert (V.NAT_TCP, V.NAT_TCP_REWRITES, V.S_MSS_ABSENT) == (T.NAT_TCP, T.NAT_TCP_REWRITES, T.S_MSS_ABSENT)
    assert (V.TCP_SEQ_ADD, V.TCP_SET_FLAGS, V.TCP_CLAMP_MSS) == (T.SEQ_ADD, T.SET_FLAGS, T.CLAMP_MSS)
    a, b = np.zeros(3, V.NAT_DTYPE), np.zeros(3, O.NAT_DTYPE)
    a["mask"] = b["mask"] = [0, 3, 0x15]
    V.nat_tcp_fill(a[0], seq_add=-28, max_mss=1400)
    T.fill(b[0], T.SEQ_ADD | T.CLAMP_MSS, 0, 1400, -28)
    V.nat_tcp_fill(a[1], seq_add=-1, flags=0x12)
    T.fill(b[1], T.SEQ_ADD | T.SET_FLAGS, 0x12, 0, 0xFFFFFFFF)
    V.nat_tcp_fill(a[2], flags=0xFF, max_mss=0)
    T.fill(b[2], T.SET_FLAGS | T.CLAMP_MSS, 0x3F, 0, 0)
    assert a.tobytes() == b.tobytes()
    assert a.tobytes()[36:48] == bytes([0x40, 0, 5, 0, 0x05, 0x78, 0xFF, 0xFF, 0xFF, 0xE4, 0, 0])


def test_header_constants():
    """include/vpcsum.h carries the constants at the values the tests use; the ABI version stays."""
    h = open(os.path.join(REPO, "include", "vpcsum.h")).read()
    for name, val in (("VPCSUM_NAT_TCP", 0x40), ("VPCSUM_NAT_TCP_REWRITES", 0x02), ("VPCSUM_S_MSS_ABSENT", 0x08),
                      ("VPCSUM_TCP_SEQ_ADD", 1), ("VPCSUM_TCP_SET_FLAGS", 2), ("VPCSUM_TCP_CLAMP_MSS", 4),
                      ("VPCSUM_ABI_VERSION", 4)):
        m = re.search(r"#define\s+%s\s+(\w+)" % name, h)
        assert m and int(m.group(1).rstrip("u"), 0) == val, name


def test_no_scratch_in_tcp_kernel():
    """k_nat_tcp, every phase: no scratch (the rewrite's result struct stays in registers), no LDS."""
    ks = {k: v for k, v in kernels("nat.hip.o").items() if "k_nat_tcp" in k}
    assert len(ks) == 3, sorted(ks)
    for k, v in ks.items():
        assert v["private_segment_fixed_size"] == 0 and v["group_segment_fixed_size"] == 0, (k, v)
