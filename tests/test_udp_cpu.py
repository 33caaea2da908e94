"""CPU-side checks of the UDP datagram build and receive (vpcsum_udp_build_async,
vpcsum_udp_recv_async, their ctx and PNI forms): the Python restatement of the rules
(tests/udpvec.py) against the reference's own test frame and the oracle, the datagram whose sum
computes to 0, every refusal of both rules, vswitch.plan_udp_store, the rules of udp_build.h /
udp_recv.h in a stand-alone program under ASan / UBSan, the layouts and exports, the kernels' budgets
read from the code object, and the argument refusals that need no device."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import udpvec as U
from oracle import oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kat(name="udpIpv4Example"):
    ks = json.load(open(os.path.join(REPO, "tests", "golden", "kat.json")))["kats"]
    return next(k for k in ks if k["name"] == name)


@pytest.fixture(scope="module")
def L():
    from vproxy_amd import build
    lib = ctypes.CDLL(build.build())
    lib.vpcsum_last_error.restype = ctypes.c_char_p
    return lib


# ------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------
def test_restatement_rebuilds_the_reference_frame():
    """udpIpv4Example (a DNS answer: IHL 5, ident 37bd, DF set, 61 payload bytes): the template read
    out of the fixture, the frame rebuilt by the rule -- byte-equal to the fixture's 89-byte IP
    packet behind its Ethernet header, with its pinned sums 0x7f41 / 0xdf0d."""
    k = kat()
    raw = bytes.fromhex(k["hex"])
    assert len(raw) == 14 + 89 and (k["pinned"]["ip"], k["pinned"]["l4"]) == (0x7f41, 0xdf0d)
    h, payload = U.from_frame(raw)
    assert len(payload) == 61 and h["ident"].tobytes() == b"\x37\xbd" and h["frag"].tobytes() == b"\x40\x00"
    src = np.frombuffer(b"\x11" * 5 + payload + b"\x22" * 3, np.uint8)
    dst = np.full(7 + len(raw) + 9, 0xEE, np.uint8)
    dg = np.array([U.mk_dg(7, 5, 61)], U.UDPDG_DTYPE)
    after, flen, out, st = U.build(dst, src, np.array([h], U.HDR_DTYPE), dg)
    assert after[7:7 + len(raw)].tobytes() == raw
    assert (after[:7] == 0xEE).all() and (after[7 + len(raw):] == 0xEE).all() and (dst == 0xEE).all()
    assert list(flen) == [103] and list(st) == [U.S_DONE] and int(out[0]) == 0x7f41 | (0xdf0d << 16)


@pytest.mark.parametrize("ver,l2", [(4, 14), (6, 14), (6, 0), (4, 0)])
def test_restatement_frames_verify_with_the_oracle(ver, l2, orc):
    """What the restatement builds, described as the parse would, verifies with the oracle: S_L4_OK
    (and S_IP_OK), for payloads of 0..70 bytes."""
    rng = np.random.default_rng(90 + ver + l2)
    src16 = bytes(range(16)) if ver == 6 else b"\x0a\x01\x02\x03"
    h = U.mk_hdr(ver, l2, src16, bytes(range(32, 48)) if ver == 6 else b"\xc0\xa8\x00\x09", tos=0x2e, ttl=7, ident=0x1234, frag=0x4000)
    ipl = 20 if ver == 4 else 40
    for d in range(0, 71):
        f, ipc, l4c = U.frame(h, rng.integers(0, 256, d, dtype=np.uint8).tobytes())
        assert len(f) == l2 + ipl + 8 + d and l4c != 0
        arena = np.frombuffer(f, np.uint8)
        desc = np.array([U.mk_desc(l2, ipl + 8 + d, ipl, ver)], O.DESC_DTYPE)
        out, st = orc.process(arena, desc, O.MODE_VERIFY)
        assert st[0] == U.S_DONE | U.S_L4_OK | (U.S_IP_OK if ver == 4 else 0) and int(out[0]) == ipc | (l4c << 16)
        assert int.from_bytes(f[l2 + ipl + 4:l2 + ipl + 6], "big") == 8 + d


@pytest.mark.parametrize("ver", [4, 6])
def test_a_sum_of_zero_is_stored_as_ffff(ver, orc):
    """One aligned payload word zeroed, the sum computed, the value written into the word: the UDP
    sum now computes to 0 and 0xffff is stored.  Checked with the oracle on the CPU: Utils'
    checksum over pseudo-header and segment with the field 0 is 0, the oracle's UDP sum 0xffff, and
    the built frame verifies S_L4_OK with 0xffff stored and S_UDP_NOCSUM (not OK) with 0 stored."""
    rng = np.random.default_rng(95 + ver)
    h = U.mk_hdr(ver, 14, bytes(range(16)) if ver == 6 else b"\x0a\x00\x00\x01", bytes(range(16, 32)) if ver == 6 else b"\x0a\x00\x00\x02")
    body = U.sum_zero_payload(h, 64, rng)
    f, _, l4c = U.frame(h, body)
    ipl = 20 if ver == 4 else 40
    assert l4c == 0xffff and f[14 + ipl + 6:14 + ipl + 8] == b"\xff\xff"
    desc = np.array([U.mk_desc(14, ipl + 72, ipl, ver)], O.DESC_DTYPE)
    out, st = orc.process(np.frombuffer(f, np.uint8), desc, O.MODE_VERIFY)
    assert st[0] & U.S_L4_OK and not st[0] & U.S_UDP_NOCSUM and int(out[0]) >> 16 == 0xffff
    z = f[:14 + ipl + 6] + b"\0\0" + f[14 + ipl + 8:]
    out, st = orc.process(np.frombuffer(z, np.uint8), desc, O.MODE_VERIFY)
    assert st[0] & U.S_UDP_NOCSUM and not st[0] & U.S_L4_OK and int(out[0]) >> 16 == 0xffff


def test_restatement_build_refusals():
    """Every refusal of the build, each at the value accepted and the first refused."""
    h4, h6 = U.mk_hdr(4, 14), U.mk_hdr(6, 0, bytes(16), bytes(16))
    hdrs = np.array([h4, h6, U.mk_hdr(5), U.mk_hdr(4, 13), U.mk_hdr(4, rsv=1), U.mk_hdr(4, ack=1), U.mk_hdr(6, window=0x100)], U.HDR_DTYPE)
    big = 1 << 40

    def ref(dst_len=big, src_len=big, **kw):
        args = dict(frame_off=0, data_off=0, data_len=10, hlen=62)
        args.update(kw)
        return U.refused(hdrs, U.mk_dg(**args), dst_len, src_len)
    assert not ref() and not ref(hdr=1)
    assert ref(hdr=7) and ref(hdr=0xffffffff)                                            # hdr >= n_hdr
    assert all(ref(hdr=k) for k in (2, 3, 4, 5, 6))                                      # the template
    assert ref(rsv=1) and ref(rsv=1 << 31)
    assert not ref(data_len=65507, frame_cap=70000) and ref(data_len=65508, frame_cap=70000)               # IPv4: 28 + d
    assert not ref(hdr=1, data_len=65527, frame_cap=70000) and ref(hdr=1, data_len=65528, frame_cap=70000)  # IPv6: 8 + d
    assert ref(data_len=0xffffffff, frame_cap=0xffffffff) and ref(hdr=1, data_len=0xfffffff8, frame_cap=0xffffffff)
    assert not ref(frame_cap=52) and ref(frame_cap=51) and not ref(hdr=1, frame_cap=58) and ref(hdr=1, frame_cap=57)
    assert not ref(frame_off=948, dst_len=1000) and ref(frame_off=949, dst_len=1000) and ref(frame_off=(1 << 64) - 1, dst_len=1000)
    assert not ref(data_off=990, src_len=1000) and ref(data_off=991, src_len=1000) and ref(data_off=(1 << 64) - 5, src_len=1000)
    assert not ref(data_len=0, data_off=1000, src_len=1000, frame_cap=42)               # data_len 0 is a legal datagram


def test_restatement_recv_refusals():
    """Every refusal of the receive, each at the value accepted and the first refused."""
    def ok(d, r=None, dst_len=1000, arena_len=200):
        return U.plan(arena_len, d, U.mk_rx(0, 1000) if r is None else r, dst_len)
    v4, v6 = U.mk_desc(10, 120, 20, 4), U.mk_desc(130, 70, 62, 6)
    assert ok(v4) == 92 and ok(v6) == 0                                                   # seg_len exactly 8 stores 0 bytes
    assert ok(U.mk_desc(10, 120, 20, 4, proto=6)) is None and ok(U.mk_desc(10, 120, 20, 5)) is None
    for fl in (O.F_IP, 0, O.F_L4 | O.F_L4P, O.F_L4 | O.F_RAW, O.F_L4 | O.F_PRE):
        assert ok(U.mk_desc(10, 120, 20, 4, flags=fl)) is None
    assert ok(U.mk_desc(130, 70, 62, 6, flags=O.F_L4 | O.F_IP)) is None
    assert ok(U.mk_desc(10, 120, 124, 4)) is None and ok(U.mk_desc(10, 120, 16, 4)) is None and ok(U.mk_desc(10, 120, 22, 4)) is None
    assert ok(U.mk_desc(130, 70, 39, 6)) is None
    assert ok(U.mk_desc(131, 70, 62, 6)) is None and ok(U.mk_desc((1 << 64) - 8, 70, 62, 6)) is None
    assert ok(U.mk_desc(130, 69, 62, 6)) is None and ok(U.mk_desc(10, 27, 20, 4)) is None and ok(U.mk_desc(10, 28, 20, 4)) == 0
    assert ok(v4, U.mk_rx(0, 1000, ops=2)) is None and ok(v4, U.mk_rx(0, 1000, ops=0x81)) is None
    assert all(ok(v4, U.mk_rx(0, 1000, rsv=1 << (8 * k))) is None for k in range(3))
    assert ok(v4, U.mk_rx((1 << 64) - 1, 0, ops=0), dst_len=0) == 0                       # verify only: no destination
    assert ok(v4, U.mk_rx(0, 92)) == 92 and ok(v4, U.mk_rx(0, 91)) is None
    assert ok(v4, U.mk_rx(908, 92)) == 92 and ok(v4, U.mk_rx(909, 92)) is None and ok(v4, U.mk_rx((1 << 64) - 4, 92)) is None


def test_plan_udp_store():
    """ReceivingQueue.store's connect filter on plain values, vswitch's and the restatement's: an
    unconnected socket takes every datagram, a connected one only its peer's (address, then port)."""
    from vproxy_amd import vswitch
    peer = (b"\x0a\x00\x00\x01", 53)
    for f in (vswitch.plan_udp_store, U.plan_udp_store):
        assert f(None, b"\x0a\x00\x00\x09", 9) is True
        assert f(peer, b"\x0a\x00\x00\x01", 53) is True
        assert f(peer, b"\x0a\x00\x00\x02", 53) is False
        assert f(peer, b"\x0a\x00\x00\x01", 54) is False
        assert f((bytes(range(16)), 5353), bytes(range(16)), 5353) is True


# ------------------------------------------------------------------------------------------
# udp_build.h / udp_recv.h under sanitizers
# ------------------------------------------------------------------------------------------
def test_udp_rules_under_sanitizers(tmp_path):
    """tests/cpp/udp_rules_test.cpp over udp_build.h / udp_recv.h alone, under ASan / UBSan: header
    bytes and sums against a byte-wise restatement, the 0 -> 0xffff rule, every refusal at its
    boundary (data_len near 2^32, offsets near 2^64), the receive's verdicts, and the reference
    frame's 42 header bytes -- its hex passed on the command line from kat.json -- rebuilt."""
    exe = tmp_path / "udp_rules_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "vproxy_amd", "csrc"),
                           os.path.join(REPO, "tests", "cpp", "udp_rules_test.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe), kat()["hex"]], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "udp_rules ok (with the reference frame)" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert "reference header 42 bytes, 61 payload bytes, ip sum 7f41, udp sum df0d" in r.stdout


# ------------------------------------------------------------------------------------------
# layouts, exports, budgets, refusals
# ------------------------------------------------------------------------------------------
def test_dtypes_are_the_headers_layouts():
    from vproxy_amd import vpcsum as V
    src = open(os.path.join(REPO, "include", "vpcsum.h")).read()
    assert V.UDPDG_DTYPE == U.UDPDG_DTYPE and V.UDPRX_DTYPE == U.UDPRX_DTYPE and V.TCPHDR_DTYPE == U.HDR_DTYPE
    assert V.UDPDG_DTYPE.itemsize == 32 and [V.UDPDG_DTYPE.fields[k][1] for k in V.UDPDG_DTYPE.names] == [0, 8, 16, 20, 24, 28]
    assert V.UDPRX_DTYPE.itemsize == 16 and [V.UDPRX_DTYPE.fields[k][1] for k in V.UDPRX_DTYPE.names] == [0, 8, 12, 13]
    for tag, dt in (("vpcsum_udpdg", V.UDPDG_DTYPE), ("vpcsum_udprx", V.UDPRX_DTYPE)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (tag, tag), src, re.S).group(1)
        names = re.findall(r"u?int\d+_t\s+(\w+)\s*(?:\[\d+\])?\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
        assert tuple(names) == dt.names
    assert "typedef vpcsum_tcphdr_t vpcsum_udphdr_t;" in src and re.search(r"#define VPCSUM_UDPRX_STORE\s+0x01u", src)
    assert re.search(r"#define VPCSUM_ABI_VERSION\s+4\b", src)   # additive: the version stays
    assert V.UDPRX_STORE == U.STORE == 1 and V.S_UDP_NOCSUM == U.S_UDP_NOCSUM


NEW = ("vpcsum_udp_build_async", "vpcsum_udp_recv_async", "vpcsum_ctx_build_udp_frames", "vpcsum_ctx_recv_udp_frames",
       "Java_io_vproxy_vpcsum_VPCsum_buildUdpFrames", "Java_io_vproxy_vpcsum_VPCsum_recvUdpFrames")


def test_exports_name_the_new_entry_points(L):
    from vproxy_amd import vpcsum as V
    for name in NEW:
        assert name in V.EXPORTS and hasattr(L, name), name
    assert set(NEW[:4]) <= set(V._PROBED)   # an older library still loads
    assert callable(V.udp_build) and callable(V.udp_recv) and callable(V.Context.build_udp_frames) and callable(V.Context.recv_udp_frames)


def test_udp_kernel_budgets():
    """k_udp_build and k_udp_recv in udp.hip.o: two kernels, no scratch, no LDS, and no more VGPRs than
    their TCP twins' 66 and 53."""
    from test_kernel_resources import kernels
    ks = kernels("udp.hip.o")
    assert len(ks) == 2, list(ks)
    b = next(v for k, v in ks.items() if "k_udp_build" in k)
    r = next(v for k, v in ks.items() if "k_udp_recv" in k)
    for v in (b, r):
        assert v["private_segment_fixed_size"] == 0 and v["group_segment_fixed_size"] == 0, v
    assert b["vgpr_count"] <= 66 and r["vgpr_count"] <= 53, (b, r)


def test_udp_entry_points_refuse_bad_arguments(L):
    """The device-pointer entries answer a NULL / misaligned argument with an error naming them before
    they touch a device; n == 0 succeeds; the ctx and PNI forms refuse a NULL context / negative n."""
    U32, U64, P = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    err = L.vpcsum_last_error
    buf = (ctypes.c_uint8 * 256)()
    p = (ctypes.addressof(buf) + 15) & ~15

    def bld(dst=p, src=p, hdr=p, dg=p, flen=p, out=p, st=p, n=1, n_hdr=1, src_len=64):
        return L.vpcsum_udp_build_async(P(dst), U64(64), P(src), U64(src_len), P(hdr), U32(n_hdr), P(dg), U32(n), P(flen),
                                        P(out), P(st), None)
    for kw, msg in ((dict(dst=None), b"NULL destination arena"), (dict(src=None), b"NULL source arena"),
                    (dict(hdr=None), b"NULL templates"), (dict(dg=None), b"NULL records"),
                    (dict(flen=None), b"NULL frame lengths"), (dict(dg=p + 4), b"records not 8-byte aligned"),
                    (dict(hdr=p + 2), b"templates not 4-byte aligned"), (dict(flen=p + 1), b"frame lengths not 4-byte aligned"),
                    (dict(out=p + 2), b"out words not 4-byte aligned"), (dict(n=(1 << 28) + 1), b"records > 2^28")):
        assert bld(**kw) != 0, kw
        assert b"vpcsum_udp_build_async: " in err() and msg in err(), (kw, err())
    assert bld(dst=None, src=None, hdr=None, dg=None, flen=None, out=None, st=None, n=0) == 0

    def rcv(arena=p, desc=p, rx=p, dst=p, stored=p, out=p, st=p, n=1):
        return L.vpcsum_udp_recv_async(P(arena), U64(64), P(desc), P(rx), U32(n), P(dst), U64(64), P(stored), P(out), P(st), None)
    for kw, msg in ((dict(arena=None), b"NULL arena"), (dict(desc=None), b"NULL descriptors or records"),
                    (dict(rx=None), b"NULL descriptors or records"), (dict(dst=None), b"NULL destination arena"),
                    (dict(stored=None), b"NULL stored counts"), (dict(rx=p + 4), b"not 8-byte aligned"),
                    (dict(stored=p + 2), b"stored counts not 4-byte aligned"), (dict(out=p + 1), b"out words not 4-byte aligned"),
                    (dict(n=(1 << 28) + 1), b"records > 2^28")):
        assert rcv(**kw) != 0, kw
        assert b"vpcsum_udp_recv_async: " in err() and msg in err(), (kw, err())
    assert rcv(arena=None, desc=None, rx=None, dst=None, stored=None, out=None, st=None, n=0) == 0
    t = U64()
    assert L.vpcsum_ctx_build_udp_frames(None, P(p), U64(64), P(p), U64(64), P(p), U32(1), P(p), U32(0), P(p), None, None,
                                         ctypes.byref(t)) != 0 and b"vpcsum_ctx_build_udp_frames: NULL context or ticket" in err()
    assert L.vpcsum_ctx_recv_udp_frames(None, P(p), U64(64), P(p), P(p), U32(0), P(p), U64(64), P(p), None, None,
                                        ctypes.byref(t)) != 0 and b"vpcsum_ctx_recv_udp_frames: " in err()

    class Env(ctypes.Structure):
        _fields_ = [("type", ctypes.c_char_p), ("message", ctypes.c_char * 4096), ("errno_", ctypes.c_int32), ("ret", ctypes.c_int64),
                    ("pad", ctypes.c_int64)]
    I32, I64 = ctypes.c_int32, ctypes.c_int64
    env = Env()
    assert L.Java_io_vproxy_vpcsum_VPCsum_buildUdpFrames(ctypes.byref(env), I64(0), P(p), I64(64), P(p), I64(64), P(p), I32(1), P(p),
                                                         I32(-1), P(p), None, None) != 0
    assert env.type == b"java.lang.IllegalArgumentException" and env.message == b"buildUdpFrames: negative size"
    env = Env()
    assert L.Java_io_vproxy_vpcsum_VPCsum_recvUdpFrames(ctypes.byref(env), I64(0), P(p), I64(64), P(p), P(p), I32(-1), P(p), I64(64),
                                                        P(p), None, None) != 0
    assert env.type == b"java.lang.IllegalArgumentException" and env.message == b"recvUdpFrames: negative size"
