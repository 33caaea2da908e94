"""CPU-side checks of the ICMP replies (vpcsum_icmp_reply_async, its ctx and PNI forms): the Python
restatement of the three Java builders (tests/icmpvec.py) against the oracle and the reference's two
echo test packets, the all-zero echo and the echo whose words sum to 0xffff, every refusal,
vswitch.plan_icmp_replies, the rules of icmp_reply.h in a stand-alone program under ASan / UBSan, the
layouts and exports, the kernel's budget read from the code object, and the argument refusals that
need no device."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

import icmpvec as C
from oracle import oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kat(name):
    ks = json.load(open(os.path.join(REPO, "tests", "golden", "kat.json")))["kats"]
    return next(k for k in ks if k["name"] == name)


@pytest.fixture(scope="module")
def L():
    from vproxy_amd import build
    lib = ctypes.CDLL(build.build())
    lib.vpcsum_last_error.restype = ctypes.c_char_p
    return lib


def tmpl(ver, l2, **kw):
    """The template of a reply to a request from icmpvec's default addresses."""
    return C.mk_hdr(ver, l2, C.V4_DST if ver == 4 else C.V6_DST, C.V4_SRC if ver == 4 else C.V6_SRC, **kw)


# ------------------------------------------------------------------------------------------
# the restatement
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ver,l2", [(4, 14), (6, 14), (6, 0), (4, 0)])
def test_restatement_replies_verify_with_the_oracle(ver, l2, orc):
    """What the restatement builds for each kind, described as the parse would, verifies with the
    oracle: S_L4_OK (and S_IP_OK on IPv4) with the sums it reports, for requests of many lengths, with
    IP options / an extension header that the reply does not carry over."""
    rng = np.random.default_rng(160 + ver + l2)
    h = tmpl(ver, l2, tos=0x2e, ttl=64, ident=0x1234, frag=0x4000)
    ipl = 20 if ver == 4 else 40
    want_st = C.S_DONE | C.S_L4_OK | (C.S_IP_OK if ver == 4 else 0)
    for n in list(range(4, 80)) + [1468]:
        body = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        for kw in ({}, {"ihl": 7} if ver == 4 else {"ext": 8}):
            for kind, (l3, l4_off) in ((C.ECHO, C.echo_l3(ver, body, code=5, **kw)), (C.UNREACH, C.udp_l3(ver, body, **kw)),
                                       (C.TIMEX, C.udp_l3(ver, body, **kw))):
                f, ipc, c = C.frame(h, kind, l3, l4_off)
                M = len(l3) - l4_off if kind == C.ECHO else 8 + min(len(l3), l4_off + 64)
                assert len(f) == l2 + ipl + M
                out, st = C.verify_reply(orc, f, h)
                assert st == want_st and out == ipc | (c << 16), (n, kind, kw)
                t, code = C.TYPE_CODE[(kind, ver == 4)]
                assert f[l2 + ipl] == t and f[l2 + ipl + 1] == code
                if kind == C.ECHO:
                    assert f[l2 + ipl + 4:] == l3[l4_off + 4:]
                else:
                    assert f[l2 + ipl + 4:l2 + ipl + 8] == bytes(4) and f[l2 + ipl + 8:] == l3[:l4_off + 64]


@pytest.mark.parametrize("name,ver", [("ipv4ByIcmpExample", 4), ("ipv6ByIcmpExample", 6)])
def test_restatement_answers_the_reference_echo_requests(name, ver, orc):
    """TestPacket's two pings: the request verifies with its pinned sum, the restatement's reply is
    the request with type 0 / 129, the addresses swapped by the template and a sum the oracle accepts."""
    k = kat(name)
    l3 = bytes.fromhex(k["hex"])
    l4_off = 20 if ver == 4 else 40
    assert l3[l4_off] == (8 if ver == 4 else 128) and k["proto"] == (1 if ver == 4 else 58)
    src, dst = (l3[12:16], l3[16:20]) if ver == 4 else (l3[8:24], l3[24:40])
    h = C.mk_hdr(ver, 14, src=dst, dst=src)
    arena = np.frombuffer(b"\xee" * 14 + l3, np.uint8)
    desc = np.array([C.mk_desc(14, len(l3), l4_off, ver, k["proto"])], O.DESC_DTYPE)
    rps = np.array([C.mk_rp(3, C.ECHO, frame_cap=14 + len(l3))], C.ICMPRP_DTYPE)
    dst_arena = np.full(3 + 14 + len(l3) + 5, 0xEE, np.uint8)
    after, flen, cs, out, st = C.reply(dst_arena, arena, desc, np.array([h], C.HDR_DTYPE), rps)
    assert list(flen) == [14 + len(l3)] and st[0] & C.S_L4_OK and int(out[0]) >> 16 == k["pinned"]["l4"]
    if ver == 4:
        assert st[0] & C.S_IP_OK and int(out[0]) & 0xffff == k["pinned"]["ip"]
    f = after[3:3 + int(flen[0])].tobytes()
    assert (after[:3] == 0xEE).all() and (after[3 + len(f):] == 0xEE).all()
    assert f[14 + l4_off] == (0 if ver == 4 else 129) and f[14 + l4_off + 4:] == l3[l4_off + 4:]
    o2, s2 = C.verify_reply(orc, f, h)
    assert s2 == C.S_DONE | C.S_L4_OK | (C.S_IP_OK if ver == 4 else 0) and o2 == int(cs[0])
    # the reply's sum differs from the request's by the type alone: 8 -> 0 adds 0x0800, 128 -> 129 takes 0x0100 (no carry here)
    if ver == 4:
        assert int(cs[0]) >> 16 == k["pinned"]["l4"] + 0x0800


def test_the_all_zero_echo_stores_ffff(orc):
    """An IPv4 echo request whose bytes 4.. are all zero: the reply (type 0, code 0) is all zero, Java's
    sum is an integer 0 and its complement 0xffff is stored -- where taking the request's first dword
    out of the whole-segment sum by one's complement subtraction would give 0x0000."""
    for n in (4, 8, 60):
        l3, l4_off = C.echo_l3(4, bytes(n), code=9)
        f, _, c = C.frame(tmpl(4, 14), C.ECHO, l3, l4_off)
        assert c == 0xffff and f[34:38] == b"\x00\x00\xff\xff" and not any(f[38:])
        assert C.verify_reply(orc, f, tmpl(4, 14))[1] & C.S_L4_OK
    # ICMPv6 has the pseudo-header: never an integer 0
    l3, l4_off = C.echo_l3(6, bytes(8))
    assert C.frame(tmpl(6, 14), C.ECHO, l3, l4_off)[2] not in (0, 0xffff)


def test_an_echo_whose_words_sum_to_ffff_stores_0000(orc):
    """Bytes 4..7 = ff ff 00 00, the rest zero: the reply's words sum to 0xffff and the field is 0x0000,
    stored as it is (ICMP has no UDP-style 0 -> 0xffff rule)."""
    l3, l4_off = C.echo_l3(4, b"\xff\xff\x00\x00" + bytes(24))
    h = tmpl(4, 14)
    f, _, c = C.frame(h, C.ECHO, l3, l4_off)
    assert c == 0 and f[34:40] == b"\x00\x00\x00\x00\xff\xff"
    out, st = C.verify_reply(orc, f, h)
    assert st & C.S_L4_OK and out >> 16 == 0


def test_restatement_refusals():
    """Every refusal, each at the value accepted and the first refused."""
    hdrs = np.array([tmpl(4, 14), tmpl(6, 0), C.mk_hdr(5), C.mk_hdr(4, 13), C.mk_hdr(4, rsv=1), C.mk_hdr(4, ack=1),
                     C.mk_hdr(6, window=0x100), C.mk_hdr(4, sport=1), C.mk_hdr(4, dport=0x100)], C.HDR_DTYPE)
    e4, o4 = C.echo_l3(4, bytes(range(56)))
    e6, o6 = C.echo_l3(6, bytes(range(56)))
    u4, _ = C.udp_l3(4, bytes(range(56)))
    ns, _ = C.echo_l3(6, bytes(20), typ=135)
    na, _ = C.echo_l3(6, bytes(20), typ=136)
    arena = np.frombuffer(e4 + e6 + u4 + ns + na + e6[:41], np.uint8)
    a4, a6, au, ans, ana, a1 = 0, len(e4), len(e4) + len(e6), len(e4) + len(e6) + len(u4), len(e4) + len(e6) + len(u4) + len(ns), \
        len(e4) + len(e6) + len(u4) + len(ns) + len(na)
    big = 1 << 40

    def ok(d, dst_len=big, arena=arena, **kw):
        args = dict(frame_off=0, kind=C.ECHO)
        args.update(kw)
        return C.plan(arena, d, hdrs, C.mk_rp(**args), dst_len)
    d4, d6, du = C.mk_desc(a4, 80, 20, 4, 1), C.mk_desc(a6, 100, 40, 6, 58), C.mk_desc(au, 84, 20, 4, 17)
    assert ok(d4) == 14 + 20 + 60 and ok(d6, hdr=1) == 40 + 60 and ok(du, kind=C.UNREACH) == 14 + 20 + 8 + 84
    assert ok(du, kind=C.TIMEX) == 126 and ok(d4, kind=C.TIMEX) == 14 + 20 + 8 + 80
    assert ok(d4, hdr=9) is None and ok(d4, hdr=0xffffffff) is None                     # hdr >= n_hdr
    assert all(ok(d4, hdr=k) is None for k in range(2, 9))                               # the template
    assert ok(d4, hdr=1) is None and ok(d6, hdr=0) is None                               # its version
    assert ok(d4, kind=0) is None and ok(d4, kind=4) is None and ok(d4, kind=255) is None
    assert all(ok(d4, rsv=1 << (8 * k)) is None for k in range(7))
    for fl in (O.F_L4P, O.F_RAW, O.F_PRE):
        assert ok(C.mk_desc(a4, 80, 20, 4, 1, flags=O.F_L4 | fl)) is None
        assert ok(C.mk_desc(au, 84, 20, 4, 17, flags=O.F_L4 | fl), kind=C.UNREACH) is None
        assert ok(C.mk_desc(au, 84, 20, 4, 17, flags=fl), kind=C.TIMEX) is None
    assert ok(C.mk_desc(a6, 100, 40, 6, 58, flags=O.F_L4 | O.F_IP), hdr=1) is None       # F_IP on IPv6
    assert ok(C.mk_desc(au, 84, 88, 4, 17), kind=C.TIMEX) is None and ok(C.mk_desc(au, 84, 16, 4, 17), kind=C.TIMEX) is None
    assert ok(C.mk_desc(au, 84, 22, 4, 17), kind=C.TIMEX) is None and ok(C.mk_desc(a6, 100, 39, 6, 17), kind=C.TIMEX, hdr=1) is None
    assert ok(C.mk_desc(au, 84, 84, 4, 17), kind=C.TIMEX) == 14 + 20 + 8 + 84            # all header: legal
    assert ok(C.mk_desc(len(arena) - 80, 80, 20, 4, 17), kind=C.TIMEX) is not None
    assert ok(C.mk_desc(len(arena) - 79, 80, 20, 4, 17), kind=C.TIMEX) is None and ok(C.mk_desc((1 << 64) - 8, 80, 20, 4, 17), kind=C.TIMEX) is None
    assert ok(d4, frame_cap=94) == 94 and ok(d4, frame_cap=93) is None                   # the chunk's room
    assert ok(d4, frame_off=906, dst_len=1000) == 94 and ok(d4, frame_off=907, dst_len=1000) is None
    assert ok(d4, frame_off=(1 << 64) - 1, dst_len=1000) is None
    # echo
    assert ok(C.mk_desc(a4, 80, 20, 4, 1, flags=O.F_IP)) is None                         # no F_L4
    assert ok(C.mk_desc(a4, 80, 20, 4, 58)) is None and ok(C.mk_desc(a6, 100, 40, 6, 1), hdr=1) is None
    assert ok(C.mk_desc(a4, 28, 20, 4, 1)) == 42 and ok(C.mk_desc(a4, 27, 20, 4, 1)) is None
    assert ok(C.mk_desc(au, 84, 20, 4, 1)) is None                                       # type 0x12, not 8
    assert ok(C.mk_desc(ans, 64, 40, 6, 58), hdr=1) is None                              # type 135, not 128
    # port unreachable: UDP only
    assert ok(d4, kind=C.UNREACH) is None and ok(C.mk_desc(au, 84, 20, 4, 6), kind=C.UNREACH) is None
    # time exceeded: NS / NA of at least one byte
    assert ok(C.mk_desc(ans, 64, 40, 6, 58), kind=C.TIMEX, hdr=1) is None and ok(C.mk_desc(ana, 64, 40, 6, 58), kind=C.TIMEX, hdr=1) is None
    assert ok(C.mk_desc(ans, 41, 40, 6, 58, flags=0), kind=C.TIMEX, hdr=1) is None
    assert ok(C.mk_desc(ans, 40, 40, 6, 58, flags=0), kind=C.TIMEX, hdr=1) == 40 + 8 + 40
    assert ok(C.mk_desc(ans, 64, 40, 6, 17), kind=C.TIMEX, hdr=1) is not None            # the byte is a port's
    assert ok(C.mk_desc(a1, 41, 40, 6, 58, flags=0), kind=C.TIMEX, hdr=1) == 40 + 8 + 41  # type 128: answered


def test_a_refused_record_leaves_the_destination_alone():
    l3, l4_off = C.echo_l3(4, bytes(range(20)))
    arena = np.frombuffer(l3, np.uint8)
    desc = np.array([C.mk_desc(0, len(l3), l4_off, 4, 1)] * 2, O.DESC_DTYPE)
    rps = np.array([C.mk_rp(0, C.ECHO, frame_cap=57), C.mk_rp(64, C.ECHO)], C.ICMPRP_DTYPE)
    dst = np.full(200, 0xEE, np.uint8)
    after, flen, cs, out, st = C.reply(dst, arena, desc, np.array([tmpl(4, 14)], C.HDR_DTYPE), rps)
    assert list(flen) == [0, 58] and list(st) == [C.S_BAD_DESC, C.S_DONE | C.S_IP_OK | C.S_L4_OK] and cs[0] == 0 and out[0] == 0
    assert (after[:64] == 0xEE).all() and (after[64 + 58:] == 0xEE).all() and not (after[64:64 + 58] == 0xEE).all()


def test_plan_icmp_replies():
    """vswitch.plan_icmp_replies: the NAT's S_TTL_EXPIRED gives time exceeded (and only that), a UDP
    descriptor the caller marks gives port unreachable, ICMP of its own family to a local address an
    echo candidate; a frame the parse refused, TCP, ICMP of the other family and everything unmarked
    get nothing."""
    from vproxy_amd import vpcsum as V
    from vproxy_amd import vswitch
    D = C.mk_desc
    desc = np.array([D(0, 84, 20, 4, 17), D(0, 84, 20, 4, 17), D(0, 84, 20, 4, 1), D(0, 84, 40, 6, 58), D(0, 84, 20, 4, 6),
                     D(0, 84, 40, 6, 1), D(0, 84, 20, 4, 1), D(0, 84, 20, 4, 17), D(0, 84, 20, 4, 1), D(0, 84, 20, 4, 6),
                     D(0, 84, 20, 4, 1, flags=O.F_IP)], O.DESC_DTYPE)
    st = np.full(len(desc), V.S_DONE, np.uint8)
    st[4] = V.S_BAD_DESC | V.S_TTL_EXPIRED      # TCP, TTL expired
    st[7] = V.S_BAD_DESC                        # the parse refused it
    st[8] = V.S_BAD_DESC | V.S_TTL_EXPIRED      # ICMP to a local address AND expired: the route node comes first
    miss = np.array([1, 0, 0, 0, 0, 0, 0, 1, 0, 1, 0], bool)
    local = np.array([1, 1, 1, 1, 0, 1, 0, 1, 1, 1, 1], bool)
    idx, kinds = vswitch.plan_icmp_replies(st, desc, miss, local)
    assert list(idx) == [0, 2, 3, 4, 8] and list(kinds) == [V.ICMP_PORT_UNREACH, V.ICMP_ECHO_REPLY, V.ICMP_ECHO_REPLY,
                                                            V.ICMP_TIME_EXCEEDED, V.ICMP_TIME_EXCEEDED]
    idx, kinds = vswitch.plan_icmp_replies(st, desc, miss, np.zeros(len(desc), bool))
    assert list(idx) == [0, 4, 8] and list(kinds) == [2, 3, 3]
    with pytest.raises(TypeError):   # which frames are local is the caller's to say: no default
        vswitch.plan_icmp_replies(st, desc, miss)
    idx, kinds = vswitch.plan_icmp_replies(st[:0], desc[:0], miss[:0], local[:0])
    assert len(idx) == 0 and len(kinds) == 0
    assert (V.ICMP_ECHO_REPLY, V.ICMP_PORT_UNREACH, V.ICMP_TIME_EXCEEDED) == (C.ECHO, C.UNREACH, C.TIMEX)


# ------------------------------------------------------------------------------------------
# icmp_reply.h under sanitizers
# ------------------------------------------------------------------------------------------
def test_icmp_rules_under_sanitizers(tmp_path):
    """tests/cpp/icmp_rules_test.cpp over icmp_reply.h alone, under ASan / UBSan: the lengths, q at
    its three cases, every refusal at its boundary (offsets near 2^64), the one type byte read last,
    and the header words with both sums against a byte-wise restatement."""
    exe = tmp_path / "icmp_rules_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "vproxy_amd", "csrc"),
                           os.path.join(REPO, "tests", "cpp", "icmp_rules_test.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "icmp_rules ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


# ------------------------------------------------------------------------------------------
# layouts, exports, budgets, refusals
# ------------------------------------------------------------------------------------------
def test_dtypes_are_the_headers_layouts():
    from vproxy_amd import vpcsum as V
    src = open(os.path.join(REPO, "include", "vpcsum.h")).read()
    assert V.ICMPRP_DTYPE == C.ICMPRP_DTYPE and V.TCPHDR_DTYPE == C.HDR_DTYPE
    assert V.ICMPRP_DTYPE.itemsize == 24 and [V.ICMPRP_DTYPE.fields[k][1] for k in V.ICMPRP_DTYPE.names] == [0, 8, 12, 16, 17]
    body = re.search(r"typedef struct vpcsum_icmprp \{(.*?)\} vpcsum_icmprp_t;", src, re.S).group(1)
    names = re.findall(r"u?int\d+_t\s+(\w+)\s*(?:\[\d+\])?\s*;", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert tuple(names) == V.ICMPRP_DTYPE.names
    assert "typedef vpcsum_tcphdr_t vpcsum_icmphdr_t;" in src
    for name, val in (("ECHO_REPLY", 1), ("PORT_UNREACH", 2), ("TIME_EXCEEDED", 3)):
        assert re.search(r"#define VPCSUM_ICMP_%s\s+%du" % (name, val), src) and getattr(V, "ICMP_" + name) == val
    assert re.search(r"#define VPCSUM_ABI_VERSION\s+4\b", src)   # additive: the version stays


NEW = ("vpcsum_icmp_reply_async", "vpcsum_ctx_reply_icmp_frames", "Java_io_vproxy_vpcsum_VPCsum_replyIcmpFrames")


def test_exports_name_the_new_entry_points(L):
    from vproxy_amd import vpcsum as V
    for name in NEW:
        assert name in V.EXPORTS and hasattr(L, name), name
    assert set(NEW[:2]) <= set(V._PROBED)   # an older library still loads
    assert callable(V.icmp_reply) and callable(V.Context.reply_icmp_frames)
    java = open(os.path.join(REPO, "java", "io", "vproxy", "vpcsum", "VPCsum.java")).read()
    assert "replyIcmpFrames" in java and "icmpRp" in java


def test_icmp_kernel_budget():
    """k_icmp_reply in icmp.hip.o: one kernel, no scratch, no LDS; the mover's groups in flight, the
    template's 16 words and the record fit in 96 VGPRs, which keeps 5 waves per SIMD of 512."""
    from test_kernel_resources import kernels
    ks = kernels("icmp.hip.o")
    assert len(ks) == 1 and "k_icmp_reply" in next(iter(ks)), list(ks)
    v = next(iter(ks.values()))
    assert v["private_segment_fixed_size"] == 0 and v["group_segment_fixed_size"] == 0, v
    assert v["vgpr_count"] <= 96, v


def test_icmp_entry_points_refuse_bad_arguments(L):
    """The device-pointer entry answers a NULL / misaligned argument with an error naming it before
    it touches a device; n == 0 succeeds; the ctx and PNI forms refuse a NULL context / negative n."""
    U32, U64, P = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    err = L.vpcsum_last_error
    buf = (ctypes.c_uint8 * 256)()
    p = (ctypes.addressof(buf) + 15) & ~15

    def rp(arena=p, desc=p, hdr=p, rps=p, dst=p, flen=p, cs=p, out=p, st=p, n=1, n_hdr=1):
        return L.vpcsum_icmp_reply_async(P(arena), U64(64), P(desc), P(hdr), U32(n_hdr), P(rps), U32(n), P(dst), U64(64), P(flen),
                                         P(cs), P(out), P(st), None)
    for kw, msg in ((dict(arena=None), b"NULL arena"), (dict(desc=None), b"NULL descriptors or records"),
                    (dict(rps=None), b"NULL descriptors or records"), (dict(hdr=None), b"NULL templates"),
                    (dict(dst=None), b"NULL destination arena"), (dict(flen=None), b"NULL frame lengths"),
                    (dict(rps=p + 4), b"not 8-byte aligned"), (dict(desc=p + 4), b"not 8-byte aligned"),
                    (dict(hdr=p + 2), b"templates not 4-byte aligned"), (dict(flen=p + 1), b"frame lengths not 4-byte aligned"),
                    (dict(cs=p + 2), b"sum or out words not 4-byte aligned"), (dict(out=p + 1), b"sum or out words not 4-byte aligned"),
                    (dict(n=(1 << 28) + 1), b"records > 2^28")):
        assert rp(**kw) != 0, kw
        assert b"vpcsum_icmp_reply_async: " in err() and msg in err(), (kw, err())
    assert rp(arena=None, desc=None, hdr=None, rps=None, dst=None, flen=None, cs=None, out=None, st=None, n=0) == 0
    t = U64()
    assert L.vpcsum_ctx_reply_icmp_frames(None, P(p), U64(64), P(p), P(p), U32(1), P(p), U32(0), P(p), U64(64), P(p), None, None, None,
                                          ctypes.byref(t)) != 0 and b"vpcsum_ctx_reply_icmp_frames: NULL context or ticket" in err()

    class Env(ctypes.Structure):
        _fields_ = [("type", ctypes.c_char_p), ("message", ctypes.c_char * 4096), ("errno_", ctypes.c_int32), ("ret", ctypes.c_int64),
                    ("pad", ctypes.c_int64)]
    I32, I64 = ctypes.c_int32, ctypes.c_int64
    env = Env()
    assert L.Java_io_vproxy_vpcsum_VPCsum_replyIcmpFrames(ctypes.byref(env), I64(0), P(p), I64(64), P(p), P(p), I32(1), P(p), I32(-1),
                                                          P(p), I64(64), P(p), None, None, None) != 0
    assert env.type == b"java.lang.IllegalArgumentException" and env.message == b"replyIcmpFrames: negative size"
