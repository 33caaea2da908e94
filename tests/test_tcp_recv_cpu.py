"""CPU-side checks of the TCP receive (vpcsum_tcp_recv_async, vpcsum_tcp_digest_async,
vpcsum_ctx_recv_tcp_frames, VPCsum.recvTcpFrames): the layouts the binding, the header and the
kernels share, the rules of tcp_recv.h in a stand-alone program under ASan / UBSan, the kernels'
budgets read from the code object, the argument refusals that need no device, plan_tcp_store, and
the Python restatement of the rule (tests/tcprecvvec.py) on the TCP frames of cap-ether.pcap."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import tcprecvvec as R
from oracle import oracle as O
from pcaputil import l3_offset, read_pcap

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")


@pytest.fixture(scope="module")
def L():
    from vproxy_amd import build
    lib = ctypes.CDLL(build.build())
    lib.vpcsum_last_error.restype = ctypes.c_char_p
    return lib


# ------------------------------------------------------------------------------------------
# layouts, exports, budgets
# ------------------------------------------------------------------------------------------
def _struct_fields(src, tag):
    m = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (tag, tag), src, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    out = []
    for ty, names in re.findall(r"(\w+)\s+([^;]+);", body):
        for nm in names.split(","):
            m2 = re.match(r"\s*(\w+)\s*(?:\[(\d+)\])?\s*$", nm)
            out.append((ty, m2.group(1), m2.group(2)))
    return out


CTYPE = {"uint8_t": "u1", "uint16_t": "<u2", "uint32_t": "<u4", "uint64_t": "<u8"}


def test_dtypes_are_the_headers_layouts():
    """TCPRX_DTYPE / TCPINFO_DTYPE (the binding's and the restatement's) equal vpcsum_tcprx_t /
    vpcsum_tcpinfo_t as the header declares them: names, types, natural offsets, 16 bytes each; the
    ABI version stays 4."""
    from vproxy_amd import vpcsum as V
    src = open(os.path.join(REPO, "include", "vpcsum.h")).read()
    for tag, dts, nf in (("vpcsum_tcprx", (V.TCPRX_DTYPE, R.TCPRX_DTYPE), 5), ("vpcsum_tcpinfo", (V.TCPINFO_DTYPE, R.TCPINFO_DTYPE), 7)):
        fields = _struct_fields(src, tag)
        assert len(fields) == nf, fields
        want = np.dtype([(nm, CTYPE[ty], int(cnt)) if cnt else (nm, CTYPE[ty]) for ty, nm, cnt in fields], align=True)
        assert want.itemsize == 16
        for dt in dts:
            assert dt.itemsize == 16 and dt.names == want.names
            assert [dt.fields[k][1] for k in dt.names] == [want.fields[k][1] for k in want.names]
            assert [dt.fields[k][0] for k in dt.names] == [want.fields[k][0] for k in want.names]
    assert [V.TCPRX_DTYPE.fields[k][1] for k in V.TCPRX_DTYPE.names] == [0, 8, 12, 14, 15]
    assert [V.TCPINFO_DTYPE.fields[k][1] for k in V.TCPINFO_DTYPE.names] == [0, 4, 8, 10, 12, 13, 14]
    assert re.search(r"#define VPCSUM_TCPRX_STORE\s+0x01u", src) and V.TCPRX_STORE == R.STORE == 1
    assert re.search(r"#define VPCSUM_ABI_VERSION\s+4\b", src)   # additive: the version stays


def test_exports_name_the_new_entry_points(L):
    from vproxy_amd import vpcsum as V
    for name in ("vpcsum_tcp_recv_async", "vpcsum_tcp_digest_async", "vpcsum_ctx_recv_tcp_frames",
                 "Java_io_vproxy_vpcsum_VPCsum_recvTcpFrames"):
        assert name in V.EXPORTS and hasattr(L, name), name
    assert callable(V.tcp_recv) and callable(V.tcp_digest) and callable(V.Context.recv_tcp_frames)
    assert L.vpcsum_abi_version() == 4
    from vproxy_amd import build
    assert "tcp_recv.hip" in build.SOURCES and "tcp_recv.h" in build.HEADERS


def test_tcp_recv_kernel_budgets():
    """tcp_recv.hip.o holds k_tcp_recv and k_tcp_digest and nothing else; neither uses scratch or
    LDS; k_tcp_recv stays within 80 VGPRs (6 waves per SIMD, K2's bar)."""
    from test_kernel_resources import kernels
    ks = kernels("tcp_recv.hip.o")
    assert len(ks) == 2, list(ks)
    rv = [v for k, v in ks.items() if "k_tcp_recv" in k]
    dg = [v for k, v in ks.items() if "k_tcp_digest" in k]
    assert len(rv) == 1 and len(dg) == 1, list(ks)
    for v in rv + dg:
        assert v["private_segment_fixed_size"] == 0 and v["group_segment_fixed_size"] == 0, v
    print("k_tcp_recv vgprs", rv[0]["vgpr_count"], "k_tcp_digest vgprs", dg[0]["vgpr_count"])
    assert rv[0]["vgpr_count"] <= 80, rv[0]


# ------------------------------------------------------------------------------------------
# tcp_recv.h under sanitizers
# ------------------------------------------------------------------------------------------
def test_tcp_recv_rules_under_sanitizers(tmp_path):
    """tests/cpp/tcp_recv_test.cpp over tcp_recv.h alone, under ASan / UBSan: every refusal at its
    edge and inside it, the no-wrap bounds at UINT64_MAX, skip == data_len."""
    exe = tmp_path / "tcp_recv_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "vproxy_amd", "csrc"),
                           os.path.join(REPO, "tests", "cpp", "tcp_recv_test.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tcp_recv ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


# ------------------------------------------------------------------------------------------
# argument refusals without a device
# ------------------------------------------------------------------------------------------
def test_tcp_recv_entry_points_refuse_bad_arguments(L):
    """Each new entry point answers a NULL / misaligned / negative argument with an error and a
    message naming it, before it touches a device; n == 0 succeeds."""
    U32, U64, P = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    err = L.vpcsum_last_error
    buf = (ctypes.c_uint8 * 256)()
    p = (ctypes.addressof(buf) + 15) & ~15

    def dev(arena=p, desc=p, rx=p, dst=p, stored=p, out=p, st=p, n=1, dst_len=64):
        return L.vpcsum_tcp_recv_async(P(arena), U64(64), P(desc), P(rx), U32(n), P(dst), U64(dst_len), P(stored), P(out), P(st),
                                       None)
    for kw, msg in ((dict(arena=None), b"NULL arena"), (dict(desc=None), b"NULL descriptors or records"),
                    (dict(rx=None), b"NULL descriptors or records"), (dict(dst=None), b"NULL destination arena"),
                    (dict(stored=None), b"NULL stored counts"), (dict(desc=p + 4), b"descriptors or records not 8-byte aligned"),
                    (dict(rx=p + 4), b"descriptors or records not 8-byte aligned"),
                    (dict(stored=p + 2), b"stored counts not 4-byte aligned"), (dict(out=p + 1), b"out words not 4-byte aligned"),
                    (dict(n=(1 << 28) + 1), b"records > 2^28")):
        assert dev(**kw) != 0, kw
        assert b"vpcsum_tcp_recv_async: " in err() and msg in err(), (kw, err())
    assert dev(arena=None, desc=None, rx=None, dst=None, stored=None, out=None, st=None, n=0) == 0   # nothing to do

    def dig(arena=p, desc=p, info=p, n=1):
        return L.vpcsum_tcp_digest_async(P(arena), U64(64), P(desc), U32(n), P(info), None)
    for kw, msg in ((dict(arena=None), b"NULL arena"), (dict(desc=None), b"NULL descriptors or records"),
                    (dict(info=None), b"NULL descriptors or records"), (dict(desc=p + 4), b"descriptors not 8-byte aligned"),
                    (dict(info=p + 8), b"records not 16-byte aligned")):
        assert dig(**kw) != 0, kw
        assert b"vpcsum_tcp_digest_async: " in err() and msg in err(), (kw, err())
    assert dig(arena=None, desc=None, info=None, n=0) == 0
    t = U64()

    def ctx(c=None, n=0, tk=ctypes.byref(t)):
        return L.vpcsum_ctx_recv_tcp_frames(P(c), P(p), U64(64), P(p), P(p), U32(n), P(p), U64(64), P(p), None, None, tk)
    assert ctx() != 0 and b"vpcsum_ctx_recv_tcp_frames: NULL context or ticket" in err()
    assert ctx(c=p, n=1, tk=None) != 0 and b"vpcsum_ctx_recv_tcp_frames: NULL context or ticket" in err()

    def pni(ctx_h=0, arena_len=64, dst_len=64, n=0):
        env = (ctypes.c_uint8 * 4128)()   # a PNIEnv_vpcsum_long
        rc = L.Java_io_vproxy_vpcsum_VPCsum_recvTcpFrames(ctypes.byref(env), ctypes.c_int64(ctx_h), P(p), ctypes.c_int64(arena_len),
                                                          P(p), P(p), ctypes.c_int32(n), P(p), ctypes.c_int64(dst_len), P(p), None,
                                                          None)
        return rc, bytes(env[8:8 + 80]).split(b"\0")[0], ctypes.cast(ctypes.byref(env), ctypes.POINTER(ctypes.c_char_p))[0]
    for kw in (dict(n=-1), dict(arena_len=-1), dict(dst_len=-1)):
        rc, msg, typ = pni(**kw)
        assert rc != 0 and msg == b"recvTcpFrames: negative size" and typ == b"java.lang.IllegalArgumentException", (kw, msg)
    rc, msg, typ = pni()
    assert rc != 0 and b"vpcsum_ctx_recv_tcp_frames: NULL context or ticket" in msg and typ == b"java.io.IOException"


# ------------------------------------------------------------------------------------------
# ReceivingQueue.store on integers
# ------------------------------------------------------------------------------------------
def test_plan_tcp_store_branches():
    """The four branches of ReceivingQueue.store, at their edges: past the expected byte -> dropped;
    ending at or before it -> dropped; beginning before it -> trimmed by the difference; beginning
    on it -> whole.  vswitch.plan_tcp_store against the tests' own restatement over a grid."""
    from vproxy_amd.vswitch import plan_tcp_store
    assert plan_tcp_store(1000, 1001, 10) is None and plan_tcp_store(1000, 5000, 1) is None
    assert plan_tcp_store(1000, 990, 10) is None and plan_tcp_store(1000, 900, 10) is None
    assert plan_tcp_store(1000, 1000, 0) is None and plan_tcp_store(1000, 999, 1) is None
    assert plan_tcp_store(1000, 990, 11) == (10, 1) and plan_tcp_store(1000, 999, 1460) == (1, 1459)
    assert plan_tcp_store(1000, 1000, 1) == (0, 1) and plan_tcp_store(1000, 1000, 1460) == (0, 1460)
    assert plan_tcp_store((1 << 32) + 5, (1 << 32) + 2, 4) == (3, 1)   # the stack's seqs are longs
    for e in (0, 7, 1000):
        for s in range(max(0, e - 5), e + 4):
            for d in range(0, 8):
                assert plan_tcp_store(e, s, d) == R.plan_tcp_store(e, s, d), (e, s, d)


# ------------------------------------------------------------------------------------------
# the restatement on the reference's captured frames
# ------------------------------------------------------------------------------------------
def cap_ether():
    """(arena, desc) of cap-ether.pcap's IP frames laid at 2,048-byte chunks + 384."""
    lt, pkts = read_pcap(os.path.join(GOLD, "pcap", "cap-ether.pcap"))
    arena = np.full(len(pkts) * 2048, 0x5a, np.uint8)
    desc = []
    for i, p in enumerate(pkts):
        off = l3_offset(lt, p)
        if off is None:
            continue
        info, err = O.parse_l3(p, off, len(p) - off)
        assert err is None, err
        at = i * 2048 + 384
        arena[at:at + len(p)] = np.frombuffer(p, np.uint8)
        desc.append((at + off, info.l3_len, info.l4_off, info.ver, info.proto, O.desc_flags_for(info), 0))
    return arena, np.array(desc, O.DESC_DTYPE)


def test_restatement_on_the_captured_frames(orc):
    """cap-ether.pcap: 13 TCP frames, 3 with payload (77, 81 and 305 bytes), header lengths 20 and 40,
    7 correct stored sums and 6 CHECKSUM_PARTIAL ones.  The restatement stores exactly the payload
    bytes, its status equals the oracle's for all 13, and its digest names each header."""
    arena, desc = cap_ether()
    assert len(desc) == 13 and (desc["l4_proto"] == 6).all()
    n = len(desc)
    info = R.digest(arena, desc)
    assert sorted(int(x) for x in info["data_len"] if x) == [77, 81, 305]
    assert set(int(x) for x in info["hlen"]) == {20, 40}
    rx = np.zeros(n, R.TCPRX_DTYPE)
    pos = 3
    for i in range(n):
        rx[i] = R.mk_rx(pos, int(info["data_len"][i]), 0, R.STORE if info["data_len"][i] else 0)
        pos += int(info["data_len"][i]) + 3
    dst = np.full(pos, 0xEE, np.uint8)
    before = arena.copy()
    after, stored, out, st = R.recv(dst, arena, desc, rx)
    o_out, o_st = orc.process(arena, desc, O.MODE_VERIFY)
    assert (st == o_st).all() and (out == o_out).all() and (arena == before).all() and (dst == 0xEE).all()
    assert int(np.count_nonzero(st & O.S_L4_OK)) == 7 and (st & O.S_IP_OK).all() and (st & O.S_DONE).all()
    assert sorted(int(x) for x in stored if x) == [77, 81, 305] and int(stored.sum()) == 463
    want = np.full(pos, 0xEE, np.uint8)
    for i in range(n):
        k = int(info["data_len"][i])
        a = int(desc[i]["l3_off"]) + int(desc[i]["l4_off"]) + int(info["hlen"][i])
        want[int(rx[i]["dst_off"]):int(rx[i]["dst_off"]) + k] = arena[a:a + k]
        # the digest against the frame's own bytes
        t = arena[a - int(info["hlen"][i]):a].tobytes()
        assert int(info["seq"][i]) == int.from_bytes(t[4:8], "big") and int(info["flags"][i]) == t[13] & 0x3f
        assert O._tcp_from(arena[a - int(info["hlen"][i]):int(desc[i]["l3_off"]) + int(desc[i]["l3_len"])].tobytes()) is None
    assert (after == want).all()
    # a trimmed segment: skip 5 of the 77-byte payload
    i = int(np.flatnonzero(info["data_len"] == 77)[0])
    rx2 = rx.copy()
    rx2[i]["skip"], rx2[i]["dst_cap"] = 5, 72
    after2, stored2, _, st2 = R.recv(dst, arena, desc, rx2)
    a = int(desc[i]["l3_off"]) + int(desc[i]["l4_off"]) + int(info["hlen"][i])
    do = int(rx[i]["dst_off"])
    assert stored2[i] == 72 and (after2[do:do + 72] == arena[a + 5:a + 77]).all() and (after2[do + 72:do + 77] == 0xEE).all()
    assert (st2 == o_st).all()
