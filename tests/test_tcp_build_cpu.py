"""CPU-side checks of the TCP segment build (vpcsum_tcp_build_async, vpcsum_ctx_build_tcp_frames,
VPCsum.buildTcpFrames): the Python restatement of the frame rule (tests/tcpbuildvec.py) against the
reference's own test frame and the oracle's parser, the host-checkable rules of tcp_build.h and the
payload mover of team_move.h in stand-alone programs under ASan / UBSan, the layouts the binding,
the header and the kernel share, the kernel's budget read from the code object, and the argument
refusals that need no device."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import tcpbuildvec as B
from oracle import oracle as O

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kat(name="tcpIpv4PshExample"):
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
    """tcpIpv4PshExample (PSH|ACK, IHL 5, data offset 5, 517 payload bytes, DF set): template and
    record read out of the fixture, the frame rebuilt by the rule -- byte-equal to the 571-byte
    fixture, with its pinned sums 0x85f7 / 0x0aa9."""
    k = kat()
    raw = bytes.fromhex(k["hex"])
    assert len(raw) == 571 and (k["pinned"]["ip"], k["pinned"]["l4"]) == (0x85f7, 0x0aa9)
    h, rec, payload = B.from_frame(raw)
    assert len(payload) == 517 and rec["flags"] == B.PSH | B.ACK and h["frag"].tobytes() == b"\x40\x00"
    src = np.frombuffer(b"\x11" * 5 + payload + b"\x22" * 3, np.uint8)
    dst = np.full(7 + 571 + 9, 0xEE, np.uint8)
    seg = np.array([B.mk_seg(7, 5, 517, seq=rec["seq"], flags=rec["flags"])], B.TCPSEG_DTYPE)
    after, flen, out, st = B.build(dst, src, np.array([h], B.TCPHDR_DTYPE), seg)
    assert after[7:7 + 571].tobytes() == raw
    assert (after[:7] == 0xEE).all() and (after[7 + 571:] == 0xEE).all() and (dst == 0xEE).all()
    assert list(flen) == [571] and list(st) == [B.S_DONE] and int(out[0]) == 0x85f7 | (0x0aa9 << 16)


@pytest.mark.parametrize("ver,l2", [(4, 14), (6, 14), (6, 0), (4, 0)])
def test_restatement_frames_parse_and_carry_their_sums(ver, l2):
    """Every IPv6 and every l2_len 14 frame the restatement builds parses with the oracle's
    EthernetPacket.from rules, and l4_csum over it equals the stored field; the header's first 8
    bytes equal hand-written hex."""
    rng = np.random.default_rng(31)
    src16, dst16 = bytes(range(0x20, 0x30)), bytes(range(0x40, 0x50))
    h = B.mk_hdr(ver, l2, src16 if ver == 6 else src16[:4], dst16 if ver == 6 else dst16[:4], 0x1234, 443, 0xdeadbeef, 0x7fff,
                 tos=0x5c, ttl=64, ident=0xabcd, frag=0x4000)
    for d in (0, 1, 2, 517, 1460):
        payload = bytes(rng.integers(0, 256, d, dtype=np.uint8))
        s = B.mk_seg(0, 0, d, seq=0x01020304, flags=B.PSH | B.ACK, hlen=B.header_len(h))
        f, ipc, l4c = B.frame(h, s, payload)
        assert len(f) == l2 + (20 if ver == 4 else 40) + 20 + d
        l3 = f[l2:]
        if ver == 4:
            assert l3[:8].hex() == "455c" + f"{40 + d:04x}" + "abcd4000"
            assert O.ipv4_header_csum(l3, 20) == ipc == int.from_bytes(l3[10:12], "big")
        else:
            assert l3[:8].hex() == "65c00000" + f"{20 + d:04x}" + "0640" and ipc == 0
        if l2:
            assert f[:14].hex() == "0200" "0000" "0a01" "0200" "0000" "0b02" + ("0800" if ver == 4 else "86dd")
        l4o = 20 if ver == 4 else 40
        assert l3[l4o:l4o + 16].hex() == "123401bb" "01020304" "deadbeef" "5018" "7fff"
        assert l3[l4o + 18:l4o + 20] == b"\x00\x00" and l3[l4o + 20:] == payload
        assert O.l4_csum(l3, len(l3), l4o, ver, 6) == l4c == int.from_bytes(l3[l4o + 16:l4o + 18], "big")
        if l2:
            info, why = O.parse_ether(f)
            assert info is not None, why
            assert (info.l3_off, info.l3_len, info.l4_off, info.ver, info.proto) == (14, len(l3), l4o, ver, 6)
        else:
            info, why = O.parse_l3(f, 0, len(f))
            assert info is not None and (info.l3_len, info.l4_off, info.proto) == (len(l3), l4o, 6), why


def test_restatement_refusals_and_lengths():
    """Each refusal of the header's list at the value that is accepted and one past it; a refused
    record writes nothing and reports frame_len 0, out 0, S_BAD_DESC."""
    hs = np.array([B.mk_hdr(4, 14), B.mk_hdr(6, 0), B.mk_hdr(5, 14), B.mk_hdr(4, 18), B.mk_hdr(4, 14, rsv=1)], B.TCPHDR_DTYPE)
    ok = lambda s, dl=1 << 20, sl=1 << 20, hdrs=hs: not B.refused(hdrs, s, dl, sl)   # noqa: E731
    assert ok(B.mk_seg(0, 0, 10)) and ok(B.mk_seg(0, 0, 10, hdr=1, hlen=60))
    assert not ok(B.mk_seg(0, 0, 10, hdr=5)) and not ok(B.mk_seg(0, 0, 10, hdr=0), hdrs=hs[:0])
    assert not ok(B.mk_seg(0, 0, 10, hdr=2)) and not ok(B.mk_seg(0, 0, 10, hdr=3, hlen=58)) and not ok(B.mk_seg(0, 0, 10, hdr=4))
    assert ok(B.mk_seg(0, 0, 0, flags=0x3f)) and not ok(B.mk_seg(0, 0, 0, flags=0x40)) and not ok(B.mk_seg(0, 0, 0, rsv=1))
    assert ok(B.mk_seg(0, 0, 10, frame_cap=64)) and not ok(B.mk_seg(0, 0, 10, frame_cap=63))
    assert ok(B.mk_seg(0, 0, 65495, frame_cap=1 << 17)) and not ok(B.mk_seg(0, 0, 65496, frame_cap=1 << 17))
    assert ok(B.mk_seg(0, 0, 65515, hdr=1, frame_cap=1 << 17)) and not ok(B.mk_seg(0, 0, 65516, hdr=1, frame_cap=1 << 17))
    assert ok(B.mk_seg(100 - 64, 0, 10), dl=100) and not ok(B.mk_seg(100 - 63, 0, 10), dl=100)
    assert ok(B.mk_seg(0, 90, 10), sl=100) and not ok(B.mk_seg(0, 91, 10), sl=100)
    assert not ok(B.mk_seg((1 << 64) - 8, 0, 10)) and not ok(B.mk_seg(0, (1 << 64) - 4, 10))
    dst = np.full(200, 0xEE, np.uint8)
    src = np.arange(50, dtype=np.uint8)
    segs = np.array([B.mk_seg(3, 1, 10), B.mk_seg(100, 45, 10), B.mk_seg(100, 1, 10, hdr=2)], B.TCPSEG_DTYPE)
    after, flen, out, st = B.build(dst, src, hs, segs)
    assert list(flen) == [64, 0, 0] and list(st) == [B.S_DONE, B.S_BAD_DESC, B.S_BAD_DESC] and out[1] == out[2] == 0
    assert (after[67:] == 0xEE).all() and (after[:3] == 0xEE).all() and after[57:67].tobytes() == bytes(range(1, 11))


# ------------------------------------------------------------------------------------------
# tcp_build.h under sanitizers
# ------------------------------------------------------------------------------------------
def test_tcp_build_rules_under_sanitizers(tmp_path):
    """tests/cpp/tcp_build_test.cpp over tcp_build.h alone, under ASan / UBSan: header bytes and L
    for IPv4 / IPv6 x l2_len 0 / 14, every refusal at its boundary and one past it (offsets near
    2^64 included), and the reference frame's 54 header bytes -- its hex and record fields passed
    on the command line from kat.json -- rebuilt with both sums."""
    exe = tmp_path / "tcp_build_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "vproxy_amd", "csrc"),
                           os.path.join(REPO, "tests", "cpp", "tcp_build_test.cpp"), "-o", str(exe)])
    k = kat()
    raw = bytes.fromhex(k["hex"])
    _, rec, _ = B.from_frame(raw)
    r = subprocess.run([str(exe), k["hex"], str(rec["seq"]), str(rec["flags"])], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tcp_build ok (with the reference frame)" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert "reference header 54 bytes, ip sum 85f7, tcp sum 0aa9" in r.stdout


def test_team_move_under_sanitizers(tmp_path):
    """tests/cpp/team_move_test.cpp: team_move.h's mover, the one k_tcp_build and k_tcp_recv run,
    compiled for the host alone and run under ASan / UBSan over a source block that is exactly the
    segment's 4-byte aligned hull and a destination block that ends at the last stored byte --
    lengths 0..80 and 1,460, every destination residue mod 16 and source residue mod 4, the stored
    range from every offset of the segment (none, inside one dword, inside one group), stored bytes
    and the sum against a byte-wise reference."""
    from vproxy_amd import build
    cc = shutil.which(build.hipcc())
    if cc is None:
        pytest.skip("hipcc not found")
    exe = tmp_path / "team_move_test"
    subprocess.check_call([cc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(REPO, "include"),
                           "-I", os.path.join(REPO, "vproxy_amd", "csrc"),
                           os.path.join(REPO, "tests", "cpp", "team_move_test.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "team_move ok: " in r.stdout, (r.returncode, r.stdout, r.stderr)


# ------------------------------------------------------------------------------------------
# layouts, exports, budgets, refusals
# ------------------------------------------------------------------------------------------
def _struct_fields(src, tag):
    m = re.search(r"typedef struct %s \{(.*?)\} %s_t;" % (tag, tag), src, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    return re.findall(r"(\w+)\s+(\w+)\s*(?:\[(\d+)\])?\s*;", body)


CTYPE = {"uint8_t": "u1", "uint16_t": "<u2", "uint32_t": "<u4", "uint64_t": "<u8"}


def test_dtypes_are_the_headers_layouts():
    """TCPHDR_DTYPE / TCPSEG_DTYPE (the binding's and the restatement's) equal vpcsum_tcphdr_t /
    vpcsum_tcpseg_t as the header declares them: names, types, array sizes, natural offsets, 64 and
    32 bytes; the ABI version stays 4."""
    from vproxy_amd import vpcsum as V
    src = open(os.path.join(REPO, "include", "vpcsum.h")).read()
    for tag, dts, size in (("vpcsum_tcphdr", (V.TCPHDR_DTYPE, B.TCPHDR_DTYPE), 64),
                           ("vpcsum_tcpseg", (V.TCPSEG_DTYPE, B.TCPSEG_DTYPE), 32)):
        fields = _struct_fields(src, tag)
        assert len(fields) == (15 if size == 64 else 8)
        want = np.dtype([(nm, CTYPE[ty], int(cnt)) if cnt else (nm, CTYPE[ty]) for ty, nm, cnt in fields], align=True)
        assert want.itemsize == size
        for dt in dts:
            assert dt.itemsize == size and dt.names == want.names
            assert [dt.fields[k][1] for k in dt.names] == [want.fields[k][1] for k in want.names]
            assert [dt.fields[k][0] for k in dt.names] == [want.fields[k][0] for k in want.names]
    assert [V.TCPSEG_DTYPE.fields[k][1] for k in V.TCPSEG_DTYPE.names] == [0, 8, 16, 20, 24, 28, 30, 31]
    assert V.TCPHDR_DTYPE.fields["src"][1] == 16 and V.TCPHDR_DTYPE.fields["sport"][1] == 48 and V.TCPHDR_DTYPE.fields["rsv"][1] == 62
    assert re.search(r"#define VPCSUM_ABI_VERSION\s+4\b", src)   # additive: the version stays
    assert (B.S_DONE, B.S_BAD_DESC) == (V.S_DONE, V.S_BAD_DESC)


def test_exports_name_the_new_entry_points(L):
    from vproxy_amd import vpcsum as V
    for name in ("vpcsum_tcp_build_async", "vpcsum_ctx_build_tcp_frames", "Java_io_vproxy_vpcsum_VPCsum_buildTcpFrames"):
        assert name in V.EXPORTS and hasattr(L, name), name
    assert callable(V.tcp_build) and callable(V.Context.build_tcp_frames)


def test_tcp_build_kernel_budget():
    """k_tcp_build in tcp_build.hip.o: one kernel, no scratch, no LDS, at most 72 VGPRs -- 7 waves
    per SIMD, the occupancy DESIGN.md §7 states for it; none of test_kernel_resources' patterns
    matches its name."""
    from test_kernel_resources import kernels
    ks = kernels("tcp_build.hip.o")
    tb = {k: v for k, v in ks.items() if "k_tcp_build" in k}
    assert len(tb) == 1 and len(ks) == 1, list(ks)
    name, v = next(iter(tb.items()))
    assert v["private_segment_fixed_size"] == 0 and v["group_segment_fixed_size"] == 0, v
    assert v["vgpr_count"] <= 72, v
    assert not re.search(r"k_natq|k_natw|k_natILi|k_parse_ether|k_csum|k_pattern_probe|k_read_probe|k_pre|k_flow", name)


def test_tcp_build_entry_points_refuse_bad_arguments(L):
    """Each of the three new entry points answers a NULL / misaligned / negative argument with an
    error and a message naming it, before it touches a device; n == 0 succeeds."""
    U32, U64, P = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    err = L.vpcsum_last_error
    buf = (ctypes.c_uint8 * 256)()
    p = (ctypes.addressof(buf) + 15) & ~15

    def dev(dst=p, src=p, hdr=p, seg=p, flen=p, out=p, st=p, n=1, n_hdr=1, src_len=64):
        return L.vpcsum_tcp_build_async(P(dst), U64(64), P(src), U64(src_len), P(hdr), U32(n_hdr), P(seg), U32(n), P(flen),
                                        P(out), P(st), None)
    for kw, msg in ((dict(dst=None), b"NULL destination arena"), (dict(src=None), b"NULL source arena"),
                    (dict(hdr=None), b"NULL templates"), (dict(seg=None), b"NULL records"),
                    (dict(flen=None), b"NULL frame lengths"), (dict(seg=p + 4), b"records not 8-byte aligned"),
                    (dict(hdr=p + 2), b"templates not 4-byte aligned"), (dict(flen=p + 1), b"frame lengths not 4-byte aligned"),
                    (dict(out=p + 2), b"out words not 4-byte aligned"), (dict(n=(1 << 28) + 1), b"records > 2^28")):
        assert dev(**kw) != 0, kw
        assert b"vpcsum_tcp_build_async: " in err() and msg in err(), (kw, err())
    assert dev(dst=None, src=None, hdr=None, seg=None, flen=None, out=None, st=None, n=0) == 0   # nothing to do
    t = U64()

    def ctx(c=None, n=0):
        return L.vpcsum_ctx_build_tcp_frames(P(c), P(p), U64(64), P(p), U64(64), P(p), U32(1), P(p), U32(n), P(p), None, None,
                                             ctypes.byref(t))
    assert ctx() != 0 and b"vpcsum_ctx_build_tcp_frames: NULL context or ticket" in err()
    assert L.vpcsum_ctx_build_tcp_frames(P(p), P(p), U64(64), P(p), U64(64), P(p), U32(1), P(p), U32(1), P(p), None, None,
                                         None) != 0
    assert b"vpcsum_ctx_build_tcp_frames: NULL context or ticket" in err()

    def pni(ctx_h=0, dst_len=64, src_len=64, n_hdr=1, n=0):
        env = (ctypes.c_uint8 * 4128)()   # a PNIEnv_vpcsum_long
        rc = L.Java_io_vproxy_vpcsum_VPCsum_buildTcpFrames(ctypes.byref(env), ctypes.c_int64(ctx_h), P(p), ctypes.c_int64(dst_len),
                                                           P(p), ctypes.c_int64(src_len), P(p), ctypes.c_int32(n_hdr), P(p),
                                                           ctypes.c_int32(n), P(p), None, None)
        return rc, bytes(env[8:8 + 80]).split(b"\0")[0], ctypes.cast(ctypes.byref(env), ctypes.POINTER(ctypes.c_char_p))[0]
    for kw in (dict(n=-1), dict(n_hdr=-1), dict(dst_len=-1), dict(src_len=-1)):
        rc, msg, typ = pni(**kw)
        assert rc != 0 and msg == b"buildTcpFrames: negative size" and typ == b"java.lang.IllegalArgumentException", (kw, msg)
    rc, msg, typ = pni()
    assert rc != 0 and b"vpcsum_ctx_build_tcp_frames: NULL context or ticket" in msg and typ == b"java.io.IOException"
