"""CPU-side checks of the flow table's Fastpath: the host logic (flow_table.h set_fastpath and what
insert / erase do to the record) against a model in a stand-alone program under ASan / UBSan, the
layouts the binding, the header and the kernels share, the budgets of the two new kernels read from
the code object, the argument refusals that need no device, and the Python restatement of the L2
rule (tests/fastpathvec.py) on hand-written frames."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fastpathvec as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from vproxy_amd import build
    lib = ctypes.CDLL(build.build())
    lib.vpcsum_last_error.restype = ctypes.c_char_p
    return lib


def test_fastpath_table_under_sanitizers(tmp_path):
    """flow_table.h alone against a std::map model over random insert / replace / erase /
    set_fastpath steps on an 8-slot and a 1,024-slot table: after every step each live key's
    Fastpath is the model's -- kept by replace, moved by backward shift, gone after erase and
    re-insert, cleared by port 0 --, a missing key is counted, a malformed key refused with nothing
    changed (tests/cpp/flow_fastpath_test.cpp); the record sits at offset 112 of the slot."""
    exe = tmp_path / "flow_fastpath_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "vproxy_amd", "csrc"),
                           os.path.join(REPO, "tests", "cpp", "flow_fastpath_test.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "flow_fastpath ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
    assert "offsetof(FlowSlot, fp) = 112\n" in r.stdout


def test_fastpath_dtype_is_the_headers_layout():
    """FASTPATH_DTYPE (and the restatement's FP_DTYPE) equals vpcsum_fastpath_t as the header
    declares it: dst[6], src[6], port (uint32), 16 bytes; flow_table.h asserts the slot offset."""
    from vproxy_amd import vpcsum as V
    src = open(os.path.join(REPO, "include", "vpcsum.h")).read()
    m = re.search(r"typedef struct vpcsum_fastpath \{(.*?)\} vpcsum_fastpath_t;", src, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"(\w+)\s+(\w+)\s*(?:\[(\d+)\])?\s*;", body)
    assert fields == [("uint8_t", "dst", "6"), ("uint8_t", "src", "6"), ("uint32_t", "port", "")]
    for dt in (V.FASTPATH_DTYPE, F.FP_DTYPE):
        assert dt.names == ("dst", "src", "port") and dt.itemsize == 16
        assert [dt.fields[k][1] for k in dt.names] == [0, 6, 12]
        assert dt.fields["dst"][0] == np.dtype(("u1", 6)) and dt.fields["port"][0] == np.dtype("<u4")
    assert re.search(r"#define VPCSUM_ABI_VERSION\s+4\b", src)   # additive: the version stays
    tab = open(os.path.join(REPO, "vproxy_amd", "csrc", "flow_table.h")).read()
    assert re.search(r"static_assert\(offsetof\(FlowSlot, fp\) == 112", tab)
    assert (F.HIT, F.S_DONE, F.S_BAD_DESC) == (V.FLOW_HIT, V.S_DONE, V.S_BAD_DESC)


def test_fastpath_kernel_budgets(L):
    """The Fastpath lookup has the plain lookup's budget (no scratch, no LDS, at most 32 VGPRs) and
    a name the plain lookup's budget test does not match; the L2 kernel uses no scratch and no LDS."""
    from test_kernel_resources import kernels
    ks = kernels("flow.hip.o")
    fp = [v for name, v in ks.items() if "k_flowfp" in name]
    l2 = [v for name, v in ks.items() if "k_l2_forward" in name]
    assert len(fp) == 1 and len(l2) == 1
    assert not any("k_flow_lookup" in name for name in ks if "k_flowfp" in name or "k_l2_forward" in name)
    assert len([name for name in ks if "k_flow_lookup" in name]) == 1
    assert fp[0]["private_segment_fixed_size"] == 0 and fp[0]["group_segment_fixed_size"] == 0
    assert fp[0]["vgpr_count"] <= 32, fp[0]
    assert l2[0]["private_segment_fixed_size"] == 0 and l2[0]["group_segment_fixed_size"] == 0, l2[0]


def test_fastpath_entry_points_refuse_bad_arguments(L):
    """Each of the five new entry points (and the two PNI calls) answers a NULL handle or a NULL /
    misaligned array with an error and a message naming it, before it touches a device."""
    U32, U64 = ctypes.c_uint32, ctypes.c_uint64
    t = U64()
    err = L.vpcsum_last_error
    assert L.vpcsum_flowtab_set_fastpath(None, None, None, U32(0), None, None) != 0
    assert b"vpcsum_flowtab_set_fastpath: NULL table" in err()
    assert L.vpcsum_flow_lookup_fp_async(None, None, U32(1), None, None, None, None) != 0
    assert b"vpcsum_flow_lookup_fp_async: NULL table" in err()
    buf = (ctypes.c_uint8 * 64)()
    p = ctypes.addressof(buf)
    P = ctypes.c_void_p
    assert L.vpcsum_l2_forward_async(None, U64(64), P(p), P(p), P(p), P(p), P(p), U32(1), P(p), None) != 0
    assert b"vpcsum_l2_forward_async: NULL argument" in err()
    assert L.vpcsum_l2_forward_async(P(p), U64(64), P(p), P(p), P(p), P(p), P(p), U32(1), None, None) != 0
    assert b"vpcsum_l2_forward_async: NULL argument" in err()
    assert L.vpcsum_l2_forward_async(P(p), U64(64), P(p), P(p), P(p), P(p), P(p + 2), U32(1), P(p), None) != 0
    assert b"vpcsum_l2_forward_async" in err() and b"not 4-byte aligned" in err()
    assert L.vpcsum_l2_forward_async(P(p), U64(64), P(p + 4), P(p), P(p), P(p), P(p), U32(1), P(p), None) != 0
    assert b"not 8-byte aligned" in err()
    assert L.vpcsum_l2_forward_async(None, U64(0), None, None, None, None, None, U32(0), None, None) == 0   # nothing to do
    assert L.vpcsum_ctx_nat_flow_forward_frames(None, None, None, U64(0), None, None, U32(0), None, None, None, U32(0),
                                                ctypes.byref(t)) != 0
    assert b"vpcsum_ctx_nat_flow_forward_frames: NULL flow table" in err()

    def EnvInt():   # room for a PNIEnv_vpcsum_int / _long (4,128 bytes: the exception, then the value)
        return (ctypes.c_uint8 * 4128)()
    env = EnvInt()
    assert L.Java_io_vproxy_vpcsum_VPCsum_flowtabSetFastpath(ctypes.byref(env), ctypes.c_int64(0), None, None,
                                                             ctypes.c_int32(-1)) != 0
    assert b"flowtabSetFastpath: negative count" in err()
    env = EnvInt()
    assert L.Java_io_vproxy_vpcsum_VPCsum_flowtabSetFastpath(ctypes.byref(env), ctypes.c_int64(0), None, None,
                                                             ctypes.c_int32(0)) != 0
    assert b"vpcsum_flowtab_set_fastpath: NULL table" in err()
    env = EnvInt()
    assert L.Java_io_vproxy_vpcsum_VPCsum_natFlowForwardFrames(ctypes.byref(env), ctypes.c_int64(0), ctypes.c_int64(0), None,
                                                               ctypes.c_int64(0), None, None, ctypes.c_int32(-1), None, None,
                                                               None, ctypes.c_int32(0)) != 0
    assert b"natFlowForwardFrames: negative size" in err()


def test_exports_name_the_new_entry_points(L):
    from vproxy_amd import vpcsum as V
    for name in ("vpcsum_flowtab_set_fastpath", "vpcsum_flow_lookup_fp_async", "vpcsum_l2_forward_async",
                 "vpcsum_ctx_nat_flow_forward_frames", "Java_io_vproxy_vpcsum_VPCsum_flowtabSetFastpath",
                 "Java_io_vproxy_vpcsum_VPCsum_natFlowForwardFrames"):
        assert name in V.EXPORTS and hasattr(L, name), name


# ------------------------------------------------------------------------------------------
# the restatement of the L2 rule, on frames written by hand
# ------------------------------------------------------------------------------------------
MAC_A, MAC_B = bytes.fromhex("020000000a01"), bytes.fromhex("020000000b02")
NEW_DST, NEW_SRC = bytes.fromhex("0a1b2c3d4e5f"), bytes.fromhex("f0e1d2c3b4a5")
PLAIN = MAC_A + MAC_B + bytes.fromhex("0800") + bytes(range(0x45, 0x45 + 28))
TAGGED = MAC_A + MAC_B + bytes.fromhex("8100" "0007" "86dd") + bytes(range(0x60, 0x60 + 44))


def _arena(frames, gap=3):
    offs, buf = [], bytearray()
    for f in frames:
        offs.append(len(buf))
        buf += f + b"\xee" * gap
    return np.frombuffer(bytes(buf), np.uint8), np.array(offs, np.uint64), np.array([len(f) for f in frames], np.uint32)


def test_restatement_on_hand_written_frames():
    """A plain IPv4 frame and an 802.1Q IPv6 one: only bytes [0,12) become dst | src -- the tag, the
    EtherType, the payload and the bytes between frames are as they were -- and the port is the
    record's.  Each reason not to forward, one frame each, leaves the frame alone with port 0."""
    fp = F.mk_fp(NEW_DST, NEW_SRC, 7)
    arena, offs, lens = _arena([PLAIN, TAGGED])
    out, ports = F.l2_forward(arena, offs, lens, [F.HIT, F.HIT], [F.S_DONE, F.S_DONE | 0x08], [fp, fp])
    assert list(ports) == [7, 7]
    for o, f in zip(offs, (PLAIN, TAGGED)):
        o = int(o)
        assert out[o:o + len(f)].tobytes() == NEW_DST + NEW_SRC + f[12:]
        assert out[o + len(f):o + len(f) + 3].tobytes() == b"\xee" * 3
    o = int(offs[1])
    assert out[o + 12:o + 18].tobytes() == bytes.fromhex("8100" "0007" "86dd")   # tag and EtherType
    assert (arena[:12].tobytes(), arena[o:o + 12].tobytes()) == (MAC_A + MAC_B,) * 2   # the input is not written
    none = F.mk_fp(NEW_DST, NEW_SRC, 0)
    cases = [(2, F.S_DONE, fp), (0, F.S_DONE, fp), (F.HIT, F.S_BAD_DESC, fp), (F.HIT, F.S_BAD_DESC | 0x20, fp),
             (F.HIT, F.S_DONE | F.S_BAD_DESC, fp), (F.HIT, 0, fp), (F.HIT, F.S_DONE, none)]
    arena, offs, lens = _arena([PLAIN] * len(cases))
    out, ports = F.l2_forward(arena, offs, lens, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    assert not ports.any() and np.array_equal(out, arena)


def test_restatement_refuses_frames_outside_the_arena():
    """13 bytes hold no Ethernet header; a frame ending past the arena is not the arena's: port 0,
    nothing written.  A 14-byte frame ending exactly at the arena's end is forwarded."""
    fp = F.mk_fp(NEW_DST, NEW_SRC, 9)
    arena, offs, lens = _arena([PLAIN[:13], PLAIN[:14]], gap=0)
    assert int(offs[1]) + 14 == len(arena)
    offs = np.append(offs, np.uint64(len(arena) - 20))
    lens = np.append(lens, np.uint32(21))
    out, ports = F.l2_forward(arena, offs, lens, [F.HIT] * 3, [F.S_DONE] * 3, [fp] * 3)
    assert list(ports) == [0, 9, 0]
    assert out[:13].tobytes() == PLAIN[:13] and out[13:].tobytes() == NEW_DST + NEW_SRC + PLAIN[12:14]
