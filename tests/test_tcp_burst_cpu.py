"""CPU-side checks of the TCP send bursts (vpcsum_tcp_build_bursts_async, vpcsum_ctx_build_tcp_bursts,
VPCsum.buildTcpBursts): vswitch.plan_tcp_fetch + the Python restatement of the cut (tests/tcpburstvec.py)
against a line-by-line transcription of SendingQueue.fetch() / fetch0() on an exhaustive grid, the
rules of tcp_burst.h in a stand-alone program under ASan / UBSan, the layout the binding, the header
and the kernel share, the kernel's budget read from the code object, and the argument refusals that
need no device."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import tcpbuildvec as B
import tcpburstvec as U

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    from vproxy_amd import build
    lib = ctypes.CDLL(build.build())
    lib.vpcsum_last_error.restype = ctypes.c_char_p
    return lib


# ------------------------------------------------------------------------------------------
# fetch(): the plan and the cut against the transcription
# ------------------------------------------------------------------------------------------
def pushes(total: int, mss: int, style: int):
    """Piece lengths of a queue of `total` bytes: as apiWrite pushes it (mss at a time), in pieces
    of 1, or in uneven pieces that do not line up with any cut."""
    if style == 0:
        step = [mss]
    elif style == 1:
        step = [1]
    else:
        step = [3, 1, 5, 2]
    out, i = [], 0
    while total > 0:
        d = min(step[i % len(step)], total)
        out.append(d)
        total -= d
        i += 1
    return out


@pytest.mark.parametrize("mss", [1, 2, 7])
def test_plan_and_expand_equal_fetch_on_the_grid(mss):
    """For every window 0..3 mss + 1, queue length 0..3 mss + 1, acknowledged prefix 0..queue length
    and three ways the queue was pushed: the segments fetch() returns (sequence number and bytes)
    equal the records expand() cuts from plan_tcp_fetch's burst, read out of the contiguous send
    buffer.  The queue keeps, as SendingQueue.ack does, every piece that ends at or after ackSeq."""
    from vproxy_amd import vswitch
    base = 0xfffffff0          # the stack's longs run past 2^32: the record takes the low 32 bits
    cases = cut = 0
    for queued in range(0, 3 * mss + 2):
        data = bytes((7 * i + 3) & 0xff for i in range(queued))
        for style in (0, 1, 2):
            pieces, o = [], 0
            for d in pushes(queued, mss, style):
                pieces.append(U.Segment(base + o, data[o:o + d]))
                o += d
            for acked in range(0, queued + 1):
                ack = base + acked
                q = [s for s in pieces if s.seqEndExclusive >= ack]
                for window in range(0, 3 * mss + 2):
                    want = U.SendingQueue(q, ack, window, mss).fetch()
                    splits = any(s.seqBeginInclusive < ack < s.seqEndExclusive for s in q)
                    plan = vswitch.plan_tcp_fetch(ack, window, mss, q[0].seqBeginInclusive if q else ack,
                                                  q[-1].seqEndExclusive if q else ack, ack_splits_piece=splits)
                    cases += 1
                    if plan is None:
                        assert want == [], (mss, queued, style, acked, window)
                        continue
                    seq, data_len, count = plan
                    assert data_len == min(window, queued - acked) and count == U.count_of(data_len, mss)
                    burst = U.mk_burst(seq - base, data_len, mss, 0, seq=seq & 0xffffffff, count=count)
                    segs, marked = U.expand([burst], np.arange(count) * 64, 64)
                    assert not marked.any() and len(want) == count, (mss, queued, style, acked, window, len(want))
                    for s, w in zip(segs, want):
                        assert int(s["seq"]) == w.seqBeginInclusive & 0xffffffff
                        o, d = int(s["data_off"]), int(s["data_len"])
                        assert data[o:o + d] == w.data and (int(s["flags"]), int(s["hdr"])) == (B.PSH | B.ACK, 0)
                    cut += count
    assert cases == 3 * sum(q + 1 for q in range(3 * mss + 2)) * (3 * mss + 2) and cut > cases // 2


def test_plan_tcp_fetch_quirks():
    """The cut starts at ackSeq whatever was fetched before; the first piece is min(mss, window); a
    window of 0 gives nothing, except the bare segment of an ackSeq inside a piece; a queue that
    begins past ackSeq or ends at it gives nothing."""
    from vproxy_amd.vswitch import plan_tcp_fetch
    assert plan_tcp_fetch(1000, 10000, 1460, 1000, 6000) == (1000, 5000, 4)
    assert plan_tcp_fetch(1000, 10000, 1460, 400, 6000) == (1000, 5000, 4)      # acknowledged pieces still queued
    assert plan_tcp_fetch(1000, 100, 1460, 1000, 6000) == (1000, 100, 1)        # min(mss, window)
    assert plan_tcp_fetch(1000, 2920, 1460, 1000, 6000) == (1000, 2920, 2)
    assert plan_tcp_fetch(1000, 2921, 1460, 1000, 6000) == (1000, 2921, 3)
    assert plan_tcp_fetch(1000, 0, 1460, 1000, 6000) is None
    assert plan_tcp_fetch(1000, 0, 1460, 900, 6000) is None
    assert plan_tcp_fetch(1000, 0, 1460, 900, 6000, ack_splits_piece=True) == (1000, 0, 1)
    assert plan_tcp_fetch(1000, 500, 1460, 1001, 6000) is None
    assert plan_tcp_fetch(6000, 500, 1460, 1000, 6000) is None and plan_tcp_fetch(1000, 500, 1460, 1000, 1000) is None


def test_expand_marks_what_the_rule_refuses():
    """expand(): frames before the first burst, past a burst's count and of a refused burst come out
    as records tcpbuildvec refuses; a gap in the table leaves its frames uncovered."""
    hdrs = np.array([B.mk_hdr(4, 14), B.mk_hdr(5, 14)], B.TCPHDR_DTYPE)
    bursts = [U.mk_burst(0, 10, 4, 1), U.mk_burst(20, 0, 0, 5, flags=B.ACK), U.mk_burst(30, 8, 4, 6, hdr=1),
              U.mk_burst(95, 6, 4, 8), U.mk_burst(40, 9, 4, 10, count=2)]
    segs, marked = U.expand(bursts, np.arange(13) * 100, 64, hdrs, 100)
    assert marked.tolist() == [True, False, False, False, True, False, True, True, True, True, True, True, True]
    assert [(int(s["data_off"]), int(s["data_len"])) for s in segs[1:4]] == [(0, 4), (4, 4), (8, 2)]
    assert (int(segs[5]["data_len"]), int(segs[5]["flags"])) == (0, B.ACK)
    for s, m in zip(segs, marked):
        assert B.refused(hdrs, s, 2000, 100) == bool(m)


# ------------------------------------------------------------------------------------------
# tcp_burst.h under sanitizers
# ------------------------------------------------------------------------------------------
def test_tcp_burst_rules_under_sanitizers(tmp_path):
    """tests/cpp/tcp_burst_test.cpp over tcp_burst.h alone, under ASan / UBSan: the cut at its edges
    with seq across 2^32, data_len up to 2^32 - 1 with mss 1 and 65535, every refusal accepted on one
    side and refused on the other (offsets next to 2^64 included), the search against a linear count
    on sorted tables of 0..4,096 bursts in heap blocks of their exact size, random sorted, gappy,
    overlapping and shuffled tables whose accepted frames must lie inside the destination and their
    own burst's source range, and the staged source's span and rebase."""
    exe = tmp_path / "tcp_burst_test"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(REPO, "include"), "-I", os.path.join(REPO, "vproxy_amd", "csrc"),
                           os.path.join(REPO, "tests", "cpp", "tcp_burst_test.cpp"), "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "tcp_burst ok" in r.stdout, (r.returncode, r.stdout, r.stderr)


# ------------------------------------------------------------------------------------------
# layouts, exports, budgets, refusals
# ------------------------------------------------------------------------------------------
CTYPE = {"uint8_t": "u1", "uint16_t": "<u2", "uint32_t": "<u4", "uint64_t": "<u8"}


def test_dtype_is_the_headers_layout():
    """TCPBURST_DTYPE (the binding's and the restatement's) equals vpcsum_tcpburst_t as the header
    declares it: names, types, the offsets its comments give, 32 bytes; the ABI version stays 4 and
    the "additive since" note names the new symbols."""
    from vproxy_amd import vpcsum as V
    src = open(os.path.join(REPO, "include", "vpcsum.h")).read()
    m = re.search(r"typedef struct vpcsum_tcpburst \{(.*?)\} vpcsum_tcpburst_t;", src, re.S)
    offs = [int(x) for x in re.findall(r"/\*\s+(\d+)\s", m.group(1))]
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = re.findall(r"(\w+)\s+(\w+)\s*;", body)
    assert len(fields) == 9 and offs == [0, 8, 12, 16, 20, 24, 26, 27, 28]
    want = np.dtype([(nm, CTYPE[ty]) for ty, nm in fields], align=True)
    assert want.itemsize == 32
    for dt in (V.TCPBURST_DTYPE, U.TCPBURST_DTYPE):
        assert dt.itemsize == 32 and dt.names == want.names
        assert [dt.fields[k][1] for k in dt.names] == [want.fields[k][1] for k in want.names] == offs
        assert [dt.fields[k][0] for k in dt.names] == [want.fields[k][0] for k in want.names]
    assert re.search(r"#define VPCSUM_ABI_VERSION\s+4\b", src)
    note = src[src.index("Additive since"):src.index("#define VPCSUM_ABI_VERSION")]
    for name in ("vpcsum_tcp_build_bursts_async", "vpcsum_ctx_build_tcp_bursts", "VPCsum.buildTcpBursts"):
        assert name in note, name


def test_exports_name_the_new_entry_points(L):
    from vproxy_amd import vpcsum as V
    from vproxy_amd import vswitch
    for name in ("vpcsum_tcp_build_bursts_async", "vpcsum_ctx_build_tcp_bursts", "Java_io_vproxy_vpcsum_VPCsum_buildTcpBursts"):
        assert name in V.EXPORTS and hasattr(L, name), name
    assert {"vpcsum_tcp_build_bursts_async", "vpcsum_ctx_build_tcp_bursts"} <= set(V._PROBED)   # an older library still loads
    assert callable(V.tcp_build_bursts) and callable(V.Context.build_tcp_bursts) and callable(vswitch.plan_tcp_fetch)
    java = os.path.join(REPO, "java", "io", "vproxy", "vpcsum")
    assert "Java_io_vproxy_vpcsum_VPCsum_buildTcpBursts" in open(os.path.join(java, "VPCsum.java")).read()
    assert "buildTcpBursts" in open(os.path.join(java, "GpuCsumBatch.java")).read()


def test_tcp_burst_kernel_budget():
    """k_tcp_build_bursts in tcp_burst.hip.o: one kernel, no scratch, no LDS, at most 72 VGPRs --
    k_tcp_build's budget, 7 waves per SIMD: the search's registers are dead before the mover starts."""
    from test_kernel_resources import kernels
    ks = kernels("tcp_burst.hip.o")
    assert len(ks) == 1 and "k_tcp_build_bursts" in next(iter(ks)), list(ks)
    v = next(iter(ks.values()))
    assert v["private_segment_fixed_size"] == 0 and v["group_segment_fixed_size"] == 0, v
    assert v["vgpr_count"] <= 72, v


def test_tcp_burst_entry_points_refuse_bad_arguments(L):
    """Each of the three new entry points answers a NULL / misaligned / oversize / negative argument
    with an error and a message naming it, before it touches a device; n_frames == 0 succeeds."""
    U32, U64, P = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_void_p
    err = L.vpcsum_last_error
    buf = (ctypes.c_uint8 * 256)()
    p = (ctypes.addressof(buf) + 15) & ~15

    def dev(dst=p, src=p, hdr=p, burst=p, foff=p, flen=p, out=p, st=p, n=1, n_bursts=1, n_hdr=1, src_len=64):
        return L.vpcsum_tcp_build_bursts_async(P(dst), U64(64), P(src), U64(src_len), P(hdr), U32(n_hdr), P(burst), U32(n_bursts),
                                               P(foff), U32(n), U32(2048), P(flen), P(out), P(st), None)
    for kw, msg in ((dict(dst=None), b"NULL destination arena"), (dict(src=None), b"NULL source arena"),
                    (dict(hdr=None), b"NULL templates"), (dict(burst=None), b"NULL bursts"),
                    (dict(foff=None), b"NULL frame offsets"), (dict(flen=None), b"NULL frame lengths"),
                    (dict(burst=p + 4), b"bursts not 8-byte aligned"), (dict(foff=p + 4), b"frame offsets not 8-byte aligned"),
                    (dict(hdr=p + 2), b"templates not 4-byte aligned"), (dict(flen=p + 1), b"frame lengths not 4-byte aligned"),
                    (dict(out=p + 2), b"out words not 4-byte aligned"), (dict(n=(1 << 28) + 1), b"frames > 2^28"),
                    (dict(n_bursts=(1 << 28) + 1), b"bursts > 2^28")):
        assert dev(**kw) != 0, kw
        assert b"vpcsum_tcp_build_bursts_async: " in err() and msg in err(), (kw, err())
    assert dev(dst=None, src=None, hdr=None, burst=None, foff=None, flen=None, out=None, st=None, n=0) == 0   # nothing to do
    t = U64()

    def ctx(c=None, ticket=ctypes.byref(t)):
        return L.vpcsum_ctx_build_tcp_bursts(P(c), P(p), U64(64), P(p), U64(64), P(p), U32(1), P(p), U32(1), P(p), U32(1), U32(2048),
                                             P(p), None, None, ticket)
    assert ctx() != 0 and b"vpcsum_ctx_build_tcp_bursts: NULL context or ticket" in err()
    assert ctx(c=p, ticket=None) != 0 and b"vpcsum_ctx_build_tcp_bursts: NULL context or ticket" in err()

    def pni(ctx_h=0, dst_len=64, src_len=64, n_hdr=1, n_bursts=0, n=0, cap=2048):
        env = (ctypes.c_uint8 * 4128)()   # a PNIEnv_vpcsum_long
        rc = L.Java_io_vproxy_vpcsum_VPCsum_buildTcpBursts(ctypes.byref(env), ctypes.c_int64(ctx_h), P(p), ctypes.c_int64(dst_len),
                                                           P(p), ctypes.c_int64(src_len), P(p), ctypes.c_int32(n_hdr), P(p),
                                                           ctypes.c_int32(n_bursts), P(p), ctypes.c_int32(n), ctypes.c_int32(cap),
                                                           P(p), None, None)
        return rc, bytes(env[8:8 + 80]).split(b"\0")[0], ctypes.cast(ctypes.byref(env), ctypes.POINTER(ctypes.c_char_p))[0]
    for kw in (dict(n=-1), dict(n_bursts=-1), dict(n_hdr=-1), dict(cap=-1), dict(dst_len=-1), dict(src_len=-1)):
        rc, msg, typ = pni(**kw)
        assert rc != 0 and msg == b"buildTcpBursts: negative size" and typ == b"java.lang.IllegalArgumentException", (kw, msg)
    rc, msg, typ = pni()
    assert rc != 0 and b"vpcsum_ctx_build_tcp_bursts: NULL context or ticket" in msg and typ == b"java.io.IOException"
