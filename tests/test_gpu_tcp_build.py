"""The TCP segment build on the GPU (vpcsum_tcp_build_async, vpcsum_ctx_build_tcp_frames,
VPCsum.buildTcpFrames) against the Python restatement of the frame rule (tests/tcpbuildvec.py, sums
through the oracle).  In every case the WHOLE destination arena is compared with the
restatement's: it is prefilled with 0xEE, so a byte written outside a frame fails the case; frame
lengths, out words and status bytes are compared too, and the source arena with itself before."""
import ctypes
import json
import os

import numpy as np
import pytest

import tcpbuildvec as B
from oracle import oracle as O

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xEE


@pytest.fixture(scope="module")
def V():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vproxy_amd import vpcsum
    vpcsum.lib()
    assert vpcsum.TCPHDR_DTYPE == B.TCPHDR_DTYPE and vpcsum.TCPSEG_DTYPE == B.TCPSEG_DTYPE
    return vpcsum


def dev(a):
    """Host to device through pinned memory, as the other GPU tests copy."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).pin_memory().cuda()


def host(t):
    """Device to host through pinned memory."""
    import torch
    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    h.copy_(t)
    torch.cuda.synchronize()
    return h.numpy().copy()


def gpu_build(V, dst, src, hdrs, segs, n=None, want_out=True, want_status=True):
    """(arena_after, frame_len, out, status) of vpcsum_tcp_build_async on device copies of the arenas;
    the result arrays start as 0xAB and carry two guard rows, which must stay; the source arena
    must come back as it went."""
    import torch
    n = len(segs) if n is None else n
    d_dst, d_src = dev(dst), dev(src if len(src) else np.zeros(16, np.uint8))[:len(src)]
    assert d_dst.data_ptr() % 16 == 0 and d_src.data_ptr() % 16 == 0
    d_h = dev(hdrs) if len(hdrs) else torch.zeros(64, dtype=torch.uint8, device="cuda")
    d_s = dev(segs) if len(segs) else torch.zeros(32, dtype=torch.uint8, device="cuda")
    flen = torch.full(((n + 2) * 4,), 0xAB, dtype=torch.uint8, device="cuda")
    out = torch.full(((n + 2) * 4,), 0xAB, dtype=torch.uint8, device="cuda")
    st = torch.full((n + 2,), 0xAB, dtype=torch.uint8, device="cuda")
    V.tcp_build(d_dst, d_src, d_h, len(hdrs), d_s, n, flen, out if want_out else None, st if want_status else None)
    torch.cuda.synchronize()
    flen, out, st = host(flen).view(np.uint32), host(out).view(np.uint32), host(st)
    assert (flen[n:] == 0xABABABAB).all() and (out[n:] == 0xABABABAB).all() and (st[n:] == 0xAB).all()
    if not want_out:
        assert (out == 0xABABABAB).all()
    if not want_status:
        assert (st == 0xAB).all()
    assert np.array_equal(host(d_src), src)
    return host(d_dst), flen[:n], out[:n], st[:n]


def first_diff(got, want, segs):
    k = int(np.flatnonzero(got != want)[0])
    near = [(i, k - int(s["frame_off"])) for i, s in enumerate(segs) if int(s["frame_off"]) - 4 <= k]
    i, rel = near[-1] if near else (-1, k)
    return f"byte {k} (record {i} +{rel}): {got[k]:#x} != {want[k]:#x}"


def check(V, dst, src, hdrs, segs, n=None, want_out=True, want_status=True):
    n = len(segs) if n is None else n
    want, w_len, w_out, w_st = B.build(dst, src, hdrs, segs[:n])
    got, flen, out, st = gpu_build(V, dst, src, hdrs, segs, n, want_out, want_status)
    assert np.array_equal(flen, w_len), [(i, int(flen[i]), int(w_len[i])) for i in np.flatnonzero(flen != w_len)[:8]]
    if want_status:
        assert np.array_equal(st, w_st), [(i, hex(st[i]), hex(w_st[i])) for i in np.flatnonzero(st != w_st)[:8]]
    if want_out:
        assert np.array_equal(out, w_out), [(i, hex(out[i]), hex(w_out[i])) for i in np.flatnonzero(out != w_out)[:8]]
    assert np.array_equal(got, want), first_diff(got, want, segs[:n])
    return want, w_len, w_out, w_st


class Layout:
    """Frames and payloads laid out one after another, each at a wanted address residue mod 16
    with 3 guard bytes before and after."""

    def __init__(self, rng):
        self.rng, self.dcur, self.scur, self.segs, self.chunks = rng, 0, 0, [], []

    def add(self, h, hidx, data, dres=0, sres=0, seq=None, flags=B.PSH | B.ACK, cap=None, **kw):
        d = len(data)
        L = B.header_len(h) + d
        self.dcur += 3
        self.dcur += (dres - self.dcur) % 16
        self.scur += 3
        self.scur += (sres - self.scur) % 16
        seq = int(self.rng.integers(0, 1 << 32)) if seq is None else seq
        self.segs.append(B.mk_seg(self.dcur, self.scur, d, seq=seq, hdr=hidx, frame_cap=L if cap is None else cap, flags=flags, **kw))
        self.chunks.append((self.scur, data))
        self.dcur += L + 3
        self.scur += d + 3
        return len(self.segs) - 1

    def arenas(self):
        dst = np.full(self.dcur, FILL, np.uint8)
        src = self.rng.integers(0, 256, self.scur, dtype=np.uint8)
        for o, data in self.chunks:
            src[o:o + len(data)] = np.frombuffer(bytes(data), np.uint8)
        return dst, src, np.array(self.segs, B.TCPSEG_DTYPE)


def mk_v4(**kw):
    return B.mk_hdr(4, 14, bytes([10, 1, 2, 3]), bytes([192, 168, 7, 9]), 43210, 443, 0x89abcdef, 0x1234, **kw)


def mk_v6(l2=0, **kw):
    return B.mk_hdr(6, l2, bytes(range(0x20, 0x30)), bytes(range(0xe0, 0xf0)), 8080, 51000, 0x01020304, 0xfff0, **kw)


# ------------------------------------------------------------------------------------------
# 1. alignment x length
# ------------------------------------------------------------------------------------------
LENS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 127, 128, 129, 1360, 1460)


@pytest.mark.parametrize("ver,l2", [(4, 14), (6, 0)], ids=["ipv4_eth", "ipv6_ip"])
def test_alignment_by_length_grid(V, ver, l2):
    """data_len in LENS x destination frame_off residue 0..15 x source data_off residue 0..15 with
    random payloads: 4,352 records, each frame with 3 guard bytes before and after and frame_cap = L."""
    rng = np.random.default_rng(41 + ver)
    h = mk_v4(tos=0x10, ident=0x1c46, frag=0x4000) if ver == 4 else mk_v6(l2, tos=0xb8, ttl=255)
    lay = Layout(rng)
    for d in LENS:
        for dres in range(16):
            for sres in range(16):
                lay.add(h, 0, rng.integers(0, 256, d, dtype=np.uint8).tobytes(), dres, sres)
    dst, src, segs = lay.arenas()
    assert len(segs) == 4352
    assert {(int(s["frame_off"]) % 16, int(s["data_off"]) % 16) for s in segs} == {(a, b) for a in range(16) for b in range(16)}
    _, w_len, _, w_st = check(V, dst, src, np.array([h], B.TCPHDR_DTYPE), segs)
    assert (w_st == B.S_DONE).all() and sorted(set(w_len.tolist())) == [B.header_len(h) + d for d in LENS]


# ------------------------------------------------------------------------------------------
# 2. sums at their edges
# ------------------------------------------------------------------------------------------
def last_two_for(h, seq, flags, body: bytes):
    """{TCP sum: last two payload bytes} over all 65,536 values of the two bytes after `body`,
    through the oracle's calculateChecksumIntermediate / DoFinal on the pseudo-header and segment."""
    d = len(body) + 2
    s = B.mk_seg(0, 0, d, seq=seq, flags=flags, hlen=B.header_len(h))
    f, _, _ = B.frame(h, s, body + b"\x00\x00")
    l3 = bytearray(f[int(h["l2_len"]):])
    l4o = 20 if int(h["l3_ver"]) == 4 else 40
    l3[l4o + 16:l4o + 18] = b"\x00\x00"
    ph = O.pseudo_ipv4(l3, 6, 20 + d) if int(h["l3_ver"]) == 4 else O.pseudo_ipv6(l3, 6, 20 + d)
    pre = bytes(ph) + bytes(l3[l4o:-2])
    assert len(pre) % 2 == 0
    part = O.csum_intermediate(0, pre, len(pre))
    return {O.csum_final(O.csum_intermediate(part, x.to_bytes(2, "big"), 2)): x.to_bytes(2, "big") for x in range(65536)}


def test_sums_at_their_edges(V):
    """Each at an even and at an odd source address (and, by the layout, at varying frame addresses):
    payloads of all 0x00 and all 0xff; 0xff x 65,495 on IPv4 (its largest) and 0xff x 65,515 on IPv6;
    payloads whose last two bytes make the TCP sum 0x0000, 0x0001 and 0xfffe (stored as they are);
    a template whose IPv4 header sum is 0x0000; seq 0xffffffff.
    A TCP sum of 0xffff cannot be built: Java's end-around fold of a sum that includes the non-zero
    pseudo-header word 0x0006 is never 0, so calculateChecksumDoFinal (0xffff - s) never returns
    0xffff -- the oracle confirms it over all 65,536 values of the last two bytes, and the case is
    replaced by its neighbour 0xfffe."""
    rng = np.random.default_rng(43)
    v4, v6 = mk_v4(), mk_v6(14)
    # the IPv4 identification that makes the header sum of a 1,000-byte payload's frame 0x0000
    probe = B.frame(v4, B.mk_seg(0, 0, 1000), bytes(1000))[1]
    v4z = mk_v4(ident=probe if probe else 0xffff)
    assert B.frame(v4z, B.mk_seg(0, 0, 1000), bytes(1000))[1] == 0x0000
    hdrs = np.array([v4, v6, v4z], B.TCPHDR_DTYPE)
    body = rng.integers(0, 256, 298, dtype=np.uint8).tobytes()
    sums = {ver: last_two_for(h, 77, B.PSH | B.ACK, body) for ver, h in ((4, v4), (6, v6))}
    for m in sums.values():
        assert 0xffff not in m and len(m) == 65535 and {0x0000, 0x0001, 0xfffe} <= set(m)
    lay = Layout(rng)
    names = []
    for sres in (0, 1):
        for hi, ver in ((0, 4), (1, 6)):
            h = hdrs[hi]
            for nm, data in (("zeros", bytes(1460)), ("ones", b"\xff" * 1460), ("ones_odd", b"\xff" * 1359),
                             ("largest", b"\xff" * (65495 if ver == 4 else 65515))):
                lay.add(h, hi, data, dres=int(rng.integers(0, 16)), sres=sres)
                names.append(f"{nm}/v{ver}/s{sres}")
            for want in (0x0000, 0x0001, 0xfffe):
                lay.add(h, hi, body + sums[ver][want], dres=int(rng.integers(0, 16)), sres=sres, seq=77)
                names.append(f"sum{want:04x}/v{ver}/s{sres}")
            lay.add(h, hi, rng.integers(0, 256, 700, dtype=np.uint8).tobytes(), dres=5, sres=sres, seq=0xffffffff)
            names.append(f"seqmax/v{ver}/s{sres}")
        lay.add(v4z, 2, bytes(1000), dres=9, sres=sres)
        names.append(f"ipsum0/s{sres}")
    dst, src, segs = lay.arenas()
    _, w_len, w_out, w_st = check(V, dst, src, hdrs, segs)
    assert (w_st == B.S_DONE).all()
    by = dict(zip(names, w_out.tolist()))
    for sres in (0, 1):
        for ver in (4, 6):
            for want in (0x0000, 0x0001, 0xfffe):
                assert by[f"sum{want:04x}/v{ver}/s{sres}"] >> 16 == want
        assert by[f"ipsum0/s{sres}"] & 0xffff == 0 and by[f"ipsum0/s{sres}"] >> 16 != 0
    assert max(w_len) == 14 + 40 + 20 + 65515


# ------------------------------------------------------------------------------------------
# 3. the reference's frame
# ------------------------------------------------------------------------------------------
def test_reference_frame_is_rebuilt_on_the_gpu(V):
    """tcpIpv4PshExample's template and record, built on the GPU at each destination residue mod 4
    from an odd source address: byte-equal to the 571-byte fixture, sums 0x85f7 / 0x0aa9."""
    ks = json.load(open(os.path.join(REPO, "tests", "golden", "kat.json")))["kats"]
    raw = bytes.fromhex(next(k for k in ks if k["name"] == "tcpIpv4PshExample")["hex"])
    h, rec, payload = B.from_frame(raw)
    lay = Layout(np.random.default_rng(44))
    for dres in (0, 1, 2, 3, 6):
        lay.add(h, 0, payload, dres, 7, seq=rec["seq"], flags=rec["flags"])
    dst, src, segs = lay.arenas()
    want, w_len, w_out, _ = check(V, dst, src, np.array([h], B.TCPHDR_DTYPE), segs)
    got, _, _, _ = gpu_build(V, dst, src, np.array([h], B.TCPHDR_DTYPE), segs)
    for s in segs:
        o = int(s["frame_off"])
        assert got[o:o + 571].tobytes() == raw
    assert set(w_out.tolist()) == {0x85f7 | (0x0aa9 << 16)} and set(w_len.tolist()) == {571}


# ------------------------------------------------------------------------------------------
# 4. refusals among good records
# ------------------------------------------------------------------------------------------
def test_refusals_among_good_records(V):
    """Each reason of the header's list once, at the boundary that is accepted and one past it, good
    records between them: a refused record reports frame_len 0, S_BAD_DESC, out 0 and leaves the arena
    untouched where its frame would lie; its neighbours are complete.  The last frame ends exactly at
    dst_len and the last payload exactly at src_len."""
    rng = np.random.default_rng(45)
    hdrs = np.array([mk_v4(), mk_v6(), B.mk_hdr(5, 14), B.mk_hdr(4, 18), B.mk_hdr(6, 0, rsv=0x0100), B.mk_hdr(4, 14, rsv=1),
                     mk_v6(14)], B.TCPHDR_DTYPE)
    n_hdr = len(hdrs)
    lay = Layout(rng)
    pay = lambda d: rng.integers(0, 256, d, dtype=np.uint8).tobytes()   # noqa: E731
    expect = []

    def add(ok, hi, d, **kw):
        h = hdrs[hi] if hi < n_hdr else hdrs[0]
        lay.add(h, hi, pay(d), int(rng.integers(0, 16)), int(rng.integers(0, 16)), **kw)
        expect.append(ok)

    add(True, 0, 100)
    add(True, n_hdr - 1, 100)                        # hdr = n_hdr - 1
    add(False, n_hdr, 100)                           # hdr = n_hdr
    add(False, 0xffffffff, 100)
    add(True, 1, 33)
    add(False, 2, 33); add(False, 3, 33); add(False, 4, 33); add(False, 5, 33)   # version, l2_len, template rsv
    add(True, 0, 0, flags=0x3f)
    add(False, 0, 0, flags=0x40); add(False, 0, 0, flags=0x80); add(False, 0, 7, rsv=1)
    add(True, 0, 200, cap=54 + 200)                  # L == frame_cap
    add(False, 0, 200, cap=54 + 199)                 # L == frame_cap + 1
    add(True, 1, 1, cap=61); add(False, 1, 1, cap=60)
    add(True, 0, 65495); add(False, 0, 65496, cap=1 << 17)
    add(True, 1, 65515); add(False, 1, 65516, cap=1 << 17)
    add(True, 0, 17)
    dst, src, segs = lay.arenas()
    # the bounds: the last frame ends exactly at dst_len, its payload exactly at src_len
    dst, src = dst[:-3].copy(), src[:-3].copy()
    assert int(segs[-1]["frame_off"]) + 54 + 17 == len(dst) and int(segs[-1]["data_off"]) + 17 == len(src)
    extra = [B.mk_seg(len(dst) - 70, 0, 17), B.mk_seg(0, len(src) - 16, 17, frame_cap=71),      # one past either end
             B.mk_seg(len(dst) + 1, 0, 0), B.mk_seg(0, len(src) + 1, 0, frame_cap=54),
             B.mk_seg((1 << 64) - 20, 0, 17), B.mk_seg(0, (1 << 64) - 8, 17, frame_cap=71),      # would wrap
             B.mk_seg(int(segs[0]["frame_off"]), len(src), 0, frame_cap=54)]                       # an empty payload at src_len: rebuilt below
    extra[-1]["flags"] = B.ACK
    expect += [False] * 6 + [True]
    # the accepted extra record rebuilds record 0's place with a bare ACK; record 0 itself is dropped
    segs = np.concatenate([segs[1:], np.array(extra, B.TCPSEG_DTYPE)])
    expect = expect[1:]
    want, w_len, w_out, w_st = check(V, dst, src, hdrs, segs)
    assert [bool(x) for x in w_len] == expect, [(i, bool(x), e) for i, (x, e) in enumerate(zip(w_len, expect)) if bool(x) != e]
    assert [s == B.S_DONE for s in w_st] == expect and all(s == B.S_BAD_DESC for s, e in zip(w_st, expect) if not e)
    assert all(o == 0 for o, e in zip(w_out, expect) if not e)
    for s, e in zip(segs[:len(lay.segs) - 1], expect):
        if not e:   # the place its frame would take is as it was
            o = int(s["frame_off"])
            assert (want[o:o + 40] == FILL).all()


# ------------------------------------------------------------------------------------------
# 5. batch sizes, shared templates, optional outputs
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 9, 33, 257])
def test_batch_sizes_and_optional_outputs(V, n):
    """n records over 3 templates shared unevenly (IPv4 + Ethernet, IPv6, IPv6 + Ethernet), lengths
    0..300, with d_out / d_status each NULL and non-NULL; a longer record array than n is not read
    past n (its later records name frames that must stay untouched)."""
    rng = np.random.default_rng(46 + n)
    hdrs = np.array([mk_v4(ttl=1), mk_v6(), mk_v6(14, tos=0xff)], B.TCPHDR_DTYPE)
    lay = Layout(rng)
    for i in range(n + 3):
        hi = 0 if i % 7 < 4 else 1 if i % 7 < 6 else 2
        d = int(rng.integers(0, 301))
        lay.add(hdrs[hi], hi, rng.integers(0, 256, d, dtype=np.uint8).tobytes(), int(rng.integers(0, 16)), int(rng.integers(0, 16)),
                flags=int(rng.choice([B.ACK, B.PSH | B.ACK, B.FIN | B.ACK, B.RST])))
    dst, src, segs = lay.arenas()
    for want_out, want_status in ((True, True), (False, True), (True, False), (False, False)):
        want, _, _, _ = check(V, dst, src, hdrs, segs, n, want_out, want_status)
    assert (want[int(segs[n]["frame_off"]):] == FILL).all()
    if n == 1:
        check(V, dst, src, hdrs, segs, 0)   # n == 0 launches nothing


# ------------------------------------------------------------------------------------------
# 6. agreement with the shipped kernels
# ------------------------------------------------------------------------------------------
def test_built_frames_verify_with_the_shipped_kernels(V):
    """The l2_len 14 frames, IPv4 and IPv6, built on the GPU and handed to vpcsum_parse_ether_async +
    vpcsum_compute_async in MODE_VERIFY: every frame S_IP_OK (IPv4) and S_L4_OK, and d_out of the
    build equals the verify's recomputed words."""
    import torch
    rng = np.random.default_rng(47)
    hdrs = np.array([mk_v4(), mk_v6(14)], B.TCPHDR_DTYPE)
    lay = Layout(rng)
    for i in range(96):
        d = int(rng.choice([0, 1, 2, 63, 64, 65, 517, 1360, 1460]))
        lay.add(hdrs[i & 1], i & 1, rng.integers(0, 256, d, dtype=np.uint8).tobytes(), int(rng.integers(0, 16)), int(rng.integers(0, 16)))
    dst, src, segs = lay.arenas()
    n = len(segs)
    d_dst, d_src = dev(dst), dev(src)
    flen = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    V.tcp_build(d_dst, d_src, dev(hdrs), 2, dev(segs), n, flen, out, None)
    desc = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    vout = torch.zeros(n, dtype=torch.int32, device="cuda")
    vst = torch.zeros(n, dtype=torch.uint8, device="cuda")
    V.parse_ether(d_dst, dev(segs["frame_off"].copy()), flen, n, desc)
    V.compute(d_dst, desc, n, vout, vst, V.MODE_VERIFY)
    torch.cuda.synchronize()
    vst, vout, out = host(vst), host(vout).view(np.uint32), host(out).view(np.uint32)
    for i in range(n):
        want = V.S_DONE | V.S_L4_OK | (V.S_IP_OK if i & 1 == 0 else 0)
        assert vst[i] & want == want and not vst[i] & V.S_BAD_DESC, (i, hex(vst[i]))
    assert np.array_equal(out, vout), [(i, hex(out[i]), hex(vout[i])) for i in np.flatnonzero(out != vout)[:8]]
    want, _, w_out, _ = B.build(dst, src, hdrs, segs)
    assert np.array_equal(out, w_out) and np.array_equal(host(d_dst), want)


# ------------------------------------------------------------------------------------------
# 7. the host form, 8. PNI
# ------------------------------------------------------------------------------------------
STRIDE, HEADROOM = 2048, 384
_KEEP = []


def page_aligned(nbytes):
    raw = np.zeros(nbytes + 8192, np.uint8)
    _KEEP.append(raw)   # page-locked and released by the tests: kept for the life of the process
    skip = (-raw.ctypes.data) % 4096
    return raw[skip:skip + nbytes]


@pytest.fixture(scope="module")
def txbatch():
    """64 records at umem geometry (2,048-byte chunks, frame at +384): three templates, payloads of
    0..1,460 bytes scattered over a 256-KiB send buffer, two refused records among them."""
    rng = np.random.default_rng(48)
    hdrs = np.array([mk_v4(), mk_v6(14), mk_v6()], B.TCPHDR_DTYPE)
    n = 64
    src = rng.integers(0, 256, 256 << 10, dtype=np.uint8)
    segs = np.zeros(n, B.TCPSEG_DTYPE)
    for i in range(n):
        hi = i % 3
        d = int(rng.choice([0, 1, 100, 517, 1360, 1460]))
        segs[i] = B.mk_seg(i * STRIDE + HEADROOM, 4096 + int(rng.integers(0, 64 << 10)), d, seq=int(rng.integers(0, 1 << 32)), hdr=hi,
                           frame_cap=STRIDE - HEADROOM, flags=B.PSH | B.ACK if d else B.ACK)
    segs[10]["hdr"] = 3                      # no such template
    segs[20]["data_off"] = len(src) - 5      # its payload ends past the source
    segs[20]["data_len"] = 100
    dst = np.full(n * STRIDE, FILL, np.uint8)
    want = B.build(dst, src, hdrs, segs)
    assert [i for i in range(n) if want[1][i] == 0] == [10, 20]
    return dict(hdrs=hdrs, segs=segs, src=src, dst=dst, want=want, n=n)


def test_host_form_in_place_and_staged(V, txbatch):
    """Context.build_tcp_frames into a registered page-aligned arena at umem geometry, once with the
    source registered (read in place) and once with a heap source (the span of the payloads staged,
    data_off rebased in the library's copy): arena, frame lengths, out words and status equal the
    restatement's -- so the device form's, which the other tests hold to it -- and the caller's record
    array is unchanged.  An unregistered destination and an oversize span are refused by name."""
    tb = txbatch
    n, hdrs, segs = tb["n"], tb["hdrs"], tb["segs"]
    want, w_len, w_out, w_st = tb["want"]
    d_arena, d_len, d_out, d_st = gpu_build(V, tb["dst"], tb["src"], hdrs, segs)   # the device form on the same batch
    assert np.array_equal(d_arena, want) and np.array_equal(d_len, w_len) and np.array_equal(d_out, w_out) and np.array_equal(d_st, w_st)
    arena = page_aligned(n * STRIDE)
    src_reg = page_aligned(len(tb["src"]))
    src_reg[:] = tb["src"]
    heap = tb["src"].copy()
    ctx = V.Context(0, max_arena=128 << 10, max_pkts=n)
    ctx.register(arena)
    ctx.register(src_reg)
    try:
        for nm, s in (("in_place", src_reg), ("staged", heap), ("in_place_again", src_reg)):
            arena[:] = FILL
            before = segs.copy()
            flen, out, st = ctx.build_tcp_frames(arena, s, hdrs, segs)
            assert segs.tobytes() == before.tobytes(), nm
            assert np.array_equal(flen, w_len) and np.array_equal(out, w_out) and np.array_equal(st, w_st), nm
            assert np.array_equal(arena, want), (nm, first_diff(arena, want, segs))
            assert np.array_equal(s, tb["src"]), nm
        # the optional results, and an empty batch
        arena[:] = FILL
        flen, out, st = ctx.build_tcp_frames(arena, heap, hdrs, segs, want_out=False, want_status=False)
        assert out is None and st is None and np.array_equal(flen, w_len) and np.array_equal(arena, want)
        flen, out, st = ctx.build_tcp_frames(arena, heap, hdrs, segs[:0])
        assert len(flen) == 0
        # refusals: the frames as they were
        arena[:] = FILL
        other = np.zeros(8192, np.uint8)
        with pytest.raises(V.VpcsumError, match="vpcsum_ctx_build_tcp_frames: the destination must be registered"):
            ctx.build_tcp_frames(other, heap, hdrs, segs[:1])
        far = segs[:2].copy()
        far["data_off"] = (0, 200 << 10)
        far["data_len"] = 100
        with pytest.raises(V.VpcsumError, match=r"vpcsum_ctx_build_tcp_frames: the payloads span \d+ bytes > capacity 131072"):
            ctx.build_tcp_frames(arena, heap, hdrs, far)
        flen, _, _ = ctx.build_tcp_frames(arena, src_reg, hdrs, far)   # in place there is no span to stage
        assert list(flen) == [154, 174]
        arena[:2 * STRIDE] = FILL
        with pytest.raises(V.VpcsumError, match="vpcsum_ctx_build_tcp_frames: 65 records > capacity 64"):
            ctx.build_tcp_frames(arena, heap, hdrs, np.concatenate([segs, segs[:1]]))
        assert (arena == FILL).all()
    finally:
        ctx.unregister(src_reg)
        ctx.unregister(arena)
        ctx.close()


def test_pni_build_tcp_frames(V, txbatch):
    """Java_io_vproxy_vpcsum_VPCsum_buildTcpFrames driven through ctypes with PNI environments, as
    the JVM's downcall drives it: create, registerArena, buildTcpFrames on the 64 records (heap
    source), waitFor, close -- byte-equal frames, lengths, out words and status."""
    tb = txbatch
    n, hdrs, segs = tb["n"], tb["hdrs"], tb["segs"]
    want, w_len, w_out, w_st = tb["want"]
    L = V.lib()
    I32, I64, P = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p

    class Env(ctypes.Structure):   # PNIEnv_vpcsum_long: the exception (type, message, errno_), then the value
        _fields_ = [("type", ctypes.c_char_p), ("message", ctypes.c_char * 4096), ("errno_", I32), ("ret", I64), ("pad", I64)]
    assert ctypes.sizeof(Env) == 4128 and Env.ret.offset == 4112

    def call(f, *args):
        env = Env()
        f.restype = ctypes.c_int
        rc = f(ctypes.byref(env), *args)
        assert rc == 0, (env.type, env.message)
        return env.ret

    arena = page_aligned(n * STRIDE)
    arena[:] = FILL
    heap = tb["src"].copy()
    flen, out, st = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    ctx = call(L.Java_io_vproxy_vpcsum_VPCsum_create, I32(0), I64(128 << 10), I32(n))
    try:
        call(L.Java_io_vproxy_vpcsum_VPCsum_registerArena, I64(ctx), P(arena.ctypes.data), I64(arena.nbytes))
        t = call(L.Java_io_vproxy_vpcsum_VPCsum_buildTcpFrames, I64(ctx), P(arena.ctypes.data), I64(arena.nbytes),
                 P(heap.ctypes.data), I64(heap.nbytes), P(hdrs.ctypes.data), I32(len(hdrs)), P(segs.ctypes.data), I32(n),
                 P(flen.ctypes.data), P(out.ctypes.data), P(st.ctypes.data))
        call(L.Java_io_vproxy_vpcsum_VPCsum_waitFor, I64(ctx), I64(t))
        assert np.array_equal(flen, w_len) and np.array_equal(out, w_out) and np.array_equal(st, w_st)
        assert np.array_equal(arena, want), first_diff(arena, want, segs)
        env = Env()
        assert L.Java_io_vproxy_vpcsum_VPCsum_buildTcpFrames(ctypes.byref(env), I64(ctx), P(arena.ctypes.data), I64(arena.nbytes),
                                                             P(heap.ctypes.data), I64(heap.nbytes), P(hdrs.ctypes.data),
                                                             I32(len(hdrs)), P(segs.ctypes.data), I32(-1), P(flen.ctypes.data),
                                                             None, None) != 0
        assert env.type == b"java.lang.IllegalArgumentException" and env.message == b"buildTcpFrames: negative size"
    finally:
        call(L.Java_io_vproxy_vpcsum_VPCsum_close, I64(ctx))
