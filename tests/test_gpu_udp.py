"""The UDP datagram build and receive on the GPU (vpcsum_udp_build_async, vpcsum_udp_recv_async,
vpcsum_ctx_build_udp_frames, vpcsum_ctx_recv_udp_frames, VPCsum.buildUdpFrames / recvUdpFrames)
against the Python restatement of their rules (tests/udpvec.py: frames from the field list with the
oracle's sums; receive results from the oracle's MODE_VERIFY and numpy slices).  In every case the
WHOLE destination arena is compared with the restatement's: it is prefilled with 0xEE and every frame
or stored range has 3 guard bytes around it, so a byte written outside fails the case; lengths, out
words and status bytes are compared too (they start as 0xAB and carry two guard rows), and the source
arena must come back as it went."""
import ctypes

import numpy as np
import pytest

import udpvec as U
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FILL = 0xEE
LENGTHS = tuple(range(50)) + (63, 64, 65, 127, 128, 129, 1471, 1472, 1473)


@pytest.fixture(scope="module")
def V():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vproxy_amd import vpcsum
    vpcsum.lib()
    assert vpcsum.UDPDG_DTYPE == U.UDPDG_DTYPE and vpcsum.UDPRX_DTYPE == U.UDPRX_DTYPE and vpcsum.TCPHDR_DTYPE == U.HDR_DTYPE
    return vpcsum


def dev(a):
    """Host to device through pinned memory, as the other GPU tests copy."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).pin_memory().cuda()


def host(t):
    import torch
    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    h.copy_(t)
    torch.cuda.synchronize()
    return h.numpy().copy()


def results(n):
    import torch
    return (torch.full(((n + 2) * 4,), 0xAB, dtype=torch.uint8, device="cuda"), torch.full(((n + 2) * 4,), 0xAB, dtype=torch.uint8, device="cuda"),
            torch.full((n + 2,), 0xAB, dtype=torch.uint8, device="cuda"))


def read_results(n, a, out, st, want_out, want_status):
    a, out, st = host(a).view(np.uint32), host(out).view(np.uint32), host(st)
    assert (a[n:] == 0xABABABAB).all() and (out[n:] == 0xABABABAB).all() and (st[n:] == 0xAB).all()
    if not want_out:
        assert (out == 0xABABABAB).all()
    if not want_status:
        assert (st == 0xAB).all()
    return a[:n], out[:n], st[:n]


def first_diff(got, want):
    k = int(np.flatnonzero(got != want)[0])
    return f"byte {k}: {got[k]:#x} != {want[k]:#x}"


def same(name, got, want):
    assert np.array_equal(got, want), (name, [(int(i), hex(int(got[i])), hex(int(want[i]))) for i in np.flatnonzero(got != want)[:8]])


def empty16():
    import torch
    return torch.zeros(32, dtype=torch.uint8, device="cuda")


# ------------------------------------------------------------------------------------------
# build
# ------------------------------------------------------------------------------------------
def check_build(V, dst, src, hdrs, dgs, n=None, want_out=True, want_status=True):
    import torch
    n = len(dgs) if n is None else n
    want, w_len, w_out, w_st = U.build(dst, src, hdrs, dgs[:n])
    d_dst, d_src = dev(dst), dev(src) if len(src) else empty16()
    assert d_dst.data_ptr() % 16 == 0 and d_src.data_ptr() % 16 == 0
    flen, out, st = results(n)
    V.udp_build(d_dst, d_src[:len(src)], dev(hdrs) if len(hdrs) else empty16(), len(hdrs), dev(dgs) if len(dgs) else empty16(), n, flen,
                out if want_out else None, st if want_status else None)
    torch.cuda.synchronize()
    flen, out, st = read_results(n, flen, out, st, want_out, want_status)
    same("frame_len", flen, w_len)
    if want_status:
        same("status", st, w_st)
    if want_out:
        same("out", out, w_out)
    got = host(d_dst)
    assert np.array_equal(got, want), first_diff(got, want)
    if len(src):
        assert np.array_equal(host(d_src)[:len(src)], src)
    return want, w_len, w_out, w_st


def templates():
    return np.array([U.mk_hdr(4, 14, tos=0x10, ttl=64, ident=0x1234, frag=0x4000), U.mk_hdr(4, 0, sport=0xffff, dport=1),
                     U.mk_hdr(6, 14, bytes(range(0x20, 0x30)), bytes(range(0x40, 0x50)), tos=0xb8, ttl=3),
                     U.mk_hdr(6, 0, bytes(range(16)), bytes(range(16, 32)))], U.HDR_DTYPE)


class BuildLayout:
    """Frames one after another in the destination, each at a wanted address residue mod 16 with 3
    guard bytes around it; payloads likewise in the source."""

    def __init__(self, hdrs, rng):
        self.hdrs, self.rng, self.fcur, self.scur, self.dgs, self.pay = hdrs, rng, 0, 0, [], []

    def add(self, hi, d, fres=0, sres=0, body=None, **kw):
        H = U.header_len(self.hdrs[hi])
        self.fcur += 3
        self.fcur += (fres - self.fcur) % 16
        self.scur += 3
        self.scur += (sres - self.scur) % 16
        self.dgs.append(U.mk_dg(self.fcur, self.scur, d, hdr=hi, hlen=H, **kw))
        self.pay.append((self.scur, self.rng.integers(0, 256, d, dtype=np.uint8).tobytes() if body is None else body))
        self.fcur += H + d + 3
        self.scur += d + 3
        return len(self.dgs) - 1

    def arrays(self):
        src = np.full(self.scur + 5, 0x5a, np.uint8)
        for o, b in self.pay:
            src[o:o + len(b)] = np.frombuffer(b, np.uint8)
        return np.full(self.fcur + 7, FILL, np.uint8), src, np.array(self.dgs, U.UDPDG_DTYPE)


@pytest.mark.parametrize("hi", [0, 1, 2, 3], ids=["ipv4_eth", "ipv4_bare", "ipv6_eth", "ipv6_bare"])
def test_build_alignment_by_length(V, hi):
    """Every length of LENGTHS at every frame residue 0..15 with a rotating source residue, and at
    every source residue with a rotating frame residue: the payload behind an 8-byte header lands on
    every residue of the 16-B grid."""
    hdrs = templates()
    lay = BuildLayout(hdrs, np.random.default_rng(70 + hi))
    for k, d in enumerate(LENGTHS):
        for r in range(16):
            lay.add(hi, d, r, (r * 7 + k) % 16)
            lay.add(hi, d, (r * 5 + k) % 16, r)
    dst, src, dgs = lay.arrays()
    _, w_len, _, w_st = check_build(V, dst, src, hdrs, dgs)
    assert (w_st == U.S_DONE).all() and int(w_len.sum()) == 32 * sum(U.header_len(hdrs[hi]) + d for d in LENGTHS)


def test_build_sum_of_zero_is_ffff(V):
    """The datagram whose UDP sum computes to 0, IPv4 and IPv6, at several alignments: the field and
    d_out bits 16..31 are 0xffff."""
    hdrs = templates()
    rng = np.random.default_rng(74)
    lay = BuildLayout(hdrs, rng)
    idx = []
    for hi in range(4):
        body = U.sum_zero_payload(hdrs[hi], 64, rng)
        for fres, sres in ((0, 0), (5, 9), (10, 3), (15, 14)):
            idx.append((hi, lay.add(hi, 64, fres, sres, body=body)))
        lay.add(hi, 64, 3, 3)
    dst, src, dgs = lay.arrays()
    want, _, w_out, _ = check_build(V, dst, src, hdrs, dgs)
    for hi, i in idx:
        assert int(w_out[i]) >> 16 == 0xffff
        at = int(dgs[i]["frame_off"]) + U.header_len(hdrs[hi]) - 2
        assert want[at:at + 2].tobytes() == b"\xff\xff"
    assert sum(int(w) >> 16 == 0xffff for w in w_out) == len(idx)


def test_build_refusals_among_good_records(V):
    """Each refusal once, its neighbours built: a refused record writes nothing and reports 0, 0,
    S_BAD_DESC."""
    good = templates()
    hdrs = np.concatenate([good, np.array([U.mk_hdr(5), U.mk_hdr(4, 13), U.mk_hdr(4, rsv=0x100), U.mk_hdr(4, ack=0x01000000),
                                           U.mk_hdr(6, window=1)], U.HDR_DTYPE)])
    rng = np.random.default_rng(75)
    lay = BuildLayout(hdrs, rng)
    muts = [("hdr_past", lambda s: s.__setitem__("hdr", len(hdrs))), ("hdr_max", lambda s: s.__setitem__("hdr", 0xffffffff)),
            ("ver5", lambda s: s.__setitem__("hdr", 4)), ("l2_13", lambda s: s.__setitem__("hdr", 5)),
            ("hdr_rsv", lambda s: s.__setitem__("hdr", 6)), ("ack", lambda s: s.__setitem__("hdr", 7)),
            ("window", lambda s: s.__setitem__("hdr", 8)), ("rsv", lambda s: s.__setitem__("rsv", 1)),
            ("len_2_32", lambda s: (s.__setitem__("data_len", 0xffffffe4), s.__setitem__("frame_cap", 0xffffffff))),
            ("len_65508", lambda s: (s.__setitem__("data_len", 65508), s.__setitem__("frame_cap", 70000))),
            ("cap_short", lambda s: s.__setitem__("frame_cap", int(s["frame_cap"]) - 1)),
            ("frame_off_max", lambda s: s.__setitem__("frame_off", (1 << 64) - 8)),
            ("frame_off_far", lambda s: s.__setitem__("frame_off", 1 << 40)),
            ("data_off_max", lambda s: s.__setitem__("data_off", (1 << 64) - 8)),
            ("data_off_end", None)]                              # set below, once the source's length is known
    bad = {}
    for k, (name, f) in enumerate(muts):
        lay.add(k % 4, int(rng.integers(0, 200)), int(rng.integers(0, 16)), int(rng.integers(0, 16)))
        bad[name] = lay.add(k % 4, 40, int(rng.integers(0, 16)), int(rng.integers(0, 16)))
    last = lay.add(0, 40, 5, 5)
    dst, src, dgs = lay.arrays()
    dst = dst[:int(dgs[last]["frame_off"]) + 42 + 40]           # the last frame ends the destination
    for name, f in muts:
        s = dgs[bad[name]]
        if name == "data_off_end":
            s["data_off"] = len(src) - 39                        # one byte past the source
        else:
            f(s)
    _, w_len, w_out, w_st = check_build(V, dst, src, hdrs, dgs)
    refused = set(int(i) for i in np.flatnonzero(w_st == U.S_BAD_DESC))
    assert refused == set(bad.values()), (sorted(refused ^ set(bad.values())), bad)
    assert all(w_len[i] == 0 and w_out[i] == 0 for i in refused) and w_st[last] == U.S_DONE
    _, _, _, st2 = check_build(V, dst[:-1].copy(), src, hdrs, dgs)   # one byte shorter: the last no longer fits
    assert st2[last] == U.S_BAD_DESC


@pytest.mark.parametrize("n", [0, 1, 31, 33])
def test_build_batch_sizes_and_optional_outputs(V, n):
    hdrs = templates()
    rng = np.random.default_rng(76)
    lay = BuildLayout(hdrs, rng)
    for i in range(40):
        lay.add(i % 4, int(rng.choice([0, 1, 17, 200, 1472])), int(rng.integers(0, 16)), int(rng.integers(0, 16)))
    dst, src, dgs = lay.arrays()
    check_build(V, dst, src, hdrs, dgs, n)
    check_build(V, dst, src, hdrs, dgs, n, want_out=False, want_status=False)


def test_build_largest_datagrams(V):
    """IPv4 data_len 65,507 and IPv6 65,527 of 0xff are built (the accumulators' width); 65,508 and
    65,528 are refused."""
    hdrs = np.array([U.mk_hdr(4, 14, b"\xff" * 4, b"\xff" * 4, 0xffff, 0xffff, tos=0xff, ttl=0xff, ident=0xffff, frag=0xffff),
                     U.mk_hdr(6, 14, b"\xff" * 16, b"\xff" * 16, 0xffff, 0xffff, tos=0xff, ttl=0xff)], U.HDR_DTYPE)
    src = np.full(65531 + 9, 0xff, np.uint8)
    dgs, cur = [], 0
    for hi, d, fres in ((0, 65507, 5), (0, 65508, 0), (1, 65527, 11), (1, 65528, 0)):
        cur += 3
        cur += (fres - cur) % 16
        dgs.append(U.mk_dg(cur, 3 if d & 1 else 2, d, hdr=hi, hlen=U.header_len(hdrs[hi])))
        cur += U.header_len(hdrs[hi]) + d + 3
    dgs = np.array(dgs, U.UDPDG_DTYPE)
    _, w_len, _, w_st = check_build(V, np.full(cur + 5, FILL, np.uint8), src, hdrs, dgs)
    assert list(w_len) == [42 + 65507, 0, 62 + 65527, 0] and list(w_st) == [U.S_DONE, U.S_BAD_DESC, U.S_DONE, U.S_BAD_DESC]


def test_build_the_reference_frame(V):
    """udpIpv4Example of kat.json rebuilt on the GPU, byte for byte, sums 0x7f41 / 0xdf0d."""
    from test_udp_cpu import kat
    raw = bytes.fromhex(kat()["hex"])
    h, payload = U.from_frame(raw)
    src = np.frombuffer(b"\x11" * 5 + payload + b"\x22" * 3, np.uint8).copy()
    dst = np.full(7 + len(raw) + 9, FILL, np.uint8)
    want, _, w_out, _ = check_build(V, dst, src, np.array([h], U.HDR_DTYPE), np.array([U.mk_dg(7, 5, 61)], U.UDPDG_DTYPE))
    assert want[7:7 + len(raw)].tobytes() == raw and int(w_out[0]) == 0x7f41 | (0xdf0d << 16)


# ------------------------------------------------------------------------------------------
# receive
# ------------------------------------------------------------------------------------------
def check_recv(V, dst, arena, desc, rx, n=None, want_out=True, want_status=True):
    import torch
    n = len(desc) if n is None else n
    want, w_stored, w_out, w_st = U.recv(dst, arena, desc[:n], rx[:n])
    d_dst, d_arena = dev(dst) if len(dst) else empty16(), dev(arena)
    assert d_dst.data_ptr() % 16 == 0 and d_arena.data_ptr() % 16 == 0
    stored, out, st = results(n)
    V.udp_recv(d_arena, dev(desc) if len(desc) else empty16(), dev(rx) if len(rx) else empty16(), n, d_dst[:len(dst)], stored,
               out if want_out else None, st if want_status else None)
    torch.cuda.synchronize()
    stored, out, st = read_results(n, stored, out, st, want_out, want_status)
    same("stored", stored, w_stored)
    if want_status:
        same("status", st, w_st)
    if want_out:
        same("out", out, w_out)
    got = host(d_dst)[:len(dst)]
    assert np.array_equal(got, want), first_diff(got, want)
    assert np.array_equal(host(d_arena), arena)
    return want, w_stored, w_out, w_st


class RecvLayout:
    """Packets one after another in the source arena, the UDP segment's first byte at a wanted
    address residue mod 16 (`pad` bytes of 0xff L2 padding behind the packet), and their stored ranges
    in the destination at a wanted residue, 3 guard bytes around each."""

    def __init__(self):
        self.scur, self.dcur, self.desc, self.rx, self.chunks = 0, 0, [], [], []

    def add(self, l3: bytes, l4_off: int, ver: int, sres=0, dres=0, ops=U.STORE, pad=0, flags=None, cap=None):
        stored = max(len(l3) - l4_off - 8, 0)
        self.scur += 3
        self.scur += (sres - (self.scur + l4_off)) % 16
        self.dcur += 3
        self.dcur += (dres - self.dcur) % 16
        self.desc.append(U.mk_desc(self.scur, len(l3), l4_off, ver, flags=flags))
        self.rx.append(U.mk_rx(self.dcur, stored if cap is None else cap, ops))
        self.chunks.append((self.scur, l3 + b"\xff" * pad))
        self.scur += len(l3) + pad + 3
        if ops & U.STORE:
            self.dcur += stored + 3
        return len(self.desc) - 1

    def arrays(self, dst_tail=3):
        arena = np.full(self.scur + 13, 0x5a, np.uint8)
        for o, b in self.chunks:
            arena[o:o + len(b)] = np.frombuffer(b, np.uint8)
        dst = np.full(self.dcur + dst_tail, FILL, np.uint8)
        return dst, arena, np.array(self.desc, O.DESC_DTYPE), np.array(self.rx, U.UDPRX_DTYPE)


def payload(rng, d):
    return rng.integers(0, 256, d, dtype=np.uint8).tobytes()


@pytest.mark.parametrize("ver", [4, 6], ids=["ipv4", "ipv6"])
def test_recv_alignment_grid(V, ver):
    """Every length of LENGTHS at every segment residue 0..15 with a rotating destination residue and
    the other way round; length 0 is a segment of exactly 8 bytes (stores 0 bytes) that lies inside
    one 16-B group (residues 0..8) or straddles two (9..15), with STORE and verify-only."""
    rng = np.random.default_rng(80 + ver)
    lay = RecvLayout()
    for k, d in enumerate(LENGTHS):
        l3, l4o = U.udp_l3(ver, payload(rng, d), sport=int(rng.integers(1, 65536)))
        for r in range(16):
            lay.add(l3, l4o, ver, r, (r * 7 + k) % 16)
            lay.add(l3, l4o, ver, (r * 5 + k) % 16, r, ops=U.STORE if d else 0)
    dst, arena, desc, rx = lay.arrays()
    _, w_stored, _, w_st = check_recv(V, dst, arena, desc, rx)
    ok = U.S_DONE | U.S_L4_OK | (U.S_IP_OK if ver == 4 else 0)
    assert (w_st == ok).all() and int(w_stored.sum()) == 32 * sum(LENGTHS)


def test_recv_verdicts(V, orc):
    """Good; one flipped payload bit (not OK, bytes still stored); a stored 0 (S_UDP_NOCSUM, not
    S_L4_OK, stored); a stored 0xffff on a sum-zero datagram (S_L4_OK); a stored 0xffff on another
    (not OK); a wrong IPv4 header sum clears S_IP_OK only."""
    rng = np.random.default_rng(82)
    lay = RecvLayout()
    idx = {}
    for ver in (4, 6):
        l3, o = U.udp_l3(ver, payload(rng, 101))
        idx["good", ver] = lay.add(l3, o, ver, 3, 9)
        b = bytearray(l3)
        b[o + 8 + 50] ^= 0x04
        idx["flip", ver] = lay.add(bytes(b), o, ver, 7, 2)
        idx["nocsum", ver] = lay.add(U.udp_l3(ver, payload(rng, 33), field=0)[0], o, ver, 11, 5)
        idx["ffff_wrong", ver] = lay.add(U.udp_l3(ver, payload(rng, 33), field=0xffff)[0], o, ver, 1, 15)
        h = U.mk_hdr(ver, 0, bytes(range(16)) if ver == 6 else b"\x0a\x00\x00\x01", bytes(range(16, 32)) if ver == 6 else b"\x0a\x00\x00\x02")
        f, _, c = U.frame(h, U.sum_zero_payload(h, 64, rng))
        assert c == 0xffff
        idx["zero_ffff", ver] = lay.add(f, o, ver, 13, 1)
        idx["zero_0", ver] = lay.add(f[:o + 6] + b"\0\0" + f[o + 8:], o, ver, 6, 6)
    b = bytearray(U.udp_l3(4, payload(rng, 40))[0])
    b[8] ^= 0x10                                                   # TTL: not in the pseudo-header
    idx["ttl"] = lay.add(bytes(b), 20, 4, 3, 11)
    dst, arena, desc, rx = lay.arrays()
    _, w_stored, w_out, w_st = check_recv(V, dst, arena, desc, rx)
    o_out, o_st = orc.process(arena, desc, O.MODE_VERIFY)
    assert np.array_equal(w_out, o_out) and np.array_equal(w_st, o_st)
    for ver in (4, 6):
        ip = U.S_IP_OK if ver == 4 else 0
        assert w_st[idx["good", ver]] == U.S_DONE | U.S_L4_OK | ip and w_stored[idx["good", ver]] == 101
        assert w_st[idx["flip", ver]] == U.S_DONE | ip and w_stored[idx["flip", ver]] == 101
        assert w_st[idx["nocsum", ver]] == U.S_DONE | U.S_UDP_NOCSUM | ip and w_stored[idx["nocsum", ver]] == 33
        assert w_st[idx["ffff_wrong", ver]] == U.S_DONE | ip
        assert w_st[idx["zero_ffff", ver]] == U.S_DONE | U.S_L4_OK | ip and int(w_out[idx["zero_ffff", ver]]) >> 16 == 0xffff
        assert w_st[idx["zero_0", ver]] == U.S_DONE | U.S_UDP_NOCSUM | ip and int(w_out[idx["zero_0", ver]]) >> 16 == 0xffff
    assert w_st[idx["ttl"]] == U.S_DONE | U.S_L4_OK


def test_recv_headers_padding_and_length_field(V):
    """IPv4 with options (IHL 6..15) with and without F_IP, and with a wrong header sum; IPv6 behind
    an extension header; 0xff L2 padding behind l3_len that would break the sum if read, with the
    guard pattern behind the stored range; a UDP length field that disagrees with seg_len (too
    short, too long, 0): the data is still bytes 8..seg_len and the verdict the oracle's."""
    rng = np.random.default_rng(83)
    lay = RecvLayout()
    wrong = []
    for ihl in range(6, 16):
        for d in (0, 1, 37, 300):
            l3, o = U.udp_l3(4, payload(rng, d), ihl=ihl)
            lay.add(l3, o, 4, int(rng.integers(0, 16)), int(rng.integers(0, 16)), pad=int(rng.integers(1, 9)))
            lay.add(l3, o, 4, int(rng.integers(0, 16)), int(rng.integers(0, 16)), pad=int(rng.integers(1, 9)), flags=O.F_L4)
        b = bytearray(l3)
        b[10] ^= 0x01
        wrong.append(lay.add(bytes(b), o, 4, int(rng.integers(0, 16)), int(rng.integers(0, 16))))
    for ext in (8, 16, 40):
        for d in (0, 5, 64, 301):
            l3, o = U.udp_l3(6, payload(rng, d), ext=ext)
            lay.add(l3, o, 6, int(rng.integers(0, 16)), int(rng.integers(0, 16)), pad=int(rng.integers(1, 9)))
    lens = []
    for ver in (4, 6):
        for length in (8, 20, 108 + 5, 0, 0xffff):
            l3, o = U.udp_l3(ver, payload(rng, 100), length=length)
            lens.append(lay.add(l3, o, ver, int(rng.integers(0, 16)), int(rng.integers(0, 16)), pad=4))
    dst, arena, desc, rx = lay.arrays()
    assert set(desc["l4_off"][desc["l3_ver"] == 4]) >= set(range(24, 64, 4)) and set(desc["l4_off"][desc["l3_ver"] == 6]) >= {48, 56, 80}
    _, w_stored, _, w_st = check_recv(V, dst, arena, desc, rx)
    assert (w_st & U.S_L4_OK).all() and all(w_stored[i] == 100 for i in lens)
    assert all(not w_st[i] & U.S_IP_OK for i in wrong) and (w_st[desc["flags"] == O.F_L4] & U.S_IP_OK == 0).all()


def test_recv_refusals_among_good_records(V):
    """Every refusal in one batch between stored and verify-only records: a refused record writes
    nothing and reports 0, 0, S_BAD_DESC; dst_cap exact is taken and one byte short refused."""
    rng = np.random.default_rng(84)
    lay = RecvLayout()
    v4, o4 = U.udp_l3(4, payload(rng, 50))
    v6, o6 = U.udp_l3(6, payload(rng, 50))
    muts = [
        ("proto", 4, lambda d, r: d.__setitem__("l4_proto", 6)),
        ("ver5", 4, lambda d, r: d.__setitem__("l3_ver", 5)),
        ("ver0", 6, lambda d, r: d.__setitem__("l3_ver", 0)),
        ("no_l4", 4, lambda d, r: d.__setitem__("flags", O.F_IP)),
        ("l4p", 4, lambda d, r: d.__setitem__("flags", O.F_L4 | O.F_L4P)),
        ("raw", 6, lambda d, r: d.__setitem__("flags", O.F_L4 | O.F_RAW)),
        ("pre", 4, lambda d, r: d.__setitem__("flags", O.F_L4 | O.F_PRE)),
        ("ip_on_v6", 6, lambda d, r: d.__setitem__("flags", O.F_L4 | O.F_IP)),
        ("l4_off_past", 4, lambda d, r: d.__setitem__("l4_off", int(d["l3_len"]) + 4)),
        ("l4_off_16", 4, lambda d, r: d.__setitem__("l4_off", 16)),
        ("l4_off_22", 4, lambda d, r: d.__setitem__("l4_off", 22)),
        ("l4_off_39", 6, lambda d, r: d.__setitem__("l4_off", 39)),
        ("l3_off_max", 4, lambda d, r: d.__setitem__("l3_off", (1 << 64) - 8)),
        ("l3_off_far", 6, lambda d, r: d.__setitem__("l3_off", 1 << 40)),
        ("short_7", 4, lambda d, r: d.__setitem__("l3_len", 20 + 7)),
        ("ops_2", 4, lambda d, r: r.__setitem__("ops", 2)),
        ("ops_81", 6, lambda d, r: r.__setitem__("ops", 0x81)),
        ("rsv0", 4, lambda d, r: r["rsv"].__setitem__(0, 1)),
        ("rsv2", 6, lambda d, r: r["rsv"].__setitem__(2, 0x80)),
        ("cap_short", 4, lambda d, r: r.__setitem__("dst_cap", 49)),
        ("dst_off_max", 6, lambda d, r: r.__setitem__("dst_off", (1 << 64) - 4)),
    ]
    patches, bad = [], {}
    for k, (name, ver, f) in enumerate(muts):
        lay.add(v4 if k & 1 else v6, o4 if k & 1 else o6, 4 if k & 1 else 6, int(rng.integers(0, 16)), int(rng.integers(0, 16)),
                ops=U.STORE if k % 3 else 0)
        l3, o = (v4, o4) if ver == 4 else (v6, o6)
        patches.append((lay.add(l3, o, ver, int(rng.integers(0, 16)), int(rng.integers(0, 16))), name, f))
    lay.add(v6, o6, 6, 1, 1, cap=50)                                          # dst_cap exact
    last = lay.add(v4, o4, 4, 15, 15)                                         # ends the destination
    dst, arena, desc, rx = lay.arrays(dst_tail=-3)
    for i, name, f in patches:
        f(desc[i], rx[i])
        bad[name] = i
    assert int(rx[last]["dst_off"]) + 50 == len(dst)
    _, w_stored, w_out, w_st = check_recv(V, dst, arena, desc, rx)
    refused = set(int(i) for i in np.flatnonzero(w_st == U.S_BAD_DESC))
    assert refused == set(bad.values()), (sorted(refused ^ set(bad.values())), bad)
    assert all(w_stored[i] == 0 and w_out[i] == 0 for i in refused)
    assert (w_st[sorted(set(range(len(desc))) - refused)] & U.S_L4_OK).all()
    _, s2, _, st2 = check_recv(V, dst[:-1].copy(), arena, desc, rx)
    assert st2[last] == U.S_BAD_DESC and s2[last] == 0


@pytest.mark.parametrize("n", [0, 1, 31, 33])
def test_recv_batch_sizes_and_optional_outputs(V, n):
    rng = np.random.default_rng(85)
    lay = RecvLayout()
    for i in range(40):
        ver = 4 if i & 1 else 6
        l3, o = U.udp_l3(ver, payload(rng, int(rng.choice([0, 1, 17, 200, 1472]))))
        lay.add(l3, o, ver, int(rng.integers(0, 16)), int(rng.integers(0, 16)), ops=U.STORE if i % 5 else 0)
    dst, arena, desc, rx = lay.arrays()
    check_recv(V, dst, arena, desc, rx, n)
    check_recv(V, dst, arena, desc, rx, n, want_out=False, want_status=False)


def test_recv_largest_segments_of_ff(V):
    """IPv4 and IPv6 packets of l3_len 65,535 whose every segment byte but the field is 0xff, stored
    and verify only, at odd alignments: the accumulators' width."""
    lay = RecvLayout()
    l4, o4 = U.udp_l3(4, b"\xff" * (65515 - 8), sport=0xffff, dport=0xffff, src=b"\xff" * 4, dst=b"\xff" * 4, length=0xffff)
    l6, o6 = U.udp_l3(6, b"\xff" * (65495 - 8), sport=0xffff, dport=0xffff, src=b"\xff" * 16, dst=b"\xff" * 16, length=0xffff)
    assert len(l4) == 65535 and len(l6) == 65535
    lay.add(l4, o4, 4, 5, 11)
    lay.add(l4, o4, 4, 14, 0, ops=0)
    lay.add(l6, o6, 6, 1, 6)
    dst, arena, desc, rx = lay.arrays()
    _, w_stored, _, w_st = check_recv(V, dst, arena, desc, rx)
    assert list(w_stored) == [65507, 0, 65487] and (w_st & U.S_L4_OK).all()


# ------------------------------------------------------------------------------------------
# both directions, host forms and PNI
# ------------------------------------------------------------------------------------------
def test_round_trip(V):
    """vpcsum_udp_build_async builds 64 Ethernet frames (IPv4 and IPv6, mixed alignments), parsed by
    vpcsum_parse_ether_async, received by vpcsum_udp_recv_async into a fresh buffer at each record's
    data_off: all S_L4_OK (and S_IP_OK on IPv4), the send buffer comes back."""
    import torch
    rng = np.random.default_rng(86)
    hdrs = templates()[[0, 2]]
    lay = BuildLayout(hdrs, rng)
    for i in range(64):
        lay.add(i & 1, int(rng.choice([0, 1, 2, 63, 64, 65, 517, 1360, 1472])), int(rng.integers(0, 16)), int(rng.integers(0, 16)))
    dst, send, dgs = lay.arrays()
    n = len(dgs)
    d_frames, d_send = dev(dst), dev(send)
    flen = torch.zeros(n, dtype=torch.int32, device="cuda")
    V.udp_build(d_frames, d_send, dev(hdrs), 2, dev(dgs), n, flen, None, None)
    d_desc = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    V.parse_ether(d_frames, dev(dgs["frame_off"].copy()), flen, n, d_desc)
    torch.cuda.synchronize()
    desc = host(d_desc).view(O.DESC_DTYPE)
    assert (desc["l4_proto"] == 17).all() and (desc["l3_off"] == dgs["frame_off"] + 14).all()
    rx = np.array([U.mk_rx(int(s["data_off"]), int(s["data_len"])) for s in dgs], U.UDPRX_DTYPE)
    d_back = dev(np.full(len(send), 0x5a, np.uint8))
    stored = torch.zeros(n, dtype=torch.int32, device="cuda")
    st = torch.zeros(n, dtype=torch.uint8, device="cuda")
    V.udp_recv(d_frames, d_desc, dev(rx), n, d_back, stored, None, st)
    torch.cuda.synchronize()
    st = host(st)
    assert np.array_equal(host(stored).view(np.uint32), dgs["data_len"])
    assert (st[0::2] == U.S_DONE | U.S_L4_OK | U.S_IP_OK).all() and (st[1::2] == U.S_DONE | U.S_L4_OK).all(), [hex(x) for x in st]
    assert np.array_equal(host(d_back), send)


STRIDE, HEADROOM = 2048, 384
_KEEP = []


def page_aligned(nbytes):
    raw = np.zeros(nbytes + 8192, np.uint8)
    _KEEP.append(raw)   # page-locked and released by the tests: kept for the life of the process
    skip = (-raw.ctypes.data) % 4096
    return raw[skip:skip + nbytes]


@pytest.fixture(scope="module")
def txbatch():
    """48 datagrams into umem chunks (2,048 bytes, frame at +384) from a send buffer; two refused."""
    rng = np.random.default_rng(87)
    hdrs = templates()
    n = 48
    dgs, pos = np.zeros(n, U.UDPDG_DTYPE), 0
    for i in range(n):
        d = int(rng.choice([0, 1, 100, 517, 1360, 1472]))
        dgs[i] = U.mk_dg(i * STRIDE + HEADROOM, pos + 1, d, hdr=i % 4, frame_cap=STRIDE - HEADROOM)
        pos += d + 3
    dgs[9]["rsv"] = 1
    dgs[20]["hdr"] = 4
    src = rng.integers(0, 256, pos + 8, dtype=np.uint8)
    dst = np.full(n * STRIDE, FILL, np.uint8)
    want = U.build(dst, src, hdrs, dgs)
    assert [i for i in range(n) if want[3][i] == U.S_BAD_DESC] == [9, 20]
    return dict(hdrs=hdrs, dgs=dgs, src=src, dst=dst, want=want, n=n)


@pytest.fixture(scope="module")
def rxbatch():
    """48 received Ethernet frames at umem geometry, IPv4 and IPv6; one bad sum, one without a
    checksum, two refused records."""
    rng = np.random.default_rng(88)
    n = 48
    arena = np.full(n * STRIDE, 0x5a, np.uint8)
    desc, rx = np.zeros(n, O.DESC_DTYPE), np.zeros(n, U.UDPRX_DTYPE)
    pos = 0
    for i in range(n):
        ver = 6 if i % 4 == 3 else 4
        d = int(rng.choice([0, 1, 100, 517, 1360, 1472]))
        l3, o = U.udp_l3(ver, payload(rng, d), field=0 if i == 5 else None)
        at = i * STRIDE + HEADROOM
        eth = b"\x02\0\0\0\x0a\x01\x02\0\0\0\x0b\x02" + (b"\x08\x00" if ver == 4 else b"\x86\xdd")
        arena[at:at + 14 + len(l3)] = np.frombuffer(eth + l3, np.uint8)
        desc[i] = U.mk_desc(at + 14, len(l3), o, ver)
        rx[i] = U.mk_rx(pos + 1, d, U.STORE if i % 6 else 0)
        pos += d + 4
    arena[int(desc[7]["l3_off"]) + int(desc[7]["l3_len"]) - 1] ^= 0x20
    rx[10]["rsv"][1] = 1
    desc[20]["l4_proto"] = 6
    dst = np.full(pos + 64, FILL, np.uint8)
    want = U.recv(dst, arena, desc, rx)
    assert [i for i in range(n) if want[3][i] == U.S_BAD_DESC] == [10, 20] and want[3][5] & U.S_UDP_NOCSUM
    return dict(arena=arena, desc=desc, rx=rx, dst=dst, want=want, n=n)


def test_host_form_build(V, txbatch):
    """Context.build_udp_frames into a registered umem, the source registered (read in place) and a
    heap copy (staged as one span): the device form's results; an unregistered destination is refused."""
    tb = txbatch
    want, w_len, w_out, w_st = tb["want"]
    check_build(V, tb["dst"], tb["src"], tb["hdrs"], tb["dgs"])
    umem, sbuf = page_aligned(len(tb["dst"])), page_aligned(len(tb["src"]))
    sbuf[:] = tb["src"]
    heap = tb["src"].copy()
    ctx = V.Context(0, max_arena=256 << 10, max_pkts=tb["n"])
    ctx.register(umem)
    ctx.register(sbuf)
    try:
        for nm, s in (("in_place", sbuf), ("staged", heap)):
            umem[:] = FILL
            g0 = tb["dgs"].copy()
            flen, out, st = ctx.build_udp_frames(umem, s, tb["hdrs"], tb["dgs"])
            assert tb["dgs"].tobytes() == g0.tobytes(), nm
            assert np.array_equal(flen, w_len) and np.array_equal(out, w_out) and np.array_equal(st, w_st), nm
            assert np.array_equal(umem, want), (nm, first_diff(umem, want))
            assert np.array_equal(s, tb["src"]), nm
        flen, _, _ = ctx.build_udp_frames(umem, heap, tb["hdrs"], tb["dgs"][:0])
        assert len(flen) == 0
        umem[:] = FILL
        with pytest.raises(V.VpcsumError, match="vpcsum_ctx_build_udp_frames: the destination must be registered"):
            ctx.build_udp_frames(np.zeros(8192, np.uint8), heap, tb["hdrs"], tb["dgs"][:1])
        assert (umem == FILL).all()
    finally:
        ctx.unregister(sbuf)
        ctx.unregister(umem)
        ctx.close()


def test_host_form_recv(V, rxbatch):
    """Context.recv_udp_frames into a registered receive buffer, the RX arena registered (read in
    place) and a heap copy (staged): the device form's results; an unregistered destination is refused."""
    rb = rxbatch
    desc, rx = rb["desc"], rb["rx"]
    want, w_stored, w_out, w_st = rb["want"]
    check_recv(V, rb["dst"], rb["arena"], desc, rx)
    rbuf, umem = page_aligned(len(rb["dst"])), page_aligned(len(rb["arena"]))
    umem[:] = rb["arena"]
    heap = rb["arena"].copy()
    ctx = V.Context(0, max_arena=128 << 10, max_pkts=rb["n"])
    ctx.register(rbuf)
    ctx.register(umem)
    try:
        for nm, a in (("in_place", umem), ("staged", heap)):
            rbuf[:] = FILL
            d0, r0 = desc.copy(), rx.copy()
            stored, out, st = ctx.recv_udp_frames(a, desc, rx, rbuf)
            assert desc.tobytes() == d0.tobytes() and rx.tobytes() == r0.tobytes(), nm
            assert np.array_equal(stored, w_stored) and np.array_equal(out, w_out) and np.array_equal(st, w_st), nm
            assert np.array_equal(rbuf, want), (nm, first_diff(rbuf, want))
            assert np.array_equal(a, rb["arena"]), nm
        stored, _, _ = ctx.recv_udp_frames(heap, desc[:0], rx[:0], rbuf)
        assert len(stored) == 0
        rbuf[:] = FILL
        with pytest.raises(V.VpcsumError, match="vpcsum_ctx_recv_udp_frames: the destination must be registered"):
            ctx.recv_udp_frames(umem, desc[:1], rx[:1], np.zeros(8192, np.uint8))
        assert (rbuf == FILL).all()
    finally:
        ctx.unregister(umem)
        ctx.unregister(rbuf)
        ctx.close()


def test_pni_build_and_recv_udp_frames(V, txbatch, rxbatch):
    """Java_io_vproxy_vpcsum_VPCsum_buildUdpFrames / recvUdpFrames driven through ctypes with PNI
    environments, as the JVM's downcall drives them: create, registerArena, the call on heap sources,
    waitFor, close -- byte-equal arenas, lengths, out words and status."""
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

    tb, rb = txbatch, rxbatch
    umem, rbuf = page_aligned(len(tb["dst"])), page_aligned(len(rb["dst"]))
    umem[:] = FILL
    rbuf[:] = FILL
    n = tb["n"]
    assert rb["n"] == n
    a, out, st = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    src, hdrs, dgs = tb["src"].copy(), np.ascontiguousarray(tb["hdrs"]), np.ascontiguousarray(tb["dgs"])
    heap, desc, rx = rb["arena"].copy(), np.ascontiguousarray(rb["desc"]), np.ascontiguousarray(rb["rx"])
    ctx = call(L.Java_io_vproxy_vpcsum_VPCsum_create, I32(0), I64(256 << 10), I32(n))
    try:
        call(L.Java_io_vproxy_vpcsum_VPCsum_registerArena, I64(ctx), P(umem.ctypes.data), I64(umem.nbytes))
        call(L.Java_io_vproxy_vpcsum_VPCsum_registerArena, I64(ctx), P(rbuf.ctypes.data), I64(rbuf.nbytes))
        t = call(L.Java_io_vproxy_vpcsum_VPCsum_buildUdpFrames, I64(ctx), P(umem.ctypes.data), I64(umem.nbytes), P(src.ctypes.data),
                 I64(src.nbytes), P(hdrs.ctypes.data), I32(len(hdrs)), P(dgs.ctypes.data), I32(n), P(a.ctypes.data), P(out.ctypes.data),
                 P(st.ctypes.data))
        call(L.Java_io_vproxy_vpcsum_VPCsum_waitFor, I64(ctx), I64(t))
        want, w_len, w_out, w_st = tb["want"]
        assert np.array_equal(a, w_len) and np.array_equal(out, w_out) and np.array_equal(st, w_st)
        assert np.array_equal(umem, want), first_diff(umem, want)
        t = call(L.Java_io_vproxy_vpcsum_VPCsum_recvUdpFrames, I64(ctx), P(heap.ctypes.data), I64(heap.nbytes), P(desc.ctypes.data),
                 P(rx.ctypes.data), I32(n), P(rbuf.ctypes.data), I64(rbuf.nbytes), P(a.ctypes.data), P(out.ctypes.data),
                 P(st.ctypes.data))
        call(L.Java_io_vproxy_vpcsum_VPCsum_waitFor, I64(ctx), I64(t))
        want, w_stored, w_out, w_st = rb["want"]
        assert np.array_equal(a, w_stored) and np.array_equal(out, w_out) and np.array_equal(st, w_st)
        assert np.array_equal(rbuf, want), first_diff(rbuf, want)
        assert np.array_equal(heap, rb["arena"]) and np.array_equal(src, tb["src"])
    finally:
        call(L.Java_io_vproxy_vpcsum_VPCsum_close, I64(ctx))
