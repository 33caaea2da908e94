"""The ICMP replies on the GPU (vpcsum_icmp_reply_async, vpcsum_ctx_reply_icmp_frames,
VPCsum.replyIcmpFrames) against the Python restatement of the three Java builders (tests/icmpvec.py:
frames from the field list with the oracle's sums; an echo's out / status from the oracle's
MODE_VERIFY).  In every case the WHOLE destination arena is compared with the restatement's: it is
prefilled with 0xEE and every reply frame has 3 guard bytes around it, so a byte written outside
[frame_off, frame_off + L) fails the case; lengths, sums, out words and status bytes are compared too
(they start as 0xAB and carry two guard rows), and the source arena must come back as it went.  The
requests lie in a source prefilled with 0x5a, L2 padding included: a byte read past l3_len changes a
sum."""
import ctypes

import numpy as np
import pytest

import icmpvec as C
from oracle import oracle as O

pytestmark = pytest.mark.gpu

FILL, SRC_FILL = 0xEE, 0x5A
SEG_LENS = (8, 9, 11, 12, 19, 20, 21, 35, 36, 64, 1472)


@pytest.fixture(scope="module")
def V():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vproxy_amd import vpcsum
    vpcsum.lib()
    assert vpcsum.ICMPRP_DTYPE == C.ICMPRP_DTYPE and vpcsum.TCPHDR_DTYPE == C.HDR_DTYPE
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


def first_diff(got, want):
    k = int(np.flatnonzero(got != want)[0])
    return f"byte {k}: {got[k]:#x} != {want[k]:#x}"


def same(name, got, want):
    assert np.array_equal(got, want), (name, [(int(i), hex(int(got[i])), hex(int(want[i]))) for i in np.flatnonzero(got != want)[:8]])


def empty16():
    import torch
    return torch.zeros(32, dtype=torch.uint8, device="cuda")


def check_reply(V, dst, arena, desc, hdrs, rps, n=None, want_csum=True, want_out=True, want_status=True):
    """The device form on copies of the arenas; everything it writes against the restatement."""
    import torch
    n = len(desc) if n is None else n
    want, w_len, w_cs, w_out, w_st = C.reply(dst, arena, desc[:n], hdrs, rps[:n])
    d_dst, d_arena = dev(dst), dev(arena)
    assert d_dst.data_ptr() % 16 == 0 and d_arena.data_ptr() % 16 == 0
    u32 = [torch.full(((n + 2) * 4,), 0xAB, dtype=torch.uint8, device="cuda") for _ in range(3)]
    st = torch.full((n + 2,), 0xAB, dtype=torch.uint8, device="cuda")
    V.icmp_reply(d_arena, dev(desc) if len(desc) else empty16(), dev(hdrs) if len(hdrs) else empty16(), len(hdrs),
                 dev(rps) if len(rps) else empty16(), n, d_dst, u32[0], u32[1] if want_csum else None, u32[2] if want_out else None,
                 st if want_status else None)
    torch.cuda.synchronize()
    flen, cs, out = (host(t).view(np.uint32) for t in u32)
    st = host(st)
    for a, wanted in ((flen, True), (cs, want_csum), (out, want_out)):
        assert (a[n:] == 0xABABABAB).all() and (wanted or (a == 0xABABABAB).all())
    assert (st[n:] == 0xAB).all() and (want_status or (st == 0xAB).all())
    same("frame_len", flen[:n], w_len)
    if want_csum:
        same("csum", cs[:n], w_cs)
    if want_out:
        same("out", out[:n], w_out)
    if want_status:
        same("status", st[:n], w_st)
    got = host(d_dst)
    assert np.array_equal(got, want), first_diff(got, want)
    assert np.array_equal(host(d_arena), arena)
    return want, w_len, w_cs, w_out, w_st


def templates():
    return np.array([C.mk_hdr(4, 14, tos=0x10, ident=0x1234, frag=0x4000), C.mk_hdr(4, 0),
                     C.mk_hdr(6, 14, C.V6_DST, C.V6_SRC, tos=0xb8, ttl=3), C.mk_hdr(6, 0, bytes(range(16)), bytes(range(16, 32)))],
                    C.HDR_DTYPE)


class Layout:
    """Requests one after another in the source, each with its SEGMENT (echo) or its IP header (the
    errors) at a wanted address residue mod 16, with `pad` bytes of L2 padding and 3 guard bytes behind
    it; reply frames likewise in the destination, the reply's ICMP byte 0 at the wanted residue."""

    def __init__(self, hdrs):
        self.hdrs, self.scur, self.fcur, self.desc, self.rps, self.pkts = hdrs, 0, 0, [], [], []

    def add(self, hi, kind, l3, l4_off, proto, sres=0, dres=0, pad=2, flags=None, **kw):
        h = self.hdrs[hi]
        ver = 4 if l3[0] >> 4 == 4 else 6
        at = l4_off if kind == C.ECHO else 0
        self.scur += 3
        self.scur += (sres - (self.scur + at)) % 16
        self.desc.append(C.mk_desc(self.scur, len(l3), l4_off, ver, proto, flags))
        self.pkts.append((self.scur, l3))
        self.scur += len(l3) + pad + 3
        H = int(h["l2_len"]) + (20 if int(h["l3_ver"]) == 4 else 40)
        L = H + C.msg_len(kind, len(l3), l4_off)
        self.fcur += 3
        self.fcur += (dres - (self.fcur + H)) % 16
        args = dict(frame_cap=L)
        args.update(kw)
        self.rps.append(C.mk_rp(self.fcur, kind, hdr=hi, **args))
        self.fcur += L + 3
        return len(self.desc) - 1

    def arrays(self):
        arena = np.full(self.scur + 5, SRC_FILL, np.uint8)
        for o, b in self.pkts:
            arena[o:o + len(b)] = np.frombuffer(b, np.uint8)
        return np.full(self.fcur + 7, FILL, np.uint8), arena, np.array(self.desc, O.DESC_DTYPE), np.array(self.rps, C.ICMPRP_DTYPE)


def body(rng, n):
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


VARIANTS = [(0, 4, {}), (1, 4, {"ihl": 6}), (3, 6, {}), (2, 6, {"ext": 8})]
VARIANT_IDS = ["ipv4_eth", "ipv4_options_bare", "ipv6_bare", "ipv6_ext_eth"]


# ------------------------------------------------------------------------------------------
# echo
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hi,ver,kw", VARIANTS, ids=VARIANT_IDS)
def test_echo_alignment_grid(V, hi, ver, kw):
    """Every seg_len of SEG_LENS at every source residue x every destination residue of the 16-B grid:
    8 stores four bytes, the others sit on the group and dword edges; the first dword straddles the
    first group at destination residues 13..15."""
    rng = np.random.default_rng(170 + hi)
    lay = Layout(templates())
    for n in SEG_LENS:
        for sres in range(16):
            for dres in range(16):
                l3, o = C.echo_l3(ver, body(rng, n - 4), **kw)
                lay.add(hi, C.ECHO, l3, o, 1 if ver == 4 else 58, sres, dres)
    dst, arena, desc, rps = lay.arrays()
    _, w_len, _, _, w_st = check_reply(V, dst, arena, desc, lay.hdrs, rps)
    assert (w_len > 0).all() and (w_st == C.S_DONE | C.S_L4_OK | (C.S_IP_OK if ver == 4 else 0)).all()


def test_echo_verdicts_and_special_sums(V):
    """Stored sums right, wrong and, for ICMPv4, zero: out / status equal the oracle's verify, and the
    reply is written whatever the verdict.  The all-zero echo (reply field 0xffff), the echo whose
    reply words sum to 0xffff (field 0x0000), each at every destination residue -- the first dword
    out of one accumulator or two --, a request whose code is not 0, and an all-zero ICMPv6 body."""
    rng = np.random.default_rng(175)
    lay = Layout(templates())
    special = {}
    for dres in range(16):
        for n in (4, 8, 24, 60):
            special[lay.add(dres & 1, C.ECHO, *C.echo_l3(4, bytes(n), code=dres), 1, (5 * dres) % 16, dres)] = 0xffff
            special[lay.add(dres & 1, C.ECHO, *C.echo_l3(4, bytes(n), field=0), 1, (3 * dres) % 16, dres)] = 0xffff
        special[lay.add(0, C.ECHO, *C.echo_l3(4, b"\xff\xff\x00\x00" + bytes(24)), 1, dres, dres)] = 0
        special[lay.add(0, C.ECHO, *C.echo_l3(4, bytes(2) + b"\xff\xff" + bytes(7)), 1, 15 - dres, dres)] = 0
        special[lay.add(0, C.ECHO, *C.echo_l3(4, b"\xff\xff\x00\x00", field=0xffff), 1, 15 - dres, dres)] = 0
        lay.add(2 + (dres & 1), C.ECHO, *C.echo_l3(6, bytes(12)), 58, dres, dres)
    for ver, hi in ((4, 0), (6, 2)):
        proto = 1 if ver == 4 else 58
        for n in (8, 37, 64, 517):
            good, o = C.echo_l3(ver, body(rng, n - 4), code=int(rng.integers(1, 256)))
            c = int.from_bytes(good[o + 2:o + 4], "big")
            for field in (None, c ^ 0x0100, c ^ 0xffff, 0, 0xffff):
                lay.add(hi, C.ECHO, *C.echo_l3(ver, good[o + 4:], code=good[o + 1], field=field), proto, n % 16, (n + 5) % 16)
            flipped = bytearray(good)
            flipped[-1] ^= 0x40
            lay.add(hi, C.ECHO, bytes(flipped), o, proto, 3, 9)
            if ver == 4:   # a bad IPv4 header sum
                bad = bytearray(good)
                bad[10] ^= 1
                lay.add(hi, C.ECHO, bytes(bad), o, proto, 7, 2)
                lay.add(hi, C.ECHO, good, o, proto, 7, 2, flags=O.F_L4)   # no F_IP: no header verdict
    dst, arena, desc, rps = lay.arrays()
    want, w_len, w_cs, w_out, w_st = check_reply(V, dst, arena, desc, lay.hdrs, rps)
    assert (w_len > 0).all()
    for i, field in special.items():
        assert int(w_cs[i]) >> 16 == field, (i, hex(int(w_cs[i])))
    st = set(int(s) for s in w_st)
    assert {C.S_DONE, C.S_DONE | C.S_L4_OK, C.S_DONE | C.S_IP_OK, C.S_DONE | C.S_IP_OK | C.S_L4_OK} <= st
    # the reply's code is 0 whatever the request's was
    for r, d in zip(rps, desc):
        H = int(lay.hdrs[int(r["hdr"])]["l2_len"]) + (20 if int(d["l3_ver"]) == 4 else 40)
        assert want[int(r["frame_off"]) + H + 1] == 0


def test_echo_largest_segments_of_ff(V):
    """seg_len 65,515 (an IPv4 packet of 65,535 bytes) filled with 0xff, at three alignments: 2,048
    dwords of 0xffffffff per lane in the 64-bit accumulators, the first dword taken out exactly."""
    lay = Layout(templates())
    for hi, sres, dres in ((0, 0, 0), (1, 5, 14), (0, 15, 3)):
        l3, o = C.echo_l3(4, b"\xff" * 65511)
        assert len(l3) == 65535
        lay.add(hi, C.ECHO, l3, o, 1, sres, dres)
    l3, o = C.echo_l3(6, b"\xff" * 65491)
    lay.add(2, C.ECHO, l3, o, 58, 9, 13)
    dst, arena, desc, rps = lay.arrays()
    _, w_len, _, _, w_st = check_reply(V, dst, arena, desc, lay.hdrs, rps)
    assert list(w_len[:3]) == [65549, 65535, 65549] and (w_st & C.S_L4_OK).all()


def test_echo_padding_is_neither_read_nor_copied(V):
    """Frames with 0..40 bytes of L2 padding (0x5a, like the rest of the source) behind l3_len: the
    reply ends with the segment and its sum covers the segment alone."""
    rng = np.random.default_rng(177)
    lay = Layout(templates())
    for pad in range(0, 41, 5):
        for n in (8, 18, 46):
            lay.add(0, C.ECHO, *C.echo_l3(4, body(rng, n - 4)), 1, pad % 16, (n + pad) % 16, pad=pad)
            lay.add(3, C.ECHO, *C.echo_l3(6, body(rng, n - 4)), 58, (pad + 7) % 16, n % 16, pad=pad)
    dst, arena, desc, rps = lay.arrays()
    _, w_len, _, _, w_st = check_reply(V, dst, arena, desc, lay.hdrs, rps)
    assert (w_len > 0).all() and (w_st & C.S_L4_OK).all()


# ------------------------------------------------------------------------------------------
# errors
# ------------------------------------------------------------------------------------------
def test_error_quote_lengths_and_header_lengths(V):
    """Port unreachable and time exceeded with l3_len below, at and above l4_off + 64 and l3_len ==
    l4_off (time exceeded on a packet that is all header), l4_off 20 / 24 / 60 (IPv4) and 40 / 48
    (IPv6): the quote is the first min(l3_len, l4_off + 64) bytes as they lie, TTL 1 included."""
    rng = np.random.default_rng(178)
    lay = Layout(templates())
    k = 0
    for ver, his, kws in ((4, (0, 1), ({}, {"ihl": 6}, {"ihl": 15})), (6, (2, 3), ({}, {"ext": 8}))):
        for kw in kws:
            for d in (0, 1, 55, 56, 57, 200, 1472):     # the segment: 8 + d bytes; 64 at d = 56
                for kind in (C.UNREACH, C.TIMEX):
                    l3, o = C.udp_l3(ver, body(rng, d), **kw)
                    lay.add(his[k & 1], kind, l3, o, 17, (7 * k) % 16, (3 * k + 1) % 16)
                    k += 1
            for seg in (b"", b"\x01", bytes(63), bytes(64), bytes(65)):   # not UDP: time exceeded only
                l3, o = C.ip_l3(ver, 6, seg, **kw)
                lay.add(his[k & 1], C.TIMEX, l3, o, 6, (7 * k) % 16, (3 * k + 1) % 16, flags=0)
                k += 1
            lay.add(his[0], C.TIMEX, *C.echo_l3(ver, body(rng, 20), **kw), 1 if ver == 4 else 58, k % 16, 5)   # a ping that expired
    dst, arena, desc, rps = lay.arrays()
    _, w_len, w_cs, w_out, w_st = check_reply(V, dst, arena, desc, lay.hdrs, rps)
    assert (w_len > 0).all() and (w_st == C.S_DONE).all() and (w_out == 0).all()


@pytest.mark.parametrize("hi,ver,kw", VARIANTS[:1] + VARIANTS[2:3], ids=["ipv4_eth", "ipv6_bare"])
def test_error_alignment_grid(V, hi, ver, kw):
    """q = 84 (IPv4: l4_off 20 + 64) and 104 (IPv6) at every source residue x every destination residue."""
    rng = np.random.default_rng(179 + hi)
    lay = Layout(templates())
    for sres in range(16):
        for dres in range(16):
            l3, o = C.udp_l3(ver, body(rng, 100), **kw)
            lay.add(hi, C.UNREACH if (sres + dres) & 1 else C.TIMEX, l3, o, 17, sres, dres)
    dst, arena, desc, rps = lay.arrays()
    _, w_len, _, _, _ = check_reply(V, dst, arena, desc, lay.hdrs, rps)
    assert (w_len == (14 + 20 + 8 + 84 if ver == 4 else 40 + 8 + 104)).all()


# ------------------------------------------------------------------------------------------
# batches
# ------------------------------------------------------------------------------------------
def mixed_batch(n, seed):
    rng = np.random.default_rng(seed)
    lay = Layout(templates())
    for i in range(n):
        ver = 6 if i % 3 == 2 else 4
        hi = (i & 1) + (2 if ver == 6 else 0)
        kind = (C.ECHO, C.UNREACH, C.TIMEX)[(i // 2) % 3]
        d = int(rng.choice([4, 5, 30, 100, 517, 1468]))
        l3, o = C.echo_l3(ver, body(rng, d)) if kind == C.ECHO else C.udp_l3(ver, body(rng, d))
        lay.add(hi, kind, l3, o, (1 if ver == 4 else 58) if kind == C.ECHO else 17, int(rng.integers(0, 16)), int(rng.integers(0, 16)))
    return lay


@pytest.mark.parametrize("n", [0, 1, 31, 33])
def test_batch_sizes_and_optional_outputs(V, n):
    """n records of a 33-record batch (one block is 32 teams), with all outputs and with each optional
    output NULL in turn: nothing past record n is touched, a NULL output changes nothing else."""
    lay = mixed_batch(33, 180)
    dst, arena, desc, rps = lay.arrays()
    check_reply(V, dst, arena, desc, lay.hdrs, rps, n=n)
    for off in ("want_csum", "want_out", "want_status"):
        check_reply(V, dst, arena, desc, lay.hdrs, rps, n=n, **{off: False})


def test_refusals_among_good_records(V):
    """Every refusal, each between two good records whose frames come out intact: frame_len 0, csum 0,
    out 0, S_BAD_DESC and not one byte written for the refused one."""
    rng = np.random.default_rng(181)
    hdrs = np.concatenate([templates(), np.array([C.mk_hdr(5), C.mk_hdr(4, 13), C.mk_hdr(4, rsv=1), C.mk_hdr(4, ack=1),
                                                   C.mk_hdr(6, window=0x100), C.mk_hdr(4, sport=1)], C.HDR_DTYPE)])
    lay = Layout(hdrs)
    bad = []

    def good():
        lay.add(0, C.ECHO, *C.echo_l3(4, body(rng, 33)), 1, len(lay.desc) % 16, (5 * len(lay.desc)) % 16)

    def refused(*a, **kw):
        mut = kw.pop("mut", None)
        good()
        i = lay.add(*a, **kw)
        if mut:
            mut(lay.desc[i], lay.rps[i])
        bad.append(i)
    e4, e6, u4, u6 = C.echo_l3(4, body(rng, 40)), C.echo_l3(6, body(rng, 40)), C.udp_l3(4, body(rng, 40)), C.udp_l3(6, body(rng, 40))

    def setf(field, val, rec=False):
        def f(d, r):
            (r if rec else d)[field] = val
        return f
    refused(0, C.ECHO, *e4, 1, mut=setf("hdr", len(hdrs), True))                  # hdr >= n_hdr
    refused(0, C.ECHO, *e4, 1, mut=setf("hdr", 0xffffffff, True))
    for h in range(4, 10):                                                        # the template
        refused(0, C.ECHO, *e4, 1, mut=setf("hdr", h, True))
    refused(0, C.ECHO, *e4, 1, mut=setf("hdr", 2, True))                          # its version is not the descriptor's
    refused(2, C.ECHO, *e6, 58, mut=setf("hdr", 1, True))
    for kind in (0, 4, 0x81):
        refused(0, C.ECHO, *e4, 1, mut=setf("kind", kind, True))
    for k in range(7):
        refused(0, C.ECHO, *e4, 1, rsv=1 << (8 * k + 7))
    for fl in (O.F_L4P, O.F_RAW, O.F_PRE):
        refused(0, C.ECHO, *e4, 1, flags=O.F_L4 | O.F_IP | fl)
        refused(0, C.UNREACH, *u4, 17, flags=O.F_L4 | fl)
        refused(3, C.TIMEX, *u6, 17, flags=fl)
    refused(2, C.ECHO, *e6, 58, flags=O.F_L4 | O.F_IP)                            # F_IP on IPv6
    refused(0, C.TIMEX, *u4, 17, mut=setf("l3_ver", 5))
    refused(0, C.TIMEX, *u4, 17, mut=setf("l4_off", 16))                          # an l4_off the checksum kernel refuses
    refused(0, C.TIMEX, *u4, 17, mut=setf("l4_off", 22))
    refused(3, C.TIMEX, *u6, 17, mut=setf("l4_off", 36))
    refused(0, C.TIMEX, *u4, 17, mut=setf("l4_off", len(u4[0]) + 4))              # l4_off > l3_len
    refused(0, C.TIMEX, *u4, 17, mut=setf("l3_off", 1 << 40))                     # outside the arena
    refused(0, C.TIMEX, *u4, 17, mut=setf("l3_off", (1 << 64) - 8))               # would wrap
    refused(0, C.ECHO, *e4, 1, frame_cap=14 + 20 + 44 - 1)                        # L > frame_cap
    refused(1, C.UNREACH, *u4, 17, frame_cap=20 + 8 + 68 - 1)
    refused(0, C.ECHO, *e4, 1, mut=setf("frame_off", (1 << 64) - 16, True))       # frame_off + L wraps
    refused(0, C.ECHO, *e4, 1, mut=setf("frame_off", 1 << 33, True))              # past the destination
    refused(0, C.ECHO, *e4, 1, flags=O.F_IP)                                      # echo: no F_L4
    refused(0, C.ECHO, *e4, 58)                                                   # ICMPv6 in IPv4
    refused(2, C.ECHO, *e6, 1)                                                    # ICMPv4 in IPv6
    refused(0, C.ECHO, *u4, 17)                                                   # not ICMP
    refused(0, C.ECHO, *C.ip_l3(4, 1, b"\x08\x00\xf7\xff\x00\x00\x00"), 1)        # seg_len 7
    refused(0, C.ECHO, *C.echo_l3(4, body(rng, 20), typ=0), 1)                    # a reply, not a request
    refused(0, C.ECHO, *C.echo_l3(4, body(rng, 20), typ=128), 1)
    refused(2, C.ECHO, *C.echo_l3(6, body(rng, 20), typ=8), 58)
    refused(2, C.ECHO, *C.echo_l3(6, body(rng, 20), typ=135), 58)                 # NS goes to NDP
    refused(0, C.UNREACH, *e4, 1)                                                 # port unreachable: UDP only
    refused(0, C.UNREACH, *C.ip_l3(4, 6, bytes(20)), 6)
    refused(3, C.TIMEX, *C.echo_l3(6, body(rng, 20), typ=135), 58)                # time exceeded on NS / NA
    refused(3, C.TIMEX, *C.echo_l3(6, body(rng, 20), typ=136), 58, flags=0)
    refused(3, C.TIMEX, *C.ip_l3(6, 58, b"\x87"), 58, flags=0)                    # one byte is enough
    good()
    at = len(lay.desc)
    lay.add(3, C.TIMEX, *C.ip_l3(6, 58, b""), 58, flags=0)                        # an empty ICMPv6 segment: answered, nothing read
    lay.add(3, C.TIMEX, *C.ip_l3(6, 17, b"\x87" + bytes(7)), 17, flags=0)         # 135 in a UDP port: answered
    lay.add(0, C.TIMEX, *C.echo_l3(4, body(rng, 20), typ=135), 1)                 # ICMPv4 has no NDP
    lay.add(0, C.UNREACH, *u4, 17, frame_cap=14 + 20 + 8 + 68)                    # exactly the room
    good()
    dst, arena, desc, rps = lay.arrays()
    want, w_len, w_cs, w_out, w_st = check_reply(V, dst, arena, desc, hdrs, rps)
    refused_idx = [i for i in range(len(desc)) if w_st[i] == C.S_BAD_DESC]
    assert refused_idx == bad, (refused_idx, bad)
    assert (w_len[bad] == 0).all() and (w_cs[bad] == 0).all() and (w_out[bad] == 0).all()
    assert (w_len[at:] > 0).all()
    for i in bad:   # the restatement left the refused frames' room untouched, so the device did too
        fo = int(rps[i]["frame_off"])
        if fo < len(want):
            assert (want[fo:fo + 40] == FILL).all()


# ------------------------------------------------------------------------------------------
# round trip, the reference's requests
# ------------------------------------------------------------------------------------------
def test_round_trip(V):
    """The written replies (Ethernet templates) go through vpcsum_parse_ether_async and
    vpcsum_compute_async with MODE_VERIFY: S_IP_OK | S_L4_OK on IPv4, S_L4_OK on IPv6, protocol 1 / 58."""
    import torch
    rng = np.random.default_rng(182)
    lay = Layout(templates())
    for i in range(66):
        ver = 6 if i & 1 else 4
        kind = (C.ECHO, C.UNREACH, C.TIMEX)[i % 3]
        d = int(rng.choice([4, 5, 61, 64, 517, 1360, 1468]))
        l3, o = C.echo_l3(ver, body(rng, d)) if kind == C.ECHO else C.udp_l3(ver, body(rng, d))
        lay.add(0 if ver == 4 else 2, kind, l3, o, (1 if ver == 4 else 58) if kind == C.ECHO else 17, int(rng.integers(0, 16)),
                int(rng.integers(0, 16)))
    dst, arena, desc, rps = lay.arrays()
    n = len(desc)
    d_frames = dev(dst)
    flen = torch.zeros(n, dtype=torch.int32, device="cuda")
    V.icmp_reply(dev(arena), dev(desc), dev(lay.hdrs), len(lay.hdrs), dev(rps), n, d_frames, flen)
    d_desc = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    V.parse_ether(d_frames, dev(rps["frame_off"].copy()), flen, n, d_desc)
    st = torch.zeros(n, dtype=torch.uint8, device="cuda")
    V.compute(d_frames, d_desc, n, None, st, V.MODE_VERIFY)
    torch.cuda.synchronize()
    got = host(d_desc).view(O.DESC_DTYPE)
    st = host(st)
    assert (host(flen) > 0).all()
    assert (got["l4_proto"][0::2] == 1).all() and (got["l4_proto"][1::2] == 58).all() and (got["l3_off"] == rps["frame_off"] + 14).all()
    assert (st[0::2] == C.S_DONE | C.S_L4_OK | C.S_IP_OK).all() and (st[1::2] == C.S_DONE | C.S_L4_OK).all(), [hex(x) for x in st]


def test_the_reference_echo_requests_are_answered(V):
    """TestPacket's ipv4ByIcmpExample / ipv6ByIcmpExample: verified with their pinned sums and
    answered, the replies byte-equal to the restatement's."""
    import json
    import os
    ks = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kat.json")))["kats"]
    reqs = {k["ver"]: k for k in ks if k["name"] in ("ipv4ByIcmpExample", "ipv6ByIcmpExample")}
    l4, l6 = bytes.fromhex(reqs[4]["hex"]), bytes.fromhex(reqs[6]["hex"])
    hdrs = np.array([C.mk_hdr(4, 14, l4[16:20], l4[12:16]), C.mk_hdr(6, 14, l6[24:40], l6[8:24])], C.HDR_DTYPE)
    lay = Layout(hdrs)
    lay.add(0, C.ECHO, l4, 20, 1, 2, 0)
    lay.add(1, C.ECHO, l6, 40, 58, 6, 6)
    dst, arena, desc, rps = lay.arrays()
    _, w_len, _, w_out, w_st = check_reply(V, dst, arena, desc, hdrs, rps)
    assert list(w_len) == [14 + len(l4), 14 + len(l6)] and list(w_st) == [C.S_DONE | C.S_IP_OK | C.S_L4_OK, C.S_DONE | C.S_L4_OK]
    assert int(w_out[0]) == reqs[4]["pinned"]["ip"] | (reqs[4]["pinned"]["l4"] << 16) and int(w_out[1]) >> 16 == reqs[6]["pinned"]["l4"]


# ------------------------------------------------------------------------------------------
# host form, PNI
# ------------------------------------------------------------------------------------------
STRIDE, HEADROOM = 2048, 384
_KEEP = []


def page_aligned(nbytes):
    raw = np.zeros(nbytes + 8192, np.uint8)
    _KEEP.append(raw)   # page-locked and released by the tests: kept for the life of the process
    skip = (-raw.ctypes.data) % 4096
    return raw[skip:skip + nbytes]


@pytest.fixture(scope="module")
def umembatch():
    """48 received Ethernet frames in the RX chunks of a umem (2,048 bytes, frame at +384), answered
    into its TX chunks -- the 48 chunks behind them: echoes (one with a bad sum), port unreachables,
    time exceededs, IPv4 and IPv6, three refused records."""
    rng = np.random.default_rng(183)
    n = 48
    hdrs = templates()[[0, 2]]
    arena = np.full(2 * n * STRIDE, SRC_FILL, np.uint8)
    desc, rps = np.zeros(n, O.DESC_DTYPE), np.zeros(n, C.ICMPRP_DTYPE)
    for i in range(n):
        ver = 6 if i % 4 == 3 else 4
        kind = (C.ECHO, C.UNREACH, C.TIMEX)[i % 3]
        d = int(rng.choice([4, 5, 100, 517, 1360, 1468]))
        l3, o = C.echo_l3(ver, body(rng, d)) if kind == C.ECHO else C.udp_l3(ver, body(rng, d))
        at = i * STRIDE + HEADROOM
        eth = b"\x02\0\0\0\x0a\x01\x02\0\0\0\x0b\x02" + (b"\x08\x00" if ver == 4 else b"\x86\xdd")
        arena[at:at + 14 + len(l3)] = np.frombuffer(eth + l3, np.uint8)
        desc[i] = C.mk_desc(at + 14, len(l3), o, ver, (1 if ver == 4 else 58) if kind == C.ECHO else 17)
        rps[i] = C.mk_rp((n + i) * STRIDE + HEADROOM, kind, hdr=0 if ver == 4 else 1, frame_cap=STRIDE - HEADROOM)
    arena[int(desc[6]["l3_off"]) + int(desc[6]["l3_len"]) - 1] ^= 0x20   # an echo (i % 3 == 0) with a bad sum
    rps[10]["rsv"][3] = 1
    rps[20]["hdr"] = 2
    desc[30]["l4_proto"] = 6                                             # an echo record on TCP
    want = C.reply(arena, arena, desc, hdrs, rps)
    assert [i for i in range(n) if want[4][i] == C.S_BAD_DESC] == [10, 20, 30] and not want[4][6] & C.S_L4_OK
    return dict(arena=arena, desc=desc, rps=rps, hdrs=hdrs, want=want, n=n)


def test_host_form(V, umembatch):
    """Context.reply_icmp_frames with RX and TX chunks in one registered umem (read and written in
    place), with the requests in a heap copy (staged) answered into the umem, and with the optional
    outputs left out; the device form on one allocation gives the same; an unregistered destination
    is refused."""
    import torch
    ub = umembatch
    desc, rps, hdrs, n = ub["desc"], ub["rps"], ub["hdrs"], ub["n"]
    want, w_len, w_cs, w_out, w_st = ub["want"]
    # the device form, source and destination one allocation
    d_umem = dev(ub["arena"])
    flen = torch.zeros(n, dtype=torch.int32, device="cuda")
    st = torch.zeros(n, dtype=torch.uint8, device="cuda")
    V.icmp_reply(d_umem, dev(desc), dev(hdrs), len(hdrs), dev(rps), n, d_umem, flen, None, None, st)
    torch.cuda.synchronize()
    got = host(d_umem)
    assert np.array_equal(got, want), first_diff(got, want)
    assert np.array_equal(host(flen).view(np.uint32), w_len) and np.array_equal(host(st), w_st)

    umem = page_aligned(len(ub["arena"]))
    heap = ub["arena"].copy()
    ctx = V.Context(0, max_arena=256 << 10, max_pkts=n)
    ctx.register(umem)
    try:
        for nm, a in (("in_place", umem), ("staged", heap)):
            umem[:] = ub["arena"]
            d0, r0 = desc.copy(), rps.copy()
            flen, cs, out, st = ctx.reply_icmp_frames(a, desc, hdrs, rps, umem)
            assert desc.tobytes() == d0.tobytes() and rps.tobytes() == r0.tobytes(), nm
            assert np.array_equal(flen, w_len) and np.array_equal(cs, w_cs) and np.array_equal(out, w_out) and np.array_equal(st, w_st), nm
            assert np.array_equal(umem, want), (nm, first_diff(umem, want))
            assert np.array_equal(heap, ub["arena"]), nm
        umem[:] = ub["arena"]
        flen, cs, out, st = ctx.reply_icmp_frames(umem, desc, hdrs, rps, umem, want_csum=False, want_out=False, want_status=False)
        assert cs is None and out is None and st is None and np.array_equal(flen, w_len) and np.array_equal(umem, want)
        flen, _, _, _ = ctx.reply_icmp_frames(heap, desc[:0], hdrs, rps[:0], umem)
        assert len(flen) == 0
        umem[:] = ub["arena"]
        with pytest.raises(V.VpcsumError, match="vpcsum_ctx_reply_icmp_frames: the destination must be registered"):
            ctx.reply_icmp_frames(umem, desc[:1], hdrs, rps[:1], np.zeros(len(umem), np.uint8))
        assert np.array_equal(umem, ub["arena"])
    finally:
        ctx.unregister(umem)
        ctx.close()


def test_pni_reply_icmp_frames(V, umembatch):
    """Java_io_vproxy_vpcsum_VPCsum_replyIcmpFrames driven through ctypes with PNI environments, as the
    JVM's downcall drives it: create, registerArena, the call on one umem, waitFor, close -- a
    byte-equal umem, lengths, sums, out words and status."""
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

    ub = umembatch
    n = ub["n"]
    umem = page_aligned(len(ub["arena"]))
    umem[:] = ub["arena"]
    a, cs, out, st = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    hdrs, desc, rps = np.ascontiguousarray(ub["hdrs"]), np.ascontiguousarray(ub["desc"]), np.ascontiguousarray(ub["rps"])
    ctx = call(L.Java_io_vproxy_vpcsum_VPCsum_create, I32(0), I64(256 << 10), I32(n))
    try:
        call(L.Java_io_vproxy_vpcsum_VPCsum_registerArena, I64(ctx), P(umem.ctypes.data), I64(umem.nbytes))
        t = call(L.Java_io_vproxy_vpcsum_VPCsum_replyIcmpFrames, I64(ctx), P(umem.ctypes.data), I64(umem.nbytes), P(desc.ctypes.data),
                 P(hdrs.ctypes.data), I32(len(hdrs)), P(rps.ctypes.data), I32(n), P(umem.ctypes.data), I64(umem.nbytes),
                 P(a.ctypes.data), P(cs.ctypes.data), P(out.ctypes.data), P(st.ctypes.data))
        call(L.Java_io_vproxy_vpcsum_VPCsum_waitFor, I64(ctx), I64(t))
        want, w_len, w_cs, w_out, w_st = ub["want"]
        assert np.array_equal(a, w_len) and np.array_equal(cs, w_cs) and np.array_equal(out, w_out) and np.array_equal(st, w_st)
        assert np.array_equal(umem, want), first_diff(umem, want)
    finally:
        call(L.Java_io_vproxy_vpcsum_VPCsum_close, I64(ctx))
