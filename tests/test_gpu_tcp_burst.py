"""The TCP send bursts on the GPU (vpcsum_tcp_build_bursts_async, vpcsum_ctx_build_tcp_bursts,
VPCsum.buildTcpBursts).  A burst is by definition the list of per-segment records fetch() +
sendTcpPsh produce, so in every case the expected arena is tests/tcpbuildvec.py's build -- the
oracle's -- on tests/tcpburstvec.py's expand(...), compared over the WHOLE destination arena (prefilled
with 0xEE, guard bytes between the chunks included) along with frame_len, out and status.  The
unsorted-table case is not run here: tests/cpp/tcp_burst_test.cpp carries it on the host."""
import ctypes

import numpy as np
import pytest

import tcpbuildvec as B
import tcpburstvec as U
from test_gpu_tcp_build import FILL, dev, first_diff, host, mk_v4, mk_v6, page_aligned

pytestmark = pytest.mark.gpu

CAP = 2048   # the room at every frame: a umem chunk's


@pytest.fixture(scope="module")
def V():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vproxy_amd import vpcsum
    vpcsum.lib()
    assert vpcsum.TCPBURST_DTYPE == U.TCPBURST_DTYPE
    return vpcsum


def gpu_bursts(V, dst, src, hdrs, bursts, frame_off, frame_cap=CAP, want_out=True, want_status=True):
    """(arena_after, frame_len, out, status) of vpcsum_tcp_build_bursts_async on device copies; the
    result arrays start as 0xAB and carry two guard rows, which must stay; the source arena must come
    back as it went."""
    import torch
    n = len(frame_off)
    bursts = np.array(bursts, U.TCPBURST_DTYPE)
    d_dst, d_src = dev(dst), dev(src if len(src) else np.zeros(16, np.uint8))[:len(src)]
    d_h = dev(hdrs) if len(hdrs) else torch.zeros(64, dtype=torch.uint8, device="cuda")
    d_b = dev(bursts) if len(bursts) else torch.zeros(32, dtype=torch.uint8, device="cuda")
    d_fo = dev(np.ascontiguousarray(frame_off, np.uint64)) if n else torch.zeros(8, dtype=torch.uint8, device="cuda")
    flen = torch.full(((n + 2) * 4,), 0xAB, dtype=torch.uint8, device="cuda")
    out = torch.full(((n + 2) * 4,), 0xAB, dtype=torch.uint8, device="cuda")
    st = torch.full((n + 2,), 0xAB, dtype=torch.uint8, device="cuda")
    V.tcp_build_bursts(d_dst, d_src, d_h, len(hdrs), d_b, len(bursts), d_fo, n, frame_cap, flen, out if want_out else None,
                       st if want_status else None)
    torch.cuda.synchronize()
    flen, out, st = host(flen).view(np.uint32), host(out).view(np.uint32), host(st)
    assert (flen[n:] == 0xABABABAB).all() and (out[n:] == 0xABABABAB).all() and (st[n:] == 0xAB).all()
    if not want_out:
        assert (out == 0xABABABAB).all()
    if not want_status:
        assert (st == 0xAB).all()
    assert np.array_equal(host(d_src), src)
    return host(d_dst), flen[:n], out[:n], st[:n]


def expected(dst, src, hdrs, bursts, frame_off, frame_cap=CAP):
    segs, _ = U.expand(bursts, frame_off, frame_cap, hdrs, len(src))
    return B.build(dst, src, hdrs, segs) + (segs,)


def compare(got, want, segs, want_out=True, want_status=True):
    arena, flen, out, st = got
    w_arena, w_len, w_out, w_st = want
    assert np.array_equal(flen, w_len), [(i, int(flen[i]), int(w_len[i])) for i in np.flatnonzero(flen != w_len)[:8]]
    if want_status:
        assert np.array_equal(st, w_st), [(i, hex(st[i]), hex(w_st[i])) for i in np.flatnonzero(st != w_st)[:8]]
    if want_out:
        assert np.array_equal(out, w_out), [(i, hex(out[i]), hex(w_out[i])) for i in np.flatnonzero(out != w_out)[:8]]
    assert np.array_equal(arena, w_arena), first_diff(arena, w_arena, segs)


def check(V, dst, src, hdrs, bursts, frame_off, frame_cap=CAP, **kw):
    want = expected(dst, src, hdrs, bursts, frame_off, frame_cap)
    compare(gpu_bursts(V, dst, src, hdrs, bursts, frame_off, frame_cap, **kw), want[:4], want[4], **kw)
    return want


class Table:
    """Bursts laid out one after another: each burst's payload run at a wanted source residue mod 16
    with 3 guard bytes around it, each frame at its own destination residue with 3 guard bytes."""

    def __init__(self, rng, hlen_of):
        self.rng, self.hlen_of = rng, hlen_of
        self.bursts, self.frame_off, self.dcur, self.scur = [], [], 0, 0

    def frame(self, room, dres=None):
        """One more entry of the frame table with `room` bytes before the next."""
        dres = len(self.frame_off) * 7 % 16 if dres is None else dres
        self.dcur += 3
        self.dcur += (dres - self.dcur) % 16
        self.frame_off.append(self.dcur)
        self.dcur += room + 3

    def add(self, hidx, data_len, mss, sres=None, **kw):
        sres = len(self.bursts) * 5 % 16 if sres is None else sres
        self.scur += 3
        self.scur += (sres - self.scur) % 16
        b = U.mk_burst(self.scur, data_len, mss, len(self.frame_off), hdr=hidx, **kw)
        self.bursts.append(b)
        self.scur += data_len + 3
        cnt = U.count_of(data_len, mss) if mss or not data_len else 1
        H = self.hlen_of(hidx)
        for k in range(cnt):
            self.frame(H + (min(mss, data_len - k * mss) if data_len else 0))
        return len(self.bursts) - 1

    def arenas(self):
        dst = np.full(self.dcur, FILL, np.uint8)
        src = self.rng.integers(0, 256, self.scur, dtype=np.uint8)
        return dst, src, np.array(self.frame_off, np.uint64)


def hlen_of(hdrs):
    return lambda i: B.header_len(hdrs[i]) if i < len(hdrs) else 54


# ------------------------------------------------------------------------------------------
# 1. the cut at its edges
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ver,l2", [(4, 14), (6, 0)], ids=["ipv4_eth", "ipv6_ip"])
def test_cut_edges(V, ver, l2):
    """mss in {1, 7, 536, 1460} x data_len in {1, mss - 1, mss, mss + 1, 2 mss, 2 mss + 1, 45 mss,
    45 mss + 1}, one burst each (mss 1 makes mss - 1 a burst without payload), random sequence
    numbers: source and frame addresses at every residue mod 16 somewhere in the batch."""
    rng = np.random.default_rng(61 + ver)
    hdrs = np.array([mk_v4(ident=0x1c46, frag=0x4000) if ver == 4 else mk_v6(l2, tos=0xb8)], B.TCPHDR_DTYPE)
    t = Table(rng, hlen_of(hdrs))
    for mss in (1, 7, 536, 1460):
        for d in (1, mss - 1, mss, mss + 1, 2 * mss, 2 * mss + 1, 45 * mss, 45 * mss + 1):
            t.add(0, d, mss, seq=int(rng.integers(0, 1 << 32)))
    dst, src, fo = t.arenas()
    want = check(V, dst, src, hdrs, t.bursts, fo)
    segs = want[4]
    assert len(t.bursts) == 32 and len(fo) == 4 * (1 + 1 + 1 + 2 + 2 + 3 + 45 + 46) and (want[3] == B.S_DONE).all()
    assert {int(o) % 16 for o in fo} == set(range(16))
    assert {int(s["data_off"]) % 16 for s in segs if s["data_len"]} == set(range(16))
    H = B.header_len(hdrs[0])
    assert sorted(set(want[1].tolist())) == sorted({H + x for x in (0, 1, 6, 7, 535, 536, 1459, 1460)})


def test_seq_wraps_inside_a_burst(V):
    """seq = 2^32 - 1000, mss 536: the second frame's sequence number has wrapped, IPv4 and IPv6."""
    rng = np.random.default_rng(63)
    hdrs = np.array([mk_v4(), mk_v6(14)], B.TCPHDR_DTYPE)
    t = Table(rng, hlen_of(hdrs))
    for hi in (0, 1):
        t.add(hi, 5 * 536 + 1, 536, seq=(1 << 32) - 1000)
    dst, src, fo = t.arenas()
    want = check(V, dst, src, hdrs, t.bursts, fo)
    assert [int(s["seq"]) for s in want[4][:6]] == [(1 << 32) - 1000, (1 << 32) - 464, 72, 608, 1144, 1680]
    assert (want[3] == B.S_DONE).all() and len(fo) == 12


# ------------------------------------------------------------------------------------------
# 2. the search at its edges
# ------------------------------------------------------------------------------------------
def search_table(rng, hdrs, n_bursts):
    """n_bursts bursts: counts of 1 next to counts of 40 (mss 8), bursts without payload among them,
    a frame table whose length is no multiple of 8."""
    t = Table(rng, hlen_of(hdrs))
    for i in range(n_bursts):
        hi = i % len(hdrs)
        if i % 16 == 1 or n_bursts <= 2 and i == 0:
            t.add(hi, 40 * 8 - int(rng.integers(0, 8)), 8, seq=int(rng.integers(0, 1 << 32)))      # 40 frames
        elif i % 5 == 3:
            t.add(hi, 0, int(rng.choice([0, 1460])), flags=int(rng.choice([B.ACK, B.FIN | B.ACK, B.RST])))
        else:
            t.add(hi, int(rng.integers(1, 9)), 8, seq=int(rng.integers(0, 1 << 32)))                 # 1 frame
    return t


@pytest.mark.parametrize("n_bursts", [1, 2, 7, 8, 9, 63, 64, 65, 513])
def test_search_edges(V, n_bursts):
    """Tables of 1..513 bursts (the 9-ary search's interval sizes around 8, 64 and 512), counts of 1
    next to counts of 40, zero-payload bursts among data bursts.  Then the first and the last burst
    of the table each alone over the same frame table: the frames the lone burst does not cover --
    those before the last burst, those after the first -- are refused and untouched."""
    rng = np.random.default_rng(70 + n_bursts)
    hdrs = np.array([mk_v4(), mk_v6(14), mk_v6()], B.TCPHDR_DTYPE)
    t = search_table(rng, hdrs, n_bursts)
    if len(t.frame_off) % 8 == 0:
        t.add(0, 0, 0, flags=B.ACK)
    dst, src, fo = t.arenas()
    assert len(fo) % 8 and len(fo) % 32
    want = check(V, dst, src, hdrs, t.bursts, fo)
    assert (want[3] == B.S_DONE).all()
    counts = [int(b["count"]) for b in t.bursts]
    assert 40 in counts and (n_bursts < 7 or (1 in counts and any(int(b["data_len"]) == 0 for b in t.bursts)))
    for lone in ({0, len(t.bursts) - 1} if len(t.bursts) > 1 else ()):
        b = t.bursts[lone]
        w = check(V, dst, src, hdrs, [b], fo)
        covered = np.zeros(len(fo), bool)
        covered[int(b["first"]):int(b["first"]) + int(b["count"])] = True
        assert np.array_equal(w[3] == B.S_DONE, covered) and np.array_equal(w[1] > 0, covered)


def test_bursts_across_wave_and_workgroup_edges(V):
    """A burst whose frames are 31..33 (two workgroups of 32 teams) and one that is 255..257, between
    bursts of 31 and 221 frames; 261 frames in all."""
    rng = np.random.default_rng(81)
    hdrs = np.array([mk_v4()], B.TCPHDR_DTYPE)
    t = Table(rng, hlen_of(hdrs))
    for cnt in (31, 3, 221, 3, 3):
        t.add(0, cnt * 8 - 3, 8, seq=int(rng.integers(0, 1 << 32)))
    dst, src, fo = t.arenas()
    assert [int(b["first"]) for b in t.bursts] == [0, 31, 34, 255, 258] and len(fo) == 261
    want = check(V, dst, src, hdrs, t.bursts, fo)
    assert (want[3] == B.S_DONE).all()


# ------------------------------------------------------------------------------------------
# 3. refusals among good bursts
# ------------------------------------------------------------------------------------------
def refusal_table(rng, hdrs, big: bool):
    """(table, expected acceptance per burst).  big: the call's frame_cap is 2^17 and the length
    field's edge is in; else frame_cap is 154 and its own edge is in."""
    n_hdr = len(hdrs)
    t = Table(rng, hlen_of(hdrs))
    expect = []

    def add(ok, hi, d, mss, **kw):
        t.add(hi, d, mss, seq=int(rng.integers(0, 1 << 32)), **kw)
        expect.append(ok)

    add(True, 0, 100, 40)
    add(True, n_hdr - 1, 100, 40)                  # hdr = n_hdr - 1
    add(False, n_hdr, 100, 40)                     # hdr = n_hdr
    add(False, 0xffffffff, 100, 40)
    add(True, 1, 33, 40)
    add(False, 2, 33, 40); add(False, 3, 33, 40); add(False, 4, 33, 40)   # version, l2_len, template rsv
    add(True, 0, 0, 0, flags=0x3f)
    add(False, 0, 0, 0, flags=0x40); add(False, 0, 7, 40, flags=0x80); add(False, 0, 7, 40, rsv=1)
    add(True, 0, 0, 0, flags=B.ACK)                # no payload: mss is not read
    add(False, 0, 7, 0, count=1)                   # payload and mss 0
    add(True, 0, 81, 40)                           # count 3
    add(False, 0, 81, 40, count=2); add(False, 0, 81, 40, count=4); add(False, 0, 0, 40, count=0); add(False, 0, 0, 40, count=2)
    if big:
        add(True, 0, 65495 + 5, 65495); add(False, 0, 65496 + 5, 65496)     # IPv4: 40 + mss <= 65535
        add(True, 1, 65515 + 5, 65515); add(False, 1, 65516 + 5, 65516)     # IPv6: 20 + mss
        add(True, 0, 65495, 65535); add(False, 0, 65496, 65535)             # min(mss, data_len)
    else:
        add(True, 0, 250, 100); add(False, 0, 250, 101)                     # 54 + mss <= 154
        add(True, 1, 250, 94); add(False, 1, 250, 95)                       # 60 + mss
        add(True, 0, 100, 1460); add(False, 0, 101, 1460)                   # min(mss, data_len)
    add(True, 0, 17, 40)
    return t, expect


@pytest.mark.parametrize("big", [True, False], ids=["cap_2e17", "cap_154"])
def test_refusals_among_good_bursts(V, big):
    """Each whole-burst rule accepted on one side of its edge and refused on the other, good bursts
    between them: every frame of a refused burst reports frame_len 0, out 0, S_BAD_DESC and the arena
    where it would lie is untouched; the source range's edges and the table's end follow; the good
    bursts' frames are byte-identical to a run without the bad ones."""
    rng = np.random.default_rng(90 + big)
    hdrs = np.array([mk_v4(), mk_v6(), B.mk_hdr(5, 14), B.mk_hdr(4, 18), B.mk_hdr(4, 14, rsv=1), mk_v6(14)], B.TCPHDR_DTYPE)
    cap = 1 << 17 if big else 154
    t, expect = refusal_table(rng, hdrs, big)
    dst, src, fo = t.arenas()
    # the source's edges: the last burst's payload ends exactly at src_len, then one past it, one that
    # would wrap, and bursts without payload at and past src_len
    src = src[:-3].copy()
    assert int(t.bursts[-1]["data_off"]) + 17 == len(src)
    nf = len(fo)
    extra = [U.mk_burst(len(src) - 16, 17, 40, nf), U.mk_burst((1 << 64) - 8, 17, 40, nf + 1), U.mk_burst(len(src), 0, 0, nf + 2, flags=B.ACK),
             U.mk_burst(len(src) + 1, 0, 0, nf + 3, flags=B.ACK)]
    expect += [False, False, True, False]
    bursts = t.bursts + extra
    for _ in range(4 + 3):          # their frames, and three frames past the last burst's coverage
        t.frame(80)
    dst, _, fo = t.arenas()
    want = check(V, dst, src, hdrs, bursts, fo, cap)
    _, w_len, w_out, w_st, segs = want
    firsts = [int(b["first"]) for b in bursts] + [len(fo) - 3]
    for i, (b, e) in enumerate(zip(bursts, expect)):
        sl = slice(firsts[i], firsts[i + 1])   # the frames laid out for it: also those a wrong count leaves uncovered
        assert ((w_st[sl] == B.S_DONE) == e).all() and ((w_len[sl] > 0) == e).all(), (b, e)
        if not e:
            assert (w_out[sl] == 0).all() and (w_st[sl] == B.S_BAD_DESC).all()
            for o in fo[sl]:
                assert (want[0][int(o):int(o) + 54] == FILL).all()
    assert (w_st[-3:] == B.S_BAD_DESC).all() and (w_len[-3:] == 0).all()
    # without the bad ones: the good bursts renumbered over their own frames only
    good, gfo = [], []
    for b, e in zip(bursts, expect):
        if e:
            g = b.copy()
            g["first"] = len(gfo)
            good.append(g)
            gfo += [int(o) for o in fo[int(b["first"]):int(b["first"]) + int(b["count"])]]
    got2 = gpu_bursts(V, dst, src, hdrs, good, np.array(gfo, np.uint64), cap)
    assert np.array_equal(got2[0], want[0]) and (got2[3] == B.S_DONE).all()
    keep = w_st == B.S_DONE
    assert np.array_equal(got2[1], w_len[keep]) and np.array_equal(got2[2], w_out[keep])


def test_single_frame_refusals_and_no_bursts(V):
    """Only its own destination refuses a single frame: the burst's last frame ends exactly at
    dst_len and is built; a frame_off one byte further, one past dst_len and one that would wrap are
    refused while their siblings are built.  n_bursts == 0 refuses every frame and writes nothing."""
    rng = np.random.default_rng(92)
    hdrs = np.array([mk_v4()], B.TCPHDR_DTYPE)
    t = Table(rng, hlen_of(hdrs))
    t.add(0, 6 * 100, 100)
    t.add(0, 50, 100)
    dst, src, fo = t.arenas()
    dst = dst[:int(fo[-1]) + 54 + 50].copy()                      # the last frame ends at dst_len
    fo = fo.copy()
    fo[1], fo[3], fo[4] = len(dst) - 153, len(dst) + 1, (1 << 64) - 20
    want = check(V, dst, src, hdrs, t.bursts, fo)
    assert (want[1] > 0).tolist() == [True, False, True, False, False, True, True]
    assert want[3].tolist() == [B.S_DONE if x else B.S_BAD_DESC for x in want[1]]
    want = check(V, dst, src, hdrs, [], fo)
    assert (want[3] == B.S_BAD_DESC).all() and (want[0] == FILL).all() and not want[1].any() and not want[2].any()


# ------------------------------------------------------------------------------------------
# 4. batch sizes, optional outputs
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 9, 33, 257])
def test_batch_sizes_and_optional_outputs(V, n):
    """n frames in bursts of 1..6 over 3 templates, with d_out / d_status each NULL and non-NULL; a
    longer frame table than n_frames is not read past n_frames (its later frames must stay untouched)."""
    rng = np.random.default_rng(100 + n)
    hdrs = np.array([mk_v4(ttl=1), mk_v6(), mk_v6(14, tos=0xff)], B.TCPHDR_DTYPE)
    t = Table(rng, hlen_of(hdrs))
    while len(t.frame_off) < n + 3:
        mss = int(rng.integers(1, 200))
        t.add(len(t.bursts) % 3, int(rng.integers(0, 6 * mss)), mss, seq=int(rng.integers(0, 1 << 32)),
              flags=int(rng.choice([B.ACK, B.PSH | B.ACK, B.FIN | B.ACK])))
    dst, src, fo = t.arenas()
    for want_out, want_status in ((True, True), (False, True), (True, False), (False, False)):
        want = check(V, dst, src, hdrs, t.bursts, fo[:n], want_out=want_out, want_status=want_status)
    assert (want[0][int(fo[n]):] == FILL).all()
    if n == 1:
        check(V, dst, src, hdrs, t.bursts, fo[:0])   # n_frames == 0 launches nothing


# ------------------------------------------------------------------------------------------
# 5. round trip through the shipped kernels
# ------------------------------------------------------------------------------------------
def test_round_trip_build_parse_verify_receive(V):
    """Bursts built into Ethernet frames, parsed (vpcsum_parse_ether_async), verified
    (vpcsum_compute_async, MODE_VERIFY: every frame S_L4_OK, the IPv4 ones S_IP_OK) and received
    (vpcsum_tcp_recv_async, dst_off at the running sum of the payload lengths): the receive buffer
    equals the send buffer's bytes."""
    import torch
    rng = np.random.default_rng(110)
    hdrs = np.array([mk_v4(), mk_v6(14)], B.TCPHDR_DTYPE)
    bursts, fo, scur, sent = [], [], 0, []
    src = rng.integers(0, 256, 40000, dtype=np.uint8)
    for i, (d, mss) in enumerate([(1460 * 5 + 3, 1460), (1, 1460), (536 * 7, 536), (999, 1000), (0, 0), (1360 * 9 + 1359, 1360)]):
        b = U.mk_burst(scur, d, mss, len(fo), seq=int(rng.integers(0, 1 << 32)), hdr=i & 1, flags=B.PSH | B.ACK if d else B.ACK)
        bursts.append(b)
        sent.append(src[scur:scur + d])
        scur += d + int(rng.integers(0, 40))
        fo += [(len(fo) + k) * CAP + 384 + (i + k) % 16 for k in range(int(b["count"]))]
    n = len(fo)
    sent = np.concatenate(sent)
    dst = np.full(n * CAP + CAP, FILL, np.uint8)
    want = expected(dst, src, hdrs, bursts, fo)
    d_dst, d_fo = dev(dst), dev(np.array(fo, np.uint64))
    flen = torch.zeros(n, dtype=torch.int32, device="cuda")
    out = torch.zeros(n, dtype=torch.int32, device="cuda")
    V.tcp_build_bursts(d_dst, dev(src), dev(hdrs), 2, dev(np.array(bursts, U.TCPBURST_DTYPE)), len(bursts), d_fo, n, CAP, flen, out, None)
    desc = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    vout = torch.zeros(n, dtype=torch.int32, device="cuda")
    vst = torch.zeros(n, dtype=torch.uint8, device="cuda")
    V.parse_ether(d_dst, d_fo, flen, n, desc)
    V.compute(d_dst, desc, n, vout, vst, V.MODE_VERIFY)
    rx = np.zeros(n, V.TCPRX_DTYPE)
    lens = want[4]["data_len"].astype(np.uint64)
    rx["dst_off"] = np.concatenate([[0], np.cumsum(lens)[:-1]])
    rx["dst_cap"], rx["ops"] = lens, V.TCPRX_STORE
    recv = torch.full((len(sent) + 16,), FILL, dtype=torch.uint8, device="cuda")
    stored = torch.zeros(n, dtype=torch.int32, device="cuda")
    rst = torch.zeros(n, dtype=torch.uint8, device="cuda")
    V.tcp_recv(d_dst, desc, dev(rx), n, recv[:len(sent)], stored, None, rst)
    torch.cuda.synchronize()
    vst, rst, stored, recv = host(vst), host(rst), host(stored).view(np.uint32), host(recv)
    v4 = np.array([int(s["hdr"]) == 0 for s in want[4]])
    ok = V.S_DONE | V.S_L4_OK
    assert ((vst & ok) == ok).all() and not (vst & V.S_BAD_DESC).any() and (((vst & V.S_IP_OK) != 0) == v4).all()
    assert ((rst & ok) == ok).all() and np.array_equal(stored, lens.astype(np.uint32))
    assert np.array_equal(host(out).view(np.uint32), host(vout).view(np.uint32)) and np.array_equal(host(d_dst), want[0])
    assert np.array_equal(recv[:len(sent)], sent) and (recv[len(sent):] == FILL).all() and int(lens.sum()) == len(sent)


# ------------------------------------------------------------------------------------------
# 6. the host form, 7. PNI
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def txround():
    """A transmit round at umem geometry (2,048-byte chunks, frame at +384): 12 bursts over three
    templates -- data bursts of 1..7 frames, two without payload, one refused (no such template), one
    whose payload ends past the source -- payload runs scattered over a 256-KiB send buffer."""
    rng = np.random.default_rng(120)
    hdrs = np.array([mk_v4(), mk_v6(14), mk_v6()], B.TCPHDR_DTYPE)
    src = rng.integers(0, 256, 256 << 10, dtype=np.uint8)
    bursts, nf = [], 0
    for i, (d, mss) in enumerate([(1460 * 6 + 100, 1460), (0, 0), (536, 536), (1, 1460), (1360 * 3, 1360), (7000, 1000), (0, 1460),
                                  (2921, 1460), (500, 100), (100, 1460), (3000, 1460), (64, 8)]):
        b = U.mk_burst(4096 + int(rng.integers(0, 64 << 10)), d, mss, nf, seq=int(rng.integers(0, 1 << 32)), hdr=i % 3,
                       flags=B.PSH | B.ACK if d else B.FIN | B.ACK)
        bursts.append(b)
        nf += int(b["count"])
    bursts[8]["hdr"] = 3                          # no such template
    bursts[9]["data_off"] = len(src) - 50         # its payload ends past the source
    bursts = np.array(bursts, U.TCPBURST_DTYPE)
    fo = np.arange(nf, dtype=np.uint64) * 2048 + 384
    dst = np.full(nf * 2048, FILL, np.uint8)
    segs, marked = U.expand(bursts, fo, 2048 - 384, hdrs, len(src))
    assert marked.sum() == 5 + 1
    return dict(hdrs=hdrs, bursts=bursts, fo=fo, src=src, dst=dst, segs=segs, n=nf, cap=2048 - 384)


def test_host_form_in_place_and_staged(V, txround):
    """Context.build_tcp_bursts into a registered arena, with the source registered (read in place)
    and with a heap source (the span of the bursts' payloads staged, data_off rebased in the library's
    copy): arena, frame lengths, out words and status equal Context.build_tcp_frames' on the expanded
    records -- and the restatement's -- and the caller's arrays are unchanged.  An unregistered
    destination and an oversize span are refused by name."""
    tr = txround
    n, hdrs, bursts, fo, cap = tr["n"], tr["hdrs"], tr["bursts"], tr["fo"], tr["cap"]
    want, w_len, w_out, w_st = B.build(tr["dst"], tr["src"], hdrs, tr["segs"])
    arena = page_aligned(len(tr["dst"]))
    src_reg = page_aligned(len(tr["src"]))
    src_reg[:] = tr["src"]
    heap = tr["src"].copy()
    ctx = V.Context(0, max_arena=128 << 10, max_pkts=n)
    ctx.register(arena)
    ctx.register(src_reg)
    try:
        arena[:] = FILL
        r_len, r_out, r_st = ctx.build_tcp_frames(arena, src_reg, hdrs, tr["segs"])     # the per-segment form on the expansion
        assert np.array_equal(r_len, w_len) and np.array_equal(r_out, w_out) and np.array_equal(r_st, w_st)
        by_records = arena.copy()
        assert np.array_equal(by_records, want)
        for nm, s in (("in_place", src_reg), ("staged", heap), ("in_place_again", src_reg)):
            arena[:] = FILL
            before_b, before_fo = bursts.copy(), fo.copy()
            flen, out, st = ctx.build_tcp_bursts(arena, s, hdrs, bursts, fo, cap)
            assert bursts.tobytes() == before_b.tobytes() and fo.tobytes() == before_fo.tobytes(), nm
            assert np.array_equal(flen, r_len) and np.array_equal(out, r_out) and np.array_equal(st, r_st), nm
            assert np.array_equal(arena, by_records), (nm, first_diff(arena, by_records, tr["segs"]))
            assert np.array_equal(s, tr["src"]), nm
        # the optional results, and an empty frame table
        arena[:] = FILL
        flen, out, st = ctx.build_tcp_bursts(arena, heap, hdrs, bursts, fo, cap, want_out=False, want_status=False)
        assert out is None and st is None and np.array_equal(flen, r_len) and np.array_equal(arena, by_records)
        flen, _, _ = ctx.build_tcp_bursts(arena, heap, hdrs, bursts, fo[:0], cap)
        assert len(flen) == 0
        # refusals: the frames as they were
        arena[:] = FILL
        with pytest.raises(V.VpcsumError, match="vpcsum_ctx_build_tcp_bursts: the destination must be registered"):
            ctx.build_tcp_bursts(np.zeros(8192, np.uint8), heap, hdrs, bursts[:1], fo[:1], cap)
        far = bursts[:2].copy()
        far["data_off"], far["data_len"], far["mss"], far["count"], far["first"] = (0, 200 << 10), 100, 100, 1, (0, 1)
        with pytest.raises(V.VpcsumError, match=r"vpcsum_ctx_build_tcp_bursts: the payloads span \d+ bytes > capacity 131072"):
            ctx.build_tcp_bursts(arena, heap, hdrs, far, fo[:2], cap)
        flen, _, _ = ctx.build_tcp_bursts(arena, src_reg, hdrs, far, fo[:2], cap)   # in place there is no span to stage
        assert list(flen) == [154, 174]
        arena[:2 * 2048] = FILL
        with pytest.raises(V.VpcsumError, match=f"vpcsum_ctx_build_tcp_bursts: {n + 1} frames > capacity {n}"):
            ctx.build_tcp_bursts(arena, heap, hdrs, bursts, np.concatenate([fo, fo[:1]]), cap)
        assert (arena == FILL).all()
    finally:
        ctx.unregister(src_reg)
        ctx.unregister(arena)
        ctx.close()


def test_pni_build_tcp_bursts(V, txround):
    """Java_io_vproxy_vpcsum_VPCsum_buildTcpBursts driven through ctypes with PNI environments, as the
    JVM's downcall drives it: create, registerArena, buildTcpBursts (heap source), waitFor, close."""
    tr = txround
    n, hdrs, bursts, fo, cap = tr["n"], tr["hdrs"], tr["bursts"], tr["fo"], tr["cap"]
    want, w_len, w_out, w_st = B.build(tr["dst"], tr["src"], hdrs, tr["segs"])
    L = V.lib()
    I32, I64, P = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p

    class Env(ctypes.Structure):   # PNIEnv_vpcsum_long: the exception (type, message, errno_), then the value
        _fields_ = [("type", ctypes.c_char_p), ("message", ctypes.c_char * 4096), ("errno_", I32), ("ret", I64), ("pad", I64)]

    def call(f, *args):
        env = Env()
        f.restype = ctypes.c_int
        rc = f(ctypes.byref(env), *args)
        assert rc == 0, (env.type, env.message)
        return env.ret

    arena = page_aligned(len(tr["dst"]))
    arena[:] = FILL
    heap = tr["src"].copy()
    flen, out, st = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    ctx = call(L.Java_io_vproxy_vpcsum_VPCsum_create, I32(0), I64(128 << 10), I32(n))
    try:
        call(L.Java_io_vproxy_vpcsum_VPCsum_registerArena, I64(ctx), P(arena.ctypes.data), I64(arena.nbytes))
        t = call(L.Java_io_vproxy_vpcsum_VPCsum_buildTcpBursts, I64(ctx), P(arena.ctypes.data), I64(arena.nbytes),
                 P(heap.ctypes.data), I64(heap.nbytes), P(hdrs.ctypes.data), I32(len(hdrs)), P(bursts.ctypes.data), I32(len(bursts)),
                 P(fo.ctypes.data), I32(n), I32(cap), P(flen.ctypes.data), P(out.ctypes.data), P(st.ctypes.data))
        call(L.Java_io_vproxy_vpcsum_VPCsum_waitFor, I64(ctx), I64(t))
        assert np.array_equal(flen, w_len) and np.array_equal(out, w_out) and np.array_equal(st, w_st)
        assert np.array_equal(arena, want), first_diff(arena, want, tr["segs"])
    finally:
        call(L.Java_io_vproxy_vpcsum_VPCsum_close, I64(ctx))
