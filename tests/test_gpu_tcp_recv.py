"""The TCP receive on the GPU (vpcsum_tcp_recv_async, vpcsum_tcp_digest_async,
vpcsum_ctx_recv_tcp_frames, VPCsum.recvTcpFrames) against the Python restatement of its rule
(tests/tcprecvvec.py: out and status from the oracle's MODE_VERIFY, stored bytes by numpy slicing).
In every case the WHOLE destination arena is compared with the restatement's: it is prefilled with
0xEE and every stored range has 3 guard bytes around it, so a byte written outside a range fails
the case; stored counts, out words and status bytes are compared too (they start as 0xAB and carry
two guard rows), and the source arena must come back as it went."""
import ctypes
import os

import numpy as np
import pytest

import tcpbuildvec as B
import tcprecvvec as R
from oracle import oracle as O
from pcaputil import l3_offset, read_pcap

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
    assert vpcsum.TCPRX_DTYPE == R.TCPRX_DTYPE and vpcsum.TCPINFO_DTYPE == R.TCPINFO_DTYPE
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


def gpu_recv(V, dst, arena, desc, rx, n=None, want_out=True, want_status=True):
    """(dst_after, stored, out, status) of vpcsum_tcp_recv_async on device copies of the arenas."""
    import torch
    n = len(desc) if n is None else n
    d_dst, d_arena = dev(dst), dev(arena)
    assert d_dst.data_ptr() % 16 == 0 and d_arena.data_ptr() % 16 == 0
    d_d = dev(desc) if len(desc) else torch.zeros(16, dtype=torch.uint8, device="cuda")
    d_r = dev(rx) if len(rx) else torch.zeros(16, dtype=torch.uint8, device="cuda")
    stored = torch.full(((n + 2) * 4,), 0xAB, dtype=torch.uint8, device="cuda")
    out = torch.full(((n + 2) * 4,), 0xAB, dtype=torch.uint8, device="cuda")
    st = torch.full((n + 2,), 0xAB, dtype=torch.uint8, device="cuda")
    V.tcp_recv(d_arena, d_d, d_r, n, d_dst, stored, out if want_out else None, st if want_status else None)
    torch.cuda.synchronize()
    stored, out, st = host(stored).view(np.uint32), host(out).view(np.uint32), host(st)
    assert (stored[n:] == 0xABABABAB).all() and (out[n:] == 0xABABABAB).all() and (st[n:] == 0xAB).all()
    if not want_out:
        assert (out == 0xABABABAB).all()
    if not want_status:
        assert (st == 0xAB).all()
    assert np.array_equal(host(d_arena), arena)
    return host(d_dst), stored[:n], out[:n], st[:n]


def gpu_digest(V, arena, desc):
    import torch
    n = len(desc)
    info = torch.full(((n + 2) * 16,), 0xAB, dtype=torch.uint8, device="cuda")
    assert info.data_ptr() % 16 == 0
    V.tcp_digest(dev(arena), dev(desc), n, info)
    torch.cuda.synchronize()
    got = host(info)
    assert (got[n * 16:] == 0xAB).all()
    return got[:n * 16].view(R.TCPINFO_DTYPE)


def first_diff(got, want, rx):
    k = int(np.flatnonzero(got != want)[0])
    near = [(i, k - int(r["dst_off"])) for i, r in enumerate(rx) if int(r["dst_off"]) - 4 <= k and int(r["ops"]) & 1]
    i, rel = min(near, key=lambda t: abs(t[1])) if near else (-1, k)
    return f"byte {k} (record {i} +{rel}): {got[k]:#x} != {want[k]:#x}"


def check(V, dst, arena, desc, rx, n=None, want_out=True, want_status=True):
    n = len(desc) if n is None else n
    want, w_stored, w_out, w_st = R.recv(dst, arena, desc[:n], rx[:n])
    got, stored, out, st = gpu_recv(V, dst, arena, desc, rx, n, want_out, want_status)
    assert np.array_equal(stored, w_stored), [(i, int(stored[i]), int(w_stored[i])) for i in np.flatnonzero(stored != w_stored)[:8]]
    if want_status:
        assert np.array_equal(st, w_st), [(i, hex(st[i]), hex(w_st[i])) for i in np.flatnonzero(st != w_st)[:8]]
    if want_out:
        assert np.array_equal(out, w_out), [(i, hex(out[i]), hex(w_out[i])) for i in np.flatnonzero(out != w_out)[:8]]
    assert np.array_equal(got, want), first_diff(got, want, rx[:n])
    return want, w_stored, w_out, w_st


class Layout:
    """Packets laid one after another in the source arena, the TCP segment's first byte at a wanted
    address residue mod 16, and their stored ranges in the destination at a wanted residue, with 3
    guard bytes (source: `pad` bytes of 0xff L2 padding first) around each."""

    def __init__(self):
        self.scur, self.dcur, self.desc, self.rx, self.chunks = 0, 0, [], [], []

    def add(self, l3: bytes, l4_off: int, ver: int, sres=0, dres=0, skip=0, ops=R.STORE, pad=0, flags=None, cap=None):
        hlen = (l3[l4_off + 12] >> 4) * 4
        stored = max(len(l3) - l4_off - hlen - skip, 0)
        self.scur += 3
        self.scur += (sres - (self.scur + l4_off)) % 16
        self.dcur += 3
        self.dcur += (dres - self.dcur) % 16
        self.desc.append(R.mk_desc(self.scur, len(l3), l4_off, ver, flags=flags))
        self.rx.append(R.mk_rx(self.dcur, stored if cap is None else cap, skip, ops))
        self.chunks.append((self.scur, l3 + b"\xff" * pad))
        self.scur += len(l3) + pad + 3
        if ops & R.STORE:
            self.dcur += stored + 3
        return len(self.desc) - 1

    def arrays(self, dst_tail=3):
        arena = np.full(self.scur + 13, 0x5a, np.uint8)
        for o, b in self.chunks:
            arena[o:o + len(b)] = np.frombuffer(b, np.uint8)
        dst = np.full(self.dcur + dst_tail, FILL, np.uint8)
        return dst, arena, np.array(self.desc, O.DESC_DTYPE), np.array(self.rx, R.TCPRX_DTYPE)


def payload(rng, d):
    return rng.integers(0, 256, d, dtype=np.uint8).tobytes()


# ------------------------------------------------------------------------------------------
# 1. alignment by length
# ------------------------------------------------------------------------------------------
LENGTHS = (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 127, 128, 129, 1360, 1460)


@pytest.mark.parametrize("ver", [4, 6], ids=["ipv4", "ipv6"])
def test_alignment_by_length_grid(V, ver):
    """Every payload length of LENGTHS at every segment residue 0..15 and every destination residue
    0..15, skip 0: 4,352 records in one batch."""
    rng = np.random.default_rng(60 + ver)
    lay = Layout()
    for d in LENGTHS:
        l3, l4o = R.tcp_l3(ver, payload(rng, d), seq=int(rng.integers(0, 1 << 32)))
        for sres in range(16):
            for dres in range(16):
                lay.add(l3, l4o, ver, sres, dres)
    dst, arena, desc, rx = lay.arrays()
    assert len(desc) == 4352
    _, w_stored, _, w_st = check(V, dst, arena, desc, rx)
    ok = R.S_DONE | R.S_L4_OK | (R.S_IP_OK if ver == 4 else 0)
    assert (w_st == ok).all() and int(w_stored.sum()) == 256 * sum(LENGTHS)


# ------------------------------------------------------------------------------------------
# 2. skip
# ------------------------------------------------------------------------------------------
def test_skip_prefix_is_summed_not_stored(V):
    """skip in {1, 2, 3, 5, 15, 16, 17, len - 1, len} at every destination residue, several lengths and
    segment residues: the summed-not-stored prefix crosses dword and group edges."""
    rng = np.random.default_rng(62)
    lay = Layout()
    for ver, d in ((4, 18), (4, 33), (6, 100), (4, 517), (6, 1460)):
        l3, l4o = R.tcp_l3(ver, payload(rng, d))
        for skip in sorted({1, 2, 3, 5, 15, 16, 17, d - 1, d}):
            for dres in range(16):
                lay.add(l3, l4o, ver, int(rng.integers(0, 16)), dres, skip=skip)
    dst, arena, desc, rx = lay.arrays()
    _, w_stored, _, w_st = check(V, dst, arena, desc, rx)
    assert (w_st & R.S_L4_OK).all() and (w_stored == 0).sum() == 5 * 16


# ------------------------------------------------------------------------------------------
# 3. headers
# ------------------------------------------------------------------------------------------
def header_batch():
    rng = np.random.default_rng(63)
    lay = Layout()
    for hlen in range(20, 64, 4):
        for ver, kw in ((4, dict(ihl=5)), (4, dict(ihl=15)), (6, dict(ext=0)), (6, dict(ext=8))):
            for d in (0, 1, 7, 64, 301):
                l3, l4o = R.tcp_l3(ver, payload(rng, d), hlen=hlen, seq=int(rng.integers(0, 1 << 32)), ack=int(rng.integers(0, 1 << 32)),
                                   window=int(rng.integers(0, 1 << 16)), flags=int(rng.integers(0, 64)), **kw)
                lay.add(l3, l4o, ver, int(rng.integers(0, 16)), int(rng.integers(0, 16)), skip=int(rng.integers(0, d + 1)),
                        pad=int(rng.integers(1, 9)), ops=R.STORE if d else 0)
    return lay.arrays()


def test_header_lengths_options_and_padding(V):
    """hlen 20..60 with options, IPv4 IHL 5 and 15, IPv6 with l4_off 40 and 48, odd segment lengths,
    and 0xff L2 padding after l3_len that must not enter the sum; the digest on the same batch."""
    dst, arena, desc, rx = header_batch()
    assert set(desc["l4_off"]) == {20, 60, 40, 48}
    _, _, _, w_st = check(V, dst, arena, desc, rx)
    assert (w_st & R.S_L4_OK).all()
    info, want = gpu_digest(V, arena, desc), R.digest(arena, desc)
    assert info.tobytes() == want.tobytes(), [i for i in range(len(desc)) if info[i] != want[i]][:8]
    assert set(want["hlen"]) == set(range(20, 64, 4))


# ------------------------------------------------------------------------------------------
# 4. verdicts
# ------------------------------------------------------------------------------------------
def test_verdicts(V, orc):
    """One bit flipped in the TCP header, a skipped byte, the first stored byte, the last byte of an
    odd-length segment, a source address and the stored field: S_L4_OK cleared, `out` still the
    recomputed sum, the bytes still stored.  A segment whose sum is 0x0000 is OK stored as such and
    not OK stored as 0xffff; a corrupted IPv4 header clears S_IP_OK only."""
    rng = np.random.default_rng(64)
    lay = Layout()
    cases = []
    for ver in (4, 6):
        l3, l4o = R.tcp_l3(ver, payload(rng, 101), hlen=24)
        seg = l4o
        for name, at in (("clean", None), ("tcp_header", seg + 5), ("skipped", seg + 24 + 3), ("first_stored", seg + 24 + 9),
                         ("last_odd", len(l3) - 1), ("src_addr", 13 if ver == 4 else 9), ("field", seg + 17)):
            b = bytearray(l3)
            if at is not None:
                b[at] ^= 1 << int(rng.integers(0, 8))
            cases.append((name, ver, lay.add(bytes(b), l4o, ver, int(rng.integers(0, 16)), int(rng.integers(0, 16)), skip=9)))
    # a sum of 0x0000: the payload's first word chosen so
    body = bytearray(payload(rng, 64))
    body[0:2] = b"\0\0"
    l3, l4o = R.tcp_l3(4, bytes(body))
    c = int.from_bytes(l3[l4o + 16:l4o + 18], "big")
    body[0:2] = c.to_bytes(2, "big")
    l3z, _ = R.tcp_l3(4, bytes(body))
    assert l3z[l4o + 16:l4o + 18] == b"\0\0" and O.l4_csum(l3z, len(l3z), l4o, 4, 6) == 0
    zero = lay.add(l3z, l4o, 4, 5, 7)
    ones = lay.add(l3z[:l4o + 16] + b"\xff\xff" + l3z[l4o + 18:], l4o, 4, 9, 2)
    # IPv4 header corrupted (TTL: not in the pseudo-header)
    b = bytearray(R.tcp_l3(4, payload(rng, 40))[0])
    b[8] ^= 0x10
    ttl = lay.add(bytes(b), 20, 4, 3, 11)
    dst, arena, desc, rx = lay.arrays()
    want, w_stored, w_out, w_st = check(V, dst, arena, desc, rx)
    o_out, _ = orc.process(arena, desc, O.MODE_VERIFY)
    assert np.array_equal(w_out, o_out)
    for name, ver, i in cases:
        assert bool(w_st[i] & R.S_L4_OK) == (name == "clean"), (name, ver, hex(w_st[i]))
        assert w_st[i] & R.S_DONE and w_stored[i] == 92
        if ver == 4:
            assert bool(w_st[i] & R.S_IP_OK) == (name != "src_addr"), (name, hex(w_st[i]))
        # `out` is the recomputed sum: what the frame should have carried
        d = desc[i]
        l3 = arena[int(d["l3_off"]):int(d["l3_off"]) + int(d["l3_len"])].tobytes()
        assert int(w_out[i]) >> 16 == O.l4_csum(l3, len(l3), int(d["l4_off"]), ver, 6)
    assert w_st[zero] == R.S_DONE | R.S_L4_OK | R.S_IP_OK and w_out[zero] >> 16 == 0
    assert w_st[ones] == R.S_DONE | R.S_IP_OK and w_out[ones] >> 16 == 0 and w_stored[ones] == 64
    assert w_st[ttl] == R.S_DONE | R.S_L4_OK


# ------------------------------------------------------------------------------------------
# 5. refusals and mixing
# ------------------------------------------------------------------------------------------
def refusal_batch():
    """Every refusal of the header's list, each on a packet of its own, between stored and
    verify-only records.  Returns the arrays and the indices that must be refused."""
    rng = np.random.default_rng(65)
    lay = Layout()
    v4, o4 = R.tcp_l3(4, payload(rng, 50))
    v6, o6 = R.tcp_l3(6, payload(rng, 50))
    bad = {}
    muts = [
        ("proto", 4, lambda d, r: d.__setitem__("l4_proto", 17)),
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
        ("short_19", 4, lambda d, r: d.__setitem__("l3_len", 20 + 19)),
        ("ops_2", 4, lambda d, r: r.__setitem__("ops", 2)),
        ("ops_81", 6, lambda d, r: r.__setitem__("ops", 0x81)),
        ("rsv", 4, lambda d, r: r.__setitem__("rsv", 1)),
        ("skip_past", 4, lambda d, r: r.__setitem__("skip", 51)),
        ("skip_past_verify", 6, lambda d, r: (r.__setitem__("skip", 51), r.__setitem__("ops", 0))),
        ("cap_short", 4, lambda d, r: r.__setitem__("dst_cap", 49)),
        ("dst_off_max", 6, lambda d, r: r.__setitem__("dst_off", (1 << 64) - 4)),
    ]
    patches = []
    for k, (name, ver, f) in enumerate(muts):
        lay.add(v4 if k & 1 else v6, o4 if k & 1 else o6, 4 if k & 1 else 6, int(rng.integers(0, 16)), int(rng.integers(0, 16)),
                skip=k % 7, ops=R.STORE if k % 3 else 0)                      # a record that works
        l3, o = (v4, o4) if ver == 4 else (v6, o6)
        patches.append((lay.add(l3, o, ver, int(rng.integers(0, 16)), int(rng.integers(0, 16))), name, f))
    # header bytes: a data offset of 4, and one past the segment (a 40-byte segment claiming 44)
    b = bytearray(v4)
    b[o4 + 12] = 0x40
    bad["doff_4"] = lay.add(bytes(b), o4, 4, 7, 3)
    b = bytearray(R.tcp_l3(6, payload(rng, 20))[0])
    b[o6 + 12] = 0xb0
    bad["hlen_44_of_40"] = lay.add(bytes(b), o6, 6, 2, 9)
    lay.add(v6, o6, 6, 1, 1, cap=50)                                          # dst_cap exact
    last = lay.add(v4, o4, 4, 15, 15)                                         # ends the destination
    dst, arena, desc, rx = lay.arrays(dst_tail=-3)
    for i, name, f in patches:
        f(desc[i], rx[i])
        bad[name] = i
    # the last stored range ends with the destination; one byte further is outside it
    assert int(rx[last]["dst_off"]) + 50 == len(dst)
    return dst, arena, desc, rx, bad, last


def test_refusals_among_good_records(V):
    """Every refusal in one batch, interleaved with stored and verify-only records, so that teams
    that leave early sit beside teams that work: a refused record writes nothing and reports 0, 0,
    S_BAD_DESC; dst_cap exact is taken and one byte short refused; the digest on the same batch."""
    dst, arena, desc, rx, bad, last = refusal_batch()
    want, w_stored, w_out, w_st = check(V, dst, arena, desc, rx)
    refused = set(int(i) for i in np.flatnonzero(w_st == R.S_BAD_DESC))
    assert refused == set(bad.values()), (sorted(refused ^ set(bad.values())), bad)
    assert all(w_stored[i] == 0 and w_out[i] == 0 for i in refused)
    assert (w_st[sorted(set(range(len(desc))) - refused)] & R.S_L4_OK).all()
    # the destination one byte shorter: the last record no longer fits
    short = dst[:-1].copy()
    _, s2, _, st2 = check(V, short, arena, desc, rx)
    assert st2[last] == R.S_BAD_DESC and s2[last] == 0
    info, w_info = gpu_digest(V, arena, desc), R.digest(arena, desc)
    assert info.tobytes() == w_info.tobytes(), [i for i in range(len(desc)) if info[i] != w_info[i]][:8]
    zero = {i for i in range(len(desc)) if w_info[i]["hlen"] == 0}
    header_only = {"ops_2", "ops_81", "rsv", "skip_past", "skip_past_verify", "cap_short", "dst_off_max"}   # the record's, not the header's
    assert zero == {i for k, i in bad.items() if k not in header_only}


@pytest.mark.parametrize("n", [0, 1, 31, 33])
def test_batch_sizes_and_optional_outputs(V, n):
    """n of 0, 1, 31 and 33 (a block's 32 teams and one more) out of a 40-record batch -- records past
    n are not touched -- with and without the optional outputs."""
    rng = np.random.default_rng(66)
    lay = Layout()
    for i in range(40):
        d = int(rng.choice([0, 1, 17, 200, 1460]))
        ver = 4 if i & 1 else 6
        l3, o = R.tcp_l3(ver, payload(rng, d))
        lay.add(l3, o, ver, int(rng.integers(0, 16)), int(rng.integers(0, 16)), skip=int(rng.integers(0, d + 1)), ops=R.STORE if i % 5 else 0)
    dst, arena, desc, rx = lay.arrays()
    check(V, dst, arena, desc, rx, n)
    check(V, dst, arena, desc, rx, n, want_out=False)
    check(V, dst, arena, desc, rx, n, want_status=False)
    check(V, dst, arena, desc, rx, n, want_out=False, want_status=False)


# ------------------------------------------------------------------------------------------
# 6. one large record
# ------------------------------------------------------------------------------------------
def test_largest_segment_of_ff(V):
    """An IPv4 segment of 65,515 bytes (l3_len 65,535), every payload byte 0xff, stored and verify
    only, at odd alignments: the accumulators' width."""
    lay = Layout()
    l3, o = R.tcp_l3(4, b"\xff" * (65515 - 20), seq=0xffffffff, ack=0xffffffff, window=0xffff, sport=0xffff, dport=0xffff,
                     src=b"\xff" * 4, dst=b"\xff" * 4)
    assert len(l3) == 65535
    lay.add(l3, o, 4, 5, 11)
    lay.add(l3, o, 4, 14, 0, ops=0)
    lay.add(l3, o, 4, 1, 6, skip=32769)
    dst, arena, desc, rx = lay.arrays()
    _, w_stored, _, w_st = check(V, dst, arena, desc, rx)
    assert list(w_stored) == [65495, 0, 65495 - 32769] and (w_st == R.S_DONE | R.S_L4_OK | R.S_IP_OK).all()


# ------------------------------------------------------------------------------------------
# 7. the digest after the GPU parse
# ------------------------------------------------------------------------------------------
def test_digest_of_the_captured_frames(V):
    """cap-ether.pcap parsed on the GPU (vpcsum_parse_ether_async), digested, received: the digest
    equals the restatement's (payloads of 77, 81 and 305 bytes, header lengths 20 and 40) and the
    receive stores those payloads with the oracle's status (7 correct sums of 13)."""
    import torch
    lt, pkts = read_pcap(os.path.join(REPO, "tests", "golden", "pcap", "cap-ether.pcap"))
    pkts = [p for p in pkts if l3_offset(lt, p) is not None]
    n = len(pkts)
    arena = np.full(n * 2048, 0x5a, np.uint8)
    for i, p in enumerate(pkts):
        arena[i * 2048 + 384:i * 2048 + 384 + len(p)] = np.frombuffer(p, np.uint8)
    foff = np.arange(n, dtype=np.uint64) * 2048 + 384
    flen = np.array([len(p) for p in pkts], np.uint32)
    d_arena = dev(arena)
    d_desc = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    V.parse_ether(d_arena, dev(foff), dev(flen), n, d_desc)
    info = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    V.tcp_digest(d_arena, d_desc, n, info)
    torch.cuda.synchronize()
    desc = host(d_desc).view(O.DESC_DTYPE)
    info = host(info).view(R.TCPINFO_DTYPE)
    want = R.digest(arena, desc)
    assert n == 13 and info.tobytes() == want.tobytes()
    assert sorted(int(x) for x in info["data_len"] if x) == [77, 81, 305] and set(int(x) for x in info["hlen"]) == {20, 40}
    rx = np.zeros(n, R.TCPRX_DTYPE)
    pos = 5
    for i in range(n):
        k = int(info["data_len"][i])
        rx[i] = R.mk_rx(pos, k, 0, R.STORE if k else 0)
        pos += k + 3
    _, w_stored, _, w_st = check(V, np.full(pos, FILL, np.uint8), arena, desc, rx)
    assert int(np.count_nonzero(w_st & R.S_L4_OK)) == 7 and int(w_stored.sum()) == 463


# ------------------------------------------------------------------------------------------
# 8. round trip with the build
# ------------------------------------------------------------------------------------------
def test_round_trip_with_the_build(V):
    """vpcsum_tcp_build_async builds 64 frames (IPv4 with Ethernet, IPv6 without, mixed alignments);
    the Ethernet ones are parsed by vpcsum_parse_ether_async, the bare IPv6 ones described by their
    records; the digest equals the records' seq, ack, window, flags and data_len; the receive with
    STORE into a fresh buffer at each record's data_off gives the send buffer back, every status
    S_L4_OK (and S_IP_OK on IPv4)."""
    import torch
    rng = np.random.default_rng(67)
    hdrs = np.array([B.mk_hdr(4, 14, ack=0x11223344, window=0x4321), B.mk_hdr(6, 0, bytes(range(16)), bytes(range(16, 32)), ack=0x55667788,
                                                                              window=0x1234)], B.TCPHDR_DTYPE)
    n = 64
    segs, fcur, scur = [], 0, 0
    for i in range(n):
        hi = i & 1
        d = int(rng.choice([1, 2, 63, 64, 65, 517, 1360, 1460]))
        fcur += 3 + int(rng.integers(0, 16))
        scur += 3 + int(rng.integers(0, 16))
        segs.append(B.mk_seg(fcur, scur, d, seq=int(rng.integers(0, 1 << 32)), hdr=hi, flags=B.PSH | B.ACK if i % 3 else B.ACK | B.FIN,
                             hlen=B.header_len(hdrs[hi])))
        fcur += B.header_len(hdrs[hi]) + d
        scur += d
    segs = np.array(segs, B.TCPSEG_DTYPE)
    send = np.full(scur + 7, FILL, np.uint8)
    for s in segs:
        send[int(s["data_off"]):int(s["data_off"]) + int(s["data_len"])] = rng.integers(0, 256, int(s["data_len"]), dtype=np.uint8)
    d_frames, d_send = dev(np.full(fcur + 5, FILL, np.uint8)), dev(send)
    flen = torch.zeros(n, dtype=torch.int32, device="cuda")
    V.tcp_build(d_frames, d_send, dev(hdrs), 2, dev(segs), n, flen, None, None)
    # descriptors: the Ethernet frames (even records) parsed on the device, the bare IPv6 ones by hand
    ev = np.arange(0, n, 2)
    d4 = torch.zeros(len(ev) * 16, dtype=torch.uint8, device="cuda")
    V.parse_ether(d_frames, dev(segs["frame_off"][ev].copy()), flen[::2].contiguous(), len(ev), d4)
    torch.cuda.synchronize()
    desc = np.zeros(n, O.DESC_DTYPE)
    desc[ev] = host(d4).view(O.DESC_DTYPE)
    for i in range(1, n, 2):
        desc[i] = R.mk_desc(int(segs[i]["frame_off"]), 60 + int(segs[i]["data_len"]), 40, 6)
    assert (desc["l4_proto"] == 6).all() and (desc["l3_off"][ev] == segs["frame_off"][ev] + 14).all()
    d_desc = dev(desc)
    info = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    V.tcp_digest(d_frames, d_desc, n, info)
    rx = np.zeros(n, R.TCPRX_DTYPE)
    for i in range(n):
        rx[i] = R.mk_rx(int(segs[i]["data_off"]), int(segs[i]["data_len"]), 0, R.STORE)
    d_back = dev(np.full(len(send), FILL, np.uint8))
    stored = torch.zeros(n, dtype=torch.int32, device="cuda")
    st = torch.zeros(n, dtype=torch.uint8, device="cuda")
    V.tcp_recv(d_frames, d_desc, dev(rx), n, d_back, stored, None, st)
    torch.cuda.synchronize()
    info = host(info).view(R.TCPINFO_DTYPE)
    for i in range(n):
        h = hdrs[i & 1]
        assert (int(info[i]["seq"]), int(info[i]["data_len"]), int(info[i]["flags"]), int(info[i]["hlen"])) == \
            (int(segs[i]["seq"]), int(segs[i]["data_len"]), int(segs[i]["flags"]), 20), i
        assert int(info[i]["ack"]) == int.from_bytes(h["ack"].tobytes(), "big") and int(info[i]["window"]) == int.from_bytes(h["window"].tobytes(), "big")
    st = host(st)
    assert np.array_equal(host(stored).view(np.uint32), segs["data_len"].astype(np.uint32))
    assert (st[0::2] == R.S_DONE | R.S_L4_OK | R.S_IP_OK).all() and (st[1::2] == R.S_DONE | R.S_L4_OK).all(), [hex(x) for x in st]
    assert np.array_equal(host(d_back), send)


# ------------------------------------------------------------------------------------------
# 9. the host form and PNI
# ------------------------------------------------------------------------------------------
STRIDE, HEADROOM = 2048, 384
_KEEP = []


def page_aligned(nbytes):
    raw = np.zeros(nbytes + 8192, np.uint8)
    _KEEP.append(raw)   # page-locked and released by the tests: kept for the life of the process
    skip = (-raw.ctypes.data) % 4096
    return raw[skip:skip + nbytes]


@pytest.fixture(scope="module")
def rxbatch():
    """64 received Ethernet frames at umem geometry (2,048-byte chunks, frame at +384), IPv4 and IPv6,
    stored into runs of a receive buffer; pure ACKs verify-only, some trimmed, one with a bad sum, two
    refused records among them."""
    rng = np.random.default_rng(68)
    n = 64
    arena = np.full(n * STRIDE, 0x5a, np.uint8)
    desc, rx = np.zeros(n, O.DESC_DTYPE), np.zeros(n, R.TCPRX_DTYPE)
    pos = 0
    for i in range(n):
        ver = 6 if i % 4 == 3 else 4
        d = int(rng.choice([0, 1, 100, 517, 1360, 1460]))
        l3, o = R.tcp_l3(ver, payload(rng, d), hlen=int(rng.choice([20, 32])), seq=int(rng.integers(0, 1 << 32)))
        at = i * STRIDE + HEADROOM
        eth = b"\x02\0\0\0\x0a\x01\x02\0\0\0\x0b\x02" + (b"\x08\x00" if ver == 4 else b"\x86\xdd")
        arena[at:at + 14 + len(l3)] = np.frombuffer(eth + l3, np.uint8)
        desc[i] = R.mk_desc(at + 14, len(l3), o, ver)
        skip = int(rng.integers(0, d + 1)) if i % 5 == 0 else 0
        rx[i] = R.mk_rx(pos + 1, d - skip, skip, R.STORE if d else 0)
        pos += d - skip + 4
    arena[int(desc[7]["l3_off"]) + int(desc[7]["l3_len"]) - 1] ^= 0x20   # a bad sum: stored all the same
    rx[10]["rsv"] = 1
    desc[20]["l4_proto"] = 17
    dst = np.full(pos + 64, FILL, np.uint8)
    want = R.recv(dst, arena, desc, rx)
    assert [i for i in range(n) if want[3][i] == R.S_BAD_DESC] == [10, 20] and not want[3][7] & R.S_L4_OK
    return dict(arena=arena, desc=desc, rx=rx, dst=dst, want=want, n=n)


def test_host_form_in_place_and_staged(V, rxbatch):
    """Context.recv_tcp_frames into a registered page-aligned receive buffer, once with the RX arena
    registered (read in place) and once with a heap copy (staged as submit stages it), then again
    with the service grid on: destination, stored counts, out words and status equal the
    restatement's -- so the device form's -- and the RX arena is unchanged.  An unregistered
    destination, n > max_pkts and a staged span above capacity are refused by name."""
    rb = rxbatch
    n, desc, rx = rb["n"], rb["desc"], rb["rx"]
    want, w_stored, w_out, w_st = rb["want"]
    check(V, rb["dst"], rb["arena"], desc, rx)   # the device form on the same batch
    rbuf = page_aligned(len(rb["dst"]))
    umem = page_aligned(len(rb["arena"]))
    umem[:] = rb["arena"]
    heap = rb["arena"].copy()
    ctx = V.Context(0, max_arena=128 << 10, max_pkts=n)
    ctx.register(rbuf)
    ctx.register(umem)
    try:
        for nm, a in (("in_place", umem), ("staged", heap), ("service_in_place", umem), ("service_staged", heap)):
            if nm == "service_in_place":
                ctx.set_service(200)
            rbuf[:] = FILL
            d0, r0 = desc.copy(), rx.copy()
            stored, out, st = ctx.recv_tcp_frames(a, desc, rx, rbuf)
            assert desc.tobytes() == d0.tobytes() and rx.tobytes() == r0.tobytes(), nm
            assert np.array_equal(stored, w_stored) and np.array_equal(out, w_out) and np.array_equal(st, w_st), nm
            assert np.array_equal(rbuf, want), (nm, first_diff(rbuf, want, rx))
            assert np.array_equal(a, rb["arena"]), nm
        ctx.set_service(0)
        # the optional results, and an empty batch
        rbuf[:] = FILL
        stored, out, st = ctx.recv_tcp_frames(heap, desc, rx, rbuf, want_out=False, want_status=False)
        assert out is None and st is None and np.array_equal(stored, w_stored) and np.array_equal(rbuf, want)
        stored, _, _ = ctx.recv_tcp_frames(heap, desc[:0], rx[:0], rbuf)
        assert len(stored) == 0
        # refusals: the receive buffer as it was
        rbuf[:] = FILL
        other = np.zeros(8192, np.uint8)
        with pytest.raises(V.VpcsumError, match="vpcsum_ctx_recv_tcp_frames: the destination must be registered"):
            ctx.recv_tcp_frames(umem, desc[:1], rx[:1], other)
        with pytest.raises(V.VpcsumError, match="vpcsum_ctx_recv_tcp_frames: 65 packets > capacity 64"):
            ctx.recv_tcp_frames(umem, np.concatenate([desc, desc[:1]]), np.concatenate([rx, rx[:1]]), rbuf)
        assert (rbuf == FILL).all()
    finally:
        ctx.unregister(umem)
        ctx.unregister(rbuf)
        ctx.close()
    # a staged span above the context's capacity: a dense batch of 48 KiB through a 32-KiB context
    small = V.Context(0, max_arena=32 << 10, max_pkts=n)
    small.register(rbuf)
    try:
        with pytest.raises(V.VpcsumError, match=r"vpcsum_ctx_recv_tcp_frames: (batch spans \d+ bytes > capacity 32768|gathered batch exceeds capacity)"):
            small.recv_tcp_frames(heap, desc, rx, rbuf)
        assert (rbuf == FILL).all()
    finally:
        small.unregister(rbuf)
        small.close()


def test_pni_recv_tcp_frames(V, rxbatch):
    """Java_io_vproxy_vpcsum_VPCsum_recvTcpFrames driven through ctypes with PNI environments, as the
    JVM's downcall drives it: create, registerArena (the receive buffer), recvTcpFrames on the 64
    frames (heap RX arena), waitFor, close -- byte-equal payloads, counts, out words and status."""
    rb = rxbatch
    n, desc, rx = rb["n"], rb["desc"], rb["rx"]
    want, w_stored, w_out, w_st = rb["want"]
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

    rbuf = page_aligned(len(rb["dst"]))
    rbuf[:] = FILL
    heap = rb["arena"].copy()
    stored, out, st = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    ctx = call(L.Java_io_vproxy_vpcsum_VPCsum_create, I32(0), I64(128 << 10), I32(n))
    try:
        call(L.Java_io_vproxy_vpcsum_VPCsum_registerArena, I64(ctx), P(rbuf.ctypes.data), I64(rbuf.nbytes))
        t = call(L.Java_io_vproxy_vpcsum_VPCsum_recvTcpFrames, I64(ctx), P(heap.ctypes.data), I64(heap.nbytes), P(desc.ctypes.data),
                 P(rx.ctypes.data), I32(n), P(rbuf.ctypes.data), I64(rbuf.nbytes), P(stored.ctypes.data), P(out.ctypes.data),
                 P(st.ctypes.data))
        call(L.Java_io_vproxy_vpcsum_VPCsum_waitFor, I64(ctx), I64(t))
        assert np.array_equal(stored, w_stored) and np.array_equal(out, w_out) and np.array_equal(st, w_st)
        assert np.array_equal(rbuf, want), first_diff(rbuf, want, rx)
        assert np.array_equal(heap, rb["arena"])
        env = Env()
        assert L.Java_io_vproxy_vpcsum_VPCsum_recvTcpFrames(ctypes.byref(env), I64(ctx), P(heap.ctypes.data), I64(heap.nbytes),
                                                            P(desc.ctypes.data), P(rx.ctypes.data), I32(-1), P(rbuf.ctypes.data),
                                                            I64(rbuf.nbytes), P(stored.ctypes.data), None, None) != 0
        assert env.type == b"java.lang.IllegalArgumentException" and env.message == b"recvTcpFrames: negative size"
    finally:
        call(L.Java_io_vproxy_vpcsum_VPCsum_close, I64(ctx))
