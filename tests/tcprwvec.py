"""TCP-header rewrites of NAT'd packets (VPCSUM_NAT_TCP entries, VPCSUM_NAT_TCP_REWRITES): the
reference's setters restated in Python, the expected bytes of a batch, and the crafted vectors.
Test infrastructure: tests/ only.

What the reference does to a NAT'd TCP packet in place besides SwitchUtils.applyNat:

* buildSynPacketForProxyProtocol (SwitchUtils.java:461-465): setSeqNum(seq - N).
* buildSynAckPacketForProxyProtocol (:467-473): setSeqNum(seq - 1), setFlags(SYN | ACK).
* checkAndUpdateMss (:46-95): on a SYN whose options parse, the first MSS option above maxMss is
  overwritten (TcpOption.setData, TcpPacket.java:561-569); without one the packet is rebuilt with
  the option added -- that branch stays on the host (S_MSS_ABSENT).

TcpPacket.setSeqNum (:57-63) and setFlags (:90-96) write and call checksumSkipped() whatever the
value; getRawPacket(0) then recomputes the TCP sum in full.
"""
from __future__ import annotations

import functools

import numpy as np

import hsumvec as H
from oracle import oracle as O

NAT_TCP, NAT_TCP_REWRITES, S_MSS_ABSENT = 0x40, 0x02, 0x08
SEQ_ADD, SET_FLAGS, CLAMP_MSS = 0x01, 0x02, 0x04
SYN, ACK, PSH = H.TCP_SYN, H.TCP_ACK, H.TCP_PSH
MAX_MSS = H.MAX_MSS


def fill(entry, ops: int, flags: int = 0, max_mss: int = 0, addend: int = 0):
    """The TCP part of one O.NAT_DTYPE entry, byte by byte as include/vpcsum.h lays it out."""
    entry["mask"] = int(entry["mask"]) | NAT_TCP
    entry["rsv"] = np.frombuffer(bytes([ops, flags]) + max_mss.to_bytes(2, "big") +
                                 (addend & 0xFFFFFFFF).to_bytes(4, "big") + b"\x00\x00", np.uint8)


def _first_mss(seg: bytes) -> int | None:
    """Offset of the first MSS option before any END, of options O._tcp_from accepted."""
    doff = (seg[12] >> 4) * 4
    o = 20
    while o < doff:
        k = seg[o]
        if k == O.TCP_OPTION_END:
            return None
        if k == O.TCP_OPTION_NOP:
            o += 1
        elif k == O.TCP_OPTION_MSS:
            return o
        else:
            o += seg[o + 1]
    return None


def java_tcp_rewrite(l3: bytearray, ver: int, proto: int, l3_len: int, l4_off: int, rw) -> tuple[bool, bool]:
    """The TCP setters of entry rw on the packet l3, in place; the sums are left alone.  Returns
    (dirty, absent): checksumSkipped() was called; a clamp found parsed options without MSS."""
    if not int(rw["mask"]) & NAT_TCP or proto != O.IP_PROTOCOL_TCP or l3_len - l4_off < 20:
        return False, False
    rsv = bytes(rw["rsv"])
    ops, flags = rsv[0], rsv[1]
    max_mss, addend = int.from_bytes(rsv[2:4], "big"), int.from_bytes(rsv[4:8], "big")
    t = l4_off
    dirty = absent = False
    if ops & SET_FLAGS:   # pktBuf.int16(12, (uint16(12) & 0xffc0) | (flags & 0x3f))
        w = (int.from_bytes(l3[t + 12:t + 14], "big") & 0xFFC0) | (flags & 0x3F)
        l3[t + 12:t + 14] = w.to_bytes(2, "big")
        dirty = True
    if ops & SEQ_ADD:     # pktBuf.int32(4, (int) seqNum)
        seq = (int.from_bytes(l3[t + 4:t + 8], "big") + addend) & 0xFFFFFFFF
        l3[t + 4:t + 8] = seq.to_bytes(4, "big")
        dirty = True
    if ops & CLAMP_MSS and l3[t + 13] & SYN:
        seg = bytes(l3[t:l3_len])
        if O._tcp_from(seg) is None:   # else ensurePartialPacketParsed makes Java return
            at = _first_mss(seg)
            if at is None:
                absent = True
            elif int.from_bytes(seg[at + 2:at + 4], "big") > max_mss:
                l3[t + at + 2:t + at + 4] = max_mss.to_bytes(2, "big")
                dirty = True
    return dirty, absent


def expected(orc, arena: np.ndarray, desc: np.ndarray, rw: np.ndarray):
    """(bytes, status) of the batch after NAT with the TCP rewrites, as Java leaves it: orc.nat_java
    for addresses, ports and TTL (it ignores mask bit 0x40), the TCP setters on every packet it did
    not refuse, and the full TCP sum where they dirtied it."""
    want = arena.copy()
    st = orc.nat_java(want, desc, rw)
    for i, d in enumerate(desc):
        if st[i] & O.S_BAD_DESC or not int(rw[i]["mask"]) & NAT_TCP:
            continue
        o, n, l4 = int(d["l3_off"]), int(d["l3_len"]), int(d["l4_off"])
        ver, proto = int(d["l3_ver"]), int(d["l4_proto"])
        l3 = bytearray(want[o:o + n].tobytes())
        dirty, absent = java_tcp_rewrite(l3, ver, proto, n, l4, rw[i])
        if dirty:
            l3[l4 + 16:l4 + 18] = O.l4_csum(bytes(l3), n, l4, ver, proto).to_bytes(2, "big")
        want[o:o + n] = np.frombuffer(bytes(l3), np.uint8)
        if absent:
            st[i] |= S_MSS_ABSENT
    return want, st


# ----------------------------------------------------------------------------------------
# Crafted vectors: the smallest shapes at which the rewrite can go wrong
# ----------------------------------------------------------------------------------------
def mss(v: int) -> bytes:
    return bytes([2, 4]) + v.to_bytes(2, "big")


NOP = b"\x01"
_received = functools.lru_cache(maxsize=2)(H.received)   # its frames are bytes: shared, never changed


def seg(rng, opts: bytes = b"", flags: int = SYN, payload: int = 6, doff: int | None = None, seq: int | None = None):
    """A TCP segment from hsumvec._tcp with `opts` (a multiple of 4 bytes) spliced in; doff: the data
    offset in bytes when it shall not match; random reserved bits in word 12 (setFlags keeps them)."""
    assert len(opts) % 4 == 0
    s = H._tcp(rng, payload, True, None, 0)
    s = s[:20] + bytearray(opts) + s[20:]
    s[12] = (((20 + len(opts) if doff is None else doff) // 4) << 4) | int(rng.integers(0, 16))
    s[13] = flags | (int(rng.integers(0, 4)) << 6)
    if seq is not None:
        s[4:8] = seq.to_bytes(4, "big")
    return s


def l3_sums(l3: bytearray, ver: int, proto: int, l4_off: int) -> bytearray:
    """Valid IPv4 header and L4 sums (hsumvec.with_sums for a bare L3 packet of known layout; it
    also takes the short and malformed segments parse_ether refuses)."""
    l3 = bytearray(l3)
    if ver == 4:
        l3[10:12] = O.ipv4_header_csum(bytes(l3), l4_off).to_bytes(2, "big")
    fld = O.L4_FIELD.get(proto)
    if fld is not None and len(l3) - l4_off >= fld + 2:
        l3[l4_off + fld:l4_off + fld + 2] = O.l4_csum(bytes(l3), len(l3), l4_off, ver, proto).to_bytes(2, "big")
    return l3


def _vec(name, rng, s, ops, want, ver=4, proto=6, ihl=5, ext=None, flags=0, max_mss=MAX_MSS, addend=0,
         nat=None, ttl=None, bad=False, l3_prefix=0):
    """want: {tcp offset: bytes} the setters write (hand-checked), plus "dirty" / "absent"."""
    l3 = H._l3(rng, ver, s, proto, ihl=ihl, ext=ext)
    l4_off = ihl * 4 if ver == 4 else 40 + (0 if ext is None else 8 + ext)
    if ttl is not None:
        l3[8 if ver == 4 else 7] = ttl
    l3 = l3_sums(l3, ver, proto, l4_off)
    rw = np.zeros(1, O.NAT_DTYPE)
    rw.view(np.uint8)[:38] = rng.integers(0, 256, 38, dtype=np.uint8)
    rw["mask"] = int(rng.integers(0, 16)) if nat is None else nat   # addresses / ports next to the TCP ops
    fill(rw[0], ops, flags, max_mss, addend)
    return dict(name=name, l3=bytes(l3), ver=ver, proto=proto, l4_off=l4_off, rw=rw[0], bad=bad, l3_prefix=l3_prefix,
                dirty=want.pop("dirty", False), absent=want.pop("absent", False), writes=want)


def _tune_sum(v, orc, incoming: bool):
    """Set the first payload word of vector v (0 so far) so that the stored TCP sum comes out 0x0000
    -- incoming, or after the rewrite: adding the word c to a segment whose sum field is c = ~S
    makes the one's complement total 0xffff, its complement 0."""
    l3 = bytearray(v["l3"])
    t = v["l4_off"]
    p = t + (l3[t + 12] >> 4) * 4
    assert l3[p:p + 2] == b"\x00\x00"
    if incoming:
        c = l3[t + 16:t + 18]
    else:
        arena = np.frombuffer(bytes(l3), np.uint8).copy()
        d = np.array([(0, len(l3), t, v["ver"], v["proto"], 0, 0)], O.DESC_DTYPE)
        got, _ = expected(orc, arena, d, np.array([v["rw"]]))
        c = got[t + 16:t + 18].tobytes()
    l3[p:p + 2] = c
    v["l3"] = bytes(l3_sums(l3, v["ver"], v["proto"], t))
    return v


def crafted(orc, seed: int = 21) -> list[dict]:
    rng = np.random.default_rng(seed)
    C, M = CLAMP_MSS, MAX_MSS
    clamp = {"dirty": True}
    hi = M.to_bytes(2, "big")
    V = []

    def add(name, s, ops=C, want=None, **kw):
        V.append(_vec(name, rng, s, ops, dict(want or {}), **kw))

    # MSS option position (the option at TCP offset `at`: its data at at + 2)
    add("mss_first", seg(rng, mss(1460)), want={22: hi, **clamp})
    add("mss_after_1_nop", seg(rng, NOP + mss(1460) + NOP * 3), want={23: hi, **clamp})
    add("mss_after_2_nops", seg(rng, NOP * 2 + mss(1460) + NOP * 2), want={24: hi, **clamp})
    add("mss_after_3_nops", seg(rng, NOP * 3 + mss(1460) + NOP), want={25: hi, **clamp})
    add("mss_after_sack_permitted", seg(rng, b"\x04\x02" + mss(1460) + NOP * 2), want={24: hi, **clamp})
    add("mss_after_timestamps", seg(rng, b"\x08\x0a" + bytes(range(8)) + mss(1460) + NOP * 2), want={32: hi, **clamp})
    add("mss_after_window_scale", seg(rng, b"\x03\x03\x07" + mss(1460) + NOP), want={25: hi, **clamp})
    add("mss_at_56_doff_15", seg(rng, NOP * 36 + mss(1460)), want={58: hi, **clamp})
    add("mss_after_end", seg(rng, b"\x00" + mss(1460) + NOP * 3), want={"absent": True})
    add("mss_twice", seg(rng, mss(1460) + mss(9000)), want={22: hi, **clamp})
    # MSS value against maxMss
    add("mss_equal", seg(rng, mss(M)))
    add("mss_plus_1", seg(rng, mss(M + 1)), want={22: hi, **clamp})
    add("max_mss_0_above", seg(rng, mss(1)), max_mss=0, want={22: b"\x00\x00", **clamp})
    add("max_mss_0_equal", seg(rng, mss(0)), max_mss=0)
    add("max_mss_ffff", seg(rng, mss(0xFFFF)), max_mss=0xFFFF)
    add("no_options", seg(rng), want={"absent": True})
    add("nops_only", seg(rng, NOP * 4), want={"absent": True})
    # malformed options: the walk fails, nothing happens (no S_MSS_ABSENT either)
    add("bad_doff_past_segment", seg(rng, payload=4, doff=60))
    add("bad_option_len_0", seg(rng, b"\x05\x00" + NOP * 2 + mss(1460)))
    add("bad_option_len_1", seg(rng, b"\x05\x01" + NOP * 2 + mss(1460)))
    add("bad_option_len_past_doff", seg(rng, mss(1460) + b"\x05\x0c" + NOP * 2))
    add("bad_mss_len_3", seg(rng, b"\x02\x03\x05" + NOP))
    add("bad_window_scale_len_4", seg(rng, mss(1460) + b"\x03\x04" + NOP * 2))
    add("bad_kind_in_last_byte", seg(rng, NOP * 3 + b"\x05"))
    # data offsets under 20: no walk, no options: absent
    add("doff_0", seg(rng, doff=0), want={"absent": True})
    add("doff_4", seg(rng, doff=4), want={"absent": True})
    add("doff_16", seg(rng, doff=16), want={"absent": True})
    # flags and protocols
    add("clamp_without_syn", seg(rng, mss(1460), flags=ACK))
    add("set_flags_creates_syn", seg(rng, mss(1460), flags=ACK), ops=C | SET_FLAGS, flags=SYN | ACK,
        want={13: None, 22: hi, **clamp})
    add("set_flags_clears_syn", seg(rng, mss(1460), flags=SYN), ops=C | SET_FLAGS, flags=ACK, want={13: None, **clamp})
    add("udp_ignored", H._udp(rng, 30), ops=7, proto=17, flags=0x3F, addend=5)
    add("icmp_ignored", bytearray(rng.integers(0, 256, 40, dtype=np.uint8).tobytes()), ops=7, proto=1, flags=0x3F, addend=5)
    add("icmpv6_ignored", bytearray(rng.integers(0, 256, 40, dtype=np.uint8).tobytes()), ops=7, proto=58, ver=6,
        flags=0x3F, addend=5)
    add("tcp_19_bytes_ignored", seg(rng, flags=SYN, payload=0)[:19], ops=7, flags=0x3F, addend=5)
    add("tcp_20_bytes", seg(rng, flags=SYN, payload=0, seq=7), ops=7, flags=SYN | ACK, addend=5,
        want={4: b"\x00\x00\x00\x0c", 13: None, "dirty": True, "absent": True})
    # SEQ_ADD
    add("seq_add_0", seg(rng, flags=ACK, seq=0x01020304), ops=SEQ_ADD, addend=0, want={4: b"\x01\x02\x03\x04", **clamp})
    add("seq_0_minus_1", seg(rng, flags=ACK, seq=0), ops=SEQ_ADD, addend=0xFFFFFFFF, want={4: b"\xff" * 4, **clamp})
    add("seq_ffffffff_plus_1", seg(rng, flags=ACK, seq=0xFFFFFFFF), ops=SEQ_ADD, addend=1, want={4: bytes(4), **clamp})
    add("proxy_syn", seg(rng, mss(1460), flags=SYN, seq=1000), ops=SEQ_ADD | C, addend=-H.PP_V2_LEN,
        want={4: (1000 - H.PP_V2_LEN).to_bytes(4, "big"), 22: hi, **clamp})
    add("proxy_synack", seg(rng, mss(1200), flags=ACK, seq=0), ops=7, flags=SYN | ACK, addend=-1,
        want={4: b"\xff" * 4, 13: None, **clamp})
    # checksum edges: the stored TCP sum 0x0000 after the rewrite / before it
    s0 = seg(rng, mss(1460), flags=SYN, payload=8)
    s0[24:26] = b"\x00\x00"
    add("sum_becomes_0000", s0, ops=7, flags=SYN, addend=77, want={4: None, 13: None, 22: hi, **clamp})
    _tune_sum(V[-1], orc, incoming=False)
    s0 = seg(rng, mss(1460), flags=SYN, payload=8)
    s0[24:26] = b"\x00\x00"
    add("sum_was_0000", s0, ops=7, flags=SYN, addend=77, want={4: None, 13: None, 22: hi, **clamp})
    _tune_sum(V[-1], orc, incoming=True)
    # header reach
    add("ipv4_ihl_15", seg(rng, NOP * 36 + mss(1460)), ihl=15, want={58: hi, **clamp})
    add("ipv6_mss_at_l3_110", seg(rng, NOP * 36 + mss(1460)), ver=6, ext=4, want={58: hi, **clamp})
    add("ipv6_no_ext", seg(rng, NOP + mss(1460) + NOP * 3), ver=6, ops=7, flags=SYN, addend=3,
        want={4: None, 13: None, 23: hi, **clamp})
    add("dot1q_offset", seg(rng, mss(1460)), l3_prefix=18, want={22: hi, **clamp})
    # refused by the first pass: untouched, status as without the TCP ops
    add("ttl_expired", seg(rng, mss(1460), seq=9), ops=7, flags=SYN, addend=1, nat=O.NAT_DEC_TTL | O.NAT_SRC, ttl=1)
    add("outside_arena", seg(rng, mss(1460), seq=9), ops=7, flags=SYN, addend=1, bad=True)
    assert {v["name"]: v for v in V}["ipv6_mss_at_l3_110"]["l4_off"] + 58 == 110
    return V


def pack(vecs: list[dict], pad: int | None):
    """(arena, desc, rw).  pad 0..15: every L3 header at 16k + pad; None: the packets back to back
    with gaps of 0..3 bytes.  A `bad` vector gets a descriptor reaching past the arena's end."""
    offs, pos = [], 0
    for i, v in enumerate(vecs):
        if v["bad"]:
            offs.append(None)
            continue
        if pad is not None:
            pos = (pos + 15) // 16 * 16 + pad
        else:
            pos += i % 4
        if v["l3_prefix"]:   # an Ethernet + 802.1Q header before L3 (hsumvec.ether)
            pos += v["l3_prefix"]
        offs.append(pos)
        pos += len(v["l3"])
    arena = np.random.default_rng(1).integers(0, 256, pos + 5, dtype=np.uint8)
    rows = []
    for v, o in zip(vecs, offs):
        if o is None:
            o = len(arena) - 10
        else:
            if v["l3_prefix"]:
                f = H.ether(np.random.default_rng(2), v["l3"], v["ver"], True)
                assert len(f) >= 18 + len(v["l3"]) and f[18:18 + len(v["l3"])] == v["l3"]
                arena[o - 18:o] = np.frombuffer(f[:18], np.uint8)
            arena[o:o + len(v["l3"])] = np.frombuffer(v["l3"], np.uint8)
        rows.append((o, len(v["l3"]), v["l4_off"], v["ver"], v["proto"], 0, 0))
    return arena, np.array(rows, O.DESC_DTYPE), np.array([v["rw"] for v in vecs], O.NAT_DTYPE)


def received_batch(n: int, seed: int = 11, corrupt: float = 0.0):
    """(arena, desc, rw, corrupted) of the first n frames of hsumvec.received(seed, 512) in umem
    chunks: every TCP entry carries random TCP ops next to random NAT bits; `corrupt`: that share
    of the frames gets a payload byte changed after its sums were taken."""
    fs = _received(seed, 512)[:n]
    arena, offs, _ = H.layout(fs, 0)
    rng = np.random.default_rng(seed * 1000 + n)
    rows, bad = [], np.zeros(n, bool)
    rw = np.zeros(n, O.NAT_DTYPE)
    rw.view(np.uint8).reshape(n, 48)[:, :38] = rng.integers(0, 256, (n, 38), dtype=np.uint8)
    rw["mask"] = rng.integers(0, 64, n)
    for i, (f, fo) in enumerate(zip(fs, offs)):
        info = H.frame_l3(f["frame"])
        o = fo + info.l3_off
        rows.append((o, info.l3_len, info.l4_off, info.ver, info.proto, 0, 0))
        bad[i] = f["corrupt"]
        body = info.l3_len - info.l4_off - 60
        if corrupt and body > 0 and rng.random() < corrupt and not f["udp0"]:
            arena[o + info.l4_off + 60 + int(rng.integers(0, body))] ^= 0xA5
            bad[i] = True
        if info.proto == 6:
            fill(rw[i], int(rng.integers(0, 8)), int(rng.integers(0, 64)),
                 MAX_MSS if rng.random() < 0.8 else int(rng.integers(0, 65536)),
                 int(rng.integers(0, 1 << 32)) if rng.random() < 0.7 else -H.PP_V2_LEN)
        elif rng.random() < 0.5:   # the bit on a UDP entry: ignored
            fill(rw[i], 7, 0x3F, 0, 1)
    return arena, np.array(rows, O.DESC_DTYPE), rw, bad
