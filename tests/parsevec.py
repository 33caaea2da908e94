"""The frame parse's geometry batch (test infrastructure: tests/ only; pure Python and numpy).

tests/edgevec.py:parse_cases() holds the parse *rules* to their edges.  This batch holds the two
compiled shapes of the parse -- k_parse_ether (one lane per frame, reading the arena) and
svc_frame_packet (one wave per frame, its first min(L, 384) bytes staged in LDS at the frame
address's residue mod 16) -- to the edges of their *geometry*: the 384-byte window, the address
residues, the bounds check and the batch sizes.  Every expectation comes from the restatements in
oracle/oracle.py (parse_ether, desc_flags_for, flow_tuple, hsum_record); nothing here is derived
from the kernels.

Classes (batch()["cls"]), in the order they lie in the batch:

* bounds   -- waves of 64 frames whose lanes 0, 1, 31, 32 and 63 hold one bounds case each (a frame
              one byte past the arena, at its end, at an offset whose sum wraps, of length
              0xffffffff; in-bounds frames cut to 0 / 13 / 14 / 17 / 18 / 33 / 34 / 53 / 54 bytes),
              the other lanes good frames.
* rules@r  -- every frame of edgevec.parse_cases() at every address residue r = 0..15.
* deep     -- Ethernet and 802.1Q x IPv6 with one extension header (8 + hdrExtLen bytes, the
              reference's ExtHeader.from rule) x L4: hdrExtLen up to 255 and a 60-byte TCP header put
              the last byte the rules read at frame offset 380, the window's edge.  Each accepted
              frame has refused twins that differ in one byte among the last 16 the rules read.
* v4       -- IHL 5..15 x TCP / UDP / ICMP x Ethernet / 802.1Q, the L4 header on every address mod
              4, 0..3 bytes of Ethernet padding after totalLength.
* egress   -- every flag byte of EGRESS_FLAGS over every kind of accepted frame, the segments too
              short to hold a checksum field included.
* last     -- a deep frame, then a plain one that ends on the arena's last byte; the arena cut after
              the deep frame (batch()["cut_n"], ["cut_len"]) is a batch whose last frame is deep.

Frames lie back to back with GUARD bytes of FILL around each, the first byte of each at a wanted
residue mod 16.  Three of every four accepted frames carry correct checksums, so that a verify has
both verdicts to give.
"""
from __future__ import annotations

import functools

import numpy as np

import edgevec as E
from oracle import oracle as O

FILL, GUARD = 0xA5, 3
WINDOW = 384                       # bytes of a frame the service grid stages (kernels.hip)
H_ALL = (0, 1, 2, 3, 7, 8, 9, 246, 247, 248, 253, 254, 255)
H_DEEP = tuple(h for h in H_ALL if h >= 246)
L4_KINDS = ("tcp5", "tcp15nop", "tcp15ts", "udp", "icmp6", "nonext")
DEEP_LENS = (383, 384, 385, 700, 1514)
# every byte below 8, F_L4P alone, a bit no flag has, and F_L4P beside F_IP / F_L4 / both (0x0a: F_L4 with F_L4P)
EGRESS_FLAGS = tuple(range(8)) + (0x08, 0x80, 0x09, 0x0A, 0x0B)
BOUNDS_LANES = (0, 1, 31, 32, 63)
TUPLE_DTYPE = np.dtype([("src", "u1", 16), ("dst", "u1", 16), ("sport", "u1", 2), ("dport", "u1", 2),
                        ("l3_ver", "u1"), ("l4_proto", "u1"), ("tcp_flags", "u1"), ("rsv", "u1")])
assert TUPLE_DTYPE.itemsize == 40

# NOP x 38, NOP, END: the walk ends on the header's last byte
TCP15_NOP = bytes([1] * 39 + [0])
# MSS, NOP, window scale, timestamps, NOP NOP, SACK (18), SACK permitted: the last option's length
# byte is the header's last byte
TCP15_TS = bytes([2, 4, 5, 0xB4, 1, 3, 3, 7, 8, 10]) + bytes(range(8)) + bytes([1, 1, 5, 18]) + bytes(range(16)) + \
    bytes([4, 2])
assert len(TCP15_NOP) == 40 and len(TCP15_TS) == 40


def _u16(b, o):
    return (b[o] << 8) | b[o + 1]


def _put16(b, o, v):
    b[o], b[o + 1] = (v >> 8) & 0xFF, v & 0xFF


def _rnd(rng, n, lo=0):
    return rng.integers(lo, 256, n, dtype=np.uint8).tobytes()


# ------------------------------------------------------------------------------------------
# reach: how far into a frame the parse rules look
# ------------------------------------------------------------------------------------------
def _reach_tcp_from(seg: bytes, l4: int, need) -> bool:
    """TcpPacket.from (TcpPacket.java:223-287) and TcpOption.from / check (:602-640)."""
    if len(seg) < 20:
        return False
    need(l4 + 13)                       # the data offset nibble
    doff = (seg[12] >> 4) * 4
    if doff > len(seg):
        return False
    off = 20
    while doff > 20 and off < doff:
        need(l4 + off + 1)              # the option's kind
        kind = seg[off]
        if kind in (O.TCP_OPTION_END, O.TCP_OPTION_NOP):
            off += 1
            if kind == O.TCP_OPTION_END:
                break
            continue
        if off + 1 >= doff:
            return False
        need(l4 + off + 2)              # its length
        ln = seg[off + 1]
        if off + ln > doff or ln < 2:
            return False
        if (kind == O.TCP_OPTION_WINDOW_SCALE and ln != 3) or (kind == O.TCP_OPTION_MSS and ln != 4):
            return False
        off += ln
    return True


def _reach_etherip(seg: bytes, l4: int, need) -> bool:
    """EtherIPPacket.initPartial / from (EtherIPPacket.java:32-71), ArpPacket.from (ArpPacket.java:22-70)."""
    if len(seg) < 2 or len(seg) - 2 < 14:
        return False
    inner, hl = seg[2:], 14
    need(l4 + 2 + 14)
    typ = _u16(inner, 12)
    if typ == O.ETHER_TYPE_8021Q:
        if len(inner) < 18:
            return False
        need(l4 + 2 + 18)
        typ, hl = _u16(inner, 16), 18
    if typ == O.ETHER_TYPE_ARP:
        a = inner[hl:]
        if len(a) < 8:
            return False
        need(l4 + 2 + hl + 6)           # hardware and protocol address sizes
        if len(a) < 8 + 2 * (a[4] + a[5]):
            return False
    return True


def _reach_l4(partial: bool, ver: int, proto: int, seg: bytes, l4: int, need) -> bool:
    """The upper-layer packet: initPartial (TcpPacket.java:187-199, UdpPacket.java:17-27,
    IcmpPacket.java:22-26: lengths alone decide) or the full from() (UdpPacket.java:40-60: the
    length field; IcmpPacket.java:33-45)."""
    if proto == O.IP_PROTOCOL_TCP:
        return len(seg) >= 20 if partial else _reach_tcp_from(seg, l4, need)
    if proto == O.IP_PROTOCOL_UDP:
        if len(seg) < 8:
            return False
        if partial:
            return True
        need(l4 + 6)                    # the length field
        return _u16(seg, 4) == len(seg)
    if proto == O.IP_PROTOCOL_ICMP or (ver == 6 and proto == O.IP_PROTOCOL_ICMPv6):
        return len(seg) >= (1 if partial else 8)
    if proto == O.IP_PROTOCOL_ETHERIP:
        return _reach_etherip(seg, l4, need)
    return True


def reach(frame: bytes) -> int:
    """How many leading bytes of `frame` the parse rules need to decide and describe it: one more
    than the largest frame offset read (0: the length alone decides).  Restated from the rules as
    oracle/oracle.py states them, not from a kernel: the EtherType and the 802.1Q tag
    (EthernetPacket.from, EthernetPacket.java:25-94); IHL, totalLength and the protocol
    (Ipv4Packet.initPartial, Ipv4Packet.java:29-63); the next header and payloadLength
    (Ipv6Packet.initPartial, Ipv6Packet.java:26-59) and, behind an extension header, the version
    nibble and the header's two bytes (Ipv6Packet.from, Ipv6Packet.java:69-159; ExtHeader.from: 8 +
    hdrExtLen bytes); the L4 initPartial or from(); then, for an accepted frame, what describes it:
    the tuple's addresses (Ipv4Packet.java:51-54, Ipv6Packet.java:47-50), ports and TCP flags
    (TcpPacket.java:192-195, UdpPacket.java:22-23), and the header sum's words (oracle.hdr_words:
    the addresses and the L4 header up to the data offset)."""
    f = bytes(frame)
    r = 0

    def need(end):
        nonlocal r
        r = max(r, end)

    if len(f) < 14:
        return r
    need(14)
    typ, hl = _u16(f, 12), 14
    if typ == O.ETHER_TYPE_8021Q:
        if len(f) < 18:
            return r
        need(18)
        typ, hl = _u16(f, 16), 18
    b = f[hl:]
    if typ == O.ETHER_TYPE_IPv4:
        if len(b) < 20:
            return r
        need(hl + 4)                    # IHL, totalLength
        ihl, total = b[0] & 15, _u16(b, 2)
        if len(b) < ihl * 4 or ihl < 5 or total < ihl * 4 or total > len(b):
            return r
        need(hl + 10)                   # the protocol
        ver, proto, l4 = 4, b[9], hl + ihl * 4
        seg = b[ihl * 4:total]
        if not _reach_l4(True, 4, proto, seg, l4, need):
            return r
        need(hl + 20)                   # the addresses
    elif typ == O.ETHER_TYPE_IPv6:
        if len(b) < 40:
            return r
        need(hl + 7)                    # payloadLength, next header
        pl, nh = _u16(b, 4), b[6]
        ver, proto, l4o = 6, nh, 40
        if nh in O.IPv6_needs_next_header:
            need(hl + 1)                # from() checks the version
            if b[0] >> 4 != 6 or pl == 0 or 40 + pl > len(b):
                return r
            if pl < 8:
                return r
            need(hl + 42)               # the extension header's next header and hdrExtLen
            if pl < 8 + b[41] or b[40] in O.IPv6_needs_next_header:
                return r
            proto, l4o = b[40], 48 + b[41]
            seg = b[l4o:40 + pl]
            if proto == O.IPv6_NO_NEXT_HEADER and len(seg):
                return r
            if not _reach_l4(False, 6, proto, seg, hl + l4o, need):
                return r
        else:
            if pl == 0 or 40 + pl > len(b):
                return r
            seg = b[40:40 + pl]
            if not _reach_l4(True, 6, proto, seg, hl + 40, need):
                return r
        l4 = hl + l4o
        need(hl + 40)                   # the addresses
    else:
        return r
    if proto in (O.IP_PROTOCOL_TCP, O.IP_PROTOCOL_UDP):
        need(l4 + 4)                    # the ports
    if proto == O.IP_PROTOCOL_TCP:
        need(l4 + 14)                   # uint16 at 12: the data offset and the flags
        hlen = (seg[12] >> 4) * 4
        if 20 <= hlen <= len(seg):
            need(l4 + hlen)             # the header sum covers the whole header
    elif proto == O.IP_PROTOCOL_UDP:
        need(l4 + 8)
    return r


# ------------------------------------------------------------------------------------------
# the flag rules
# ------------------------------------------------------------------------------------------
def ingress_flags(info: O.L3Info, want: int) -> int:
    """The flags of a received frame's descriptor for the caller's `want` (vpcsum.h
    vpcsum_parse_ether_async): those of the sums asked that the frame allows
    (oracle.desc_flags_for); F_L4P where F_L4 is not asked, not for ICMPv4, which has no pseudo
    header (IcmpPacket.java:64-74)."""
    allowed = O.desc_flags_for(info)
    fl = want & allowed & (O.F_IP | O.F_L4)
    if not fl & O.F_L4 and want & O.F_L4P and allowed & O.F_L4 and info.proto != O.IP_PROTOCOL_ICMP:
        fl |= O.F_L4P
    return fl


def egress_honoured(info: O.L3Info, w: int) -> bool:
    """Whether an egress frame's own flag byte can be honoured in full (vpcsum.h
    vpcsum_ctx_egress_frames): nothing but F_IP / F_L4 / F_L4P, not F_L4 with F_L4P, F_IP on IPv4
    only, an L4 sum only where the segment holds the field, F_L4P not for ICMPv4."""
    if w & ~(O.F_IP | O.F_L4 | O.F_L4P) or (w & O.F_L4 and w & O.F_L4P):
        return False
    return ingress_flags(info, w) == w


# ------------------------------------------------------------------------------------------
# frames
# ------------------------------------------------------------------------------------------
def _eth(rng, vlan: bool, v6: bool) -> bytes:
    et = b"\x86\xdd" if v6 else b"\x08\x00"
    return _rnd(rng, 12) + ((b"\x81\x00" + _rnd(rng, 2) + et) if vlan else et)


def _fold(b: bytes) -> int:
    a = np.frombuffer(b + (b"\0" if len(b) & 1 else b""), dtype=">u2")
    s = int(a.sum(dtype=np.uint64))
    while s > 0xFFFF:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def with_sums(frame: bytes) -> bytes:
    """`frame` with correct checksums where the oracle's parse finds fields for them (the IPv4
    header's, the L4 segment's): no byte the parse rules read changes."""
    info, _ = O.parse_ether(frame)
    if info is None:
        return frame
    f = bytearray(frame)
    l3 = f[info.l3_off:info.l3_off + info.l3_len]
    fl = O.desc_flags_for(info)
    if fl & O.F_IP:
        l3[10:12] = b"\0\0"
        _put16(l3, 10, 0xFFFF - _fold(bytes(l3[:info.l4_off])))
    if fl & O.F_L4:
        fld = info.l4_off + O.L4_FIELD[info.proto]
        l3[fld:fld + 2] = b"\0\0"
        seg = bytes(l3[info.l4_off:])
        if info.proto == O.IP_PROTOCOL_ICMP:
            ph = b""
        else:
            ph = O.pseudo_ipv4(l3, info.proto, len(seg)) if info.ver == 4 else O.pseudo_ipv6(l3, info.proto, len(seg))
        c = 0xFFFF - _fold(ph + seg)
        _put16(l3, fld, 0xFFFF if info.proto == O.IP_PROTOCOL_UDP and c == 0 else c)
    f[info.l3_off:info.l3_off + info.l3_len] = l3
    return bytes(f)


def deep_frame(rng, vlan: bool, h: int, kind: str, flen: int | None = None) -> bytes:
    """Ethernet / 802.1Q, IPv6, one extension header of 8 + h bytes, the L4 header of `kind`, and
    bytes up to a frame of `flen` (None: none): payload for TCP and UDP, Ethernet padding behind an
    8-byte ICMPv6 message or an empty no-next-header packet."""
    if kind == "tcp5":
        proto, l4 = 6, bytearray(_rnd(rng, 20))
        l4[12] = 0x50
    elif kind in ("tcp15nop", "tcp15ts"):
        proto, l4 = 6, bytearray(_rnd(rng, 60))
        l4[12] = 0xF0
        l4[20:60] = TCP15_NOP if kind == "tcp15nop" else TCP15_TS
    elif kind == "udp":
        proto, l4 = 17, bytearray(_rnd(rng, 8))
    elif kind == "icmp6":
        proto, l4 = 58, bytearray(_rnd(rng, 8))
    else:
        proto, l4 = O.IPv6_NO_NEXT_HEADER, bytearray()
    eth = _eth(rng, vlan, True)
    end = len(eth) + 48 + h + len(l4)
    extra = 0 if flen is None else flen - end
    assert extra >= 0
    payload = extra if proto in (6, 17) else 0
    if kind == "udp":
        _put16(l4, 4, 8 + payload)
    ip = bytearray(_rnd(rng, 40))
    ip[0] = 0x60 | (ip[0] & 0x0F)
    _put16(ip, 4, 8 + h + len(l4) + payload)
    ip[6] = E.V6_EXT_TYPES[h % 4]
    xh = bytearray(_rnd(rng, 8 + h))
    xh[0], xh[1] = proto, h
    data = bytearray(_rnd(rng, payload))
    if kind == "tcp5" and payload >= 4:
        data[0:2] = bytes([5, 1])      # an option of length 1 to the twin whose data offset is 6
    return eth + bytes(ip) + bytes(xh) + bytes(l4) + bytes(data) + _rnd(rng, extra - payload, lo=1)


def twins(frame: bytes, kind: str) -> list[tuple[str, bytes]]:
    """The refused twins of an accepted deep frame: each differs from it in one byte among the
    last 16 the rules read, and the full parse behind the extension header refuses it (TcpPacket.from
    and TcpOption, TcpPacket.java:223-287, 602-640; UdpPacket.from, UdpPacket.java:40-60; the
    extension header and IPv6_NO_NEXT_HEADER rules of Ipv6Packet.from, Ipv6Packet.java:69-159)."""
    info, _ = O.parse_ether(frame)
    l4 = info.l3_off + info.l4_off
    seg = info.l3_len - info.l4_off
    out = []

    def mut(name, at, v):
        f = bytearray(frame)
        assert f[at] != v
        f[at] = v
        out.append((name, bytes(f)))

    if kind == "tcp15nop":
        mut("optlen", l4 + 58, 5)      # an option whose length byte is the END at the last byte: 0
        mut("kindlast", l4 + 59, 5)    # an option kind on the header's last byte
    elif kind == "tcp15ts":
        mut("optlen", l4 + 59, 1)      # an option of length 1 at the last option position
        mut("kindlast", l4 + 58, 1)    # NOP: the walk meets the 2 on the last byte as a kind
    elif kind == "tcp5" and seg < 60:
        mut("doffpast", l4 + 12, (seg // 4 + 1) << 4)   # data offset one word past the segment
    elif kind == "tcp5":
        assert frame[l4 + 20:l4 + 22] == bytes([5, 1])
        mut("doffopt", l4 + 12, 0x60)  # data offset 6: the payload's first word is an option of length 1
    elif kind == "udp":
        mut("udplen", l4 + 5, frame[l4 + 5] ^ 1)        # the length field off by one
    elif kind == "icmp6":
        mut("nexthdr", info.l3_off + 40, O.IPv6_NO_NEXT_HEADER)   # no next header, with 8 bytes behind it
    else:   # hdrExtLen one less: a byte behind a no-next-header; 0 -> 1: the header ends past the payload
        h = frame[info.l3_off + 41]
        mut("hdrext", info.l3_off + 41, h - 1 if h else 1)
    return out


def _v4_frame(rng, vlan: bool, ihl: int, proto: int, l4len: int, pad: int = 0) -> bytes:
    p, hl = E._v4(rng, proto, l4len, ihl)
    return _eth(rng, vlan, False) + bytes(p) + _rnd(rng, pad, lo=1)


def _v6_frame(rng, vlan: bool, proto: int, l4len: int, pad: int = 0) -> bytes:
    p, _ = E._v6(rng, proto, l4len)
    return _eth(rng, vlan, True) + bytes(p) + _rnd(rng, pad, lo=1)


def _good(rng, i: int) -> bytes:
    """A small accepted frame for the lanes beside a bounds case."""
    k = i % 4
    if k == 0:
        return _v4_frame(rng, False, 5, 6, 20 + i % 7)
    if k == 1:
        return _v6_frame(rng, bool(i & 4), 17, 8 + i % 5)
    if k == 2:
        return _v4_frame(rng, True, 5 + i % 3, 17, 8 + i % 9)
    return _v6_frame(rng, False, 6, 20 + i % 3)


def _records(seed: int) -> list[dict]:
    """The batch's frames in order: {frame, cls, res (address residue, None: where it falls), L (the
    frame table's length, None: the frame's), at (an offset given relative to the arena's end: a
    function of arena_len), flag (the egress flag byte, None: one the frame can honour)}."""
    rng = np.random.default_rng(seed)
    recs = []

    def add(frame, cls, res=None, L=None, at=None, flag=None, **kw):
        recs.append(dict(frame=frame, cls=cls, res=res, L=L, at=at, flag=flag, **kw))

    # ---- bounds: one case on lanes 0, 1, 31, 32, 63 of a wave of good frames
    v4t, v4q, v6t = _v4_frame(rng, False, 5, 6, 20), _v4_frame(rng, True, 5, 6, 20), _v6_frame(rng, False, 6, 20)
    assert (len(v4t), len(v4q), len(v6t)) == (54, 58, 74)
    cases = [("end+1", dict(at=lambda n: n + 1 - 60, L=60)),
             ("o=end,L=0", dict(at=lambda n: n, L=0)),
             ("o=end,L=14", dict(at=lambda n: n, L=14)),
             ("o=end+1", dict(at=lambda n: n + 1, L=14)),
             ("o=2^64-1,L=2", dict(at=lambda n: 2 ** 64 - 1, L=2)),
             ("o=0,L=2^32-1", dict(at=lambda n: 0, L=0xFFFFFFFF))]
    cases += [(f"L={L}", dict(frame=v4t, L=L)) for L in (0, 13, 14, 18, 33, 34, 53, 54)]
    cases += [(f"802.1q L={L}", dict(frame=v4q, L=L)) for L in (17, 18, 57, 58)]
    cases += [(f"ipv6 L={L}", dict(frame=v6t, L=L)) for L in (53, 54, 73, 74)]
    for w, (name, c) in enumerate(cases):
        for lane in range(64):
            if lane in BOUNDS_LANES:
                add(c.get("frame", b""), "bounds", res=(w + lane) % 16 if "frame" in c else None, L=c["L"],
                    at=c.get("at"), case=name)
            else:
                add(_good(rng, w * 64 + lane), "bounds", res=(w * 5 + lane) % 16, case="good")
    # ---- rules@r
    for r in range(16):
        for f, _, why in E.parse_cases():
            add(f, f"rules@{r}", res=r, case=why)
    # ---- deep
    k = j = 0

    def deep(vlan, h, kind, res, flen=None):
        f = deep_frame(rng, vlan, h, kind, flen)
        add(f, "deep", res=res, case=(vlan, h, kind, flen), twin=None)
        base = len(recs) - 1
        for name, t in twins(f, kind):   # cut again in batch(), from the frame as it lies in the arena
            add(t, "deep", res=res, case=(vlan, h, kind, flen), twin=name, of=base)

    for vlan in (False, True):
        for h in H_ALL:
            if h < 246:
                for kind in L4_KINDS:
                    # no payload behind the TCP headers (the data-offset twin needs a short segment);
                    # the others ramp the frame length through the staged chunk counts
                    hdr = (18 if vlan else 14) + 48 + h + {"udp": 8, "icmp6": 8, "nonext": 0}.get(kind, 0)
                    if kind.startswith("tcp"):
                        deep(vlan, h, kind, (k * 7) % 16)
                    else:   # residue and length together step by 9: no chunk count is skipped
                        deep(vlan, h, kind, j % 16, max(hdr, 70 + 8 * j))
                    k += 1
                    j += not kind.startswith("tcp")
                continue
            for res in range(16):
                for kind in L4_KINDS:
                    deep(vlan, h, kind, res)
            for flen in DEEP_LENS:
                for kind in L4_KINDS:
                    deep(vlan, h, kind, (k * 5) % 16, flen)
                    k += 1
    # ---- v4: the L4 header on every address mod 4, 0..3 bytes of padding
    k = 0
    for vlan in (False, True):
        hl = 18 if vlan else 14
        for ihl in range(5, 16):
            for proto in (6, 17, 1):
                for m in range(4):
                    for pad in range(4):
                        res = (m - hl - ihl * 4) % 4 + 4 * (k % 4)
                        l4len = (20 if proto == 6 else 8) + k % 23
                        add(_v4_frame(rng, vlan, ihl, proto, l4len, pad), "v4", res=res, case=(vlan, ihl, proto, m, pad))
                        k += 1
    # ---- egress: every flag byte over every kind of accepted frame
    kinds = [("v4 tcp", lambda v: _v4_frame(rng, v, 5, 6, 32)), ("v4 udp", lambda v: _v4_frame(rng, v, 5, 17, 13)),
             ("v4 icmp 1", lambda v: _v4_frame(rng, v, 5, 1, 1)), ("v4 icmp 3", lambda v: _v4_frame(rng, v, 5, 1, 3)),
             ("v4 icmp 4", lambda v: _v4_frame(rng, v, 5, 1, 4)), ("v4 icmp 8", lambda v: _v4_frame(rng, v, 5, 1, 8)),
             ("v4 proto 58", lambda v: _v4_frame(rng, v, 5, 58, 10)), ("v6 tcp", lambda v: _v6_frame(rng, v, 6, 27)),
             ("v6 udp", lambda v: _v6_frame(rng, v, 17, 9)), ("v6 icmpv6", lambda v: _v6_frame(rng, v, 58, 11)),
             ("v6 icmpv4", lambda v: _v6_frame(rng, v, 1, 11))]
    k = 0
    for vlan in (False, True):
        for name, mk in kinds:
            for w in EGRESS_FLAGS:
                add(mk(vlan), "egress", res=(k * 3) % 16, flag=w, case=(name, vlan))
                k += 1
    # ---- last: a deep frame, GUARD bytes, a plain frame that ends the arena
    add(deep_frame(rng, True, 255, "tcp15ts", 386), "last", case="deep")
    add(_v4_frame(rng, False, 5, 17, 26), "last", case="plain")
    return recs


@functools.lru_cache(maxsize=2)
def batch(seed: int = 20241) -> dict:
    """The geometry batch: {arena, frame_off, frame_len, laid (the bytes laid at frame_off: more than
    frame_len where the table cuts a frame), fwant (the egress flag bytes), cls, case,
    frames (the bytes behind each in-bounds table entry), inb, twin / of (a refused twin's name and
    the index of its accepted frame), info, desc, status, tuples, hsum (the ingress expectations
    for want = F_IP | F_L4), eg_ok (egress: parsed and every flag honoured), cut_n / cut_len (the
    prefix whose arena ends on a deep frame's last byte)}.  It is cached: its arrays are read-only."""
    recs = _records(seed)
    n = len(recs)
    # three of every four frames with the checksums a verify accepts (the twins are cut below)
    for i, r in enumerate(recs):
        if r["frame"] and r.get("twin") is None and i % 4 != 3:
            full = r["frame"]
            r["frame"] = with_sums(full) if r["L"] is None else with_sums(full[:r["L"]]) + full[r["L"]:]
    for i, r in enumerate(recs):     # a twin is cut from its frame as it lies in the arena
        if r.get("twin"):
            base = recs[r["of"]]
            r["frame"] = dict(twins(base["frame"], r["case"][2]))[r["twin"]]
    buf = bytearray()
    off = np.zeros(n, np.uint64)
    ln = np.zeros(n, np.uint32)
    laid = np.zeros(n, np.uint32)      # bytes laid at off[i]: more than ln[i] where the table cuts the frame
    for i, r in enumerate(recs):
        if r["at"] is not None:
            continue
        buf += bytes([FILL]) * GUARD
        if r["res"] is not None:
            buf += bytes([FILL]) * ((r["res"] - len(buf)) % 16)
        off[i], ln[i] = len(buf), len(r["frame"]) if r["L"] is None else r["L"]
        laid[i] = len(r["frame"])
        buf += r["frame"]
        if i == n - 2:
            cut_len = len(buf)
    arena = np.frombuffer(bytes(buf), np.uint8).copy()     # no guard after the last frame
    for i, r in enumerate(recs):
        if r["at"] is not None:
            off[i], ln[i] = r["at"](arena.nbytes), r["L"]
    inb = np.array([int(o) <= arena.nbytes and int(L) <= arena.nbytes - int(o) for o, L in zip(off, ln)])
    frames, infos = [], []
    desc, status = np.zeros(n, O.DESC_DTYPE), np.zeros(n, np.uint8)
    tuples, hsum = np.zeros(n, TUPLE_DTYPE), np.zeros(n, O.HSUM_DTYPE)
    fwant, eg_ok = np.zeros(n, np.uint8), np.zeros(n, bool)
    for i, r in enumerate(recs):
        f = arena[int(off[i]):int(off[i]) + int(ln[i])].tobytes() if inb[i] else None
        info = O.parse_ether(f)[0] if f is not None else None
        frames.append(f)
        infos.append(info)
        if info is None:
            status[i] = O.S_BAD_DESC
            fwant[i] = r["flag"] if r["flag"] is not None else O.F_IP | O.F_L4
            continue
        desc[i] = (int(off[i]) + info.l3_off, info.l3_len, info.l4_off, info.ver, info.proto, O.desc_flags_for(info), 0)
        t = O.flow_tuple(f)
        for key in ("src", "dst", "sport", "dport"):
            tuples[key][i] = np.frombuffer(t[key], np.uint8)
        tuples["l3_ver"][i], tuples["l4_proto"][i], tuples["tcp_flags"][i] = t["l3_ver"], t["l4_proto"], t["tcp_flags"]
        hsum[i] = O.hsum_record(f)
        if r["flag"] is not None:
            fwant[i] = r["flag"]
        else:   # one the frame can honour: all it allows, L4 alone, IP alone, the pseudo-header sum, none
            al = O.desc_flags_for(info)
            fwant[i] = (al, al & O.F_L4, al & O.F_IP, ingress_flags(info, O.F_IP | O.F_L4P), 0)[i % 5]
        eg_ok[i] = egress_honoured(info, int(fwant[i]))
    for a in (arena, off, ln, laid, inb, fwant, desc, status, tuples, hsum, eg_ok):
        a.setflags(write=False)        # the batch is cached
    return dict(arena=arena, frame_off=off, frame_len=ln, laid=laid, fwant=fwant, cls=[r["cls"] for r in recs],
                case=[r["case"] for r in recs], frames=frames, inb=inb, twin=[r.get("twin") for r in recs],
                of=[r.get("of") for r in recs], info=infos, desc=desc, status=status, tuples=tuples, hsum=hsum,
                eg_ok=eg_ok, cut_n=n - 1, cut_len=cut_len)


def ingress_desc(b: dict, want: int) -> np.ndarray:
    """The batch's expected descriptors for another `want` than F_IP | F_L4."""
    d = b["desc"].copy()
    for i, info in enumerate(b["info"]):
        if info is not None:
            d["flags"][i] = ingress_flags(info, want)
    return d


def egress_desc(b: dict) -> np.ndarray:
    """The descriptors an egress flush works on: the frame's own flags where it is parsed and all
    of them can be honoured, all zeros (refused, nothing written) elsewhere."""
    d = b["desc"].copy()
    d["flags"] = b["fwant"]
    d[~b["eg_ok"]] = np.zeros(1, O.DESC_DTYPE)[0]
    return d
