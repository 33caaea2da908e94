"""The rules of the ICMP replies (include/vpcsum.h vpcsum_icmp_reply_async), restated in Python for the
tests: the three Java builders that end in SwitchUtils.buildEtherIpIcmpPacket -- IcmpInput.
respondIcmpPong, IcmpPortUnreachableOutput.handle, IPInputRoute.respondIcmpTimeExceeded -- from the
field list, the sums through the oracle's restatement of Utils.calculateChecksum (oracle.csum,
oracle.pseudo_ipv6, oracle.ipv4_header_csum), every refusal; an echo's out / status from
Oracle.process(arena, desc, MODE_VERIFY).  Nothing of the library is used here."""
import numpy as np

from oracle import oracle as O

HDR_DTYPE = np.dtype([("eth_dst", "u1", 6), ("eth_src", "u1", 6), ("l2_len", "u1"), ("l3_ver", "u1"), ("tos", "u1"),
                      ("ttl", "u1"), ("src", "u1", 16), ("dst", "u1", 16), ("sport", "u1", 2), ("dport", "u1", 2),
                      ("ack", "u1", 4), ("window", "u1", 2), ("ident", "u1", 2), ("frag", "u1", 2), ("rsv", "u1", 2)])
ICMPRP_DTYPE = np.dtype([("frame_off", "<u8"), ("hdr", "<u4"), ("frame_cap", "<u4"), ("kind", "u1"), ("rsv", "u1", 7)])
ECHO, UNREACH, TIMEX = 1, 2, 3
S_IP_OK, S_L4_OK, S_DONE, S_BAD_DESC = O.S_IP_OK, O.S_L4_OK, O.S_DONE, O.S_BAD_DESC
# the reply's type and code: (kind, is IPv4) -> (type, code)
TYPE_CODE = {(ECHO, True): (0, 0), (ECHO, False): (129, 0), (UNREACH, True): (3, 3), (UNREACH, False): (1, 4),
             (TIMEX, True): (11, 0), (TIMEX, False): (3, 0)}

_orc = None


def oracle():
    global _orc
    if _orc is None:
        O.build()
        _orc = O.Oracle()
    return _orc


# ------------------------------------------------------------------------------------------
# templates, records, descriptors
# ------------------------------------------------------------------------------------------
def mk_hdr(ver=4, l2_len=14, src=b"\xc0\xa8\x01\xfe", dst=b"\x0a\x00\x00\x01", eth_dst=b"\x02\x00\x00\x00\x0a\x01",
           eth_src=b"\x02\x00\x00\x00\x0b\x02", tos=0, ttl=64, ident=0, frag=0, rsv=0, sport=0, dport=0, ack=0, window=0):
    """The reply's template: src / dst are the REPLY's (dst: the request's source)."""
    h = np.zeros(1, HDR_DTYPE)
    h["eth_dst"][0] = np.frombuffer(bytes(eth_dst), np.uint8)
    h["eth_src"][0] = np.frombuffer(bytes(eth_src), np.uint8)
    h["l2_len"], h["l3_ver"], h["tos"], h["ttl"] = l2_len, ver, tos, ttl
    h["src"][0] = np.frombuffer(bytes(src).ljust(16, b"\0"), np.uint8)
    h["dst"][0] = np.frombuffer(bytes(dst).ljust(16, b"\0"), np.uint8)
    for k, v, w in (("sport", sport, 2), ("dport", dport, 2), ("ack", ack, 4), ("window", window, 2), ("ident", ident, 2),
                    ("frag", frag, 2), ("rsv", rsv, 2)):
        h[k][0] = np.frombuffer(int(v).to_bytes(w, "big"), np.uint8)
    return h[0]


def mk_rp(frame_off, kind, hdr=0, frame_cap=1 << 20, rsv=0):
    r = np.zeros(1, ICMPRP_DTYPE)
    r["frame_off"], r["hdr"], r["frame_cap"], r["kind"] = frame_off, hdr, frame_cap, kind
    r["rsv"][0] = np.frombuffer(int(rsv).to_bytes(7, "little"), np.uint8)
    return r[0]


def mk_desc(l3_off, l3_len, l4_off, ver, proto, flags=None):
    d = np.zeros(1, O.DESC_DTYPE)
    d[0] = (l3_off, l3_len, l4_off, ver, proto, (O.F_L4 | (O.F_IP if ver == 4 else 0)) if flags is None else flags, 0)
    return d[0]


def hdr_ok(h) -> bool:
    return int(h["l3_ver"]) in (4, 6) and int(h["l2_len"]) in (0, 14) and not any(
        np.any(h[k]) for k in ("rsv", "ack", "window", "sport", "dport"))


# ------------------------------------------------------------------------------------------
# the rule
# ------------------------------------------------------------------------------------------
def msg_len(kind: int, l3_len: int, l4_off: int) -> int:
    return l3_len - l4_off if kind == ECHO else 8 + min(l3_len, l4_off + 64)


def plan(arena, d, hdrs, r, dst_len: int):
    """L of the reply to descriptor d under record r, or None when the record is refused.  Of the arena
    only the segment's byte 0 is looked at, last, and only where the kind asks for it.  Python integers
    do not wrap."""
    if int(r["hdr"]) >= len(hdrs) or int(r["kind"]) not in (ECHO, UNREACH, TIMEX) or np.any(r["rsv"]):
        return None
    h = hdrs[int(r["hdr"])]
    if not hdr_ok(h):
        return None
    l3_off, l3_len, l4_off = int(d["l3_off"]), int(d["l3_len"]), int(d["l4_off"])
    ver, proto, fl, kind = int(d["l3_ver"]), int(d["l4_proto"]), int(d["flags"]), int(r["kind"])
    if ver not in (4, 6) or ver != int(h["l3_ver"]):
        return None
    if fl & (O.F_L4P | O.F_RAW | O.F_PRE) or (fl & O.F_IP and ver == 6):
        return None
    if l4_off > l3_len or (ver == 4 and (l4_off < 20 or l4_off & 3)) or (ver == 6 and l4_off < 40):
        return None
    if l3_off + l3_len > len(arena):
        return None
    seg_len = l3_len - l4_off
    if kind == ECHO and (not fl & O.F_L4 or proto != (1 if ver == 4 else 58) or seg_len < 8):
        return None
    if kind == UNREACH and proto != 17:
        return None
    M = msg_len(kind, l3_len, l4_off)
    L = int(h["l2_len"]) + (20 if ver == 4 else 40) + M
    if L > int(r["frame_cap"]) or int(r["frame_off"]) + L > dst_len:
        return None
    if kind == ECHO and int(arena[l3_off + l4_off]) != (8 if ver == 4 else 128):
        return None
    if kind == TIMEX and ver == 6 and proto == 58 and seg_len >= 1 and int(arena[l3_off + l4_off]) in (135, 136):
        return None
    return L


def message(kind: int, v4: bool, l3: bytes, l4_off: int) -> bytes:
    """The ICMP message with a zero field: IcmpPacket.buildPacket's type, code, 00 00, other."""
    t, c = TYPE_CODE[(kind, v4)]
    if kind == ECHO:
        return bytes([t, c, 0, 0]) + bytes(l3[l4_off + 4:])             # icmp.setCode(0); setOther(inIcmp.getOther())
    return bytes([t, c, 0, 0]) + bytes(4) + bytes(l3[:l4_off + 64])    # 4 unused bytes, then headerLen + 64 of the packet


def frame(h, kind: int, l3: bytes, l4_off: int) -> tuple[bytes, int, int]:
    """(frame bytes, IPv4 header sum or 0, ICMP field) of an accepted template and the request's IP
    packet l3 (exactly l3_len bytes): SwitchUtils.buildIpIcmpPacket / buildEtherIpPacket, getRawPacket(0)."""
    v4 = int(h["l3_ver"]) == 4
    msg = bytearray(message(kind, v4, l3, l4_off))
    M = len(msg)
    tos, ttl = int(h["tos"]), int(h["ttl"])
    if v4:
        ip = bytearray(bytes([0x45, tos]) + (20 + M).to_bytes(2, "big") + h["ident"].tobytes() + h["frag"].tobytes() +
                       bytes([ttl, 1]) + b"\x00\x00" + h["src"][:4].tobytes() + h["dst"][:4].tobytes())
        ipc = O.ipv4_header_csum(bytes(ip), 20)
        ip[10:12] = ipc.to_bytes(2, "big")
        c = O.csum(bytes(msg))                                    # IcmpPacket.buildPacket: no pseudo-header
        et = b"\x08\x00"
    else:
        ip = bytearray(bytes([0x60 | (tos >> 4), (tos << 4) & 0xff, 0, 0]) + M.to_bytes(2, "big") + bytes([58, ttl]) +
                       h["src"].tobytes() + h["dst"].tobytes())
        ipc = 0
        c = O.csum(O.pseudo_ipv6(bytes(ip), 58, M) + bytes(msg))  # IcmpPacket.buildICMPv6Packet
        et = b"\x86\xdd"
    msg[2:4] = c.to_bytes(2, "big")
    eth = h["eth_dst"].tobytes() + h["eth_src"].tobytes() + et if int(h["l2_len"]) == 14 else b""
    return eth + bytes(ip) + bytes(msg), ipc, c


def reply(dst: np.ndarray, arena: np.ndarray, desc: np.ndarray, hdrs: np.ndarray, rps: np.ndarray):
    """(dst_after, frame_len, csum, out, status); the inputs are not modified."""
    after = dst.copy()
    n = len(desc)
    flen, cs, out, st = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    o_out, o_st = oracle().process(arena, np.ascontiguousarray(desc), O.MODE_VERIFY) if n else (None, None)
    for i in range(n):
        d, r = desc[i], rps[i]
        L = plan(arena, d, hdrs, r, len(dst))
        if L is None:
            st[i] = S_BAD_DESC
            continue
        o = int(d["l3_off"])
        f, ipc, c = frame(hdrs[int(r["hdr"])], int(r["kind"]), arena[o:o + int(d["l3_len"])].tobytes(), int(d["l4_off"]))
        assert len(f) == L
        fo = int(r["frame_off"])
        after[fo:fo + L] = np.frombuffer(f, np.uint8)
        flen[i], cs[i] = L, ipc | (c << 16)
        if int(r["kind"]) == ECHO:
            assert o_st[i] & S_DONE and not o_st[i] & S_BAD_DESC, (i, o_st[i])
            out[i], st[i] = o_out[i], o_st[i]
        else:
            st[i] = S_DONE
    return after, flen, cs, out, st


# ------------------------------------------------------------------------------------------
# requests
# ------------------------------------------------------------------------------------------
V4_SRC, V4_DST = b"\x0a\x00\x00\x01", b"\xc0\xa8\x01\xfe"
V6_SRC, V6_DST = bytes(range(0x20, 0x30)), bytes(range(0x40, 0x50))


def ip_l3(ver: int, proto: int, seg: bytes, ihl: int = 5, ext: int = 0, src: bytes | None = None, dst: bytes | None = None,
          ttl: int = 1) -> tuple[bytes, int]:
    """(L3 packet bytes with the IPv4 header sum right, l4_off) around a finished segment: IPv4 with
    `ihl` words of header (options: NOPs), or IPv6 with `ext` bytes (0 or a multiple of 8) of a
    destination-options header."""
    n = len(seg)
    if ver == 4:
        src, dst = src or V4_SRC, dst or V4_DST
        l4_off = ihl * 4
        ip = bytearray(bytes([0x40 | ihl, 0]) + (l4_off + n).to_bytes(2, "big") + b"\xab\xcd\x40\x00" + bytes([ttl, proto]) +
                       b"\0\0" + src + dst + b"\x01" * (l4_off - 20))
        ip[10:12] = O.ipv4_header_csum(bytes(ip), l4_off).to_bytes(2, "big")
    else:
        src, dst = src or V6_SRC, dst or V6_DST
        assert ext % 8 == 0
        l4_off = 40 + ext
        eh = bytes([proto, ext // 8 - 1, 1, ext - 4]) + b"\0" * (ext - 4) if ext else b""
        ip = bytearray(b"\x60\0\0\0" + (ext + n).to_bytes(2, "big") + bytes([60 if ext else proto, ttl]) + src + dst + eh)
    return bytes(ip) + bytes(seg), l4_off


def echo_l3(ver: int, body: bytes, code: int = 0, field: int | None = None, typ: int | None = None, **kw) -> tuple[bytes, int]:
    """An echo request (type 8 / 128) whose bytes 4.. are `body`, its sum right unless `field` is given."""
    proto = 1 if ver == 4 else 58
    seg = bytes([(8 if ver == 4 else 128) if typ is None else typ, code, 0, 0]) + bytes(body)
    l3, l4_off = ip_l3(ver, proto, seg, **kw)
    c = O.l4_csum(l3, len(l3), l4_off, ver, proto) if field is None else field
    return l3[:l4_off + 2] + c.to_bytes(2, "big") + l3[l4_off + 4:], l4_off


def udp_l3(ver: int, payload: bytes, **kw) -> tuple[bytes, int]:
    """A UDP datagram for a port nobody listens on, its sum right."""
    seg = b"\x12\x34\x9c\x40" + (8 + len(payload)).to_bytes(2, "big") + b"\0\0" + bytes(payload)
    l3, l4_off = ip_l3(ver, 17, seg, **kw)
    c = O.l4_csum(l3, len(l3), l4_off, ver, 17)
    return l3[:l4_off + 6] + c.to_bytes(2, "big") + l3[l4_off + 8:], l4_off


def verify_reply(orc, f: bytes, h) -> tuple[int, int]:
    """(out, status) of the oracle's MODE_VERIFY on a reply frame built from template h, described
    as the parse would describe it."""
    ver, l2 = int(h["l3_ver"]), int(h["l2_len"])
    ipl = 20 if ver == 4 else 40
    d = np.array([mk_desc(l2, len(f) - l2, ipl, ver, 1 if ver == 4 else 58)], O.DESC_DTYPE)
    out, st = orc.process(np.frombuffer(f, np.uint8), d, O.MODE_VERIFY)
    return int(out[0]), int(st[0])
