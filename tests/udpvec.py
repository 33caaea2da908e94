"""The rules of the UDP datagram build and receive (include/vpcsum.h vpcsum_udp_build_async /
vpcsum_udp_recv_async), restated in Python for the tests: the frame from the field list, the two sums
through the oracle's restatement of Java (oracle.ipv4_header_csum / l4_csum with protocol 17, which
gives 0xffff for a computed 0), the refusals; receive expectations from Oracle.process(arena, desc,
MODE_VERIFY) plus numpy slices.  Nothing of the library is used here."""
import numpy as np

from oracle import oracle as O

HDR_DTYPE = np.dtype([("eth_dst", "u1", 6), ("eth_src", "u1", 6), ("l2_len", "u1"), ("l3_ver", "u1"), ("tos", "u1"),
                      ("ttl", "u1"), ("src", "u1", 16), ("dst", "u1", 16), ("sport", "u1", 2), ("dport", "u1", 2),
                      ("ack", "u1", 4), ("window", "u1", 2), ("ident", "u1", 2), ("frag", "u1", 2), ("rsv", "u1", 2)])
UDPDG_DTYPE = np.dtype([("frame_off", "<u8"), ("data_off", "<u8"), ("hdr", "<u4"), ("frame_cap", "<u4"), ("data_len", "<u4"),
                        ("rsv", "<u4")])
UDPRX_DTYPE = np.dtype([("dst_off", "<u8"), ("dst_cap", "<u4"), ("ops", "u1"), ("rsv", "u1", 3)])
STORE = 0x01
S_IP_OK, S_L4_OK, S_UDP_NOCSUM, S_DONE, S_BAD_DESC = O.S_IP_OK, O.S_L4_OK, 0x04, O.S_DONE, O.S_BAD_DESC

_orc = None


def oracle():
    global _orc
    if _orc is None:
        O.build()
        _orc = O.Oracle()
    return _orc


# ------------------------------------------------------------------------------------------
# build
# ------------------------------------------------------------------------------------------
def mk_hdr(ver=4, l2_len=14, src=b"\x0a\x00\x00\x01", dst=b"\x0a\x00\x00\x02", sport=53, dport=40000,
           eth_dst=b"\x02\x00\x00\x00\x0a\x01", eth_src=b"\x02\x00\x00\x00\x0b\x02", tos=0, ttl=64, ident=0, frag=0, rsv=0,
           ack=0, window=0):
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


def header_len(h) -> int:
    return int(h["l2_len"]) + (20 if int(h["l3_ver"]) == 4 else 40) + 8


def mk_dg(frame_off, data_off, data_len, hdr=0, frame_cap=None, rsv=0, hlen=42):
    s = np.zeros(1, UDPDG_DTYPE)
    s["frame_off"], s["data_off"], s["hdr"] = frame_off, data_off, hdr
    s["frame_cap"] = hlen + data_len if frame_cap is None else frame_cap
    s["data_len"], s["rsv"] = data_len, rsv
    return s[0]


def hdr_ok(h) -> bool:
    return int(h["l3_ver"]) in (4, 6) and int(h["l2_len"]) in (0, 14) and not np.any(h["rsv"]) and not np.any(h["ack"]) and \
        not np.any(h["window"])


def refused(hdrs, s, dst_len: int, src_len: int) -> bool:
    """The refusals of a record, in the header's order.  Python integers do not wrap."""
    if int(s["hdr"]) >= len(hdrs):
        return True
    h = hdrs[int(s["hdr"])]
    if not hdr_ok(h) or int(s["rsv"]) != 0:
        return True
    d = int(s["data_len"])
    if (28 if int(h["l3_ver"]) == 4 else 8) + d > 65535:
        return True
    L = header_len(h) + d
    if L > int(s["frame_cap"]):
        return True
    return int(s["frame_off"]) + L > dst_len or int(s["data_off"]) + d > src_len


def frame(h, payload: bytes) -> tuple[bytes, int, int]:
    """(frame bytes, IPv4 header sum or 0, stored UDP field) of an accepted template and a payload."""
    d = len(payload)
    udp = h["sport"].tobytes() + h["dport"].tobytes() + (8 + d).to_bytes(2, "big") + b"\x00\x00"
    tos, ttl = int(h["tos"]), int(h["ttl"])
    if int(h["l3_ver"]) == 4:
        ip = bytearray(bytes([0x45, tos]) + (28 + d).to_bytes(2, "big") + h["ident"].tobytes() + h["frag"].tobytes() +
                       bytes([ttl, 0x11]) + b"\x00\x00" + h["src"][:4].tobytes() + h["dst"][:4].tobytes())
        ipc = O.ipv4_header_csum(bytes(ip), 20)
        ip[10:12] = ipc.to_bytes(2, "big")
        et = b"\x08\x00"
    else:
        ip = bytearray(bytes([0x60 | (tos >> 4), (tos << 4) & 0xff, 0, 0]) + (8 + d).to_bytes(2, "big") + bytes([0x11, ttl]) +
                       h["src"].tobytes() + h["dst"].tobytes())
        ipc = 0
        et = b"\x86\xdd"
    l3 = bytes(ip) + udp + bytes(payload)
    l4c = O.l4_csum(l3, len(l3), len(ip), int(h["l3_ver"]), 17)   # the oracle's UDP sum: a computed 0 is 0xffff
    l3 = l3[:len(ip) + 6] + l4c.to_bytes(2, "big") + l3[len(ip) + 8:]
    eth = h["eth_dst"].tobytes() + h["eth_src"].tobytes() + et if int(h["l2_len"]) == 14 else b""
    return eth + l3, ipc, l4c


def build(dst_arena: np.ndarray, src_arena: np.ndarray, hdrs: np.ndarray, dgs: np.ndarray):
    """(arena_after, frame_len, out, status); the input arenas are not modified."""
    after = dst_arena.copy()
    n = len(dgs)
    flen, out, st = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    for i, s in enumerate(dgs):
        if refused(hdrs, s, len(dst_arena), len(src_arena)):
            st[i] = S_BAD_DESC
            continue
        o, d = int(s["data_off"]), int(s["data_len"])
        f, ipc, l4c = frame(hdrs[int(s["hdr"])], src_arena[o:o + d].tobytes())
        fo = int(s["frame_off"])
        after[fo:fo + len(f)] = np.frombuffer(f, np.uint8)
        flen[i], out[i], st[i] = len(f), ipc | (l4c << 16), S_DONE
    return after, flen, out, st


def from_frame(raw: bytes):
    """(template, payload) read out of an Ethernet / IPv4 (IHL 5) / UDP frame."""
    assert raw[12:14] == b"\x08\x00" and raw[14] == 0x45 and raw[14 + 9] == 17
    ip, udp = raw[14:34], raw[34:42]
    h = mk_hdr(4, 14, ip[12:16], ip[16:20], int.from_bytes(udp[0:2], "big"), int.from_bytes(udp[2:4], "big"), raw[0:6], raw[6:12],
               ip[1], ip[8], int.from_bytes(ip[4:6], "big"), int.from_bytes(ip[6:8], "big"))
    return h, raw[42:14 + int.from_bytes(ip[2:4], "big")]


def sum_zero_payload(h, d: int, rng) -> bytes:
    """A payload of d >= 4 bytes (d even) with which the UDP sum of template h computes to 0: one
    aligned payload word is zeroed, the sum computed -- the word then takes that value, and the
    complement of what remains becomes 0.  Checked with the oracle, which stores 0xffff for it."""
    body = bytearray(rng.integers(0, 256, d, dtype=np.uint8).tobytes())
    body[2:4] = b"\0\0"
    _, _, c = frame(h, bytes(body))
    body[2:4] = c.to_bytes(2, "big")
    f, _, c2 = frame(h, bytes(body))
    l3 = f[int(h["l2_len"]):]
    ipl = 20 if int(h["l3_ver"]) == 4 else 40
    zeroed = l3[:ipl + 6] + b"\0\0" + l3[ipl + 8:]
    assert O.csum(_pseudo(l3, ipl, int(h["l3_ver"])) + zeroed[ipl:]) == 0 and c2 == 0xffff
    return bytes(body)


def _pseudo(l3: bytes, ipl: int, ver: int) -> bytes:
    n = len(l3) - ipl
    if ver == 4:
        return l3[12:20] + bytes([0, 17]) + n.to_bytes(2, "big")
    return l3[8:40] + n.to_bytes(4, "big") + bytes([0, 0, 0, 17])


# ------------------------------------------------------------------------------------------
# receive
# ------------------------------------------------------------------------------------------
def mk_rx(dst_off=0, dst_cap=0, ops=STORE, rsv=0):
    r = np.zeros(1, UDPRX_DTYPE)
    r["dst_off"], r["dst_cap"], r["ops"] = dst_off, dst_cap, ops
    r["rsv"][0] = np.frombuffer(int(rsv).to_bytes(3, "little"), np.uint8)
    return r[0]


def mk_desc(l3_off, l3_len, l4_off, ver, proto=17, flags=None):
    d = np.zeros(1, O.DESC_DTYPE)
    d[0] = (l3_off, l3_len, l4_off, ver, proto, (O.F_L4 | (O.F_IP if ver == 4 else 0)) if flags is None else flags, 0)
    return d[0]


def plan(arena_len: int, d, r, dst_len: int):
    """The bytes a record stores, or None when it is refused.  Nothing of the arena is looked at."""
    l3_off, l3_len, l4_off = int(d["l3_off"]), int(d["l3_len"]), int(d["l4_off"])
    ver, fl = int(d["l3_ver"]), int(d["flags"])
    if int(d["l4_proto"]) != 17 or ver not in (4, 6):
        return None
    if not fl & O.F_L4 or fl & (O.F_L4P | O.F_RAW | O.F_PRE) or (fl & O.F_IP and ver == 6):
        return None
    if l4_off > l3_len or l3_off + l3_len > arena_len:   # Python integers do not wrap
        return None
    if (ver == 4 and (l4_off < 20 or l4_off & 3)) or (ver == 6 and l4_off < 40):
        return None
    seg_len = l3_len - l4_off
    if seg_len < 8 or int(r["ops"]) & ~STORE or np.any(r["rsv"]):
        return None
    if not int(r["ops"]) & STORE:
        return 0
    stored = seg_len - 8
    if stored > int(r["dst_cap"]) or int(r["dst_off"]) + stored > dst_len:
        return None
    return stored


def recv(dst: np.ndarray, arena: np.ndarray, desc: np.ndarray, rx: np.ndarray):
    """(dst_after, stored, out, status); the inputs are not modified."""
    after = dst.copy()
    n = len(desc)
    o_out, o_st = oracle().process(arena, np.ascontiguousarray(desc), O.MODE_VERIFY)
    stored, out, st = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    for i in range(n):
        k = plan(len(arena), desc[i], rx[i], len(dst))
        if k is None:
            st[i] = S_BAD_DESC
            continue
        assert o_st[i] & S_DONE and not o_st[i] & S_BAD_DESC, (i, o_st[i])
        out[i], st[i], stored[i] = o_out[i], o_st[i], k
        if k:
            a = int(desc[i]["l3_off"]) + int(desc[i]["l4_off"]) + 8
            do = int(rx[i]["dst_off"])
            after[do:do + k] = arena[a:a + k]
    return after, stored, out, st


def udp_l3(ver: int, payload: bytes, ihl: int = 5, ext: int = 0, src: bytes | None = None, dst: bytes | None = None,
           sport: int = 0x1234, dport: int = 53, length: int | None = None, field: int | None = None) -> tuple[bytes, int]:
    """(L3 packet bytes with both sums right, l4_off): IPv4 with `ihl` words of header (options: NOPs),
    or IPv6 with `ext` bytes (0 or a multiple of 8) of a destination-options header; the UDP length
    field `length` (default: the segment's), the sum over what is there; `field`: stored instead."""
    n = 8 + len(payload)
    seg = sport.to_bytes(2, "big") + dport.to_bytes(2, "big") + (n if length is None else length).to_bytes(2, "big") + b"\0\0" + \
        bytes(payload)
    if ver == 4:
        src, dst = src or b"\x0a\x00\x00\x01", dst or b"\xc0\xa8\x01\xfe"
        l4_off = ihl * 4
        ip = bytearray(bytes([0x40 | ihl, 0]) + (l4_off + n).to_bytes(2, "big") + b"\xab\xcd\x40\x00" + bytes([64, 17]) +
                       b"\0\0" + src + dst + b"\x01" * (l4_off - 20))
        ip[10:12] = O.ipv4_header_csum(bytes(ip), l4_off).to_bytes(2, "big")
    else:
        src, dst = src or bytes(range(0x20, 0x30)), dst or bytes(range(0x40, 0x50))
        assert ext % 8 == 0
        l4_off = 40 + ext
        eh = bytes([17, ext // 8 - 1, 1, ext - 4]) + b"\0" * (ext - 4) if ext else b""
        ip = bytearray(b"\x60\0\0\0" + (ext + n).to_bytes(2, "big") + bytes([60 if ext else 17, 64]) + src + dst + eh)
    l3 = bytes(ip) + seg
    c = O.l4_csum(l3, len(l3), l4_off, ver, 17) if field is None else field
    return l3[:l4_off + 6] + c.to_bytes(2, "big") + l3[l4_off + 8:], l4_off


def plan_udp_store(connect, src, sport):
    """ReceivingQueue.store's filter (UdpListenEntry.java:51-65) on plain values: a connected socket
    takes datagrams of its peer only.  True: enqueue."""
    return connect is None or connect == (src, sport)
