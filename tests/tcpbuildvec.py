"""The frame rule of the TCP segment build (include/vpcsum.h vpcsum_tcp_build_async), restated in
Python for the tests: the header bytes from a template and a record, the two sums through the
oracle's restatement of Java (oracle.ipv4_header_csum / l4_csum), L, and the refusals.  Nothing of
the library is used here."""
import numpy as np

from oracle import oracle as O

TCPHDR_DTYPE = np.dtype([("eth_dst", "u1", 6), ("eth_src", "u1", 6), ("l2_len", "u1"), ("l3_ver", "u1"), ("tos", "u1"),
                         ("ttl", "u1"), ("src", "u1", 16), ("dst", "u1", 16), ("sport", "u1", 2), ("dport", "u1", 2),
                         ("ack", "u1", 4), ("window", "u1", 2), ("ident", "u1", 2), ("frag", "u1", 2), ("rsv", "u1", 2)])
TCPSEG_DTYPE = np.dtype([("frame_off", "<u8"), ("data_off", "<u8"), ("seq", "<u4"), ("hdr", "<u4"), ("frame_cap", "<u4"),
                         ("data_len", "<u2"), ("flags", "u1"), ("rsv", "u1")])
S_DONE, S_BAD_DESC = 0x40, 0x80
FIN, SYN, RST, PSH, ACK = 0x01, 0x02, 0x04, 0x08, 0x10


def mk_hdr(ver=4, l2_len=14, src=b"\x0a\x00\x00\x01", dst=b"\x0a\x00\x00\x02", sport=1000, dport=80, ack=0, window=65535,
           eth_dst=b"\x02\x00\x00\x00\x0a\x01", eth_src=b"\x02\x00\x00\x00\x0b\x02", tos=0, ttl=64, ident=0, frag=0, rsv=0):
    h = np.zeros(1, TCPHDR_DTYPE)
    h["eth_dst"][0] = np.frombuffer(bytes(eth_dst), np.uint8)
    h["eth_src"][0] = np.frombuffer(bytes(eth_src), np.uint8)
    h["l2_len"], h["l3_ver"], h["tos"], h["ttl"] = l2_len, ver, tos, ttl
    h["src"][0] = np.frombuffer(bytes(src).ljust(16, b"\0"), np.uint8)
    h["dst"][0] = np.frombuffer(bytes(dst).ljust(16, b"\0"), np.uint8)
    for k, v, w in (("sport", sport, 2), ("dport", dport, 2), ("ack", ack, 4), ("window", window, 2), ("ident", ident, 2),
                    ("frag", frag, 2), ("rsv", rsv, 2)):
        h[k][0] = np.frombuffer(int(v).to_bytes(w, "big"), np.uint8)
    return h[0]


def mk_seg(frame_off, data_off, data_len, seq=0, hdr=0, frame_cap=None, flags=PSH | ACK, rsv=0, hlen=54):
    s = np.zeros(1, TCPSEG_DTYPE)
    s["frame_off"], s["data_off"], s["seq"], s["hdr"] = frame_off, data_off, seq, hdr
    s["frame_cap"] = hlen + data_len if frame_cap is None else frame_cap
    s["data_len"], s["flags"], s["rsv"] = data_len, flags, rsv
    return s[0]


def header_len(h) -> int:
    return int(h["l2_len"]) + (20 if int(h["l3_ver"]) == 4 else 40) + 20


def hdr_ok(h) -> bool:
    return int(h["l3_ver"]) in (4, 6) and int(h["l2_len"]) in (0, 14) and not np.any(h["rsv"])


def refused(hdrs, s, dst_len: int, src_len: int) -> bool:
    """The refusals of a record, in the header's order."""
    if int(s["hdr"]) >= len(hdrs):
        return True
    h = hdrs[int(s["hdr"])]
    if not hdr_ok(h):
        return True
    if int(s["flags"]) & ~0x3f or int(s["rsv"]) != 0:
        return True
    d = int(s["data_len"])
    L = header_len(h) + d
    if L > int(s["frame_cap"]):
        return True
    if (40 if int(h["l3_ver"]) == 4 else 20) + d > 65535:
        return True
    if int(s["frame_off"]) + L > dst_len or int(s["data_off"]) + d > src_len:   # Python integers do not wrap
        return True
    return False


def frame(h, s, payload: bytes) -> tuple[bytes, int, int]:
    """(frame bytes, IPv4 header sum or 0, TCP sum) of an accepted template and record."""
    d = len(payload)
    assert d == int(s["data_len"])
    tcp = bytearray(h["sport"].tobytes() + h["dport"].tobytes() + int(s["seq"]).to_bytes(4, "big") + h["ack"].tobytes() +
                    bytes([0x50, int(s["flags"])]) + h["window"].tobytes() + b"\x00\x00" + b"\x00\x00")
    tos, ttl = int(h["tos"]), int(h["ttl"])
    if int(h["l3_ver"]) == 4:
        ip = bytearray(bytes([0x45, tos]) + (40 + d).to_bytes(2, "big") + h["ident"].tobytes() + h["frag"].tobytes() +
                       bytes([ttl, 6]) + b"\x00\x00" + h["src"][:4].tobytes() + h["dst"][:4].tobytes())
        ipc = O.ipv4_header_csum(bytes(ip), 20)
        ip[10:12] = ipc.to_bytes(2, "big")
        et = b"\x08\x00"
    else:
        ip = bytearray(bytes([0x60 | (tos >> 4), (tos << 4) & 0xff, 0, 0]) + (20 + d).to_bytes(2, "big") + bytes([6, ttl]) +
                       h["src"].tobytes() + h["dst"].tobytes())
        ipc = 0
        et = b"\x86\xdd"
    l3 = bytes(ip) + bytes(tcp) + bytes(payload)
    l4c = O.l4_csum(l3, len(l3), len(ip), int(h["l3_ver"]), 6)   # 0x0000 stays 0x0000: no substitution for TCP
    l3 = l3[:len(ip) + 16] + l4c.to_bytes(2, "big") + l3[len(ip) + 18:]
    eth = h["eth_dst"].tobytes() + h["eth_src"].tobytes() + et if int(h["l2_len"]) == 14 else b""
    return eth + l3, ipc, l4c


def build(dst_arena: np.ndarray, src_arena: np.ndarray, hdrs: np.ndarray, segs: np.ndarray):
    """(arena_after, frame_len, out, status); the input arenas are not modified."""
    after = dst_arena.copy()
    n = len(segs)
    flen, out, st = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    for i, s in enumerate(segs):
        if refused(hdrs, s, len(dst_arena), len(src_arena)):
            st[i] = S_BAD_DESC
            continue
        h = hdrs[int(s["hdr"])]
        o, d = int(s["data_off"]), int(s["data_len"])
        f, ipc, l4c = frame(h, s, src_arena[o:o + d].tobytes())
        fo = int(s["frame_off"])
        after[fo:fo + len(f)] = np.frombuffer(f, np.uint8)
        flen[i], out[i], st[i] = len(f), ipc | (l4c << 16), S_DONE
    return after, flen, out, st


def from_frame(raw: bytes):
    """(template, record fields, payload) read out of an Ethernet / IPv4 / TCP frame without options."""
    assert raw[12:14] == b"\x08\x00" and raw[14] == 0x45 and raw[14 + 9] == 6 and raw[34 + 12] == 0x50
    ip, tcp = raw[14:34], raw[34:54]
    h = mk_hdr(4, 14, ip[12:16], ip[16:20], int.from_bytes(tcp[0:2], "big"), int.from_bytes(tcp[2:4], "big"),
               int.from_bytes(tcp[8:12], "big"), int.from_bytes(tcp[14:16], "big"), raw[0:6], raw[6:12], ip[1], ip[8],
               int.from_bytes(ip[4:6], "big"), int.from_bytes(ip[6:8], "big"))
    total = int.from_bytes(ip[2:4], "big")
    payload = raw[54:14 + total]
    return h, dict(seq=int.from_bytes(tcp[4:8], "big"), flags=tcp[13] & 0x3f), payload
