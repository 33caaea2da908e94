"""The rule of the TCP receive (include/vpcsum.h vpcsum_tcp_recv_async / vpcsum_tcp_digest_async),
restated in Python for the tests.  The yardsticks are the oracle's own: Oracle.process(arena, desc,
MODE_VERIFY) for `out` and `status`, numpy slicing of the arena for the stored bytes, and
O._tcp_from for the two header refusals it knows (a segment under 20 bytes, a data offset past the
segment).  Nothing of the library is used here."""
import numpy as np

from oracle import oracle as O

TCPRX_DTYPE = np.dtype([("dst_off", "<u8"), ("dst_cap", "<u4"), ("skip", "<u2"), ("ops", "u1"), ("rsv", "u1")])
TCPINFO_DTYPE = np.dtype([("seq", "<u4"), ("ack", "<u4"), ("window", "<u2"), ("data_len", "<u2"), ("hlen", "u1"),
                          ("flags", "u1"), ("rsv", "u1", 2)])
STORE = 0x01
S_IP_OK, S_L4_OK, S_DONE, S_BAD_DESC = O.S_IP_OK, O.S_L4_OK, O.S_DONE, O.S_BAD_DESC
FIN, SYN, RST, PSH, ACK = 0x01, 0x02, 0x04, 0x08, 0x10

_orc = None


def oracle():
    global _orc
    if _orc is None:
        O.build()
        _orc = O.Oracle()
    return _orc


def mk_rx(dst_off=0, dst_cap=0, skip=0, ops=STORE, rsv=0):
    r = np.zeros(1, TCPRX_DTYPE)
    r["dst_off"], r["dst_cap"], r["skip"], r["ops"], r["rsv"] = dst_off, dst_cap, skip, ops, rsv
    return r[0]


def mk_desc(l3_off, l3_len, l4_off, ver, proto=6, flags=None):
    d = np.zeros(1, O.DESC_DTYPE)
    d[0] = (l3_off, l3_len, l4_off, ver, proto, (O.F_L4 | (O.F_IP if ver == 4 else 0)) if flags is None else flags, 0)
    return d[0]


def header_of(arena: np.ndarray, d):
    """(hlen, data_len) of descriptor d's segment, or None when the header rule refuses it.  The
    descriptor's own refusals first: nothing of the arena is looked at for those."""
    l3_off, l3_len, l4_off = int(d["l3_off"]), int(d["l3_len"]), int(d["l4_off"])
    ver, fl = int(d["l3_ver"]), int(d["flags"])
    if int(d["l4_proto"]) != 6 or ver not in (4, 6):
        return None
    if not fl & O.F_L4 or fl & (O.F_L4P | O.F_RAW | O.F_PRE) or (fl & O.F_IP and ver == 6):
        return None
    if l4_off > l3_len or l3_off + l3_len > len(arena):   # Python integers do not wrap
        return None
    # what vpcsum_compute_async itself refuses of an L4 offset (the oracle's rule)
    if (ver == 4 and (l4_off < 20 or l4_off & 3)) or (ver == 6 and l4_off < 40):
        return None
    seg = arena[l3_off + l4_off:l3_off + l3_len].tobytes()
    why = O._tcp_from(seg)
    if why in ("input packet length too short for a tcp packet", "dataOffset too big"):
        return None
    hlen = (seg[12] >> 4) * 4
    if hlen < 20:
        return None
    return hlen, len(seg) - hlen


def plan(arena: np.ndarray, d, r, dst_len: int):
    """(hlen, data_len, stored) of a record, or None when it is refused."""
    h = header_of(arena, d)
    if h is None or int(r["ops"]) & ~STORE or int(r["rsv"]) != 0:
        return None
    hlen, data_len = h
    skip = int(r["skip"])
    if skip > data_len:
        return None
    if not int(r["ops"]) & STORE:
        return hlen, data_len, 0
    stored = data_len - skip
    if stored > int(r["dst_cap"]) or int(r["dst_off"]) + stored > dst_len:
        return None
    return hlen, data_len, stored


def recv(dst: np.ndarray, arena: np.ndarray, desc: np.ndarray, rx: np.ndarray):
    """(dst_after, stored, out, status); the inputs are not modified."""
    after = dst.copy()
    n = len(desc)
    o_out, o_st = oracle().process(arena, np.ascontiguousarray(desc), O.MODE_VERIFY)
    stored, out, st = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
    for i in range(n):
        p = plan(arena, desc[i], rx[i], len(dst))
        if p is None:
            st[i] = S_BAD_DESC
            continue
        hlen, data_len, k = p
        assert o_st[i] & S_DONE and not o_st[i] & S_BAD_DESC, (i, o_st[i])
        out[i], st[i], stored[i] = o_out[i], o_st[i], k
        if k:
            a = int(desc[i]["l3_off"]) + int(desc[i]["l4_off"]) + hlen + int(rx[i]["skip"])
            do = int(rx[i]["dst_off"])
            after[do:do + k] = arena[a:a + k]
    return after, stored, out, st


def digest(arena: np.ndarray, desc: np.ndarray) -> np.ndarray:
    info = np.zeros(len(desc), TCPINFO_DTYPE)
    for i, d in enumerate(desc):
        h = header_of(arena, d)
        if h is None:
            continue
        a = int(d["l3_off"]) + int(d["l4_off"])
        t = arena[a:a + 16].tobytes()
        info[i]["seq"], info[i]["ack"] = int.from_bytes(t[4:8], "big"), int.from_bytes(t[8:12], "big")
        info[i]["window"], info[i]["data_len"] = int.from_bytes(t[14:16], "big"), h[1]
        info[i]["hlen"], info[i]["flags"] = h[0], int.from_bytes(t[12:14], "big") & 0x3f
    return info


# ------------------------------------------------------------------------------------------
# frames for the tests
# ------------------------------------------------------------------------------------------
def tcp_l3(ver: int, payload: bytes, hlen: int = 20, ihl: int = 5, ext: int = 0, seq: int = 0x01020304, ack: int = 0x0a0b0c0d,
           flags: int = PSH | ACK, window: int = 0x7fff, src: bytes | None = None, dst: bytes | None = None,
           sport: int = 0x1234, dport: int = 443) -> tuple[bytes, int]:
    """(L3 packet bytes with both sums right, l4_off): IPv4 with `ihl` words of header (options: NOPs
    and an end), or IPv6 with `ext` bytes (0 or a multiple of 8) of a destination-options header;
    a TCP header of `hlen` bytes (options: NOPs)."""
    assert hlen % 4 == 0 and 20 <= hlen <= 60
    tcp = (sport.to_bytes(2, "big") + dport.to_bytes(2, "big") + seq.to_bytes(4, "big") + ack.to_bytes(4, "big") +
           bytes([(hlen // 4) << 4, flags]) + window.to_bytes(2, "big") + b"\0\0\0\0" + b"\x01" * (hlen - 20))
    seg = tcp + bytes(payload)
    if ver == 4:
        src, dst = src or b"\x0a\x00\x00\x01", dst or b"\xc0\xa8\x01\xfe"
        l4_off = ihl * 4
        ip = bytearray(bytes([0x40 | ihl, 0]) + (l4_off + len(seg)).to_bytes(2, "big") + b"\xab\xcd\x40\x00" + bytes([64, 6]) +
                       b"\0\0" + src + dst + b"\x01" * (l4_off - 20))
        ip[10:12] = O.ipv4_header_csum(bytes(ip), l4_off).to_bytes(2, "big")
    else:
        src, dst = src or bytes(range(0x20, 0x30)), dst or bytes(range(0x40, 0x50))
        assert ext % 8 == 0
        l4_off = 40 + ext
        eh = bytes([6, ext // 8 - 1, 1, ext - 4]) + b"\0" * (ext - 4) if ext else b""
        ip = bytearray(b"\x60\0\0\0" + (ext + len(seg)).to_bytes(2, "big") + bytes([60 if ext else 6, 64]) + src + dst + eh)
    l3 = bytes(ip) + seg
    c = O.l4_csum(l3, len(l3), l4_off, ver, 6)
    return l3[:l4_off + 16] + c.to_bytes(2, "big") + l3[l4_off + 18:], l4_off


def plan_tcp_store(expecting: int, seq: int, data_len: int):
    """ReceivingQueue.store's four branches (TcpEntry.java:390-426) on plain integers: the yardstick
    of vswitch.plan_tcp_store.  (skip, stored), or None: dropped."""
    if seq > expecting:
        return None          # a hole before it: not stored
    if seq + data_len <= expecting:
        return None          # all of it already received
    if seq < expecting:
        return expecting - seq, data_len - (expecting - seq)
    return 0, data_len
