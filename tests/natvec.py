"""Crafted vectors for the NAT rewrite kernels' window, store and loop geometry (test infrastructure:
tests/ only).  As in edgevec.py and tcprwvec.py every edge is hit by construction, not by chance,
and check_classes() recomputes from the descriptors that it is.

What the kernels of vproxy_amd/csrc/nat.hip decide per packet, restated in geometry():

* r0    the L3 address mod 16 (the window starts at the 16-B aligned address below L3);
* need  the header through the L4 checksum field (20 / 40 when the segment holds no field);
* wend  r0 + need when that fits the window of CH 16-B chunks, else 0: the byte-access path;
* tail  (r0 + l3_len) & 3: where the last dword of the changed range would pass the packet end.

The batch (batch()) is laid out in waves of 64 consecutive packets, the unit the quads of k_natq
work on, and ends with packets packed back to back whose last one ends on the arena's last byte:

  mixed    window, byte-path, refused (outside the arena, version 5, IPv6 under the 16-B formats)
           and TTL-expired packets inside one wave, each kind in every lane-mod-4 position.
  win4     IPv4 with r0 + need in {63, 64, 65}: the limit of a 4-chunk window, TCP / UDP / ICMP
           at every IHL that reaches it.
  win6     IPv6 behind one extension header with r0 + need in {95, 96, 97}: the limit of a 6-chunk
           window (IPv4 never reaches it: 15 + 60 + 18 = 93), TCP / UDP / ICMPv6 / ICMPv4, odd and
           even l4_off.
  round2   waves in which no packet, exactly one packet, and every packet has wend > 64, the
           threshold of k_natq's second quad round (IPv4 with options; IPv6 without extension
           header under the 48-B entries).
  tails    packets that end right after their L4 checksum field (UDP 8, ICMP 4, TCP 18 bytes of
           segment), one byte short of it (no field: the ports stay) and at l4_off, at every tail,
           back to back with gaps of 0..3 random bytes.
  sums     UDP stored 0 (recomputed in full) and 0xffff, rewrites whose new sum is 0 (UDP stores
           0xffff, TCP 0x0000), IPv4 and IPv6.
  masks    every mask bit alone, all together, SET_TTL + DEC_TTL with the set value 0, 1, 2.

Every packet carries valid incoming sums, so RFC 1624 equals Java's full recompute; corrupted()
is the same batch with wrong incoming sums, for the strict-Java mode only.
"""
from __future__ import annotations

import numpy as np

import edgevec as E
import hsumvec as H
import tcprwvec as T
from oracle import oracle as O

WAVE = 64
ADDR_PORTS = O.NAT_SRC | O.NAT_DST | O.NAT_SPORT | O.NAT_DPORT
NAT4R_DTYPE = np.dtype([("desc", O.DESC_DTYPE), ("rw", O.NAT4_DTYPE)])   # vpcsum_nat4_rec_t
PROTO_NAME = {6: "tcp", 17: "udp", 1: "icmp", 58: "icmpv6"}
MIXED_KINDS = ("win4", "win6", "byte6", "byte4", "outside", "far", "ver5", "ttl_win", "ttl_set", "ttl_byte4", "ttl_byte6")


# ----------------------------------------------------------------------------------------
# The kernels' per-packet decisions (nat.hip: nat_desc_ok, nat_l4sum, the window test)
# ----------------------------------------------------------------------------------------
def desc_ok(d, arena_len: int, fmt: int) -> bool:
    off, ln, l4o, ver = int(d["l3_off"]), int(d["l3_len"]), int(d["l4_off"]), int(d["l3_ver"])
    if off > arena_len or ln > arena_len - off:
        return False
    if ver == 4:
        return ln >= 20 and 20 <= l4o <= ln and l4o % 4 == 0
    if ver == 6:
        return fmt == 1 and ln >= 40 and 40 <= l4o <= ln
    return False


def l4sum(ver: int, proto: int, ln: int, l4o: int) -> bool:
    fld = O.L4_FIELD.get(proto, -1)
    return fld >= 0 and not (ver == 4 and proto == 58) and ln - l4o >= fld + 2


def geometry(d, arena_len: int, fmt: int, ch: int, base: int = 0):
    """(ok, r0, need, wend, tail) of descriptor d for entry format fmt and a window of ch chunks, the
    arena at an address that is `base` mod 16."""
    off, ln, l4o = int(d["l3_off"]), int(d["l3_len"]), int(d["l4_off"])
    ver, proto = int(d["l3_ver"]), int(d["l4_proto"])
    ok = desc_ok(d, arena_len, fmt)
    r0 = (base + off) & 15 if ok else 0
    need = 20 if ver == 4 else 40
    if l4sum(ver, proto, ln, l4o):
        need = max(need, l4o + O.L4_FIELD[proto] + 2)
    wend = r0 + need if ok and r0 + need <= 16 * ch else 0
    return ok, r0, need, wend, (r0 + ln) & 3


def expired(l3: bytes, ver: int, rw) -> bool:
    m = int(rw["mask"])
    if not m & O.NAT_DEC_TTL:
        return False
    return (int(rw["ttl"]) if m & O.NAT_SET_TTL else l3[8 if ver == 4 else 7]) <= 1


# ----------------------------------------------------------------------------------------
# One vector
# ----------------------------------------------------------------------------------------
def _seg(rng, proto: int, n: int | None = None) -> bytearray:
    """An L4 segment from hsumvec's builders, cut to n bytes when given."""
    if proto == 6:
        s = H._tcp(rng, int(rng.integers(0, 24)), bool(rng.integers(0, 2)), None, 0)
    elif proto == 17:
        s = H._udp(rng, int(rng.integers(0, 24)))
    else:
        s = bytearray(rng.integers(0, 256, 8 + int(rng.integers(0, 24)), dtype=np.uint8).tobytes())
    if n is not None:
        s = (s + bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes()))[:n]
    return s


def _vec(rng, cls: str, ver: int, proto: int, r0: int | None = None, ihl: int = 5, ext: int | None = None,
         seg_len: int | None = None, mask: int | None = None, set_ttl: int | None = None, ttl: int | None = None,
         bad: str | None = None, tail: int | None = None, sum_edge: str | None = None) -> dict:
    l3 = H._l3(rng, ver, _seg(rng, proto, seg_len), proto, ihl=ihl, ext=ext)
    l4_off = ihl * 4 if ver == 4 else 40 + (0 if ext is None else 8 + ext)
    if ttl is not None:
        l3[8 if ver == 4 else 7] = ttl
    if sum_edge == "udp_ffff":     # the true sum is 0: the sender stored 0xffff
        E.force_l4_zero(l3, len(l3), l4_off, ver, proto)
    l3 = T.l3_sums(l3, ver, proto, l4_off)   # valid incoming sums (no L4 field in a segment too short for one)
    if sum_edge in ("udp0", "udp0_ttl"):
        l3[l4_off + 6:l4_off + 8] = b"\x00\x00"
    rw = np.zeros(1, O.NAT_DTYPE)
    rw.view(np.uint8)[:36] = rng.integers(0, 256, 36, dtype=np.uint8)
    if mask is None:   # addresses and ports, half of them with a TTL decrement of the header's 64
        mask = ADDR_PORTS | (O.NAT_DEC_TTL if rng.integers(0, 2) else 0)
    rw["mask"] = mask
    rw["ttl"] = int(rng.integers(2, 256)) if set_ttl is None else set_ttl
    v = dict(cls=cls, l3=bytes(l3), ver=ver, proto=proto, l4_off=l4_off, rw=rw[0], r0=r0, tail=tail, bad=bad,
             sum_edge=sum_edge)
    if sum_edge in ("new0",):
        _force_new_zero(v)
    return v


def _force_new_zero(v: dict):
    """Choose the new destination port so that Java's recompute after the rewrite gives an L4
    result of 0 (test_gpu_edges._force_nat_zero, for IPv6 too): with the port 0 the recompute
    stores c = ~S, and a port word of c makes the total 0xffff."""
    rw = v["rw"]
    rw["dport"] = 0
    l3 = bytearray(v["l3"])
    assert O.nat_java_pure(l3, v["ver"], v["proto"], len(l3), v["l4_off"], rw) == O.S_DONE
    f = v["l4_off"] + O.L4_FIELD[v["proto"]]
    c = int.from_bytes(l3[f:f + 2], "big")
    if v["proto"] == 17 and c == 0xFFFF:
        c = 0
    rw["dport"] = [c >> 8, c & 0xFF]


# ----------------------------------------------------------------------------------------
# The classes
# ----------------------------------------------------------------------------------------
def _win4(rng) -> list[dict]:
    out = []
    for ihl in range(5, 16):
        for proto in (6, 17, 1):
            need = ihl * 4 + O.L4_FIELD[proto] + 2
            for t in (63, 64, 65):
                if 0 <= t - need <= 15:
                    out.append(_vec(rng, f"win4:{PROTO_NAME[proto]} ihl {ihl} r0+need {t}", 4, proto, r0=t - need, ihl=ihl))
    return out


def _win6(rng) -> list[dict]:
    out = []
    for proto in (6, 17, 58, 1):
        for t in (95, 96, 97):
            for r0 in (0, 1, 6, 7, 8, 15):
                h = t - r0 - (48 + O.L4_FIELD[proto] + 2)
                if 0 <= h <= 255:
                    out.append(_vec(rng, f"win6:{PROTO_NAME[proto]} ext {h} r0+need {t}", 6, proto, r0=r0, ext=h))
    return out


def _round2_v6(rng) -> list[dict]:
    """IPv6 without extension header around wend 64: TCP (need 58) at r0 5, 6, 7; UDP (need 48) at 15."""
    out = [_vec(rng, f"round2:v6 tcp r0+need {58 + r0}", 6, 6, r0=r0) for r0 in (5, 6, 7)]
    out.append(_vec(rng, "round2:v6 udp r0+need 63", 6, 17, r0=15))
    return out


def _hi4(rng, n: int) -> list[dict]:
    """IPv4 with options whose window ends past 64 B under 6 chunks (the byte path under 4)."""
    out = []
    for i in range(n):
        proto = (6, 17, 1)[i % 3]
        ihl = {6: 8 + i % 8, 17: 11 + i % 5, 1: 12 + i % 4}[proto]
        need = ihl * 4 + O.L4_FIELD[proto] + 2
        r0 = max(65 - need, 0) + (i * 7) % (16 - max(65 - need, 0))
        out.append(_vec(rng, f"round2:v4 {PROTO_NAME[proto]} ihl {ihl} r0+need {r0 + need}", 4, proto, r0=r0, ihl=ihl))
    return out


def _hi6(rng, n: int) -> list[dict]:
    return [_vec(rng, f"round2:v6 tcp r0+need {58 + 7 + i % 9}", 6, 6, r0=7 + i % 9) for i in range(n)]


def _masks(rng) -> list[dict]:
    out = []
    kinds = [(4, 6), (4, 17), (4, 1), (6, 6), (6, 17), (6, 58), (6, 1)]
    masks = [(m, None, None) for m in (0, 1, 2, 4, 8, 16, 32, 63)] + \
            [(O.NAT_SET_TTL | O.NAT_DEC_TTL, s, None) for s in (0, 1, 2)] + \
            [(63, 0, None), (O.NAT_DEC_TTL, None, 2), (O.NAT_DEC_TTL | O.NAT_SRC, None, 1), (O.NAT_DEC_TTL, None, 0)]
    for k, (ver, proto) in enumerate(kinds):
        for j, (m, s, ttl) in enumerate(masks):
            r0 = (3 * j + k) % (7 if ver == 6 else 16)   # IPv6 TCP: need 58, within 64 up to r0 6
            out.append(_vec(rng, f"masks:v{ver} {PROTO_NAME[proto]} mask {m:#x} set {s} ttl {ttl}", ver, proto, r0=r0,
                            mask=m, set_ttl=s, ttl=ttl))
    return out


def _sums(rng) -> list[dict]:
    out = []
    for ver, ihl, ext, r0s in ((4, 5, None, (1, 14)), (4, 8, None, (0, 11)), (6, 5, None, (0, 5)), (6, 5, 2, (3, 12))):
        for r0 in r0s:
            name = f"v{ver} ihl {ihl} ext {ext} r0 {r0}"
            out.append(_vec(rng, f"sums:udp stored 0 {name}", ver, 17, r0=r0, ihl=ihl, ext=ext, mask=ADDR_PORTS, sum_edge="udp0"))
            out.append(_vec(rng, f"sums:udp stored 0, ttl only {name}", ver, 17, r0=r0, ihl=ihl, ext=ext,
                            mask=O.NAT_DEC_TTL, sum_edge="udp0_ttl"))
            out.append(_vec(rng, f"sums:udp stored ffff {name}", ver, 17, r0=r0, ihl=ihl, ext=ext, mask=ADDR_PORTS,
                            sum_edge="udp_ffff"))
            for proto in (17, 6):
                out.append(_vec(rng, f"sums:new sum 0 {PROTO_NAME[proto]} {name}", ver, proto, r0=r0, ihl=ihl, ext=ext,
                                mask=ADDR_PORTS, sum_edge="new0"))
    return out


def _mixed(rng, i: int) -> dict:
    """Packet i of a mixed wave: eleven kinds in turn, so each lands on every lane mod 4."""
    kind = MIXED_KINDS[i % len(MIXED_KINDS)]
    j = i // len(MIXED_KINDS)
    cls = f"mixed:{kind}"
    if kind == "win4":
        return _vec(rng, cls, 4, (6, 17, 1)[j % 3], r0=(5 * j) % 16, mask=ADDR_PORTS)
    if kind == "win6":
        return _vec(rng, cls, 6, (6, 17, 58)[j % 3], r0=j % 7, mask=ADDR_PORTS)
    if kind == "byte6":   # l4_off 88: past any window
        return _vec(rng, cls, 6, (6, 17, 58, 1)[j % 4], r0=(3 * j + 1) % 16, ext=40, mask=ADDR_PORTS)
    if kind == "byte4":   # IHL 15, TCP: need 78, past a 4-chunk window
        return _vec(rng, cls, 4, 6, r0=(7 * j) % 16, ihl=15, mask=ADDR_PORTS)
    if kind in ("outside", "far"):
        return _vec(rng, cls, 4, 17, bad=kind)
    if kind == "ver5":
        return _vec(rng, cls, 4, 6, r0=(3 * j) % 16, bad="ver5")
    if kind == "ttl_win":   # TTL 1 / 0 in a window
        return _vec(rng, cls, 4, (6, 17, 1)[j % 3], r0=(3 * j) % 16, mask=O.NAT_DEC_TTL | O.NAT_SRC, ttl=1 - j % 2)
    if kind == "ttl_set":   # the set value expires, the header's TTL is fine; IPv6: the hop limit
        if j % 2:
            return _vec(rng, cls, 6, 6, r0=j % 7, mask=O.NAT_DEC_TTL | O.NAT_DST, ttl=1)
        return _vec(rng, cls, 4, 17, r0=j % 16, mask=63, set_ttl=(j // 2) % 2)
    if kind == "ttl_byte4":   # refused on the byte path of a 4-chunk window
        return _vec(rng, cls, 4, 6, r0=(5 * j) % 16, ihl=15, mask=O.NAT_DEC_TTL | ADDR_PORTS, ttl=j % 2)
    return _vec(rng, cls, 6, 17, r0=j % 16, ext=40, mask=O.NAT_DEC_TTL | ADDR_PORTS, ttl=1)   # ... of any window


TAIL_KINDS = {"field_end": {6: 18, 17: 8, 1: 4}, "short": {6: 17, 17: 7, 1: 3}, "no_l4": {6: 0, 17: 0, 1: 0}}


def _tails(rng) -> list[dict]:
    out = []
    for ver, ihl in ((4, 5), (4, 7), (6, 5)):
        for kind, lens in TAIL_KINDS.items():
            for proto, n in lens.items():
                p = 58 if ver == 6 and proto == 1 and kind != "short" else proto   # ICMPv4 in IPv6 too (short)
                for tail in range(4):
                    out.append(_vec(rng, f"tails:{kind} v{ver} ihl {ihl} {PROTO_NAME[p]}", ver, p, ihl=ihl, seg_len=n,
                                    tail=tail, mask=ADDR_PORTS | (O.NAT_DEC_TTL if tail & 1 else 0)))
    return out


# ----------------------------------------------------------------------------------------
# The batch
# ----------------------------------------------------------------------------------------
def _wend6(v: dict) -> int:
    """wend under a 6-chunk window and the 48-B entries, from the vector's own placement."""
    need = 20 if v["ver"] == 4 else 40
    if l4sum(v["ver"], v["proto"], len(v["l3"]), v["l4_off"]):
        need = max(need, v["l4_off"] + O.L4_FIELD[v["proto"]] + 2)
    return v["r0"] + need if v["r0"] + need <= 96 else 0


def vectors(seed: int = 31) -> list[dict]:
    """The vectors in batch order: whole waves of 64, then the packed tails."""
    rng = np.random.default_rng(seed)
    out = [_mixed(rng, i) for i in range(2 * WAVE)]
    pool = _win4(rng) + _win6(rng) + _round2_v6(rng) + _masks(rng) + _sums(rng)
    hi4 = [v for v in pool if v["ver"] == 4 and _wend6(v) > 64]
    hi6 = [v for v in pool if v["ver"] == 6 and _wend6(v) > 64]
    lo = [v for v in pool if _wend6(v) <= 64]
    assert len(hi4) >= 6 and len(hi6) >= 8 and len(lo) >= WAVE
    ones = [(0, hi4), (1, hi6), (2, hi4), (3, hi6), (34, hi4), (63, hi4)]   # lane of the one packet past 64
    while len(ones) * (WAVE - 1) < len(lo):
        ones.append((5 * len(ones) % WAVE, hi4))
    fresh = iter(lo)

    def low():   # the next unused low vector, or another copy of one already placed
        v = next(fresh, None)
        return v if v is not None else dict(lo[int(rng.integers(0, len(lo)))])

    for lane, src in ones:
        wave = [low() for _ in range(WAVE - 1)]
        wave.insert(lane, src.pop())
        out += wave
    out += [low() for _ in range(WAVE)]                      # no packet past 64
    out += hi4 + _hi4(rng, WAVE - len(hi4) % WAVE)                  # every packet past 64 (IPv4)
    out += hi6 + _hi6(rng, WAVE - len(hi6) % WAVE)           # every packet past 64 (IPv6; refused under 16-B formats)
    assert next(fresh, None) is None and len(out) % WAVE == 0
    return out + _tails(rng)


def pack(vecs: list[dict], seed: int = 5) -> dict:
    """{arena, desc, rw, vecs}: a vector with r0 goes to the next address that is r0 mod 16, one with
    a tail follows its neighbour after the 0..3 bytes that give (r0 + len) & 3 == tail.  Random filler
    everywhere else; the last packet ends on the arena's last byte."""
    rng = np.random.default_rng(seed)
    pos, offs = 0, []
    for v in vecs:
        if v["bad"] in ("outside", "far"):
            offs.append(None)
            continue
        if v["r0"] is not None:
            p = (pos & ~15) + v["r0"]
            p += 16 if p < pos else 0
        else:
            p = pos + ((v["tail"] - (pos + len(v["l3"]))) & 3)
        offs.append(p)
        pos = p + len(v["l3"])
    assert offs[-1] is not None
    arena = rng.integers(0, 256, pos, dtype=np.uint8)
    rows = []
    for v, o in zip(vecs, offs):
        if o is None:   # reaching past the arena's end / starting beyond it
            o = len(arena) - 10 if v["bad"] == "outside" else (1 << 40) + 64
        else:
            arena[o:o + len(v["l3"])] = np.frombuffer(v["l3"], np.uint8)
        rows.append((o, len(v["l3"]), v["l4_off"], 5 if v["bad"] == "ver5" else v["ver"], v["proto"], 0, 0))
    return dict(arena=arena, desc=np.array(rows, O.DESC_DTYPE), rw=np.array([v["rw"] for v in vecs], O.NAT_DTYPE),
                vecs=vecs)


def batch(seed: int = 31) -> dict:
    return pack(vectors(seed))


def corrupted(b: dict) -> dict:
    """The batch with wrong incoming sums (IPv4 header sum and the L4 field, where the packet has
    one): RFC 1624 would carry the error on, strict Java recomputes and must equal the oracle."""
    a = b["arena"].copy()
    for v, d in zip(b["vecs"], b["desc"]):
        if v["bad"] in ("outside", "far"):
            continue
        o, ln, l4o = int(d["l3_off"]), int(d["l3_len"]), int(d["l4_off"])
        if v["ver"] == 4:
            a[o + 10] ^= 0x5A
        if l4sum(v["ver"], v["proto"], ln, l4o):
            a[o + l4o + O.L4_FIELD[v["proto"]] + 1] ^= 0x33
    return dict(b, arena=a)


def strided(n: int, seed: int = 41) -> dict:
    """{arena, desc, rw}: n IPv4 packets of 28..60 bytes (IHL 5; TCP, UDP, ICMP) at a 64-byte
    stride with valid sums and random filler behind each, for the grid-stride loop's second trip:
    built with numpy, a quarter of a million packets in well under a second.  TCP segments under
    18 bytes hold no checksum field; 3% of the UDP fields are a stored 0."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(28, 61, n)
    proto = rng.choice(np.array([6, 17, 1]), n)
    A = rng.integers(0, 256, (n, 64), dtype=np.uint8)
    A[:, 0], A[:, 2], A[:, 3], A[:, 9] = 0x45, 0, lens, proto
    A[:, 8] = np.where(rng.random(n) < 0.02, rng.integers(0, 2, n), rng.integers(2, 256, n))   # a few expire
    udp, tcp = proto == 17, proto == 6
    A[udp, 24], A[udp, 25] = 0, (lens - 20)[udp]
    A[:, 10:12] = 0
    ip = A[:, :20].reshape(n, 10, 2).astype(np.uint32)
    s = (ip[:, :, 0] << 8 | ip[:, :, 1]).sum(axis=1)
    s = (s & 0xFFFF) + (s >> 16)
    s = ~((s & 0xFFFF) + (s >> 16)) & 0xFFFF
    A[:, 10], A[:, 11] = s >> 8, s & 0xFF
    fld = 20 + np.select([tcp, udp], [16, 6], 2)
    has = lens >= fld + 2
    M = A.astype(np.uint32)
    M[np.arange(64)[None, :] >= lens[:, None]] = 0
    rows = np.arange(n)
    M[rows[has], fld[has]] = 0
    M[rows[has], fld[has] + 1] = 0
    w = M.reshape(n, 32, 2)
    w = (w[:, :, 0] << 8 | w[:, :, 1]).astype(np.int64)
    s = w[:, 10:].sum(axis=1) + np.where(tcp | udp, w[:, 6:10].sum(axis=1) + proto + (lens - 20), 0)
    s = (s & 0xFFFF) + (s >> 16)
    s = ~((s & 0xFFFF) + (s >> 16)) & 0xFFFF
    s = np.where(udp & (s == 0), 0xFFFF, s)
    s = np.where(udp & (rng.random(n) < 0.03), 0, s)
    A[rows[has], fld[has]] = (s >> 8)[has]
    A[rows[has], fld[has] + 1] = (s & 0xFF)[has]
    desc = np.zeros(n, O.DESC_DTYPE)
    desc["l3_off"], desc["l3_len"], desc["l4_off"], desc["l3_ver"], desc["l4_proto"] = rows * 64, lens, 20, 4, proto
    rw = np.zeros(n, O.NAT_DTYPE)
    rw.view(np.uint8).reshape(n, 48)[:, :36] = rng.integers(0, 256, (n, 36), dtype=np.uint8)
    rw["mask"], rw["ttl"] = rng.integers(0, 64, n), rng.integers(0, 256, n)
    return dict(arena=A.reshape(-1), desc=desc, rw=rw)


def nat4_entries(rw48: np.ndarray) -> np.ndarray:
    """The 16-B IPv4 entries of 48-B ones (rsv[0]: the SET_TTL value)."""
    r4 = np.zeros(len(rw48), O.NAT4_DTYPE)
    r4["src"], r4["dst"] = rw48["src"][:, :4], rw48["dst"][:, :4]
    r4["sport"], r4["dport"], r4["mask"] = rw48["sport"], rw48["dport"], rw48["mask"]
    r4["rsv"][:, 0] = rw48["ttl"]
    return r4


def entries(desc: np.ndarray, rw48: np.ndarray, fmt: int) -> np.ndarray:
    """The rewrite table of entry format fmt as bytes: vpcsum_nat4_t, vpcsum_nat_t, or
    vpcsum_nat4_rec_t records (which carry the descriptors too)."""
    if fmt == 1:
        return np.ascontiguousarray(rw48).view(np.uint8)
    if fmt == 0:
        return nat4_entries(rw48).view(np.uint8)
    rec = np.zeros(len(desc), NAT4R_DTYPE)
    rec["desc"], rec["rw"] = desc, nat4_entries(rw48)
    return rec.view(np.uint8)


def expect(orc, arena: np.ndarray, desc: np.ndarray, rw48: np.ndarray, fmt: int, n: int | None = None):
    """(arena, status) after the first n packets' rewrites, from the C oracle: orc.nat_java for the
    48-B entries, orc.nat4_java (IPv6 refused) for the 16-B entries and the records."""
    n = len(desc) if n is None else n
    want = arena.copy()
    if fmt == 1:
        st = orc.nat_java(want, desc[:n], rw48[:n])
    else:
        st = orc.nat4_java(want, desc[:n], nat4_entries(rw48[:n]))
    return want, st


def describe(b: dict, i: int, fmt: int, ch: int, base: int = 0) -> str:
    """Packet i's class and geometry, for a failing comparison's message."""
    ok, r0, need, wend, tail = geometry(b["desc"][i], len(b["arena"]), fmt, ch, base)
    return f"packet {i} [{b['vecs'][i]['cls']}] ok {ok} r0 {r0} need {need} wend {wend} tail {tail} wave lane {i % WAVE}"


def first_diff(b: dict, got: np.ndarray, want: np.ndarray, fmt: int, ch: int, base: int = 0) -> str:
    """Which packet (or gap) the first differing arena byte belongs to."""
    at = int(np.nonzero(got != want)[0][0])
    for i, d in enumerate(b["desc"]):
        o = int(d["l3_off"])
        if o <= at < o + int(d["l3_len"]) and b["vecs"][i]["bad"] not in ("outside", "far"):
            return f"arena byte {at} (L3 + {at - o}): " + describe(b, i, fmt, ch, base)
    return f"arena byte {at}: in no packet"


# ----------------------------------------------------------------------------------------
# The classes, recomputed from the descriptors
# ----------------------------------------------------------------------------------------
def check_classes(b: dict, orc) -> dict:
    """Asserts that every class above is in the batch, from the descriptors, the entries and the
    arena alone (the vectors' own labels are not consulted); returns the classes' sizes."""
    arena, desc, rw = b["arena"], b["desc"], b["rw"]
    n, alen = len(desc), len(arena)
    G = {(fmt, ch): [geometry(d, alen, fmt, ch) for d in desc] for fmt, ch in ((0, 4), (0, 6), (1, 6), (2, 4), (2, 6))}
    size = {}

    def l3(i):
        o = int(desc[i]["l3_off"])
        return arena[o:o + int(desc[i]["l3_len"])].tobytes()

    # win4: IPv4 around the 4-chunk limit, per protocol, every IHL that reaches it
    for proto in (6, 17, 1):
        hit = {}
        for i, (ok, r0, need, wend, _) in enumerate(G[(0, 4)]):
            if ok and desc[i]["l4_proto"] == proto and r0 + need in (63, 64, 65):
                hit.setdefault(int(desc[i]["l4_off"]), set()).add(r0 + need)
                assert (wend == 0) == (r0 + need == 65)
        fld = O.L4_FIELD[proto]
        reach = {l4o for l4o in range(20, 64, 4) for t in (63, 64, 65) if 0 <= t - (l4o + fld + 2) <= 15}
        assert set(hit) >= reach, ("win4", proto, sorted(reach - set(hit)))
        for l4o in reach:
            assert hit[l4o] == {t for t in (63, 64, 65) if 0 <= t - (l4o + fld + 2) <= 15}, ("win4", proto, l4o)
        size[f"win4 {PROTO_NAME[proto]}"] = sum(len(s) for s in hit.values())
    # win6: IPv6 with an extension header around the 6-chunk limit
    for proto in (6, 17, 58, 1):
        ts, parity = set(), set()
        for i, (ok, r0, need, wend, _) in enumerate(G[(1, 6)]):
            if ok and desc[i]["l3_ver"] == 6 and desc[i]["l4_proto"] == proto and r0 + need in (95, 96, 97):
                assert desc[i]["l4_off"] >= 48 and (wend == 0) == (r0 + need == 97)
                ts.add(r0 + need)
                parity.add((r0 + need, int(desc[i]["l4_off"]) & 1))
        assert ts == {95, 96, 97} and len(parity) >= 5, ("win6", proto, ts, parity)
        size[f"win6 {PROTO_NAME[proto]}"] = len(parity)
    assert not any(ok and desc[i]["l3_ver"] == 4 and r0 + need > 93 for i, (ok, r0, need, _, _) in enumerate(G[(0, 6)]))
    # round2: waves with none, exactly one, and all of their packets past 64, under every 6-chunk format
    for fmt in (0, 1, 2):
        per_wave = [sum(1 for g in G[(fmt, 6)][w:w + WAVE] if g[3] > 64) for w in range(0, n - WAVE + 1, WAVE)]
        assert {0, 1, WAVE} <= set(per_wave), ("round2", fmt, per_wave)
        ones = [w for w, c in enumerate(per_wave) if c == 1]
        lanes = {next(k for k in range(WAVE) if G[(fmt, 6)][w * WAVE + k][3] > 64) for w in ones}
        assert len(lanes) >= 4 and len({k & 3 for k in lanes}) >= 3, ("round2 lanes", fmt, lanes)
        size[f"round2 fmt {fmt} waves none/one/all"] = (per_wave.count(0), len(ones), per_wave.count(WAVE))
        near = {g[3] for i, g in enumerate(G[(fmt, 6)]) if g[3] in (63, 64, 65)}
        assert near == {63, 64, 65}, ("round2 threshold", fmt, near)
        if fmt == 1:
            near6 = {g[3] for i, g in enumerate(G[(1, 6)]) if desc[i]["l3_ver"] == 6 and desc[i]["l4_off"] == 40}
            assert {63, 64, 65} <= near6
    # mixed: one wave holding every kind, each on every lane mod 4
    for fmt, ch in ((0, 4), (0, 6), (1, 6), (2, 4), (2, 6)):
        kinds = {}
        for k in range(WAVE):
            ok, r0, need, wend, _ = G[(fmt, ch)][k]
            d = desc[k]
            if not ok:
                off, ln = int(d["l3_off"]), int(d["l3_len"])
                kind = "far" if off > alen else "outside" if ln > alen - off else f"ver{int(d['l3_ver'])}"
            elif expired(l3(k), int(d["l3_ver"]), rw[k]):
                kind = "expired window" if wend else "expired byte path"
            else:
                kind = "window" if wend else "byte path"
            kinds.setdefault(kind, set()).add(k & 3)
        must = {"window", "expired window", "far", "outside", "ver5"}
        must |= {"ver6"} if fmt != 1 else set()
        must |= {"byte path", "expired byte path"} if (fmt, ch) != (0, 6) and (fmt, ch) != (2, 6) else set()
        assert must <= set(kinds), ("mixed", fmt, ch, sorted(kinds))
        assert all(kinds[k] == {0, 1, 2, 3} for k in must), ("mixed lanes", fmt, ch, kinds)
        size[f"mixed fmt {fmt} ch {ch}"] = len(kinds)
    # tails: the three packet ends, per protocol, at every tail, packed with gaps of 0..3 bytes
    placed = sorted((int(d["l3_off"]), int(d["l3_len"]), i) for i, d in enumerate(desc) if int(d["l3_off"]) + int(d["l3_len"]) <= alen)
    nxt = {i: placed[k + 1][0] - (o + ln) if k + 1 < len(placed) else None for k, (o, ln, i) in enumerate(placed)}
    assert placed[-1][0] + placed[-1][1] == alen, "the last packet ends on the arena's last byte"
    assert all(g is None or g >= 0 for g in nxt.values()), "packets overlap"
    for fmt in (0, 1):
        for ver in ((4,) if fmt == 0 else (4, 6)):
            for kind in TAIL_KINDS:
                for proto in (6, 17, 1, 58):
                    if (ver == 4 and proto == 58):
                        continue
                    fld = O.L4_FIELD[proto]
                    tails, gaps = set(), set()
                    for i, (ok, r0, need, wend, tail) in enumerate(G[(fmt, 6)]):
                        d = desc[i]
                        seg = int(d["l3_len"]) - int(d["l4_off"])
                        if not ok or d["l3_ver"] != ver or d["l4_proto"] != proto or nxt[i] is not None and nxt[i] > 3:
                            continue
                        if seg == {"field_end": fld + 2, "short": fld + 1, "no_l4": 0}[kind]:
                            tails.add(tail)
                            gaps.add(nxt[i])
                    if ver == 6 and (kind, proto) in (("short", 58), ("field_end", 1), ("no_l4", 1)):
                        continue   # ICMPv6 and ICMPv4 share one shape inside IPv6: each kind has one of them
                    assert tails == {0, 1, 2, 3}, ("tails", fmt, ver, kind, proto, tails)
                    size[f"tails v{ver} {kind} {PROTO_NAME[proto]}"] = len(gaps)
    packed_gaps = {g for i, g in nxt.items() if g is not None and G[(1, 6)][i][0] and
                   int(desc[i]["l3_len"]) - int(desc[i]["l4_off"]) <= 18}
    assert {0, 1, 2, 3} <= packed_gaps, ("tails gaps", packed_gaps)
    # sums and masks: against what the oracle leaves
    want = {fmt: expect(orc, arena, desc, rw, fmt) for fmt in (0, 1)}
    for fmt, vers in ((0, (4,)), (1, (4, 6))):
        w, st = want[fmt]
        for ver in vers:
            seen = set()
            masks = set()
            for i, (ok, r0, need, wend, _) in enumerate(G[(fmt, 6)]):
                d = desc[i]
                if not ok or d["l3_ver"] != ver:
                    continue
                m = int(rw[i]["mask"])
                masks.add((m, int(rw[i]["ttl"])) if m == O.NAT_SET_TTL | O.NAT_DEC_TTL else m)
                proto, l4o = int(d["l4_proto"]), int(d["l4_off"])
                if not l4sum(ver, proto, int(d["l3_len"]), l4o) or st[i] != O.S_DONE:
                    continue
                f = int(d["l3_off"]) + l4o + O.L4_FIELD[proto]
                old = int.from_bytes(arena[f:f + 2].tobytes(), "big")
                new = int.from_bytes(w[f:f + 2].tobytes(), "big")
                touched = m & ADDR_PORTS and proto in (6, 17)
                if proto == 17 and old == 0:
                    seen.add("udp0 recomputed" if new else "udp0 kept")
                    assert (new != 0) == bool(touched)
                elif proto == 17 and old == 0xFFFF and touched:
                    seen.add("udp ffff")
                elif proto == 17 and new == 0xFFFF and touched:
                    seen.add("udp new ffff")
                elif proto == 6 and new == 0 and touched:
                    seen.add("tcp new 0")
            assert seen == {"udp0 recomputed", "udp0 kept", "udp ffff", "udp new ffff", "tcp new 0"}, ("sums", fmt, ver, seen)
            need_masks = {0, 1, 2, 4, 8, 16, 32, 63} | {(O.NAT_SET_TTL | O.NAT_DEC_TTL, s) for s in (0, 1, 2)}
            assert need_masks <= masks, ("masks", fmt, ver, need_masks - masks)
            size[f"sums fmt {fmt} v{ver}"] = len(seen)
            size[f"masks fmt {fmt} v{ver}"] = len(masks)
    return size
