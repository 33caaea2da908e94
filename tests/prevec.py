"""Crafted vectors for the pre-image flush kernel's window, store and loop geometry (test
infrastructure: tests/ only): tests/natvec.py's batch turned into pre-image form -- Java's setters
applied, each packet's dirty flags plus F_PRE, its pre-image -- and the classes only the pre-image
path has.  check_classes() recomputes from the descriptors, the entries and the arena that every one
of them is there.

What k_pre (vproxy_amd/csrc/nat.hip) decides per packet, restated in geometry():

* act   the descriptor carries F_PRE (another one's status byte and out word are not the kernel's);
* ok    pre_desc_ok (pre_common.h): F_IP and / or F_L4 and nothing else, F_IP on IPv4 only,
        nat_desc_ok's bounds, with F_L4 an L4 checksum field inside the segment;
* need  max(20 | 40, F_L4 ? min(len, l4_off + max(field + 2, header-sum hlen)) : l4_off);
* wend  r0 + need when that fits the window of CH 16-B chunks, else 0 (the byte path);
* r2    wend > 64: the wave runs the second quad round.

The classes added to natvec's (each in whole waves of 64):

  ip_only      TTL-only masks and ICMPv4 under address rewrites: F_IP alone, need = l4_off, at
               every IHL 5..15 and every r0.
  hsum4/hsum6  VPCSUM_PRE_HSUM entries (TCP with options, UDP) with r0 + l4_off + hlen in {63, 64,
               65, 95, 96, 97}; addresses, ports, seq / ack, flags and a byte of the header's last
               4 edited in place; expected bytes are the oracle's full recompute.
  hsum_round2  waves of header-sum packets with wend > 64 in no packet, in exactly one (at four lanes,
               one of each lane mod 4) and in every packet.
  hsum_bad     records that do not describe their packet (segment length, header length, hlen 255
               on a shorter packet, a data offset changed in the frame, protocol, version, no
               record): S_BAD_DESC, out 0, the frame untouched.  One ends on the arena's last byte.
  refused      every pre_desc_ok refusal, each on every lane mod 4.
  quads        one wave whose 16 quads show all 16 F_PRE / non-F_PRE patterns (store_bytes_masked).
  svc384       IPv6 UDP behind a long extension header with r0 + need in {383, 384, 385} under the
               service grid's rule (kernels.hip svc_pre_packet: max(l4_off + field + 2, min(len,
               l4_off + 60)) against its 24 chunks); byte-path packets for k_pre.
"""
from __future__ import annotations

from collections import namedtuple

import numpy as np

import hsumvec as H
import natvec as NV
import tcprwvec as T
from oracle import oracle as O

WAVE = NV.WAVE
NAT_FIELDS = O.NAT_SRC | O.NAT_DST | O.NAT_SPORT | O.NAT_DPORT
GUARD = 0xEE                     # status bytes the kernel must leave alone
OUT_GUARD = 0xEEEEEEEE           # out words likewise
SVC_CHUNKS = 24                  # kernels.hip kSvcPreChunks
HSUM_TARGETS = (63, 64, 65, 95, 96, 97)
REFUSED_KINDS = ("l4p", "raw", "ip_on_v6", "no_field", "pre_alone", "v6", "outside", "far", "ver5")
BAD_KINDS = ("l4_len", "hlen", "hlen255_short", "hlen255_long", "doff_in_frame", "proto", "ver", "no_record")


# ----------------------------------------------------------------------------------------
# Helpers shared with tests/test_gpu_pre.py
# ----------------------------------------------------------------------------------------
def pre_images(arena, desc, rw):
    """The vswitch's pre-images (old values of the fields each entry rewrites), recorded from the
    frames before the setters run."""
    from vproxy_amd import vswitch as S
    pre = np.zeros(len(desc), O.NAT_DTYPE)
    for i, d in enumerate(desc):
        pre[i] = S.record_pre_image(arena, int(d["l3_off"]), int(d["l3_ver"]), int(d["l4_off"]), int(d["l4_proto"]),
                                    int(rw[i]["mask"]) & NAT_FIELDS)
    return pre


def nat4_of(rw48):
    r4 = np.zeros(len(rw48), O.NAT4_DTYPE)
    r4["src"], r4["dst"] = rw48["src"][:, :4], rw48["dst"][:, :4]
    r4["sport"], r4["dport"], r4["mask"] = rw48["sport"], rw48["dport"], rw48["mask"]
    return r4


def java_dirty_flags(desc, rw):
    """F_IP / F_L4 as Java's setters leave a packet (checksumSkipped): IPv4 addresses and the TTL
    dirty the header (Ipv4Packet.java:401-458); addresses dirty the L4 sum through the pseudo header
    of TCP / UDP, and of ICMP / ICMPv6 under IPv6 (pseudoHeaderChanges, Ipv4Packet.java:236-240,
    Ipv6Packet.java:238-242); ports dirty TCP / UDP; an L4 packet without its checksum field in the
    segment is never dirty.  The egress defers exactly these (SwitchUtils.checksumFlagsFor)."""
    v4 = desc["l3_ver"] == 4
    proto = desc["l4_proto"].astype(int)
    fld = np.array([O.L4_FIELD.get(int(p), -1) for p in proto])
    l4sum = (fld >= 0) & ~(v4 & (proto == 58)) & \
        (desc["l3_len"].astype(int) - desc["l4_off"].astype(int) >= fld + 2)
    m = rw["mask"].astype(int)
    tcpudp = (proto == 6) | (proto == 17)
    addr_dirty = l4sum & (tcpudp | (~v4 & ((proto == 1) | (proto == 58))))
    ip = v4 & ((m & (O.NAT_SRC | O.NAT_DST | O.NAT_SET_TTL | O.NAT_DEC_TTL)) != 0)
    l4 = (((m & (O.NAT_SRC | O.NAT_DST)) != 0) & addr_dirty) | (l4sum & tcpudp & ((m & (O.NAT_SPORT | O.NAT_DPORT)) != 0))
    return (np.where(ip, O.F_IP, 0) | np.where(l4, O.F_L4, 0)).astype(np.uint8)


# ----------------------------------------------------------------------------------------
# The kernel's per-packet decisions (pre_common.h: pre_desc_ok, pre_hsum_hlen, pre_sums' record
# check; nat.hip k_pre: need, wend, the second round)
# ----------------------------------------------------------------------------------------
Geo = namedtuple("Geo", "act ok r0 need wend r2")


def _raw(entry) -> np.ndarray:
    return np.frombuffer(np.asarray(entry, O.NAT_DTYPE).tobytes(), np.uint8)


def is_hsum(entry) -> bool:
    return bool(int(entry["mask"]) & O.PRE_HSUM)


def hsum_hlen(entry) -> int:
    """pre_hsum_hlen: the L4 header length a header-sum entry asks for (its record's byte 4)."""
    return int(_raw(entry)[4]) if is_hsum(entry) else 0


def pre_desc_ok(d, arena_len: int, fmt: int) -> bool:
    fl = int(d["flags"])
    if fl & ~(O.F_IP | O.F_L4 | O.F_PRE) or not fl & (O.F_IP | O.F_L4):
        return False
    if fl & O.F_IP and int(d["l3_ver"]) != 4:
        return False
    if not NV.desc_ok(d, arena_len, fmt):
        return False
    return not fl & O.F_L4 or NV.l4sum(int(d["l3_ver"]), int(d["l4_proto"]), int(d["l3_len"]), int(d["l4_off"]))


def geometry(d, entry, arena_len: int, fmt: int, ch: int, base: int = 0) -> Geo:
    """k_pre's decision for descriptor d and its 48-B entry, for entry format fmt and a window of ch
    chunks, the arena at an address that is `base` mod 16."""
    ln, l4o, ver, proto, fl = int(d["l3_len"]), int(d["l4_off"]), int(d["l3_ver"]), int(d["l4_proto"]), int(d["flags"])
    act = bool(fl & O.F_PRE)
    ok = act and pre_desc_ok(d, arena_len, fmt)
    r0 = (base + int(d["l3_off"])) & 15 if ok else 0
    need = l4o
    if fl & O.F_L4:
        need = min(ln, l4o + max(O.L4_FIELD.get(proto, -1) + 2, hsum_hlen(entry)))
    need = max(20 if ver == 4 else 40, need)
    wend = r0 + need if ok and r0 + need <= 16 * ch else 0
    return Geo(act, ok, r0, need, wend, wend > 64)


def svc_need(d) -> int:
    """svc_pre_packet's window rule (read in one round trip with the entry, so without its hlen)."""
    ln, l4o, ver, proto = int(d["l3_len"]), int(d["l4_off"]), int(d["l3_ver"]), int(d["l4_proto"])
    need = l4o
    if int(d["flags"]) & O.F_L4:
        need = max(l4o + O.L4_FIELD.get(proto, -1) + 2, min(ln, l4o + 60))
    return max(20 if ver == 4 else 40, need)


def record_ok(l3: bytes, d, entry) -> bool:
    """pre_sums' test that a header-sum record describes the packet now at l3."""
    ln, l4o, ver, proto = int(d["l3_len"]), int(d["l4_off"]), int(d["l3_ver"]), int(d["l4_proto"])
    rec = np.frombuffer(_raw(entry)[:8].tobytes(), O.HSUM_DTYPE)[0]
    if proto not in (6, 17):
        return False
    cur = (l3[l4o + 12] >> 4) * 4 if proto == 6 else 8
    hlen = int(rec["hlen"])
    return bool(rec["l2_len"] != 0 and rec["l3_ver"] == ver and rec["l4_proto"] == proto and
                rec["l4_len"] == ln - l4o and hlen == cur and hlen <= ln - l4o)


# ----------------------------------------------------------------------------------------
# The added classes' vectors (natvec's dicts, plus "pre": what differs from a NAT'd packet)
# ----------------------------------------------------------------------------------------
def _nat(rng, cls: str, ver: int, proto: int, **kw) -> dict:
    kw.setdefault("mask", NV.ADDR_PORTS)
    return NV._vec(rng, cls, ver, proto, **kw)


def _hsum(rng, cls: str, ver: int, proto: int, r0: int | None, hlen: int, ihl: int = 5, ext: int | None = None,
          payload: int | None = None, bad: str | None = None, tail: int | None = None) -> dict:
    """A received TCP (hlen 20..60: NOP options) / UDP (hlen 8) packet with valid sums, its ingress
    header sum (oracle.hsum_record of the packet behind an Ethernet header), then the in-place edits
    of the summed words.  bad: the way its record stops describing it."""
    payload = int(rng.integers(0, 12)) if payload is None else payload
    seg = H._tcp(rng, payload, False, None, (hlen - 20) // 4) if proto == 6 else H._udp(rng, payload)
    l4_off = ihl * 4 if ver == 4 else 40 + (0 if ext is None else 8 + ext)
    l3 = T.l3_sums(H._l3(rng, ver, seg, proto, ihl=ihl, ext=ext), ver, proto, l4_off)
    rec = O.hsum_record(H.ether(rng, bytes(l3), ver, False)).copy()
    assert rec["l2_len"] == 14 and rec["hlen"] == hlen and rec["l4_len"] == len(l3) - l4_off, cls
    e = bytearray(l3)
    a0, alen = (12, 8) if ver == 4 else (8, 32)
    e[a0:a0 + alen] = rng.integers(0, 256, alen, dtype=np.uint8).tobytes()                # addresses
    e[l4_off:l4_off + 4] = rng.integers(0, 256, 4, dtype=np.uint8).tobytes()              # ports
    if proto == 6:
        e[l4_off + 4:l4_off + 12] = rng.integers(0, 256, 8, dtype=np.uint8).tobytes()     # seq / ack
        e[l4_off + 13] ^= 0x12                                                             # flags
        k = l4_off + hlen - 1 - int(rng.integers(0, 2 if hlen == 20 else 4))               # the last option
        e[k] ^= 1 + int(rng.integers(0, 255))                                              # word / urgent pointer
    if bad == "l4_len":
        rec["l4_len"] += 4
    elif bad == "hlen":
        rec["hlen"] += 4
    elif bad in ("hlen255_short", "hlen255_long"):
        rec["hlen"] = 255
    elif bad == "doff_in_frame":
        e[l4_off + 12] = (e[l4_off + 12] & 0x0F) | (((hlen - 4 if hlen > 20 else hlen + 4) // 4) << 4)
    elif bad == "proto":
        rec["l4_proto"] ^= 6 ^ 17
    elif bad == "ver":
        rec["l3_ver"] ^= 4 ^ 6
    elif bad == "no_record":
        rec["l2_len"] = 0
    rw = np.zeros(1, O.NAT_DTYPE)[0]   # no setter runs: the edits above are the change
    return dict(cls=cls, l3=bytes(l3), ver=ver, proto=proto, l4_off=l4_off, rw=rw, r0=r0, tail=tail, bad=None,
                sum_edge=None, pre=dict(rec=rec, edited=bytes(e), flags=O.F_L4 | O.F_PRE | (O.F_IP if ver == 4 else 0)))


def _ip_only(rng) -> list[dict]:
    """176 packets: every (IHL, r0) pair once, TTL-only masks on TCP / UDP and ICMPv4 under address
    rewrites in turn; 16 more of them fill the third wave."""
    out = []
    for i in range(3 * WAVE):
        ihl, r0 = 5 + i % 11, i % 16
        if i % 2:
            out.append(_nat(rng, f"ip_only:icmp ihl {ihl}", 4, 1, r0=r0, ihl=ihl, mask=(O.NAT_SRC, O.NAT_DST, 3)[i % 3]))
        else:
            m = (O.NAT_DEC_TTL, O.NAT_SET_TTL, O.NAT_SET_TTL | O.NAT_DEC_TTL)[(i // 2) % 3]
            out.append(_nat(rng, f"ip_only:ttl ihl {ihl}", 4, (6, 17)[(i // 2) % 2], r0=r0, ihl=ihl, mask=m, set_ttl=9))
    return out


def _hsum_edges(rng, ver: int) -> list[dict]:
    """r0 + l4_off + hlen on every target: TCP at up to three header lengths (the longest first;
    from hlen 24 on l4_off + 18 stays 6 bytes and more inside; only IPv6's 63 = 3 + 40 + 20 takes a
    header without options) and UDP where an l4_off reaches it."""
    out = []
    l4offs = [(ihl * 4, ihl, None) for ihl in (5, 6, 9, 12, 13)] if ver == 4 else [(40, 5, None), (48, 5, 0), (80, 5, 32)]
    for t in HSUM_TARGETS:
        for proto in (6, 17):
            got = 0
            for l4o, ihl, ext in l4offs:
                for hlen in ((60, 56, 52, 48, 44, 40, 36, 32, 28, 24, 20) if proto == 6 else (8,)):
                    r0 = t - l4o - hlen
                    if 0 <= r0 <= 15 and got < (3 if proto == 6 else 2):
                        got += 1
                        out.append(_hsum(rng, f"hsum{ver}:{NV.PROTO_NAME[proto]} l4_off {l4o} hlen {hlen} r0+l4_off+hlen {t}",
                                         ver, proto, r0, hlen, ihl=ihl, ext=ext))
    return out


def _hsum_lo(rng, i: int, cls: str = "hsum:fill") -> dict:
    """A header-sum packet whose window ends at 40..59 under any format (IPv4, hlen 20..28, r0 0..11)."""
    return _hsum(rng, cls, 4, 6, i % 12, 20 + 4 * (i % 3))


def _hsum_hi(rng, i: int, cls: str) -> dict:
    """... and one whose window ends at 86..95: TCP with 40 bytes of options, r0 6..15."""
    return _hsum(rng, cls, 4, 6, 6 + i % 10, 60)


ROUND2_ONE_LANES = (0, 21, 42, 63)   # lane mod 4: 0, 1, 2, 3


def _hsum_round2(rng) -> list[dict]:
    out = [_hsum_lo(rng, i, "hsum_round2:none") for i in range(WAVE)]
    for lane in ROUND2_ONE_LANES:
        wave = [_hsum_lo(rng, i, "hsum_round2:one (low)") for i in range(WAVE - 1)]
        wave.insert(lane, _hsum_hi(rng, lane, f"hsum_round2:one at lane {lane}"))
        out += wave
    return out + [_hsum_hi(rng, i, "hsum_round2:all") for i in range(WAVE)]


def _hsum_bad_one(rng, kind: str, i: int, tail: int | None = None) -> dict:
    ver = 6 if i % 5 == 4 else 4
    proto = 17 if kind in ("l4_len", "proto", "ver", "no_record") and i % 2 else 6
    hlen = 8 if proto == 17 else 24 + 4 * (i % 4)
    payload = {"hlen255_short": i % 8, "hlen255_long": 120}.get(kind)
    return _hsum(rng, f"hsum_bad:{kind}", ver, proto, None if tail is not None else (3 * i) % 16, hlen, payload=payload,
                 bad=kind, tail=tail)


def _hsum_bad(rng) -> list[dict]:
    """One wave: a bad record of each kind in turn with good neighbours (every third packet)."""
    out = []
    for i in range(WAVE):
        out.append(_hsum_lo(rng, i, "hsum_bad:good neighbour") if i % 3 == 2 else
                   _hsum_bad_one(rng, BAD_KINDS[(i - i // 3) % len(BAD_KINDS)], i))
    return out


def _refused(rng) -> list[dict]:
    """One wave: the nine refusals in turn (9 and 4 share no factor: each lands on every lane mod 4)."""
    out = []
    for i in range(WAVE):
        kind = REFUSED_KINDS[i % len(REFUSED_KINDS)]
        cls, r0 = f"refused:{kind}", (5 * i) % 16
        every = O.F_IP | O.F_L4 | O.F_PRE
        if kind == "l4p":
            v, fl = _nat(rng, cls, 4, (6, 17)[i % 2], r0=r0), O.F_L4 | O.F_L4P | O.F_PRE
        elif kind == "raw":
            v, fl = _nat(rng, cls, 4, (6, 17)[i % 2], r0=r0), O.F_IP | O.F_L4 | O.F_RAW | O.F_PRE
        elif kind == "ip_on_v6":
            v, fl = _nat(rng, cls, 6, 6, r0=r0 % 7), every
        elif kind == "no_field":   # a TCP segment of 17 bytes: no checksum field
            v, fl = _nat(rng, cls, 4, 6, r0=r0, seg_len=17), every
        elif kind == "pre_alone":
            v, fl = _nat(rng, cls, 4, 17, r0=r0), O.F_PRE
        elif kind == "v6":         # refused under the 16-B entries only: flushed under the 48-B ones
            v, fl = _nat(rng, cls, 6, (6, 17, 58)[i % 3], r0=r0 % 7), None
        elif kind in ("outside", "far"):
            v, fl = _nat(rng, cls, 4, 17, bad=kind), every
        else:
            v, fl = _nat(rng, cls, 4, 6, r0=r0, bad="ver5"), every
        v["pre"] = dict(flags=fl)
        out.append(v)
    return out


def _quads(rng) -> list[dict]:
    """One wave: quad q's lane k carries F_PRE when bit k of q is set."""
    out = []
    for i in range(WAVE):
        v = _nat(rng, f"quads:pattern {i >> 2:#06b}", 4, (6, 17)[i % 2], r0=(7 * i) % 16, ihl=5 + i % 3)
        if not (i >> 2) >> (i & 3) & 1:
            v["pre"] = dict(flags=0)   # setters applied, stale sums, not this kernel's packet
        out.append(v)
    return out


def _svc384(rng) -> list[dict]:
    """IPv6, a 263-B destination-options header (the longest the reference parses: 8 + 255) and
    filler up to the descriptor's l4_off of 368, a UDP segment of 8 + 0..2 bytes: need = 376 (+ the
    payload under the service grid's rule), r0 7 / 8 / 9 -> 383, 384, 385, and r0 + payload likewise."""
    out = []
    for r0, pay in ((7, 0), (8, 0), (9, 0), (6, 1), (7, 1), (8, 1), (5, 2), (6, 2), (7, 2)):
        seg = H._udp(rng, pay)
        p = bytearray(rng.integers(0, 256, 368, dtype=np.uint8).tobytes())
        p[0], p[6], p[7], p[40], p[41] = 0x60, 60, 64, 17, 255
        H._put16(p, 4, 328 + len(seg))
        l3 = T.l3_sums(p + seg, 6, 17, 368)
        rw = np.zeros(1, O.NAT_DTYPE)
        rw.view(np.uint8)[:36] = rng.integers(0, 256, 36, dtype=np.uint8)
        rw["mask"] = NV.ADDR_PORTS
        out.append(dict(cls=f"svc384:r0 {r0} payload {pay}", l3=bytes(l3), ver=6, proto=17, l4_off=368, rw=rw[0], r0=r0,
                        tail=None, bad=None, sum_edge=None))
    return out


def _waves(vs: list[dict], fill) -> list[dict]:
    """vs padded to whole waves with fill(i)."""
    return vs + [fill(i) for i in range(-len(vs) % WAVE)]


def vectors(seed: int = 31) -> tuple[list[dict], dict]:
    """(the vectors in batch order, {class: (first, past-last) index of its waves})."""
    base = NV.vectors(seed)
    cut = next(i for i, v in enumerate(base) if v["cls"].startswith("tails:"))
    assert cut % WAVE == 0
    rng = np.random.default_rng(seed + 1000)
    out, spans = base[:cut], {}

    def add(name, vs):
        assert len(vs) % WAVE == 0
        spans[name] = (len(out), len(out) + len(vs))
        out.extend(vs)

    def fill(i):
        return _nat(rng, "fill", 4, (6, 17, 1)[i % 3], r0=(3 * i) % 16)

    add("ip_only", _ip_only(rng))
    add("hsum4", _waves(_hsum_edges(rng, 4), lambda i: _hsum_lo(rng, i)))
    add("hsum6", _waves(_hsum_edges(rng, 6), lambda i: _hsum_lo(rng, i)))
    add("hsum_round2", _hsum_round2(rng))
    add("hsum_bad", _hsum_bad(rng))
    add("refused", _refused(rng))
    add("quads", _quads(rng))
    add("svc384", _waves(_svc384(rng), fill))
    spans["tails"] = (len(out), len(out) + len(base) - cut)
    out += base[cut:]
    # a bad record on the packet that ends on the arena's last byte (hlen 255 asks for bytes past it)
    spans["hsum_bad_last"] = (len(out), len(out) + 1)
    out.append(_hsum_bad_one(rng, "hlen255_short", 1, tail=0))
    return out, spans


def batch(orc, seed: int = 31) -> dict:
    """{before, after, desc, pre, vecs, spans}: the packed frames as received, the frames after
    Java's setters and the in-place header edits (what the flush receives), the descriptors with
    their flags, and the 48-B entries (pre-images; header-sum records for the hsum classes)."""
    vecs, spans = vectors(seed)
    p = NV.pack(vecs)
    before, desc, rw = p["arena"], p["desc"].copy(), p["rw"]
    n, alen = len(desc), len(before)
    inside = np.array([int(d["l3_off"]) + int(d["l3_len"]) <= alen for d in desc])
    hs = np.array(["rec" in v.get("pre", ()) for v in vecs])
    pre = np.zeros(n, O.NAT_DTYPE)
    idx = np.nonzero(inside & ~hs)[0]
    pre[idx] = pre_images(before, desc[idx], rw[idx])
    after = before.copy()
    sst = orc.nat_setters(after, desc, rw)
    dirty = java_dirty_flags(desc, rw)
    flags = np.where(dirty != 0, dirty | O.F_PRE, 0).astype(np.uint8)
    flags[sst != O.S_DONE] = 0       # TTL expired (IPInputRoute drops them), refused descriptors
    for i, v in enumerate(vecs):
        pv = v.get("pre")
        if pv is None:
            continue
        if pv.get("flags") is not None:
            flags[i] = pv["flags"]
        if "rec" in pv:
            o = int(desc[i]["l3_off"])
            after[o:o + len(v["l3"])] = np.frombuffer(pv["edited"], np.uint8)
            raw = pre[i:i + 1].view(np.uint8)
            raw[:] = 0
            raw[:8] = np.frombuffer(pv["rec"].tobytes(), np.uint8)
            pre[i]["mask"] = O.PRE_HSUM
    desc["flags"] = flags
    return dict(before=before, after=after, arena=after, desc=desc, pre=pre, rw=rw, vecs=vecs, spans=spans)


def entries(pre48: np.ndarray, fmt: int) -> np.ndarray:
    """The entry table of format fmt as bytes: vpcsum_pre_t as it is, or vpcsum_pre4_t (the IPv4
    fields; a header-sum record keeps its 8 bytes and the VPCSUM_PRE_HSUM mask)."""
    if fmt == 1:
        return np.ascontiguousarray(pre48).view(np.uint8).reshape(-1)
    r4 = nat4_of(pre48)
    hs = (pre48["mask"] & O.PRE_HSUM) != 0
    raw4, raw48 = r4.view(np.uint8).reshape(-1, 16), np.ascontiguousarray(pre48).view(np.uint8).reshape(-1, 48)
    raw4[hs, :8] = raw48[hs, :8]
    return raw4.reshape(-1)


def entries_array(pre48: np.ndarray, fmt: int) -> np.ndarray:
    """entries() as the structured array the host context takes."""
    return entries(pre48, fmt).view(O.NAT_DTYPE if fmt == 1 else O.NAT4_DTYPE)


def strided(orc, n: int, seed: int = 41) -> dict:
    """natvec.strided in pre-image form, for the loop's second trip: {after, desc, pre, want,
    status}; the pre-images with numpy (every packet is IPv4 with l4_off 20 at a 64-byte stride)."""
    s = NV.strided(n, seed)
    before, desc, rw = s["arena"], s["desc"].copy(), s["rw"]
    A = before.reshape(n, 64)
    m = rw["mask"].astype(int)
    ports = np.isin(desc["l4_proto"], (6, 17))
    pre = np.zeros(n, O.NAT_DTYPE)
    pre["src"][:, :4] = np.where((m & O.NAT_SRC)[:, None] != 0, A[:, 12:16], 0)
    pre["dst"][:, :4] = np.where((m & O.NAT_DST)[:, None] != 0, A[:, 16:20], 0)
    pre["sport"] = np.where((ports & ((m & O.NAT_SPORT) != 0))[:, None], A[:, 20:22], 0)
    pre["dport"] = np.where((ports & ((m & O.NAT_DPORT) != 0))[:, None], A[:, 22:24], 0)
    pre["mask"] = m & np.where(ports, NAT_FIELDS, O.NAT_SRC | O.NAT_DST)
    want = before.copy()
    wst = orc.nat_java(want, desc, rw)
    after = before.copy()
    orc.nat_setters(after, desc, rw)
    dirty = java_dirty_flags(desc, rw)
    desc["flags"] = np.where((dirty != 0) & (wst == O.S_DONE), dirty | O.F_PRE, 0)
    status = np.where(desc["flags"] != 0, O.S_DONE, GUARD).astype(np.uint8)
    return dict(before=before, after=after, desc=desc, pre=pre, rw=rw, want=want, status=status)


# ----------------------------------------------------------------------------------------
# The expected result
# ----------------------------------------------------------------------------------------
def _l3(a: np.ndarray, d) -> bytes:
    o = int(d["l3_off"])
    return a[o:o + int(d["l3_len"])].tobytes()


def live_rows(b: dict, fmt: int, n: int | None = None) -> tuple[np.ndarray, np.ndarray]:
    """(act, live) over the first n packets: the F_PRE rows, and those of them the kernel flushes
    (pre_desc_ok, and a header-sum record that describes the packet)."""
    desc, pre, alen = b["desc"], b["pre"], len(b["after"])
    n = len(desc) if n is None else n
    act = np.zeros(len(desc), bool)
    live = np.zeros(len(desc), bool)
    for i in range(n):
        d = desc[i]
        act[i] = bool(int(d["flags"]) & O.F_PRE)
        live[i] = act[i] and pre_desc_ok(d, alen, fmt) and (not is_hsum(pre[i]) or record_ok(_l3(b["after"], d), d, pre[i]))
    return act, live


def expect(b: dict, orc, fmt: int, n: int | None = None) -> dict:
    """The flush of the first n packets under entry format fmt: {arena, out, status, act, live}.
    arena: `after` with every live packet's bytes from Java -- orc.nat_java on the frames as
    received, or for a header-sum packet the full recompute of its dirty sums over the edited frame;
    refused and flag-0 packets exactly as in `after`.  out: the sums Java left in the frames (live),
    0 (refused), OUT_GUARD (not F_PRE).  status: S_DONE, S_BAD_DESC, GUARD."""
    desc, pre, after = b["desc"], b["pre"], b["after"]
    act, live = live_rows(b, fmt, n)
    java = b["before"].copy()
    orc.nat_java(java, desc, b["rw"])
    hs = (pre["mask"] & O.PRE_HSUM) != 0
    full = after.copy()
    dh = desc[live & hs].copy()
    dh["flags"] &= O.F_IP | O.F_L4
    orc.process(full, dh, O.MODE_COMPUTE, write=True)
    want = after.copy()
    for i in np.nonzero(live)[0]:
        o, ln = int(desc[i]["l3_off"]), int(desc[i]["l3_len"])
        want[o:o + ln] = (full if hs[i] else java)[o:o + ln]
    dl = desc.copy()
    dl["flags"] = np.where(live, dl["flags"] & (O.F_IP | O.F_L4), 0)
    sums, _ = orc.process(want, dl)
    out = np.where(live, sums, np.where(act, 0, OUT_GUARD)).astype(np.uint32)
    status = np.where(live, O.S_DONE, np.where(act, O.S_BAD_DESC, GUARD)).astype(np.uint8)
    return dict(arena=want, out=out, status=status, act=act, live=live)


def describe(b: dict, i: int, fmt: int, ch: int, base: int = 0) -> str:
    """Packet i's class and geometry, for a failing comparison's message."""
    g = geometry(b["desc"][i], b["pre"][i], len(b["after"]), fmt, ch, base)
    d = b["desc"][i]
    return (f"packet {i} [{b['vecs'][i]['cls']}] flags {int(d['flags']):#x} act {g.act} ok {g.ok} r0 {g.r0} need {g.need} "
            f"wend {g.wend} round2 {g.r2} hlen {hsum_hlen(b['pre'][i])} wave lane {i % WAVE}")


def first_diff(b: dict, got: np.ndarray, want: np.ndarray, fmt: int, ch: int, base: int = 0) -> str:
    """Which packet (or gap) the first differing arena byte belongs to."""
    at = int(np.nonzero(got != want)[0][0])
    for i, d in enumerate(b["desc"]):
        o = int(d["l3_off"])
        if o <= at < o + int(d["l3_len"]) and o + int(d["l3_len"]) <= len(want):
            return (f"arena byte {at} (L3 + {at - o}) got {int(got[at]):#04x} want {int(want[at]):#04x}: " +
                    describe(b, i, fmt, ch, base))
    return f"arena byte {at}: in no packet"


# ----------------------------------------------------------------------------------------
# The classes, recomputed from the descriptors, the entries and the arena
# ----------------------------------------------------------------------------------------
def _refusal(d, alen: int, fmt: int) -> str | None:
    """Why pre_desc_ok refuses an F_PRE descriptor, in its order of tests (None: it does not)."""
    fl, ver = int(d["flags"]), int(d["l3_ver"])
    if fl & O.F_L4P:
        return "l4p"
    if fl & O.F_RAW:
        return "raw"
    if not fl & (O.F_IP | O.F_L4):
        return "pre_alone"
    if fl & O.F_IP and ver == 6:
        return "ip_on_v6"
    off, ln = int(d["l3_off"]), int(d["l3_len"])
    if off > alen:
        return "far"
    if ln > alen - off:
        return "outside"
    if ver not in (4, 6):
        return f"ver{ver}"
    if ver == 6 and fmt == 0:
        return "v6"
    if not NV.desc_ok(d, alen, fmt):
        return "header"
    if fl & O.F_L4 and not NV.l4sum(ver, int(d["l4_proto"]), ln, int(d["l4_off"])):
        return "no_field"
    return None


def check_classes(b: dict) -> dict:
    """Asserts that every class of the module's docstring is in the batch, from the descriptors, the
    entries and the two arenas alone (the vectors' own labels are not consulted; a class is looked
    for in the waves vectors() put it in, and its count must be the number built there); returns
    the classes' sizes."""
    desc, pre, after, before, spans = b["desc"], b["pre"], b["after"], b["before"], b["spans"]
    n, alen = len(desc), len(after)
    G = {(fmt, ch): [geometry(desc[i], pre[i], alen, fmt, ch) for i in range(n)] for fmt, ch in ((0, 4), (0, 6), (1, 6))}
    live = {fmt: live_rows(b, fmt)[1] for fmt in (0, 1)}
    size = {}
    for name, (lo, hi) in spans.items():
        assert name in ("tails", "hsum_bad_last") or (lo % WAVE == 0 and hi % WAVE == 0), name

    # both window limits from both sides, per window size, over the whole batch
    for (fmt, ch), want in (((0, 4), (63, 64, 65)), ((0, 6), (95, 96, 97)), ((1, 6), (95, 96, 97)), ((1, 6), (63, 64, 65))):
        ends = {t: sum(1 for g in G[(fmt, ch)] if g.ok and g.r0 + g.need == t) for t in want}
        assert all(ends.values()), ("window limit", fmt, ch, ends)
        for g in G[(fmt, ch)]:
            assert not g.ok or (g.wend == 0) == (g.r0 + g.need > 16 * ch)
        size[f"fmt {fmt} ch {ch} r0+need {want}"] = tuple(ends.values())

    # ip_only
    lo, hi = spans["ip_only"]
    seen = set()
    for i in range(lo, hi):
        g = G[(0, 6)][i]
        if int(desc[i]["flags"]) == O.F_IP | O.F_PRE and g.ok and g.need == int(desc[i]["l4_off"]):
            seen.add((int(desc[i]["l4_off"]), g.r0, int(desc[i]["l4_proto"]) == 1))
    assert {(l4o, r0) for l4o, r0, _ in seen} == {(4 * ihl, r0) for ihl in range(5, 16) for r0 in range(16)}, "ip_only"
    assert {icmp for _, _, icmp in seen} == {False, True}
    size["ip_only"] = sum(1 for i in range(lo, hi) if int(desc[i]["flags"]) == O.F_IP | O.F_PRE)
    assert size["ip_only"] == hi - lo

    # hsum4 / hsum6: the targets per protocol; the edits reach the header's last 4 bytes
    for ver, name, fmt in ((4, "hsum4", 0), (6, "hsum6", 1)):
        lo, hi = spans[name]
        hit, inside = {6: set(), 17: set()}, set()
        count = 0
        for i in range(lo, hi):
            d, g = desc[i], G[(fmt, 6)][i]
            if not (is_hsum(pre[i]) and live[fmt][i] and int(d["l3_ver"]) == ver):
                assert is_hsum(pre[i]) and live[1][i], (name, i)   # the filler: good IPv4 header-sum packets
                continue
            l4o, proto, hlen = int(d["l4_off"]), int(d["l4_proto"]), hsum_hlen(pre[i])
            t = g.r0 + l4o + hlen
            count += t in HSUM_TARGETS   # (the filler ends at 40..59)
            assert g.need == l4o + max(hlen, O.L4_FIELD[proto] + 2) and int(d["l3_len"]) >= l4o + hlen
            if t in HSUM_TARGETS:
                hit[proto].add(t)
                if proto == 6 and g.r0 + l4o + 18 <= t - 6:
                    inside.add(t)
            o = int(d["l3_off"]) + l4o
            if proto == 6:
                assert not np.array_equal(after[o + hlen - 4:o + hlen], before[o + hlen - 4:o + hlen]), (name, i)
            assert not np.array_equal(after[o:o + 4], before[o:o + 4])
        assert hit[6] == set(HSUM_TARGETS), (name, "tcp", hit[6])
        assert inside == set(HSUM_TARGETS) - ({63} if ver == 6 else set()), (name, "field well inside", inside)
        assert hit[17] == ({63, 64, 65} if ver == 4 else set(HSUM_TARGETS)), (name, "udp", hit[17])   # IPv4: 15 + 60 + 8 = 83
        size[name] = count
    assert size["hsum4"] == sum(1 for v in b["vecs"] if v["cls"].startswith("hsum4:"))
    assert size["hsum6"] == sum(1 for v in b["vecs"] if v["cls"].startswith("hsum6:"))

    # hsum_round2: per wave, the packets past 64 under the 6-chunk builds of both formats
    lo, hi = spans["hsum_round2"]
    for fmt in (0, 1):
        per_wave = [sum(1 for g in G[(fmt, 6)][w:w + WAVE] if g.r2) for w in range(lo, hi, WAVE)]
        assert sorted(per_wave) == [0] + [1] * len(ROUND2_ONE_LANES) + [WAVE], ("hsum_round2", fmt, per_wave)
        lanes = sorted(next(k for k in range(WAVE) if G[(fmt, 6)][w + k].r2)
                       for w, c in zip(range(lo, hi, WAVE), per_wave) if c == 1)
        assert {k & 3 for k in lanes} == {0, 1, 2, 3}, ("hsum_round2 lanes", lanes)
        for w, c in zip(range(lo, hi, WAVE), per_wave):
            if c == 1:   # the second round's chunks both hold summed bytes: the window ends past 80
                assert max(g.wend for g in G[(fmt, 6)][w:w + WAVE]) > 80
        assert all(is_hsum(pre[i]) and live[fmt][i] for i in range(lo, hi))
    size["hsum_round2 waves none/one/all"] = (1, len(ROUND2_ONE_LANES), 1)

    # hsum_bad: acceptable descriptors whose record does not describe the packet
    kinds = {}
    for lo, hi in (spans["hsum_bad"], spans["hsum_bad_last"]):
        for i in range(lo, hi):
            d, e = desc[i], pre[i]
            assert is_hsum(e) and pre_desc_ok(d, alen, 1)
            if live[1][i]:
                continue
            rec = np.frombuffer(_raw(e)[:8].tobytes(), O.HSUM_DTYPE)[0]
            l3, l4o, seg = _l3(after, d), int(d["l4_off"]), int(d["l3_len"]) - int(d["l4_off"])
            cur = (l3[l4o + 12] >> 4) * 4 if d["l4_proto"] == 6 else 8
            o = int(d["l3_off"])
            if rec["l2_len"] == 0:
                k = "no_record"
            elif rec["l3_ver"] != d["l3_ver"]:
                k = "ver"
            elif rec["l4_proto"] != d["l4_proto"]:
                k = "proto"
            elif rec["l4_len"] != seg:
                k = "l4_len"
            elif rec["hlen"] == 255:   # the whole packet is asked for: in a window, or too long for one
                g = geometry(d, e, alen, 1, 6)
                assert seg < 255 and g.need == int(d["l3_len"])
                k = "hlen255_short" if g.wend else "hlen255_long"
            elif before[o + l4o + 12] != after[o + l4o + 12]:
                k = "doff_in_frame"
            else:
                assert rec["hlen"] != cur
                k = "hlen"
            kinds.setdefault(k, []).append(i)
    assert set(kinds) == set(BAD_KINDS), sorted(kinds)
    last = spans["hsum_bad_last"][0]
    assert int(desc[last]["l3_off"]) + int(desc[last]["l3_len"]) == alen and not live[1][last]
    assert geometry(desc[last], pre[last], alen, 1, 6).need == int(desc[last]["l3_len"])
    lo, hi = spans["hsum_bad"]
    size["hsum_bad"] = sum(len(v) for v in kinds.values())
    assert size["hsum_bad"] == 1 + sum(1 for i in range(lo, hi) if i % 3 != 2)
    assert sum(1 for i in range(lo, hi) if live[1][i]) == sum(1 for i in range(lo, hi) if i % 3 == 2)

    # refused: every refusal on every lane mod 4
    lo, hi = spans["refused"]
    why = {}
    for i in range(lo, hi):
        assert int(desc[i]["flags"]) & O.F_PRE
        r = _refusal(desc[i], alen, 0)
        assert r is not None and (r == "v6") == (_refusal(desc[i], alen, 1) is None), (i, r)
        why.setdefault(r, set()).add(i & 3)
    assert set(why) == set(REFUSED_KINDS), sorted(why)
    assert all(v == {0, 1, 2, 3} for v in why.values()), why
    size["refused"] = hi - lo

    # quads: all 16 patterns; the rows without F_PRE are dirty packets (a write to them would show)
    lo, hi = spans["quads"]
    pats = {sum(1 << k for k in range(4) if int(desc[lo + 4 * q + k]["flags"]) & O.F_PRE) for q in range(16)}
    assert pats == set(range(16)), sorted(pats)
    assert all(int(desc[i]["flags"]) == 0 or live[0][i] for i in range(lo, hi))
    size["quads"] = len(pats)

    # svc384: the service grid's 24-chunk limit from both sides, byte-path packets for k_pre
    lo, hi = spans["svc384"]
    ends = {}
    for i in range(lo, hi):
        t = (int(desc[i]["l3_off"]) & 15) + svc_need(desc[i])
        if live[1][i] and t in (16 * SVC_CHUNKS - 1, 16 * SVC_CHUNKS, 16 * SVC_CHUNKS + 1):
            assert G[(1, 6)][i].ok and G[(1, 6)][i].wend == 0 and desc[i]["l3_ver"] == 6
            ends.setdefault(t, []).append(i)
    assert set(ends) == {383, 384, 385}, sorted(ends)
    size["svc384"] = sum(len(v) for v in ends.values())
    assert size["svc384"] == sum(1 for v in b["vecs"] if v["cls"].startswith("svc384:"))

    # every kind of row on every lane mod 4, per format (16-B entries: IPv4 passes 64 B, never 96)
    for fmt, ch in ((0, 4), (1, 6)):
        rows = {}
        for i in range(n):
            g = G[(fmt, ch)][i]
            kind = "not F_PRE" if not g.act else "refused" if not g.ok else "bad record" if not live[fmt][i] else \
                "header sum" if is_hsum(pre[i]) else "window" if g.wend else "byte path"
            rows.setdefault(kind, set()).add(i & 3)
        assert len(rows) == 6 and all(v == {0, 1, 2, 3} for v in rows.values()), (fmt, rows)
    size["row kinds on every lane mod 4"] = 6
    return size
