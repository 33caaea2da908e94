"""Crafted vectors for the geometry of the checksum kernels (test infrastructure: tests/ only): K2's
per-packet plan, its cost classes and tiers, its units, its loop and its sampled paths.

tests/edgevec.py is about values (sums of 0 and 0xffff); this file is about where bytes lie.  What
k2_run (vproxy_amd/csrc/kernels.hip) decides per packet in phase A is restated in plan(); batch()
builds packets that sit on each edge of those decisions by construction and lays them out in units
of 64 (a wave's packets) and workgroups of 256; check_classes() recomputes from the descriptors
alone that every class is there.  The arena's background is nonzero noise and frames are packed
chunk to chunk, so a read past a packet's end, or of a header byte that a sum should leave out,
changes the result.

Per-packet classes (flags F_IP | F_L4 on IPv4, F_L4 on IPv6 unless said):

  end16        fast-class packets with (r0 + len) & 15 = 0..15, once with kfast == 0 (end in chunk 4)
               and once with kfast >= 1 (chunk 5), IPv4 TCP at r0 14 and IPv6 TCP at r0 6.
  short_odd    r0 even, r0 + need odd and below 64: the halfword bitmaps cannot hold the odd last
               byte, the packet goes to the slow class.
  r0_odd       r0 = 1, 3, ..., 15 (slow class), IPv4 UDP and IPv6 TCP.
  l4o_odd      IPv6 descriptors with l4_off 41 and 43 (the rules accept them, the oracle follows).
  fa_edge      r0 + l4_off + fld + 2 at 62, 64 (klo 4: fast) and 66, 68 (klo 5: slow): IPv4 with
               options, IPv6 TCP, IPv6 + 8-B extension header UDP, IPv4 l4_off 60 at every even r0.
  hdr_only     segments that end inside the first 64 B (klo >= nch at one r0 or both): UDP 8 B, TCP
               20 B, ICMP 4 / 8 B.
  small_edge   nch = TS * US and one more for every small tier in the table: 4/5, 8/9, 16/17.
  trip_edge    nch = k * TEAM * U and one more, k = 1, 2, for every (TEAM, U) in the table; the
               class cap 576 / 577 of (8, 6); one packet of 65,535 B.
  flags        F_IP alone at IHL 5..15, F_L4 alone, F_L4P (TCP / UDP, both versions), flags 0, F_PRE,
               F_RAW ranges of 0, 1, 2, 15, 16, 17, 63, 64, 65, 767, 768, 769 B at even and odd r0.
  field_chunk  (verify) the IP field in chunk 0 (r0 <= 4) and chunk 1 (r0 >= 6); the L4 field in
               chunks 1, 2, 3.
  refused      one kind per branch of desc_rules and of the bounds check (REFUSED), each on lanes 0,
               1, 31, 32 and 63 of some unit; the accepted neighbour of `end_plus1` is the batch's
               last packet, which ends on the arena's last byte (arena_len % 16 != 0).

Unit classes (whole units, each at two unit positions or more):

  one_class    one large cost class (n_cls == 1: the slots rotate), live ranges ONE_CLASS_LIVE, the
               rest bad descriptors.
  n_small      N_SMALL small-tier packets (bad ones among them), the rest large.
  tail         a large tier of two classes of size 16 + r, r = 0..7 (the WT build's wide last
               iteration at remainders 1..4 and not at 5..7).
  all_keys     every cost class plan() can produce, for every build of the table, in one unit.
  slow_only, all_bad, uniform (64 packets of one small shape, contiguous: a window-unit candidate).

A packet is `small` here when nch <= 4 (the smallest TS * US) and `large` when nch >= 17 (above
the largest), so the unit classes hold for every build with a small tier.
"""
from __future__ import annotations

from collections import Counter, namedtuple

import numpy as np

import csumbuilds as CB
import edgevec as E
from oracle import oracle as O

UNIT, WG = 64, 256
FLAG_REJECTED = 0x80            # device_common.h kFlagRejected
V4F, V6F = O.F_IP | O.F_L4, O.F_L4
SMALL_MAX, LARGE_MIN = 4, 17    # nch: small / large for every small tier of the table
ONE_CLASS_LIVE = (64, 63, 57, 9, 8, 7, 1)
N_SMALL = (0, 1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)
RAW_LENS = (0, 1, 2, 15, 16, 17, 63, 64, 65, 767, 768, 769)
REFUSED_LANES = (0, 1, 31, 32, 63)
REFUSED = ("ver5", "v4_len19", "v4_l4o16", "v4_l4o_gt_len", "v4_l4o_and3", "v6_len39", "v6_l4o39", "v6_l4o_gt_len",
           "proto47_l4", "proto58_v4", "short_tcp", "short_udp", "short_icmp", "l4p_l4", "l4p_icmp", "ip_on_v6",
           "flag80", "off_past", "end_plus1")
CORRUPTIONS = ("ip", "l4", "payload", "udp0", "udp_zero")
TEAM_UNROLLS = sorted({(b.team, b.u) for b in CB.K2_BUILDS})
SMALL_TIERS = sorted({(b.ts, b.us) for b in CB.K2_BUILDS if b.ts})

Plan = namedtuple("Plan", "bad raw need nch klo kfast hbm fastc key r0 do_ip do_l4 psonly fld fa")


# ----------------------------------------------------------------------------------------
# k2_run's phase A
# ----------------------------------------------------------------------------------------
def desc_rules(ln, l4o, ver, proto, fl):
    """kernels.hip desc_rules (:734-755): (bad, do_ip, do_l4, psonly, fld)."""
    do_ip = do_l4 = psonly = False
    fld = -1
    if ver == 4:
        bad = ln < 20 or l4o < 20 or l4o > ln or bool(l4o & 3)
    elif ver == 6:
        bad = ln < 40 or l4o < 40 or l4o > ln
    else:
        bad = True
    if not bad and fl & (O.F_L4 | O.F_L4P):
        psonly = bool(fl & O.F_L4P)
        fld = O.L4_FIELD.get(proto, -1)
        if fld < 0 or (ver == 4 and proto == 58) or ln - l4o < fld + 2:
            bad = True
        elif psonly and (fl & O.F_L4 or proto == 1):
            bad = True
        else:
            do_l4 = True
    if not bad and fl & O.F_IP:
        if ver != 4:
            bad = True
        else:
            do_ip = True
    return bad, do_ip, do_l4, psonly, fld


def key_of(fastc: bool, bad: bool, nch: int, build) -> int:
    """The cost class (kernels.hip :1182-1187): bad 0, the small tier 1, trips of the large tier's
    team loop 2 + min(trips, 12), the slow class 15."""
    if bad:
        return 0
    if build.ts > 0 and fastc and nch <= build.ts * build.us:
        return 1
    tu = build.team * build.u
    return 2 + min((nch + tu - 1) // tu, 12) if fastc else 15


def plan(row, build, arena_len: int) -> Plan:
    """Phase A of k2_run for one descriptor of an arena of arena_len bytes (kernels.hip :973-979 the
    fields, :1128-1137 bounds and rules, :1144-1167 need / nch / fast_lo / fast_hi / klo / kfast /
    hbm, :1181-1187 fastc and the key), from the descriptor alone.  Window units (:995-1126) decide
    per unit, not per packet, and compute the same sums: they are not part of the plan."""
    off, ln, l4o = int(row["l3_off"]), int(row["l3_len"]), int(row["l4_off"])
    ver, proto, fl = int(row["l3_ver"]), int(row["l4_proto"]), int(row["flags"])
    if fl & O.F_PRE:           # device_common.h csum_flags
        fl = 0
    r0 = off & 15
    bad = off > arena_len or ln > arena_len - off or bool(fl & FLAG_REJECTED)
    raw = bool(fl & O.F_RAW)
    do_ip = do_l4 = psonly = False
    fld = -1
    if not bad and not raw:
        bad, do_ip, do_l4, psonly, fld = desc_rules(ln, l4o, ver, proto, fl)
    need = 0 if bad else l4o + fld + 2 if psonly else ln if (raw or do_l4) else (l4o if do_ip else 0)
    nch = 0 if (bad or not need) else (r0 + need + 15) >> 4
    fa = -64
    if raw:
        fast_lo = (r0 + 15) & ~15
    elif psonly:
        fa, fast_lo = r0 + l4o + fld, 1 << 30
    elif do_l4:
        fa = r0 + l4o + fld
        fast_lo = (fa + 2 + 15) & ~15
    else:
        fast_lo = 1 << 30
    fast_hi = (r0 + need) & ~15
    klo = min(fast_lo >> 4, nch)
    kfast = max((fast_hi >> 4) - klo, 0)
    hbm = not raw and not (r0 & 1) and not (l4o & 1) and (((r0 + need) & 1) == 0 or r0 + need >= 64)
    fastc = hbm and klo <= 4
    return Plan(bad, raw, need, nch, klo, kfast, hbm, fastc, key_of(fastc, bad, nch, build), r0, do_ip, do_l4, psonly, fld, fa)


def plans(b, build, arena_len=None):
    alen = len(b["arena"]) if arena_len is None else arena_len
    return [plan(d, build, alen) for d in b["desc"]]


def possible_keys(build) -> set:
    """Every cost class plan() can produce for a build: bad, the small tier (builds that have one;
    a build without has key 2 for packets that read nothing), 1..12 trips, the slow class."""
    return {0, 15, 1 if build.ts > 0 else 2} | set(range(3, 15))


# ----------------------------------------------------------------------------------------
# Packets
# ----------------------------------------------------------------------------------------
def _l3(rng, ver, proto, seg, l4o=None):
    """An L3 packet with a segment of seg bytes at l4_off l4o (IPv4 options / one IPv6 extension
    header where that makes it; any other IPv6 offset with the bytes between left random: the
    checksum follows the descriptor)."""
    if ver == 4:
        l4o = 20 if l4o is None else l4o
        p = bytearray(rng.integers(0, 256, l4o + seg, dtype=np.uint8).tobytes())
        p[0] = 0x40 | (l4o // 4)
        E._put16(p, 2, l4o + seg)
        p[9] = proto
        E._put16(p, 10, 0)
    else:
        l4o = 40 if l4o is None else l4o
        p = bytearray(rng.integers(0, 256, l4o + seg, dtype=np.uint8).tobytes())
        p[0] = 0x60
        E._put16(p, 4, l4o + seg - 40)
        p[6] = proto if l4o == 40 else 0
        if l4o >= 48:
            p[40], p[41] = proto, (l4o - 48) & 0xFF
    if proto == 6 and seg > 12:
        p[l4o + 12] = 0x50
    elif proto == 17 and seg >= 6:
        E._put16(p, l4o + 4, seg)
    return p, l4o


def set_fields(p: bytearray, l4o: int, ver: int, proto: int, flags: int):
    """Valid stored sums, as edgevec.pack sets them: the IPv4 header sum, the L4 sum (the
    pseudo-header sum under F_L4P) where the segment holds the field."""
    fld = O.L4_FIELD.get(proto, -1)
    if ver == 4 and l4o <= len(p) and l4o >= 20:
        E._put16(p, 10, O.ipv4_header_csum(bytes(p), l4o))
    if fld >= 0 and not (ver == 4 and proto == 58) and len(p) - l4o >= fld + 2:
        if flags & O.F_L4P:
            seg = len(p) - l4o
            ph = O.pseudo_ipv4(bytes(p), proto, seg) if ver == 4 else O.pseudo_ipv6(bytes(p), proto, seg)
            E._put16(p, l4o + fld, O.csum_intermediate(0, ph, len(ph)))
        else:
            E._put16(p, l4o + fld, E.l4_value(bytes(p), len(p), l4o, ver, proto))


class _Specs:
    """The batch under construction: packets in descriptor order."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.s = []

    def add(self, cls, ver, proto, l3_len, r0, l4o=None, flags=None, over=None, raw=None):
        """One packet of l3_len bytes at chunk offset r0.  over: descriptor fields that differ from
        the frame (refused kinds); raw: a raw range of that many bytes instead of a packet."""
        if raw is not None:
            p, l4o = bytearray(self.rng.integers(1, 256, raw, dtype=np.uint8).tobytes()), 0
            flags = O.F_RAW
        else:
            l4o0 = (20 if ver == 4 else 40) if l4o is None else l4o
            p, l4o = _l3(self.rng, ver, proto, l3_len - l4o0, l4o0)
            flags = (V4F if ver == 4 else V6F) if flags is None else flags
            set_fields(p, l4o, ver, proto, flags)
        self.s.append(dict(cls=cls, l3=p, l4o=l4o, ver=ver, proto=proto, flags=flags, r0=r0, over=over or {}))

    def nch(self, cls, n, r0=0, e=0, ver=4, proto=17):
        """A fast-class packet of exactly n chunks: r0 + len = 16 n - e."""
        self.add(cls, ver, proto, 16 * n - e - r0, r0)

    def __len__(self):
        return len(self.s)


def _small(S, cls, i):
    """Small for every small tier: nch <= 4, fast class (even r0, even end)."""
    ver, proto, ln, r0 = ((4, 17, 28, 14), (4, 6, 40, 0), (4, 1, 28, 2), (6, 17, 48, 14), (4, 17, 50, 14), (6, 58, 44, 4),
                          (4, 6, 44, 8), (4, 17, 36, 12))[i % 8]
    S.add(cls, ver, proto, ln, r0)


def _large(S, cls, i, n=None):
    """One trip of every (TEAM, U) of the table: nch 17..24."""
    n = 17 + i % 8 if n is None else n
    S.nch(cls, n, r0=(0, 14, 2, 8)[i % 4], e=(0, 14, 3, 9)[i % 4], ver=(4, 6)[i % 2], proto=17 if i % 2 else (17, 6)[(i // 2) % 2])


def _large2(S, cls, i):
    """Another class than _large's in every build: 100 chunks (2..5 trips)."""
    _large(S, cls, i, 100)


def _slow(S, cls, i):
    if i % 2:
        S.add(cls, 4, 17, 60 + i % 7, 1 + 2 * (i % 8))          # odd r0
    else:
        S.add(cls, 4, 17, 29 + 2 * (i % 8), 2 * (i % 4))        # even r0, odd end below 64


def _bad(S, cls, i):
    S.add(cls, 4, 17, 60, 2 * (i % 8), over=(dict(l3_ver=5), dict(l3_len=19), dict(l4_off=22), dict(flags=V4F | 0x80))[i % 4])


def _filler(S, cls, i):
    k = i % 16
    if k < 6:
        _small(S, cls, i)
    elif k < 10:
        S.nch(cls, 5 + (i * 7) % 12, r0=(0, 14, 6)[i % 3], e=(0, 5, 14)[i % 3])       # 5..16 chunks
    elif k < 13:
        _large(S, cls, i)
    elif k == 13:
        _slow(S, cls, i)
    elif k == 14:
        _bad(S, cls, i)
    else:
        S.add(cls, 0, 0, 0, i % 16, raw=40 + i % 50)


def _pad_to_unit(S, cls="filler"):
    i = 0
    while len(S) % UNIT:
        _filler(S, cls, len(S) + i)
        i += 1


def _refused(S, kind):
    c = f"refused/{kind}"
    a = S.add
    if kind == "ver5": a(c, 4, 17, 60, 14, over=dict(l3_ver=5))
    elif kind == "v4_len19": a(c, 4, 17, 60, 14, over=dict(l3_len=19))
    elif kind == "v4_l4o16": a(c, 4, 17, 60, 14, over=dict(l4_off=16))
    elif kind == "v4_l4o_gt_len": a(c, 4, 17, 60, 14, over=dict(l4_off=64))
    elif kind == "v4_l4o_and3": a(c, 4, 17, 60, 14, over=dict(l4_off=22))
    elif kind == "v6_len39": a(c, 6, 17, 60, 14, over=dict(l3_len=39))
    elif kind == "v6_l4o39": a(c, 6, 17, 60, 14, over=dict(l4_off=39))
    elif kind == "v6_l4o_gt_len": a(c, 6, 17, 60, 14, over=dict(l4_off=61))
    elif kind == "proto47_l4": a(c, 4, 47, 60, 14)
    elif kind == "proto58_v4": a(c, 4, 58, 60, 14)
    elif kind == "short_tcp": a(c, 4, 6, 20 + 17, 14)
    elif kind == "short_udp": a(c, 6, 17, 40 + 7, 14)
    elif kind == "short_icmp": a(c, 4, 1, 20 + 3, 14)
    elif kind == "l4p_l4": a(c, 4, 6, 60, 14, flags=O.F_L4P | O.F_L4)
    elif kind == "l4p_icmp": a(c, 4, 1, 60, 14, flags=O.F_L4P)
    elif kind == "ip_on_v6": a(c, 6, 17, 60, 14, flags=O.F_IP | O.F_L4)
    elif kind == "flag80": a(c, 4, 17, 60, 14, flags=V4F | FLAG_REJECTED)
    elif kind == "off_past": a(c, 4, 17, 60, 14, over=dict(oob="off_past"))
    elif kind == "end_plus1": a(c, 4, 17, 60, 14, over=dict(oob="end_plus1"))
    else: raise KeyError(kind)


def _per_packet(S):
    # end16: end in chunk 4 (kfast 0) and chunk 5 (kfast 1); klo 4 in both
    for base in (64, 80):
        for e in range(16):
            S.add(f"end16/v4/{base}", 4, 6, base + e - 14, 14)
            S.add(f"end16/v6/{base}", 6, 6, base + e - 6, 6)
    for r0 in (0, 2, 14):
        for end in (r0 + 29, r0 + 31, 49, 63):
            S.add("short_odd", 4, 17, end - r0, r0)
            S.add("short_odd", 4, 1, end - r0, r0)
    for r0 in range(1, 16, 2):
        S.add("r0_odd", 4, 17, 100 + r0, r0)
        S.add("r0_odd", 6, 6, 60 + r0, r0)
        S.add("r0_odd", 4, 6, 40, r0)
    for l4o in (41, 43):
        for proto in (6, 17, 58):
            for r0 in (0, 6):
                S.add("l4o_odd", 6, proto, l4o + 30, r0, l4o=l4o)
                S.add("l4o_odd", 6, proto, l4o + 200, r0, l4o=l4o)
    # fa_edge: every even r0 at which fa + 2 lands on 62, 64, 66 or 68
    for ver, l4o, proto in ((4, 40, 6), (4, 44, 6), (6, 40, 6), (6, 48, 17)):
        for r0 in range(0, 16, 2):
            if r0 + l4o + O.L4_FIELD[proto] + 2 in (62, 64, 66, 68):
                for extra in (20, 120):
                    S.add(f"fa_edge/{ver}/{l4o}", ver, proto, l4o + extra, r0, l4o=l4o)
    for proto in (6, 17, 1):
        for r0 in range(0, 16, 2):
            S.add("fa_edge/4/60", 4, proto, 60 + 40, r0, l4o=60)
    for ver in (4, 6):
        for proto, seg in ((17, 8), (6, 20), (1, 4), (1, 8)) + (((58, 4), (58, 8)) if ver == 6 else ()):
            for r0 in (0, 2):
                S.add("hdr_only", ver, proto, (20 if ver == 4 else 40) + seg, r0)
    for ts, us in SMALL_TIERS:
        for n in (ts * us, ts * us + 1):
            S.nch(f"small_edge/{n}", n, 0, 0)
            S.nch(f"small_edge/{n}", n, 14, 14, ver=6) if n > 5 else S.nch(f"small_edge/{n}", n, 2, 2, proto=6)
    for team, u in TEAM_UNROLLS:
        for k in (1, 2):
            for n in (k * team * u, k * team * u + 1):
                S.nch(f"trip_edge/{n}", n, 0, 0)
                S.nch(f"trip_edge/{n}", n, 14, 15, ver=6)
    for n in (576, 577):
        S.nch(f"trip_edge/{n}", n, 0, 0)
        S.nch(f"trip_edge/{n}", n, 2, 7, proto=6)
    S.add("big", 4, 17, 65535, 14)
    for ihl in range(5, 16):
        S.add("flags/ip", 4, 17, 4 * ihl + 8, 2 * (ihl % 8), l4o=4 * ihl, flags=O.F_IP)
    for ver in (4, 6):
        for proto in (6, 17):
            S.add("flags/l4", ver, proto, 90, 14, flags=O.F_L4)
            S.add("flags/l4p", ver, proto, 90, 14, flags=O.F_L4P)
            S.add("flags/l4p", ver, proto, 400, 0, flags=O.F_L4P)
        S.add("flags/0", ver, 17, 90, 14, flags=0)
        S.add("flags/pre", ver, 17, 90, 14, flags=O.F_PRE | (V4F if ver == 4 else V6F))
    for ln in RAW_LENS:
        for r0 in (0, 6, 1, 15):
            S.add("flags/raw", 0, 0, 0, r0, raw=ln)
    for r0 in (0, 4, 6, 14):
        S.add("field_chunk", 4, 17, 80, r0)     # IP field chunk 0 / 1; UDP field chunk 1 (r0 0, 4) / 2
    S.add("field_chunk", 4, 6, 80, 14)          # TCP field at 50: chunk 3
    S.add("field_chunk", 4, 1, 80, 0)           # ICMP field at 22: chunk 1
    S.add("field_chunk", 6, 6, 80, 0)           # TCP over IPv6 at 56: chunk 3


def _unit(S, name, makers):
    """One whole unit: makers is 64 (function, index) pairs in lane order."""
    assert len(S) % UNIT == 0 and len(makers) == UNIT, (name, len(makers))
    for f, i in makers:
        f(S, name, i)


def _mix(rng, groups):
    """Lane order of a unit made of (function, count) groups, shuffled."""
    m = [(f, i) for f, c in groups for i in range(c)]
    return [m[j] for j in rng.permutation(len(m))]


def all_key_nchs() -> list:
    return sorted({k * t * u for t, u in TEAM_UNROLLS for k in range(1, 13)})


def _unit_classes(S, pos):
    """The unit classes once; pos tells the two passes apart (other compositions of the same class)."""
    rng = S.rng
    for live in ONE_CLASS_LIVE:
        _unit(S, f"one_class/{live}", _mix(rng, [(_large, live), (_bad, UNIT - live)]))
    for k in N_SMALL:
        big = [(_large, UNIT - k)] if pos == 0 else [(_large, (UNIT - k + 1) // 2), (_large2, (UNIT - k) // 2)]
        _unit(S, f"n_small/{k}", _mix(rng, [(_small, k - k // 4), (_bad, k // 4)] + big))
    _unit(S, "filler_unit", [(_filler, i) for i in range(UNIT)])
    _unit(S, "uniform", [(lambda S, c, i: S.add(c, 4, 17, 50, 14), i) for i in range(UNIT)])
    _unit(S, "filler_unit", [(_filler, i + 5) for i in range(UNIT)])
    for r in range(8):
        size = 16 + r
        _unit(S, f"tail/{r}", _mix(rng, [(_large, 9), (_large2, size - 9), (_small, UNIT - size)]))
    ks = all_key_nchs()
    one = lambda n: (lambda S, c, i: S.nch(c, n, (0, 14)[i % 2], (0, 15)[i % 2]))
    m = [(one(n), j) for j, n in enumerate(ks)] + [(_bad, 0), (_small, 1), (_slow, 2), (_slow, 3),
                                                 (lambda S, c, i: S.add(c, 4, 17, 90, 14, flags=0), 0)]
    m += [(_filler, i) for i in range(UNIT - len(m))]
    _unit(S, "all_keys", [m[j] for j in rng.permutation(UNIT)])
    _unit(S, "slow_only", [(_slow, i) for i in range(UNIT)])
    _unit(S, "all_bad", [(_bad, i) for i in range(UNIT)])


def batch(seed: int = 2025):
    """The geometry batch: {arena, desc, cls (per packet), oob (index -> kind of the descriptors that
    are out of the arena's range by their offset), big (the 65,535-B packet's index), n}."""
    S = _Specs(seed)
    _per_packet(S)
    _pad_to_unit(S)
    # refused: unit j holds kind (j + t) % K at lane REFUSED_LANES[t]
    K = len(REFUSED)
    for j in range(K):
        at = {lane: REFUSED[(j + t) % K] for t, lane in enumerate(REFUSED_LANES)}
        for lane in range(UNIT):
            if lane in at:
                _refused(S, at[lane])
            else:
                _filler(S, "filler", j * UNIT + lane)
    _unit_classes(S, 0)
    for k in (9, 13):   # the second pass 36 units after the first: 36 * 9 is no multiple of a live range but 9 and 1
        _unit(S, "filler_unit", [(_filler, i + k) for i in range(UNIT)])
    _unit_classes(S, 1)
    for i in range(UNIT - 1):
        _filler(S, "filler", 3 * i + 1)
    S.add("arena_end", 4, 17, 61, 2)
    return _layout(S)


def _layout(S):
    specs = S.s
    n = len(specs)
    assert n % UNIT == 0
    total = sum(16 + ((len(s["l3"]) + s["r0"] + 15) & ~15) for s in specs) + 64
    arena = S.rng.integers(1, 256, total, dtype=np.uint8)    # nonzero noise
    desc = np.zeros(n, O.DESC_DTYPE)
    cur, oob, big = 0, {}, None
    for i, s in enumerate(specs):
        base = ((cur + 15) & ~15) + s["r0"]
        L = len(s["l3"])
        arena[base:base + L] = np.frombuffer(bytes(s["l3"]), np.uint8)
        cur = base + L
        desc[i] = (base, L, s["l4o"], s["ver"], s["proto"], s["flags"], 0)
        for k, v in s["over"].items():
            if k == "oob":
                oob[i] = v
            else:
                desc[k][i] = v
        if s["cls"] == "big":
            big = i
    arena = arena[:cur].copy()       # the last packet ends on the arena's last byte
    assert len(arena) % 16 != 0
    b = dict(arena=arena, desc=desc, cls=[s["cls"] for s in specs], oob=oob, big=big, n=n)
    place_oob(b["desc"], oob, len(arena))
    return b


def place_oob(desc, oob, arena_len: int):
    """The out-of-range descriptors for an arena of arena_len bytes: an offset past the arena, and a
    packet whose last byte is the first one outside."""
    for i, kind in oob.items():
        desc["l3_off"][i] = arena_len + 4096 + 14 if kind == "off_past" else arena_len + 1 - int(desc["l3_len"][i])


def live_l4(b):
    """Indices of the packets whose descriptor sums an L4 segment in full (F_L4), by the rules."""
    alen = len(b["arena"])
    out = []
    for i, d in enumerate(b["desc"]):
        p = plan(d, CB.DEFAULT_BUILD, alen)
        if not p.bad and p.do_l4 and not p.psonly:
            out.append(i)
    return out


def corrupted(b):
    """The wrong-sums copy for verify: every F_L4 packet in turn gets its IP field alone wrong
    (IPv4 with F_IP; others: the next kind), its L4 field alone wrong, a payload byte flipped (the
    packet's last byte, or the segment's first where the field is last), its UDP field stored as 0,
    or is made to compute to 0 with 0xffff stored (UDP); one in six is left valid.  Returns the
    batch with the new arena and `kinds` {index: corruption}."""
    a = b["arena"].copy()
    kinds = {}
    for j, i in enumerate(live_l4(b)):
        d = b["desc"][i]
        off, ln, l4o, ver, proto, fl = (int(d[k]) for k in ("l3_off", "l3_len", "l4_off", "l3_ver", "l4_proto", "flags"))
        fld = O.L4_FIELD[proto]
        k = j % 6
        if k == 5:
            continue
        kind = CORRUPTIONS[k]
        if kind == "ip" and not (ver == 4 and fl & O.F_IP):
            kind = "l4"
        if kind in ("udp0", "udp_zero") and proto != 17:
            kind = "payload"
        if kind == "ip":
            a[off + 10] ^= 0x01
        elif kind == "l4":
            a[off + l4o + fld + 1] ^= 0x01
        elif kind == "payload":
            at = ln - 1 if ln - 1 > l4o + fld + 1 else l4o
            a[off + at] ^= 0x80
        elif kind == "udp0":
            a[off + l4o + 6:off + l4o + 8] = 0
        else:
            p = bytearray(a[off:off + ln].tobytes())
            E.force_l4_zero(p, ln, l4o, ver, 17)
            E._put16(p, l4o + 6, 0xFFFF)
            a[off:off + ln] = np.frombuffer(bytes(p), np.uint8)
        kinds[i] = kind
    return dict(b, arena=a, kinds=kinds)


# ----------------------------------------------------------------------------------------
# The oracle's answer
# ----------------------------------------------------------------------------------------
def expect(orc, arena, desc, mode=O.MODE_COMPUTE, n=None, write=False, threads=1):
    """(out, status, arena afterwards) of the first n descriptors as the checksum kernels owe them:
    the oracle's, with the two flags it does not know applied first -- F_PRE descriptors are left to
    the pre-image kernel (no sums: device_common.h csum_flags), 0x80 marks a descriptor the NAT
    kernel rejected (S_BAD_DESC, out 0)."""
    d = np.ascontiguousarray(desc[:n]).copy()
    rej = (d["flags"] & FLAG_REJECTED) != 0
    d["flags"][(d["flags"] & O.F_PRE) != 0] = 0
    d["l3_ver"][rej] = 0      # refused by the oracle's own rules; raw is checked before them
    d["flags"][rej] = 0
    a = arena.copy()
    out, st = orc.process(a, d, mode, write=write, threads=threads)
    return out, st, a


def describe(b, i: int, build=None, arena_len=None) -> str:
    d = b["desc"][i]
    cls = b["cls"][int(b["idx"][i]) if "idx" in b else i]      # layouts: the class of the batch's packet behind it
    alen = arena_len or b.get("arena_len") or len(b["arena"])
    p = plan(d, build or CB.DEFAULT_BUILD, alen)
    return (f"packet {i} (unit {i // UNIT} lane {i % UNIT}, workgroup {i // WG}) class {cls} desc off {int(d['l3_off'])} len "
            f"{int(d['l3_len'])} l4_off {int(d['l4_off'])} v{int(d['l3_ver'])} proto {int(d['l4_proto'])} flags "
            f"{int(d['flags']):#x}; {p}")


def first_diff(b, got, want, what: str, build=None, arena_len=None):
    """None, or a message naming the first packet whose `what` (out / status) differs."""
    bad = np.nonzero(got != want)[0]
    if not len(bad):
        return None
    i = int(bad[0])
    return f"{len(bad)} {what} differ, first: got {int(got[i]):#x}, oracle {int(want[i]):#x}: {describe(b, i, build, arena_len)}"


def first_arena_diff(b, got, want):
    bad = np.nonzero(got != want)[0]
    if not len(bad):
        return None
    at = int(bad[0])
    d = b["desc"]
    own = np.nonzero((d["l3_off"] <= at) & (at < d["l3_off"] + d["l3_len"].astype(np.uint64)))[0]
    who = describe(b, int(own[0])) + f", byte {at - int(d['l3_off'][own[0]])} of it" if len(own) else "no packet's byte"
    return f"{len(bad)} arena bytes differ, first at {at}: got {int(got[at]):#x}, oracle {int(want[at]):#x}: {who}"


# ----------------------------------------------------------------------------------------
# check_classes
# ----------------------------------------------------------------------------------------
def units_of(b, name: str) -> list:
    return [u for u in range(b["n"] // UNIT) if all(c == name for c in b["cls"][u * UNIT:(u + 1) * UNIT])]


def check_classes(b, build):
    """Every class of the module docstring is in the batch, recomputed from the descriptors with
    plan() for `build` (a csumbuilds.K2).  Counts that hold for every build:

      end16        64 packets: 2 versions x (kfast 0, kfast 1) x 16 ends, all fast class, klo 4
      short_odd    24, r0_odd 24, l4o_odd 24: all slow class
      fa_edge      fa + 2 in {62, 64}: fast (klo <= 4); in {66, 68}: slow (klo 5); each value present
                   for each of the four header shapes it can occur in; IPv4 l4_off 60: 24 packets
      hdr_only     20 packets of 10 shapes ending in the first 64 B, each shape with klo >= nch at some r0
      flags        F_IP alone at IHL 5..15 (11, need = l4_off); F_L4P 8 (need = l4_off + fld + 2);
                   flags 0 and F_PRE 2 each (nch 0); raw 48 (12 lengths x r0 0, 6, 1, 15)
      refused      19 kinds x lanes 0, 1, 31, 32, 63: 95 packets, each bad, and bad for its own
                   reason: the same descriptor with the kind's field put right is accepted
      unit classes each at 2 unit positions; one_class and n_small with different (unit index * 9) mod
                   the large tier's size (the rotation's first slot), but at sizes 9 and 1
    and for `build` itself: its small tier's nch = TS * US and + 1 (keys 1 and 3), its trips' nch =
    k * TEAM * U and + 1 (keys 2 + k and 3 + k) for k = 1, 2, the cap (nch 576 and 577 in one class
    for TEAM * U = 48), n_small = N_SMALL and the tails 16 + r for builds with a small tier, and
    possible_keys(build) in each all_keys unit."""
    alen = len(b["arena"])
    P = plans(b, build)
    cls = b["cls"]
    by = {}
    for i, c in enumerate(cls):
        by.setdefault(c, []).append(i)
    grp = lambda prefix: [i for c, ix in by.items() if c == prefix or c.startswith(prefix + "/") for i in ix]
    live = lambda i: not P[i].bad

    # end16
    for ver in ("v4", "v6"):
        for base, kf in ((64, 0), (80, 1)):
            ix = by[f"end16/{ver}/{base}"]
            assert sorted((P[i].r0 + P[i].need) & 15 for i in ix) == list(range(16))
            assert all(P[i].fastc and P[i].klo == 4 and P[i].kfast == kf and P[i].nch == (base >> 4) + (1 if (P[i].r0 + P[i].need) & 15 else 0)
                       for i in ix), (ver, base)
    assert len(grp("end16")) == 64
    for name, count in (("short_odd", 24), ("r0_odd", 24), ("l4o_odd", 24)):
        ix = by[name]
        assert len(ix) == count and all(live(i) and not P[i].hbm and P[i].key == 15 for i in ix), name
    assert all(not P[i].r0 & 1 and (P[i].r0 + P[i].need) & 1 and P[i].r0 + P[i].need < 64 for i in by["short_odd"])
    assert sorted({P[i].r0 for i in by["r0_odd"]}) == list(range(1, 16, 2))
    assert {int(b["desc"]["l4_off"][i]) for i in by["l4o_odd"]} == {41, 43}
    # fa_edge
    shapes = {"fa_edge/4/40": {62, 64, 66, 68}, "fa_edge/4/44": {62, 64, 66, 68}, "fa_edge/6/40": {62, 64, 66, 68},
              "fa_edge/6/48": {62, 64, 66, 68}}
    for name, vals in shapes.items():
        assert {P[i].fa + 2 for i in by[name]} == vals, name
        for i in by[name]:
            assert live(i) and P[i].hbm and P[i].fastc == (P[i].fa + 2 <= 64) and P[i].klo == (4 if P[i].fa + 2 <= 64 else 5), i
    assert len(by["fa_edge/4/60"]) == 24 and {P[i].r0 for i in by["fa_edge/4/60"]} == set(range(0, 16, 2))
    assert sum(P[i].fastc for i in by["fa_edge/4/60"]) == 1       # ICMP at r0 0: fa + 2 = 64
    # hdr_only
    ho = by["hdr_only"]
    assert len(ho) == 20 and all(live(i) and P[i].fastc and P[i].r0 + P[i].need <= 64 and P[i].kfast == 0 for i in ho)
    shapes_ho = {tuple(int(b["desc"][k][i]) for k in ("l3_ver", "l4_proto", "l3_len")) for i in ho}
    assert len(shapes_ho) == 10
    assert shapes_ho == {tuple(int(b["desc"][k][i]) for k in ("l3_ver", "l4_proto", "l3_len")) for i in ho if P[i].klo >= P[i].nch}
    # flags
    ix = by["flags/ip"]
    assert sorted(int(b["desc"]["l4_off"][i]) // 4 for i in ix) == list(range(5, 16))
    assert all(P[i].do_ip and not P[i].do_l4 and P[i].need == int(b["desc"]["l4_off"][i]) for i in ix)
    assert len(by["flags/l4p"]) == 8 and all(P[i].psonly and P[i].need == int(b["desc"]["l4_off"][i]) + P[i].fld + 2 for i in by["flags/l4p"])
    assert len(by["flags/l4"]) == 4 and all(P[i].do_l4 and not P[i].do_ip for i in by["flags/l4"])
    assert len(by["flags/0"]) == 2 == len(by["flags/pre"]) and all(live(i) and P[i].nch == 0 for i in by["flags/0"] + by["flags/pre"])
    raws = by["flags/raw"]
    assert len(raws) == 48 and all(P[i].raw and live(i) and not P[i].fastc for i in raws)
    assert {(P[i].need, P[i].r0) for i in raws} == {(ln, r0) for ln in RAW_LENS for r0 in (0, 6, 1, 15)}
    # field_chunk: the stored fields' chunks
    fc = by["field_chunk"]
    assert {(P[i].r0 + 10) >> 4 for i in fc if P[i].do_ip} == {0, 1} and {P[i].fa >> 4 for i in fc} == {1, 2, 3}
    # refused: bad, each kind on each lane, and for its own reason
    seen = Counter()
    for i in grp("refused"):
        kind = cls[i].split("/")[1]
        assert P[i].bad and P[i].key == 0, (i, kind)
        seen[(kind, i % UNIT)] += 1
        assert not plan(_repaired(b["desc"][i], kind, alen), build, alen).bad, (i, kind)
    assert set(seen) == {(k, lane) for k in REFUSED for lane in REFUSED_LANES} and sum(seen.values()) == 95
    # the accepted neighbour: the last packet ends on the arena's last byte
    last = b["desc"][-1]
    assert cls[-1] == "arena_end" and int(last["l3_off"]) + int(last["l3_len"]) == alen and alen % 16 and live(b["n"] - 1)
    ep = [i for i in b["oob"] if b["oob"][i] == "end_plus1"]
    assert all(int(b["desc"]["l3_off"][i]) + int(b["desc"]["l3_len"][i]) == alen + 1 for i in ep)
    # big
    assert int(b["desc"]["l3_len"][b["big"]]) == 65535 and P[b["big"]].nch == 4097 and P[b["big"]].fastc
    # this build's tier and trip limits
    fast_nch = {P[i].nch: P[i].key for i in grp("small_edge") + grp("trip_edge") if P[i].fastc}
    assert all(P[i].fastc for i in grp("small_edge") + grp("trip_edge"))
    tu = build.team * build.u
    if build.ts:
        s = build.ts * build.us
        assert fast_nch[s] == 1 and fast_nch[s + 1] == 3, build
    for k in (1, 2):
        assert fast_nch[k * tu] == 2 + k and fast_nch[k * tu + 1] == 3 + k, build
    assert fast_nch[576] == 2 + min(-(-576 // tu), 12) and fast_nch[577] == 2 + min(-(-577 // tu), 12)
    if tu == 48:
        assert fast_nch[576] == fast_nch[577] == 14
    # unit classes
    def unit_keys(u):
        return [P[i].key for i in range(u * UNIT, (u + 1) * UNIT)]

    def two_positions(name, rng_):
        us = units_of(b, name)
        assert len(us) >= 2, name
        if rng_ > 1 and rng_ != 9:      # unit index * 9 (kDefaultRot) is 0 mod 9 everywhere
            assert len({(u * 9) % rng_ for u in us}) >= 2, (name, us)
        return us

    for lv in ONE_CLASS_LIVE:
        for u in two_positions(f"one_class/{lv}", lv):
            ks = unit_keys(u)
            assert ks.count(0) == UNIT - lv and len(set(ks) - {0}) == 1 and min(set(ks) - {0}) >= 2, (u, lv)
    for k in N_SMALL:
        for pos, u in enumerate(two_positions(f"n_small/{k}", UNIT - k)):
            ks = unit_keys(u)
            if build.ts:
                assert sum(x <= 1 for x in ks) == k and 15 not in ks, (u, k)
                assert len({x for x in ks if x >= 2}) == (0 if k == UNIT else 1 if (pos == 0 or k == 63) else 2), (u, k)
            else:
                assert sum(x == 0 for x in ks) == k // 4
    for r in range(8):
        for u in two_positions(f"tail/{r}", 0):
            ks = unit_keys(u)
            if build.ts:
                big_ = [x for x in ks if x >= 2]
                assert len(big_) == 16 + r and len(set(big_)) == 2 and len(big_) % 8 == r and 15 not in ks, (u, r)
    for u in two_positions("all_keys", 0):
        assert set(unit_keys(u)) == possible_keys(build), (u, sorted(set(unit_keys(u))), build)
    for u in two_positions("slow_only", 0):
        assert set(unit_keys(u)) == {15}
    for u in two_positions("all_bad", 0):
        assert set(unit_keys(u)) == {0}
    for u in two_positions("uniform", 0):
        d = b["desc"][u * UNIT:(u + 1) * UNIT]
        assert len({(int(x["l3_len"]), int(x["l4_off"]), int(x["l3_ver"]), int(x["l4_proto"]), int(x["flags"]), int(x["l3_off"]) & 15)
                    for x in d}) == 1 and int(d["l3_len"][0]) <= 64
        assert np.all(np.diff(d["l3_off"].astype(np.int64)) == 64)      # contiguous: within 4 KiB
        assert cls[u * UNIT - 1] == "filler_unit" == cls[(u + 1) * UNIT]
    return Counter(c.split("/")[0] for c in cls)


def _repaired(d, kind, arena_len):
    """The refused descriptor with the one thing its kind names put right."""
    d = d.copy()
    fix = {"ver5": dict(l3_ver=4), "v4_len19": dict(l3_len=60), "v4_l4o16": dict(l4_off=20), "v4_l4o_gt_len": dict(l4_off=20),
           "v4_l4o_and3": dict(l4_off=20), "v6_len39": dict(l3_len=60), "v6_l4o39": dict(l4_off=40), "v6_l4o_gt_len": dict(l4_off=40),
           "proto47_l4": dict(l4_proto=17), "proto58_v4": dict(l4_proto=1), "short_tcp": dict(l3_len=int(d["l3_len"]) + 1),
           "short_udp": dict(l3_len=int(d["l3_len"]) + 1), "short_icmp": dict(l3_len=int(d["l3_len"]) + 1),
           "l4p_l4": dict(flags=O.F_L4P), "l4p_icmp": dict(l4_proto=6), "ip_on_v6": dict(flags=O.F_L4), "flag80": dict(flags=V4F),
           "off_past": dict(l3_off=14), "end_plus1": dict(l3_off=int(d["l3_off"]) - 1)}[kind]
    for k, v in fix.items():
        d[k] = v
    return d


# ----------------------------------------------------------------------------------------
# Layouts for the loop and the sampled paths
# ----------------------------------------------------------------------------------------
def sampled(n: int) -> np.ndarray:
    """The 64 descriptors every wave samples (kernels.hip :884)."""
    return (n * np.arange(64, dtype=np.int64)) >> 6


def sample_class(ln: int) -> int:
    """The sample's cost class of a packet length (kernels.hip :891-892)."""
    return 0 if ln <= 64 else 1 + (ln + 15) // (16 * CB.DEFAULT_TEAM * CB.DEFAULT_UNROLL)


def _cycle(b):
    """The batch's indices without the 65,535-B packet."""
    return np.array([i for i in range(b["n"]) if i != b["big"]], dtype=np.int64)


def _oob_of(b, idx) -> dict:
    """{position in idx: kind} of the descriptors that are out of range by their offset."""
    keys = np.array(sorted(b["oob"]), dtype=np.int64)
    return {int(j): b["oob"][int(idx[j])] for j in np.nonzero(np.isin(idx, keys))[0]}


def _aliased(b, idx, arena_len):
    """Descriptors idx of the batch on a device arena of arena_len bytes that holds the batch's
    arena at its front; the out-of-range ones stay out of range."""
    d = b["desc"][idx].copy()
    place_oob(d, _oob_of(b, idx), arena_len)
    return d


def second_trip(b, cus: int):
    """cus * 256 + 256 + 65 descriptors cycling the batch: with one workgroup per CU the first
    workgroup and 65 more lanes take a second trip through the unit loop."""
    cyc = _cycle(b)
    if (cus * 256) % len(cyc) == 0:
        cyc = cyc[:-1]
    n = cus * 256 + 256 + 65
    idx = cyc[np.arange(n) % len(cyc)]
    return dict(desc=_aliased(b, idx, len(b["arena"])), arena=b["arena"], arena_len=len(b["arena"]), n=n, cycle=len(cyc),
                idx=idx, cls=b["cls"])


def staged_sizes(cus: int) -> tuple:
    W = 2 * cus * 256
    return (4 * W - 1, 4 * W, 8 * W + 256 * 5 + 37)


def units_per_wave(n: int, W: int) -> Counter:
    """How many waves of a grid covering W packets per trip take how many units of a batch of n."""
    units = -(-n // UNIT)
    waves = W // UNIT
    return Counter((units - w + waves - 1) // waves for w in range(min(waves, units)))


def staged(b, cus: int, k: int):
    """staged_sizes(cus)[k] descriptors cycling the batch, the 64 sampled ones at least 1 KiB: the
    low-concurrency grid, staged result words from 4 units per wave on."""
    n = staged_sizes(cus)[k]
    alen = n * 1024
    assert alen >= len(b["arena"])
    cyc = _cycle(b)
    idx = cyc[np.arange(n) % len(cyc)]
    big = [i for i in cyc if int(b["desc"]["l3_len"][i]) >= 1024 and int(b["desc"]["flags"][i]) in (V4F, V6F)
           and int(b["desc"]["l3_ver"][i]) in (4, 6)]
    for j, s in enumerate(sampled(n)):
        idx[s] = big[j % len(big)]
    return dict(desc=_aliased(b, idx, alen), arena=b["arena"], arena_len=alen, n=n, idx=idx, cls=b["cls"])


def materialize(b, idx, rng):
    """Descriptors idx of the batch, each with a frame of its own: its chunks copied one after the
    other into a new noise arena (out-of-range descriptors are the caller's to place)."""
    d = b["desc"][idx].copy()
    off = d["l3_off"].astype(np.int64)
    ln = d["l3_len"].astype(np.int64)
    inside = np.array([int(i) not in b["oob"] for i in idx])
    lo = np.where(inside, off & ~15, 0)
    hi = np.where(inside, np.minimum((off + ln + 15) & ~15, (len(b["arena"]) + 15) & ~15), 0)
    hi = np.maximum(hi, lo)
    size = hi - lo
    start = np.concatenate(([0], np.cumsum(size)[:-1]))
    arena = rng.integers(1, 256, int(size.sum()) + 16, dtype=np.uint8)
    src = b["arena"]
    for j in range(len(idx)):
        if size[j]:
            chunk = src[lo[j]:hi[j]]
            arena[start[j]:start[j] + len(chunk)] = chunk
    d["l3_off"] = np.where(inside, start + (off - lo), off).astype(np.uint64)
    return arena[:int(size.sum())], d


SORTED_NSMALL = (1, 31, 32, 33, 64, 65, 96, 97, 128, 129, 255)


def sorted_compositions(b):
    """The first workgroups of sorted_units as (name, 256 batch indices), by plan() keys of the
    default build (the only one with workgroup-sorted units)."""
    P = plans(b, CB.DEFAULT_BUILD)
    usable = [i for i in range(b["n"]) if i != b["big"]]
    pool = {}
    for i in usable:
        pool.setdefault(P[i].key, []).append(i)
    take = lambda key, c, s=0: [pool[key][(s + j) % len(pool[key])] for j in range(c)]
    small = lambda c, s=0: [x for j in range(c) for x in (take(0, 1, s + j) if j % 5 == 4 else take(1, 1, s + j))]
    rng = np.random.default_rng(31)
    mix = lambda ix: [ix[j] for j in rng.permutation(len(ix))]
    comps = [("one_large", take(3, WG)), ("all_small", take(1, WG)), ("all_bad", take(0, WG))]
    for k in SORTED_NSMALL:
        comps.append((f"n_small/{k}", mix(small(k) + take(3, WG - k, k))))
    # class 4 (two trips) in wave 2 only
    w = [mix(take(1, 40, 64 * q) + take(3, 24, 7 * q)) for q in range(4)]
    w[2] = mix(take(1, 30) + take(3, 20) + take(4, 14))
    comps.append(("one_wave_class", [x for q in w for x in q]))
    for nit in range(1, 6):
        for r in range(8):
            size = 8 * (nit - 1) + (r or 8)
            comps.append((f"tier/{nit}/{r}", mix(take(3, size - size // 3, r) + take(5, size // 3, nit) + small(WG - size, size))))
    comps.append(("slow_present", mix(take(15, 40) + take(1, 100) + take(3, 100) + take(0, 16))))
    comps.append(("slow_absent", mix(take(1, 100, 50) + take(3, 100, 50) + take(5, 40) + take(0, 16, 3))))
    every = [pool[k][0] for k in sorted(pool)] + [pool[k][-1] for k in sorted(pool)]
    comps.append(("every_key", mix(every + take(1, WG - len(every), 9))))
    assert all(len(ix) == WG for _, ix in comps)
    return comps


def sorted_units(b, cus: int):
    """n = 2 * cus * 256 + 256 G + 37 descriptors with frames of their own (no aliases: the write
    case is safe): G composed workgroups (sorted_compositions), then copies of the whole batch, the
    last workgroup partial.  The device arena is n * 1024 bytes, this arena at its front."""
    comps = sorted_compositions(b)
    G = len(comps)
    n = 2 * cus * 256 + WG * G + 37
    alen = n * 1024
    rng = np.random.default_rng(32)
    head_idx = np.array([i for _, ix in comps for i in ix], dtype=np.int64)
    head, dh = materialize(b, head_idx, rng)
    cyc = _cycle(b)
    stride = (len(b["arena"]) + 15 + 16) & ~15
    rest = n - len(head_idx)
    copies = -(-rest // len(cyc))
    base0 = (len(head) + 15) & ~15
    arena = np.concatenate([head, rng.integers(1, 256, base0 - len(head), dtype=np.uint8)] +
                           [np.concatenate([b["arena"], rng.integers(1, 256, stride - len(b["arena"]), dtype=np.uint8)])
                            for _ in range(copies)])
    dr = np.concatenate([b["desc"][cyc]] * copies)[:rest].copy()
    dr["l3_off"] += (base0 + stride * (np.arange(rest) // len(cyc))).astype(np.uint64)
    desc = np.concatenate([dh, dr])
    idx = np.concatenate([head_idx, np.concatenate([cyc] * copies)[:rest]])
    assert len(arena) <= alen
    place_oob(desc, _oob_of(b, idx), alen)
    return dict(desc=desc, arena=arena, arena_len=alen, n=n, G=G, names=[c for c, _ in comps], idx=idx, cls=b["cls"])


def window_slab(b, limit: int = 128 << 10):
    """A slab of at most `limit` bytes holding a selection of the batch with frames of its own:
    packets of at least 1 KiB first (the sample's), then the batch in order while it fits; the
    descriptors that are out of range by their offset are left out."""
    d = b["desc"]
    ok = [i for i in range(b["n"]) if i != b["big"] and i not in b["oob"]]
    bigs = [i for i in ok if 1024 <= int(d["l3_len"][i]) <= 4096 and int(d["flags"][i]) in (V4F, V6F)][:12]
    pick, used = list(bigs), sum((int(d["l3_len"][i]) + 31) & ~15 for i in bigs)
    for i in ok:
        sz = (int(d["l3_len"][i]) + 31) & ~15
        if i not in bigs and int(d["l3_len"][i]) < 600 and used + sz <= limit - 4096 and i % 3 == 0:
            pick.append(i)
            used += sz
    rng = np.random.default_rng(33)
    order = [pick[j] for j in rng.permutation(len(pick))]
    arena, desc = materialize(b, np.array(order, dtype=np.int64), rng)
    assert len(arena) <= limit
    return dict(arena=arena, desc=desc, cls=[b["cls"][i] for i in order], n=len(order))


def staged_window(b, cus: int, line: int = 2 << 30):
    """n = 4 W + 64 * 3 + 5 descriptors on a slab laid across `line` (the 2-GiB window line): within
    each unit even lanes take packets that start below the line and odd lanes packets at or above it,
    the sampled ones are at least 1 KiB.  Returns the slab, its base in the device arena, the
    descriptors relative to the slab (the oracle's) and absolute (the device's)."""
    slab = window_slab(b)
    W = 2 * cus * 256
    n = 4 * W + UNIT * 3 + 5
    arena_len = max(n * 1024, (4 << 30) + (128 << 10))
    off = slab["desc"]["l3_off"].astype(np.int64)
    # the line falls inside a packet of the slab's middle: it starts below and reaches across
    order = np.argsort(off)
    mid = next(j for j in order[len(order) // 2:] if int(slab["desc"]["l3_len"][j]) >= 64 and
               not plan(slab["desc"][j], CB.DEFAULT_BUILD, len(slab["arena"])).bad)
    split = (int(off[mid]) + 32) & ~15
    below = np.nonzero(off < split)[0]
    above = np.nonzero(off >= split)[0]
    lane = np.arange(n)
    idx = np.where(lane % 2 == 0, below[(lane // 2) % len(below)], above[(lane // 2) % len(above)])
    bigs = np.nonzero(slab["desc"]["l3_len"] >= 1024)[0]
    for j, s in enumerate(sampled(n)):
        side = bigs[(off[bigs] < split) == (s % 2 == 0)]
        idx[s] = side[j % len(side)] if len(side) else bigs[j % len(bigs)]
    rel = slab["desc"][idx].copy()
    base = line - split
    dev = rel.copy()
    dev["l3_off"] += np.uint64(base)
    return dict(slab=slab["arena"], base=base, rel=rel, dev=dev, desc=rel, arena=slab["arena"], n=n, arena_len=arena_len,
                split=split, idx=idx, cls=slab["cls"], line=line)
