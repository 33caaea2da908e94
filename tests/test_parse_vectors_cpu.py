"""The frame parse's geometry batch (tests/parsevec.py) held to its edges on the CPU: every class is
there with the count its construction gives, every deep frame has its refused twins, the deepest
byte the rules read is the one kernels.hip names, the staged window takes every chunk count, and
every accepted frame's descriptor gives the same sums from the C oracle and the pure-Python
restatement.  tests/test_gpu_parse_forms.py walks the same batch through every form of the parse."""
from collections import Counter

import numpy as np
import pytest

import edgevec as E
import parsevec as PV
from oracle import oracle as O


@pytest.fixture(scope="module")
def B():
    return PV.batch()


def chunks(o: int, L: int) -> int:
    """16-byte chunks the service grid stages for a frame at arena offset o (the arena 16-B aligned)."""
    return ((o & 15) + min(L, PV.WINDOW) + 15) >> 4


def test_classes_and_counts(B):
    n = len(B["cls"])
    got = Counter(c.split("@")[0] for c in B["cls"])
    n_rules = len(E.parse_cases())
    assert n_rules == 86
    tw = {"tcp5": 1, "tcp15nop": 2, "tcp15ts": 2, "udp": 1, "icmp6": 1, "nonext": 1}
    per = len(PV.L4_KINDS) + sum(tw.values())             # a frame of each L4 kind and its twins
    shallow = 2 * (len(PV.H_ALL) - len(PV.H_DEEP)) * per
    resid = 2 * len(PV.H_DEEP) * 16 * per
    longer = 2 * len(PV.H_DEEP) * len(PV.DEEP_LENS) * per
    want = {"bounds": 22 * 64, "rules": n_rules * 16, "deep": shallow + resid + longer, "v4": 2 * 11 * 3 * 16,
            "egress": 2 * 11 * len(PV.EGRESS_FLAGS), "last": 2}
    assert dict(got) == want and n == sum(want.values())
    assert want["rules"] == 1376 and want["bounds"] == 1408 and want["deep"] == 3724 and n == 7852   # as DESIGN.md §6 states
    for r in range(16):   # every rules frame at every residue, and laid there
        idx = [i for i, c in enumerate(B["cls"]) if c == f"rules@{r}"]
        assert len(idx) == n_rules
        assert all(int(B["frame_off"][i]) % 16 == r for i in idx)
        assert [B["frames"][i] is not None and len(B["frames"][i]) for i in idx] == [len(f) for f, _, _ in E.parse_cases()]
        assert [B["info"][i] is not None for i in idx] == [ok for _, ok, _ in E.parse_cases()]
    assert B["arena"].nbytes < 2 << 20 and {0x00, 0x80} == set(np.unique(B["status"]))
    assert set(range(8)) | {0x08, 0x80} <= set(PV.EGRESS_FLAGS)


def test_layout_guards_and_residues(B):
    """Frames do not overlap, GUARD fill bytes lie before each and after all but the arena's last,
    and every byte outside the frames as they were laid (a frame the table cuts lies there whole) is
    fill."""
    a, n = B["arena"], len(B["cls"])
    covered = np.zeros(a.nbytes, bool)
    for i in range(n):
        o, L = int(B["frame_off"][i]), int(B["laid"][i])
        if not L:        # a bounds case that names an offset near the arena's end: no bytes of its own
            assert B["cls"][i] == "bounds" and B["case"][i] != "good" and B["info"][i] is None, i
            continue
        assert B["inb"][i] and int(B["frame_len"][i]) <= L, i
        assert (int(B["frame_len"][i]) < L) == (B["cls"][i] == "bounds" and B["case"][i] in
                                                 ("L=0", "L=13", "L=14", "L=18", "L=33", "L=34", "L=53", "802.1q L=17",
                                                  "802.1q L=18", "802.1q L=57", "ipv6 L=53", "ipv6 L=54", "ipv6 L=73")), i
        assert not covered[o:o + L].any(), i
        covered[o:o + L] = True
        assert (a[o - PV.GUARD:o] == PV.FILL).all(), i
        if o + L < a.nbytes:
            assert (a[o + L:o + L + PV.GUARD] == PV.FILL).all(), i
    assert (a[~covered] == PV.FILL).all() and (~covered).sum() >= PV.GUARD * (covered.sum() > 0)
    assert int(covered.sum()) == int(B["laid"].astype(np.int64).sum())
    last = n - 1
    assert int(B["frame_off"][last]) + int(B["frame_len"][last]) == a.nbytes and B["info"][last] is not None
    d = B["cut_n"] - 1
    assert int(B["frame_off"][d]) + int(B["frame_len"][d]) == B["cut_len"] and B["info"][d] is not None
    assert B["case"][d] == "deep" and B["inb"][:B["cut_n"]].sum() == B["inb"].sum() - 1
    # in the cut arena every accepted frame is still inside, every bounds case still outside or refused
    assert all(int(o) + int(L) <= B["cut_len"] for o, L, info in
               zip(B["frame_off"][:B["cut_n"]], B["frame_len"][:B["cut_n"]], B["info"][:B["cut_n"]]) if info is not None)


def test_bounds_cases_on_their_lanes(B):
    a_len = B["arena"].nbytes
    idx = [i for i, c in enumerate(B["cls"]) if c == "bounds"]
    assert idx == list(range(len(idx))) and len(idx) % 64 == 0     # whole waves from the batch's start
    seen = Counter()
    for i in idx:
        lane, case = i % 64, B["case"][i]
        assert (case != "good") == (lane in PV.BOUNDS_LANES), i
        if case == "good":
            assert B["inb"][i] and B["info"][i] is not None, i
            continue
        seen[case] += 1
        assert len({B["case"][(i // 64) * 64 + k] for k in PV.BOUNDS_LANES}) == 1
    assert set(seen.values()) == {5} and len(seen) == 22
    o, L = B["frame_off"].astype(object), B["frame_len"].astype(object)
    at = lambda name: [i for i in idx if B["case"][i] == name]
    assert all(o[i] + L[i] == a_len + 1 and o[i] < a_len for i in at("end+1"))
    assert all(o[i] == a_len and L[i] == 0 and B["inb"][i] for i in at("o=end,L=0"))
    assert all(o[i] == a_len and L[i] == 14 and not B["inb"][i] for i in at("o=end,L=14"))
    assert all(o[i] == a_len + 1 and not B["inb"][i] for i in at("o=end+1"))
    assert all(o[i] == 2 ** 64 - 1 and L[i] == 2 and (o[i] + L[i]) % 2 ** 64 == 1 for i in at("o=2^64-1,L=2"))
    assert all(o[i] == 0 and L[i] == 0xFFFFFFFF for i in at("o=0,L=2^32-1"))
    for Lc, ok in ((0, False), (13, False), (14, False), (18, False), (33, False), (34, False), (53, False), (54, True)):
        assert all(L[i] == Lc and (B["info"][i] is not None) == ok for i in at(f"L={Lc}"))
    for Lc, ok in ((17, False), (18, False), (57, False), (58, True)):
        assert all(L[i] == Lc and (B["info"][i] is not None) == ok for i in at(f"802.1q L={Lc}"))
    for Lc, ok in ((53, False), (54, False), (73, False), (74, True)):
        assert all(L[i] == Lc and (B["info"][i] is not None) == ok for i in at(f"ipv6 L={Lc}"))
    assert all(B["status"][i] == O.S_BAD_DESC for i in idx if not B["inb"][i])
    # o + L == arena_len: the arena's last frame, and the cut arena's
    assert o[len(o) - 1] + L[len(L) - 1] == a_len


def test_deep_frames_and_their_twins(B):
    """Every accepted deep frame is accepted by the oracle, lies behind an extension header at an odd
    or even L4 address as hdrExtLen says, and each of its twins differs in one byte among the last
    16 the rules read and is refused."""
    idx = [i for i, c in enumerate(B["cls"]) if c == "deep"]
    twins_of = Counter(B["of"][i] for i in idx if B["twin"][i])
    seen, odd, names = set(), 0, {k: set() for k in PV.L4_KINDS}
    for i in idx:
        vlan, h, kind, flen = B["case"][i]
        f = B["frames"][i]
        if B["twin"][i]:
            base = B["of"][i]
            g = B["frames"][base]
            assert B["info"][i] is None and O.parse_ether(f)[0] is None and B["info"][base] is not None
            diff = [k for k in range(len(f)) if f[k] != g[k]]
            r = PV.reach(g)
            assert len(f) == len(g) and len(diff) == 1 and r - 16 <= diff[0] < r, (i, diff, r)
            assert int(B["frame_off"][i]) % 16 == int(B["frame_off"][base]) % 16
            continue
        info = B["info"][i]
        assert info is not None and O.parse_ether(f)[0] is not None, B["case"][i]
        assert (info.l3_off, info.l4_off, info.ver) == (18 if vlan else 14, 48 + h, 6)
        assert flen is None or len(f) == flen
        want_tw = {"tcp15nop": 2, "tcp15ts": 2}.get(kind, 1)
        assert twins_of[i] == want_tw, B["case"][i]
        if (h, flen) in ((255, None), (255, 700)):     # which twins: a header-end frame and a long one
            names[kind] |= {B["twin"][k] for k in idx if B["of"][k] == i}
        odd += (int(B["frame_off"][i]) + info.l3_off + info.l4_off) & 1
        seen.add((vlan, h, kind, flen if h >= 246 else None, int(B["frame_off"][i]) % 16 if h >= 246 and flen is None else None))
    for vlan in (False, True):
        for kind in PV.L4_KINDS:
            for h in PV.H_ALL:
                if h < 246:
                    assert (vlan, h, kind, None, None) in seen
                    continue
                assert all((vlan, h, kind, None, r) in seen for r in range(16))
                assert all((vlan, h, kind, flen, None) in seen for flen in PV.DEEP_LENS)
    assert odd > 500     # an odd L4 address: hdrExtLen and the residue decide
    assert names == {"tcp5": {"doffpast", "doffopt"}, "tcp15nop": {"optlen", "kindlast"}, "tcp15ts": {"optlen", "kindlast"},
                     "udp": {"udplen"}, "icmp6": {"nexthdr"}, "nonext": {"hdrext"}}


def test_reach_is_the_window_kernels_hip_names(B):
    """No frame needs a byte past frame offset 380, the last of 18 B of Ethernet / 802.1Q, 40 + 8 +
    255 of IPv6 and its extension header and 60 of TCP header -- 381 bytes, inside the 384 the
    service grid stages -- and the batch holds frames that need exactly those.  Behind the reach a
    frame's bytes do not matter: the oracle gives the same descriptor, tuple and header sum with
    them inverted."""
    reach = [PV.reach(f) if f is not None else 0 for f in B["frames"]]
    assert max(reach) == 381 and max(reach) <= PV.WINDOW
    for i, f in enumerate(B["frames"]):
        if f is None:
            continue
        assert reach[i] <= len(f), i
        g = f[:reach[i]] + bytes(x ^ 0xFF for x in f[reach[i]:])
        a, b = O.parse_ether(f)[0], O.parse_ether(g)[0]
        assert a == b == B["info"][i], i
        assert O.flow_tuple(f) == O.flow_tuple(g) and O.hsum_record(f).tobytes() == O.hsum_record(g).tobytes(), i
    deepest = [i for i, r in enumerate(reach) if r == 381]
    assert {int(B["frame_off"][i]) % 16 for i in deepest if B["info"][i] is not None} == set(range(16))
    assert any(B["twin"][i] for i in deepest)


def test_staged_chunks_and_line_crossings(B):
    """(r0 + min(L, 384) + 15) >> 4 takes every value from 0 to 25, and r0 + reach of accepted deep
    frames ends exactly on, and one byte past, each of the staged window's last three 16-byte lines."""
    cnt = {chunks(int(o), int(L)) for o, L, ok in zip(B["frame_off"], B["frame_len"], B["inb"]) if ok}
    assert cnt == set(range(26)), sorted(set(range(26)) - cnt)
    ends = set()
    for i, c in enumerate(B["cls"]):
        if c == "deep" and B["info"][i] is not None:
            ends.add((int(B["frame_off"][i]) & 15) + PV.reach(B["frames"][i]))
    for line in (352, 368, 384):
        assert line in ends and line + 1 in ends, line
    assert max(ends) == 15 + 381
    # frames of 383 / 384 / 385 bytes at staged ends on both sides of the window's end
    for L in (383, 384, 385):
        r0s = {int(o) & 15 for o, l, c in zip(B["frame_off"], B["frame_len"], B["cls"]) if c == "deep" and int(l) == L}
        assert len(r0s) >= 8, (L, r0s)


def test_l4_addresses(B):
    v4 = [i for i, c in enumerate(B["cls"]) if c == "v4"]
    seen = set()
    for i in v4:
        vlan, ihl, proto, m, pad = B["case"][i]
        info = B["info"][i]
        assert info is not None and (info.l4_off, info.proto) == (ihl * 4, proto)
        assert (int(B["frame_off"][i]) + info.l3_off + info.l4_off) % 4 == m
        assert int(B["frame_len"][i]) == info.l3_off + info.l3_len + pad
        seen.add((vlan, ihl, proto, m, pad))
    assert len(seen) == 2 * 11 * 3 * 4 * 4
    for h in PV.H_ALL:      # deep: odd and even L4 addresses for every hdrExtLen
        par = {(int(B["frame_off"][i]) + B["info"][i].l3_off + B["info"][i].l4_off) & 1
               for i, c in enumerate(B["cls"]) if c == "deep" and B["info"][i] is not None and B["case"][i][1] == h}
        assert par == {0, 1}, h
    # an odd hdrExtLen at an even frame address puts the L4 header at an odd one (14 / 18 + 40 + 8 + hdrExtLen)
    n_odd = 0
    for i, c in enumerate(B["cls"]):
        if c == "deep" and B["info"][i] is not None and B["case"][i][1] & 1 and not int(B["frame_off"][i]) & 1:
            assert (int(B["frame_off"][i]) + B["info"][i].l3_off + B["info"][i].l4_off) & 1, i
            n_odd += 1
    assert n_odd > 300
    for h in PV.H_ALL:      # and for every odd hdrExtLen such a frame is there
        if h & 1:
            assert any(c == "deep" and B["info"][i] is not None and B["case"][i][1] == h and not int(B["frame_off"][i]) & 1
                       for i, c in enumerate(B["cls"])), h


def test_egress_flags_over_every_kind(B):
    eg = [i for i, c in enumerate(B["cls"]) if c == "egress"]
    seen = Counter()
    for i in eg:
        info = B["info"][i]
        assert info is not None
        w = int(B["fwant"][i])
        seen[(B["case"][i], w)] += 1
        al = O.desc_flags_for(info)
        # the rule, spelled out: every flag asked must be one the frame allows
        ok = not w & ~0x0B and not (w & 2 and w & 8) and (not w & 1 or al & 1) and (not w & 2 or al & 2) and \
            (not w & 8 or (al & 2 and info.proto != 1))
        assert bool(ok) == bool(B["eg_ok"][i]), (B["case"][i], w)
    assert len(seen) == 22 * len(PV.EGRESS_FLAGS) and set(seen.values()) == {1}
    kinds = {c[0] for c, _ in seen}
    assert len(kinds) == 11
    ok_n = sum(bool(B["eg_ok"][i]) for i in eg)
    assert 0 < ok_n < len(eg)
    # a frame whose segment cannot hold the field: F_L4 refused, F_IP alone honoured
    for i in eg:
        if B["case"][i][0] in ("v4 icmp 1", "v4 icmp 3", "v4 proto 58"):
            assert bool(B["eg_ok"][i]) == (int(B["fwant"][i]) in (0, 1)), B["case"][i]
    # outside the class every parsed frame's flag byte is one it can honour
    other = [i for i, c in enumerate(B["cls"]) if c != "egress" and B["info"][i] is not None]
    assert all(B["eg_ok"][i] for i in other)
    assert len({int(B["fwant"][i]) for i in other}) >= 6


def test_sums_c_oracle_equals_pure_python(B, orc):
    """Every accepted frame's descriptor -- the ingress one, and the egress one with the frame's own
    flags -- gives the same sums from Oracle.process and oracle.pure_process; the verify of the
    batch has both verdicts."""
    arena = B["arena"]
    acc = np.flatnonzero(B["status"] == 0)
    assert len(acc) == sum(info is not None for info in B["info"])
    for desc in (B["desc"], PV.egress_desc(B)):
        out, st = orc.process(arena, np.ascontiguousarray(desc[acc]))
        for k, i in enumerate(acc):
            info, d = B["info"][i], desc[i]
            if d["l3_ver"] == 0:         # an egress frame whose flags cannot be honoured
                assert not B["eg_ok"][i] and st[k] == O.S_BAD_DESC
                continue
            o = int(B["frame_off"][i]) + info.l3_off
            assert int(d["l3_off"]) == o
            ipc, l4c = O.pure_process(arena[o:o + info.l3_len].tobytes(), info, int(d["flags"]))
            assert st[k] == O.S_DONE and int(out[k]) == ipc | (l4c << 16), (i, B["cls"][i], B["case"][i])
    _, vst = orc.process(arena, np.ascontiguousarray(B["desc"][acc]), O.MODE_VERIFY)
    fl = B["desc"]["flags"][acc]
    l4 = (fl & O.F_L4) != 0
    good = ((vst & O.S_L4_OK) != 0) & l4
    assert 0.6 * l4.sum() < good.sum() < 0.9 * l4.sum()
    ip = (fl & O.F_IP) != 0
    assert 0.6 * ip.sum() < ((vst & O.S_IP_OK) != 0)[ip].sum() < 0.9 * ip.sum()
    # refused frames: all-zero expectations
    ref = np.flatnonzero(B["status"] != 0)
    assert not B["desc"][ref].view(np.uint8).any() and not B["tuples"][ref].view(np.uint8).any()
    assert not B["hsum"][ref].view(np.uint8).any()
    # ingress flags for another `want` come from the same rule
    for want in (0, O.F_IP, O.F_L4, O.F_L4P, O.F_IP | O.F_L4 | O.F_L4P):
        d = PV.ingress_desc(B, want)
        assert not (d["flags"] & (0xFF ^ want)).any() and not ((d["flags"] & O.F_L4) != 0)[(d["flags"] & O.F_L4P) != 0].any()
    assert np.array_equal(PV.ingress_desc(B, O.F_IP | O.F_L4), B["desc"])
