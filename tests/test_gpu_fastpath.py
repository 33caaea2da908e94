"""The flow table's Fastpath on the GPU (vpcsum_flowtab_set_fastpath, vpcsum_flow_lookup_fp_async,
vpcsum_l2_forward_async, vpcsum_ctx_nat_flow_forward_frames): the expected lookup is a Python dict
over the 38 key bytes, the expected frames the oracle's NAT (natvec.expect / tcprwvec.expected) with
the dict's entries followed by the L2 rule as tests/fastpathvec.py restates it.  Everything is
compared bit for bit.  (The helpers of tests/test_gpu_flow.py this file needs are copied here.)"""
import os
import struct
import subprocess

import numpy as np
import pytest

import fastpathvec as F
import hsumvec as H
import natvec as NV
import tcprwvec as T
from oracle import oracle as O

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MISS, HIT, PUNT = 0, 1, 2
KEY = 38
ZERO_FP = bytes(16)


@pytest.fixture(scope="module")
def V():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vproxy_amd import vpcsum
    vpcsum.lib()
    return vpcsum


def dev(a):
    """Host to device through pinned memory, as the other GPU tests copy."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).pin_memory().cuda()


def host(t):
    """Device to host through pinned memory (no copy of this file touches pageable memory:
    DESIGN.md §11 item 5)."""
    import torch
    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    h.copy_(t)
    torch.cuda.synchronize()
    return h.numpy().copy()


def mk_key(V, ver=4, proto=6, src=b"\x0a\x00\x00\x01", dst=b"\x0a\x00\x00\x02", sport=1000, dport=80):
    k = np.zeros(1, V.TUPLE_DTYPE)
    k["src"][0] = np.frombuffer(bytes(src).ljust(16, b"\0"), np.uint8)
    k["dst"][0] = np.frombuffer(bytes(dst).ljust(16, b"\0"), np.uint8)
    k["sport"][0] = np.frombuffer(int(sport).to_bytes(2, "big"), np.uint8)
    k["dport"][0] = np.frombuffer(int(dport).to_bytes(2, "big"), np.uint8)
    k["l3_ver"], k["l4_proto"] = ver, proto
    return k[0]


def kb(t) -> bytes:
    return np.asarray(t).tobytes()[:KEY]


def with_flags(V, k, flags):
    m = np.array([k], V.TUPLE_DTYPE)
    m["tcp_flags"] = flags
    return m[0]


def mk_entry(V, rng, mask=None):
    e = np.zeros(1, V.NAT_DTYPE)
    e.view(np.uint8)[:36] = rng.integers(0, 256, 36, dtype=np.uint8)
    e["mask"] = int(rng.integers(1, 16)) if mask is None else mask
    e["ttl"] = int(rng.integers(2, 256))
    return e[0]


def mk_flows(V, keys, entries, cookies):
    f = np.zeros(len(keys), V.FLOW_DTYPE)
    for i, (k, e, c) in enumerate(zip(keys, entries, cookies)):
        f["key"][i], f["rw"][i], f["cookie"][i] = k, e, c
    return f


def mk_fp(rng, port):
    return F.mk_fp(bytes(rng.integers(0, 256, 6, dtype=np.uint8)), bytes(rng.integers(0, 256, 6, dtype=np.uint8)), port)


def tuples_of(V, frames):
    out = np.zeros(len(frames), V.TUPLE_DTYPE)
    for i, f in enumerate(frames):
        t = O.flow_tuple(f)
        for k in ("src", "dst", "sport", "dport"):
            out[k][i] = np.frombuffer(t[k], np.uint8)
        out["l3_ver"][i], out["l4_proto"][i], out["tcp_flags"][i] = t["l3_ver"], t["l4_proto"], t["tcp_flags"]
    return out


def model_lookup(V, table: dict, fps: dict, tuples):
    """(verdicts, entries, Fastpath records) of the dicts {38 key bytes: entry}, {38 key bytes: record}."""
    vd = np.zeros(len(tuples), np.uint8)
    rw = np.zeros(len(tuples), V.NAT_DTYPE)
    fp = np.zeros(len(tuples), V.FASTPATH_DTYPE)
    for i, t in enumerate(tuples):
        e = table.get(kb(t)) if int(t["l3_ver"]) != 0 and int(t["l4_proto"]) in (6, 17) else None
        if e is None:
            continue
        if int(t["l4_proto"]) == 6 and int(t["tcp_flags"]) & 0x07:
            vd[i] = PUNT
        else:
            vd[i], rw[i] = HIT, e
            if kb(t) in fps:
                fp[i] = fps[kb(t)]
    return vd, rw, fp


def keys_by_home(V, slots, want: dict, **kw):
    out, need = [], dict(want)
    for sp in range(1, 5000):
        k = mk_key(V, sport=sp, **kw)
        h = V.flow_hash(k) & (slots - 1)
        if need.get(h, 0) > 0:
            need[h] -= 1
            out.append(k)
        if not any(need.values()):
            return out
    raise AssertionError("no keys with the wanted home slots")


def gpu_lookup_fp(V, tab, tuples, n=None, stream=None):
    """(verdicts, entries, records) of the Fastpath lookup and (verdicts, entries) of the plain one;
    the outputs start as 0xAB and carry two guard rows, which must stay."""
    import torch
    n = len(tuples) if n is None else n
    tu = dev(tuples[:n]) if n else torch.zeros(40, dtype=torch.uint8, device="cuda")
    outs = []
    for with_fp in (True, False):
        rw = torch.full(((n + 2) * 48,), 0xAB, dtype=torch.uint8, device="cuda")
        vd = torch.full((n + 2,), 0xAB, dtype=torch.uint8, device="cuda")
        fp = torch.full(((n + 2) * 16,), 0xAB, dtype=torch.uint8, device="cuda")
        tab.lookup(tu, n, rw, vd, stream, fastpath=fp if with_fp else None)
        torch.cuda.synchronize()
        rw, vd, fp = host(rw), host(vd), host(fp)
        assert (vd[n:] == 0xAB).all() and (rw[n * 48:] == 0xAB).all() and (fp[n * 16:] == 0xAB).all()
        if not with_fp:
            assert (fp == 0xAB).all()
        outs.append((vd[:n], rw[:n * 48], fp[:n * 16]))
    return outs


def check_lookup_fp(V, tab, table, fps, tuples, n=None):
    n = len(tuples) if n is None else n
    want_vd, want_rw, want_fp = model_lookup(V, table, fps, tuples[:n])
    (vd, rw, fp), (vd0, rw0, _) = gpu_lookup_fp(V, tab, tuples, n)
    assert np.array_equal(vd, vd0) and np.array_equal(rw, rw0)          # what vpcsum_flow_lookup_async returns
    assert np.array_equal(vd, want_vd), (vd, want_vd)
    assert rw.tobytes() == want_rw.tobytes()
    got = fp.reshape(n, 16) if n else fp.reshape(0, 16)
    bad = [i for i in range(n) if got[i].tobytes() != want_fp[i].tobytes()]
    assert not bad, [(i, got[i].tobytes().hex(), want_fp[i].tobytes().hex()) for i in bad[:4]]
    for i in range(n):
        if want_vd[i] != HIT:
            assert got[i].tobytes() == ZERO_FP
    return want_vd, want_fp


# ------------------------------------------------------------------------------------------
# 1. the lookup with Fastpath on the smallest table
# ------------------------------------------------------------------------------------------
def test_lookup_with_fastpath_on_the_smallest_table(V):
    """8 slots, 4 flows: three keys share home slot 6 (slots 6, 7 and, wrapped, 0), one lies apart;
    the first and third of the chain and the fourth have a Fastpath, the second has none.  Batches
    of 0, 1, 7, 8, 9 and 33 tuples -- hits, a miss, a punt -- return each flow's own record, 16 zero
    bytes on MISS / PUNT and for a flow without one, and the entries and verdicts of the plain lookup.
    Erase the first of the chain: the shifted flows keep their own records.  A replace keeps the
    record, port 0 clears it, a key not in the table is counted, a malformed key changes nothing."""
    rng = np.random.default_rng(21)
    tab = V.FlowTable(4)
    a, b, c = keys_by_home(V, 8, {6: 3})
    d = keys_by_home(V, 8, {3: 1}, proto=17)[0]
    assert [V.flow_hash(k) & 7 for k in (a, b, c, d)] == [6, 6, 6, 3]
    keys = [a, b, c, d]
    entries = [mk_entry(V, rng) for _ in keys]
    tab.update(add=mk_flows(V, keys, entries, (1, 2, 3, 4)))
    assert tab.info() == {"slots": 8, "flows": 4, "max_probe": 2}
    table = {kb(k): e for k, e in zip(keys, entries)}
    absent = mk_key(V, sport=6001)
    syn = with_flags(V, c, 0x02)
    pool = [a, b, c, d, absent, syn, with_flags(V, a, 0x10), with_flags(V, d, 0x02)]   # a UDP flow is never punted
    tuples = np.array([pool[(i * 3) % len(pool)] for i in range(33)], V.TUPLE_DTYPE)
    fps = {}
    check_lookup_fp(V, tab, table, fps, tuples)                      # today's callers: no flow has one
    rec = {kb(k): mk_fp(rng, p) for k, p in ((a, 11), (c, 0xC0000003), (d, 1))}
    assert tab.set_fastpath(np.array([a, c, d], V.TUPLE_DTYPE), np.array([rec[kb(k)] for k in (a, c, d)], V.FASTPATH_DTYPE)) == 0
    fps.update(rec)
    for n in (0, 1, 7, 8, 9, 33):
        want_vd, want_fp = check_lookup_fp(V, tab, table, fps, tuples, n)
    assert {MISS, HIT, PUNT} <= set(want_vd.tolist()) and len({int(p) for p in want_fp["port"]}) == 4   # 0 and the three ports
    # erase the first of the chain: b and c shift back one slot each, with their own records
    tab.update(delete=np.array([a], V.TUPLE_DTYPE))
    del table[kb(a)], fps[kb(a)]
    assert tab.info() == {"slots": 8, "flows": 3, "max_probe": 1}
    want_vd, want_fp = check_lookup_fp(V, tab, table, fps, tuples)
    assert want_fp["port"][list(map(kb, tuples)).index(kb(c))] == 0xC0000003
    # a flow that takes the erased flow's place starts with none
    tab.update(add=mk_flows(V, [a], [entries[0]], (5,)))
    table[kb(a)] = entries[0]
    check_lookup_fp(V, tab, table, fps, tuples)
    # replace keeps it
    e2 = mk_entry(V, rng)
    tab.update(add=mk_flows(V, [c], [e2], (33,)))
    table[kb(c)] = e2
    check_lookup_fp(V, tab, table, fps, tuples)
    # port 0 clears it (whatever addresses come with it); a key not there is counted
    gone = mk_fp(rng, 0)
    newb = mk_fp(rng, 77)
    assert tab.set_fastpath(np.array([d, absent, b], V.TUPLE_DTYPE), np.array([gone, newb, newb], V.FASTPATH_DTYPE)) == 1
    del fps[kb(d)]
    fps[kb(b)] = newb
    check_lookup_fp(V, tab, table, fps, tuples)
    # a malformed key among good ones: refused with nothing changed
    bad = np.array([c, with_flags(V, a, 0x10)], V.TUPLE_DTYPE)
    with pytest.raises(V.VpcsumError, match="vpcsum_flowtab_set_fastpath: key 1: "):
        tab.set_fastpath(bad, np.array([gone, gone], V.FASTPATH_DTYPE))
    check_lookup_fp(V, tab, table, fps, tuples)
    tab.close()


# ------------------------------------------------------------------------------------------
# 2. the L2 write alone
# ------------------------------------------------------------------------------------------
L2_CASES = [  # (name, verdict, status, has a port)
    ("hit_done", HIT, O.S_DONE, True),
    ("hit_done_mss_absent", HIT, O.S_DONE | T.S_MSS_ABSENT, True),
    ("hit_bad", HIT, O.S_BAD_DESC, True),
    ("hit_bad_ttl", HIT, O.S_BAD_DESC | O.S_TTL_EXPIRED, True),
    ("punt", PUNT, O.S_DONE, True),
    ("miss", MISS, O.S_DONE, True),
    ("port0", HIT, O.S_DONE, False),
]


@pytest.mark.parametrize("shift", [0, 1], ids=["arena_aligned", "arena_odd"])
def test_l2_forward_alone(V, shift):
    """vpcsum_l2_forward_async on a device arena: each verdict x status combination at each frame
    address residue 0..3 mod 4 (the arena itself starting at an aligned or at an odd address), the
    first frame at arena offset 0 and the last ending at arena_len, a 13-byte frame, a frame that
    ends past arena_len and one that starts far past it.  The whole arena and every port equal the
    restatement's: no byte outside [0,12) of an eligible frame changes."""
    import torch
    rng = np.random.default_rng(22)
    offs, lens, vds, sts, fps, names = [], [], [], [], [], []
    cur = 0
    for r in range(4):
        for name, vd, st, has in L2_CASES:
            while cur % 4 != r:
                cur += 1
            ln = int(rng.integers(14, 24))
            offs.append(cur); lens.append(ln); vds.append(vd); sts.append(st)
            fps.append(mk_fp(rng, int(rng.integers(1, 1 << 32)) if has else 0)); names.append(f"{name}@{r}")
            cur += ln + int(rng.integers(0, 3))
    offs.append(cur); lens.append(13); vds.append(HIT); sts.append(O.S_DONE); fps.append(mk_fp(rng, 5)); names.append("short")
    cur += 13
    offs.append(cur); lens.append(14); vds.append(HIT); sts.append(O.S_DONE); fps.append(mk_fp(rng, 6)); names.append("last")
    arena_len = cur + 14                                    # the last eligible frame ends at arena_len
    offs.append(arena_len - 13); lens.append(14); vds.append(HIT); sts.append(O.S_DONE); fps.append(mk_fp(rng, 7)); names.append("past_end")
    offs.append(1 << 40); lens.append(64); vds.append(HIT); sts.append(O.S_DONE); fps.append(mk_fp(rng, 8)); names.append("far")
    offs.append((1 << 64) - 8); lens.append(64); vds.append(HIT); sts.append(O.S_DONE); fps.append(mk_fp(rng, 9)); names.append("wraps")
    assert offs[0] == 0 and {o % 4 for o, nm in zip(offs, names) if nm.startswith("hit_done@")} == {0, 1, 2, 3}
    n = len(offs)
    offs, lens = np.array(offs, np.uint64), np.array(lens, np.uint32)
    vds, sts, fps = np.array(vds, np.uint8), np.array(sts, np.uint8), np.array(fps, V.FASTPATH_DTYPE)
    host_bytes = rng.integers(0, 256, arena_len, dtype=np.uint8)
    want, want_port = F.l2_forward(host_bytes, offs, lens, vds, sts, fps)
    assert sorted(np.flatnonzero(want_port)) == sorted(i for i, nm in enumerate(names) if nm.startswith(("hit_done", "last")))
    guard = 64
    big = torch.full((guard + shift + arena_len + guard,), 0x5A, dtype=torch.uint8, device="cuda")
    arena = big[guard + shift:guard + shift + arena_len]
    assert arena.data_ptr() % 4 == shift
    arena.copy_(torch.from_numpy(host_bytes).pin_memory())
    port = torch.full((n + 2,), 0xEEEEEEEE - (1 << 32), dtype=torch.int32, device="cuda")
    V.l2_forward(arena, dev(offs), dev(lens), dev(vds), dev(sts), dev(fps), n, port)
    torch.cuda.synchronize()
    got_port = host(port).view(np.uint32)
    assert (got_port[n:] == 0xEEEEEEEE).all()
    bad = np.flatnonzero(got_port[:n] != want_port)
    assert not len(bad), [(names[i], int(got_port[i]), int(want_port[i])) for i in bad[:8]]
    got = host(big)
    assert (got[:guard + shift] == 0x5A).all() and (got[guard + shift + arena_len:] == 0x5A).all()
    body = got[guard + shift:guard + shift + arena_len]
    if not np.array_equal(body, want):
        k = int(np.flatnonzero(body != want)[0])
        i = max(j for j in range(n) if int(offs[j]) <= k)
        raise AssertionError(f"byte {k} ({names[i]} +{k - int(offs[i])}): {body[k]:#x} != {want[k]:#x}")
    # n = 0 launches nothing
    V.l2_forward(arena, dev(offs), dev(lens), dev(vds), dev(sts), dev(fps), 0, port)


# ------------------------------------------------------------------------------------------
# 3. end to end
# ------------------------------------------------------------------------------------------
STRIDE, HEADROOM = 2048, 384
_KEEP = []


def rx_frames():
    """{name: frame}: IPv4 and IPv6, TCP and UDP, an 802.1Q frame, a 64-byte padded frame, a SYN, a
    frame of an unknown flow, two unparsable frames (a non-IP EtherType; 10 bytes), a UDP frame with
    TTL 1, and the two TCP frames of tests/test_gpu_flow.py's TCP-rewrite entries."""
    rng = np.random.default_rng(23)

    def tcp(ver, flags=0x10, payload=30, vlan=False):
        seg = H._tcp(rng, payload, False, None, 0)
        seg[13] = flags
        return H.with_sums(H.ether(rng, H._l3(rng, ver, seg, 6), ver, vlan))

    def udp(ver, payload=40, vlan=False, ttl=None):
        f = bytearray(H.ether(rng, H._l3(rng, ver, H._udp(rng, payload), 17), ver, vlan))
        if ttl is not None:
            f[14 + 8] = ttl
        return H.with_sums(bytes(f))

    fs = {"tcp4": tcp(4), "udp4": udp(4), "tcp6": tcp(6), "udp6": udp(6), "udp6_nofp": udp(6, 100),
          "vlan_udp4": udp(4, vlan=True), "vlan_tcp6": tcp(6, vlan=True),
          "pad64": udp(4, 2) + b"\x00" * 4, "syn": tcp(4, flags=0x02, payload=0), "unknown": tcp(4),
          "arp": bytes(rng.integers(0, 256, 12, dtype=np.uint8)) + b"\x08\x06" + bytes(rng.integers(0, 256, 46, dtype=np.uint8)),
          "runt": bytes(rng.integers(0, 256, 10, dtype=np.uint8)), "ttl1": udp(4, ttl=1),
          "ack": tcp(4, flags=0x10, payload=30), "ack2": tcp(6, flags=0x18, payload=12), "tcp4_nofp": tcp(4, payload=700)}
    assert len(fs["pad64"]) == 64 and fs["vlan_udp4"][12:14] == b"\x81\x00"
    return fs


@pytest.fixture(scope="module")
def rx(V, orc):
    fs = rx_frames()
    names, frames = list(fs), list(fs.values())
    n = len(frames)
    raw = np.zeros(n * STRIDE + 8192, np.uint8)
    _KEEP.append(raw)   # page-locked and released below: kept for the life of the process
    skip = (-raw.ctypes.data) % 4096
    arena = raw[skip:skip + n * STRIDE + 4096]   # page-aligned, umem geometry: 2,048-B chunks, frame at +384
    offs = np.array([i * STRIDE + HEADROOM for i in range(n)], np.uint64)
    lens = np.array([len(f) for f in frames], np.uint32)
    for o, f in zip(offs, frames):
        arena[int(o):int(o) + len(f)] = np.frombuffer(f, np.uint8)
    tuples = tuples_of(V, frames)
    desc = np.zeros(n, O.DESC_DTYPE)
    for i, f in enumerate(frames):
        info, _ = O.parse_ether(f)
        if info is not None:   # a refused frame keeps the all-zero descriptor the parse kernel writes
            desc[i] = (int(offs[i]) + info.l3_off, info.l3_len, info.l4_off, info.ver, info.proto, O.desc_flags_for(info), 0)
    assert [nm for nm, d in zip(names, desc) if d["l3_ver"] == 0] == ["arp", "runt"]
    rng = np.random.default_rng(24)
    idx = {nm: i for i, nm in enumerate(names)}
    in_table = [nm for nm in names if nm not in ("unknown", "arp", "runt")]
    table = {kb(tuples[idx[nm]]): mk_entry(V, rng, mask=int(rng.integers(1, 16))) for nm in in_table}
    table[kb(tuples[idx["ttl1"]])] = mk_entry(V, rng, mask=O.NAT_SRC | O.NAT_DEC_TTL)
    table[kb(tuples[idx["ack"]])] = mk_entry(V, rng, mask=O.NAT_SRC | O.NAT_DPORT)
    table[kb(tuples[idx["ack2"]])] = mk_entry(V, rng, mask=O.NAT_DST | O.NAT_SPORT)
    T.fill(table[kb(tuples[idx["ack"]])], T.SEQ_ADD | T.CLAMP_MSS, max_mss=1200, addend=-77)
    T.fill(table[kb(tuples[idx["ack2"]])], T.SET_FLAGS | T.CLAMP_MSS, flags=0x12, max_mss=1200)   # a SYN-ACK built: no MSS option
    keys = [with_flags(V, tuples[idx[nm]], 0) for nm in in_table]
    flows = mk_flows(V, keys, [table[kb(k)] for k in keys], range(1, len(keys) + 1))
    cookies = {kb(k): c for k, c in zip(keys, range(1, len(keys) + 1))}
    fps = {kb(tuples[idx[nm]]): mk_fp(rng, 100 + idx[nm]) for nm in in_table if not nm.endswith("_nofp")}
    want_vd, want_rw, want_fp = model_lookup(V, table, fps, tuples)
    assert [names[i] for i in np.flatnonzero(want_vd == PUNT)] == ["syn"]
    assert [names[i] for i in np.flatnonzero(want_vd == MISS)] == ["unknown", "arp", "runt"]
    want_hit = sorted({cookies[kb(t)] for t, v in zip(tuples, want_vd) if v == HIT})
    return dict(names=names, idx=idx, arena=arena, base=arena.copy(), offs=offs, lens=lens, desc=desc, flows=flows, fps=fps,
                keys=keys, want_vd=want_vd, want_rw=want_rw, want_fp=want_fp, want_hit=want_hit, n=n)


def _first_diff(rx, got, want):
    k = int(np.flatnonzero(got != want)[0])
    i = min(k // STRIDE, rx["n"] - 1)
    return f"byte {k}: frame {rx['names'][i]} +{k - int(rx['offs'][i])}: {got[k]:#x} != {want[k]:#x}"


@pytest.mark.parametrize("tcp", [False, True], ids=["nat", "tcp_rewrites"])
def test_nat_flow_forward_frames_end_to_end(V, orc, rx, tcp):
    """Context.nat_flow_forward_frames on an RX batch in a registered page-aligned arena at umem
    geometry, under both nat_modes (and both again with VPCSUM_NAT_TCP_REWRITES): every byte of the
    arena equals the oracle's NAT followed by the L2 rule, status and verdict equal those of
    Context.nat_flow_frames on a copy of the batch (whose bytes are the oracle's NAT alone), h_port
    is the flow's port exactly for the forwarded frames, and collect returns the same cookies after
    either entry point.  The SYN (PUNT), the unknown flow (MISS), the unparsable frames, the TTL-1
    frame (S_BAD_DESC | S_TTL_EXPIRED) and the flows without a Fastpath keep their Ethernet headers
    with port 0; the 802.1Q frames keep tag and EtherType; the frame whose rewrite answers
    S_DONE | S_MSS_ABSENT is forwarded."""
    n, arena, base, desc, idx = rx["n"], rx["arena"], rx["base"], rx["desc"], rx["idx"]
    bit = V.NAT_TCP_REWRITES if tcp else 0
    if tcp:
        nat, want_st = T.expected(orc, base, desc, rx["want_rw"])
    else:
        nat, want_st = NV.expect(orc, base, desc, rx["want_rw"], 1)
    want, want_port = F.l2_forward(nat, rx["offs"], rx["lens"], rx["want_vd"], want_st, rx["want_fp"])
    # the expectation itself has the cases the issue names
    assert want_st[idx["ttl1"]] == O.S_BAD_DESC | O.S_TTL_EXPIRED and rx["want_vd"][idx["ttl1"]] == HIT
    assert want_st[idx["ack2"]] == (O.S_DONE | T.S_MSS_ABSENT if tcp else O.S_DONE)
    quiet = ("syn", "unknown", "arp", "runt", "ttl1", "udp6_nofp", "tcp4_nofp")
    for nm, i in idx.items():
        o, ln = int(rx["offs"][i]), int(rx["lens"][i])
        if nm in quiet:
            assert want_port[i] == 0 and np.array_equal(want[o:o + min(ln, 14)], base[o:o + min(ln, 14)]), nm
        else:
            assert want_port[i] == 100 + i, nm
            assert want[o:o + 12].tobytes() == rx["want_fp"][i].tobytes()[:12] != base[o:o + 12].tobytes(), nm
            assert np.array_equal(want[o + 12:o + ln], nat[o + 12:o + ln]), nm
    for nm in ("vlan_udp4", "vlan_tcp6"):
        o = int(rx["offs"][idx[nm]])
        assert np.array_equal(want[o + 12:o + 18], base[o + 12:o + 18]) and want[o + 12] == 0x81, nm
    ctx = V.Context(0, max_arena=1 << 16, max_pkts=n)
    tab = V.FlowTable(64)
    tab.update(add=rx["flows"])
    fk = [k for k in rx["keys"] if kb(k) in rx["fps"]]
    assert tab.set_fastpath(np.array(fk, V.TUPLE_DTYPE), np.array([rx["fps"][kb(k)] for k in fk], V.FASTPATH_DTYPE)) == 0
    ctx.register(arena)
    try:
        for mode in (V.NAT_STRICT_JAVA | bit, V.NAT_RFC1624 | bit):
            # today's entry point on a copy of the batch: the oracle's NAT alone, Ethernet headers as received
            arena[:] = base
            st0, vd0 = ctx.nat_flow_frames(tab, arena, rx["offs"], rx["lens"], mode)
            assert np.array_equal(arena, nat), (hex(mode), _first_diff(rx, arena, nat))
            hit0 = sorted(tab.collect().tolist())
            arena[:] = base
            st, vd, port = ctx.nat_flow_forward_frames(tab, arena, rx["offs"], rx["lens"], mode)
            assert np.array_equal(vd, rx["want_vd"]) and np.array_equal(vd, vd0), (hex(mode), vd, rx["want_vd"])
            assert np.array_equal(st, want_st) and np.array_equal(st, st0), (hex(mode), [hex(x) for x in st], [hex(x) for x in want_st])
            assert np.array_equal(port, want_port), (hex(mode), port, want_port)
            assert np.array_equal(arena, want), (hex(mode), _first_diff(rx, arena, want))
            assert sorted(tab.collect().tolist()) == hit0 == rx["want_hit"]
            assert len(tab.collect()) == 0
        # an empty batch needs no port array's contents; a second context slot works the same
        st, vd, port = ctx.nat_flow_forward_frames(tab, arena, rx["offs"][:0], rx["lens"][:0])
        assert len(st) == len(vd) == len(port) == 0
        arena[:] = base
        st, vd, port = ctx.nat_flow_forward_frames(tab, arena, rx["offs"], rx["lens"], V.NAT_STRICT_JAVA | bit)
        assert np.array_equal(port, want_port) and np.array_equal(arena, want)
        tab.collect()
        # the refusals of nat_flow_frames, under the new name; the frames as they were
        arena[:] = base
        with pytest.raises(V.VpcsumError, match="vpcsum_ctx_nat_flow_forward_frames.*bad nat_mode"):
            ctx.nat_flow_forward_frames(tab, arena, rx["offs"], rx["lens"], 0x04)
        other = np.zeros(4096, np.uint8)
        with pytest.raises(V.VpcsumError, match="vpcsum_ctx_nat_flow_forward_frames.*must be registered"):
            ctx.nat_flow_forward_frames(tab, other, np.array([0], np.uint64), np.array([64], np.uint32))
        assert np.array_equal(arena, base)
    finally:
        ctx.unregister(arena)
        tab.close()
        ctx.close()


# ------------------------------------------------------------------------------------------
# 4. stream order
# ------------------------------------------------------------------------------------------
def test_set_fastpath_is_ordered_on_the_stream(V):
    """On one stream: lookup, set_fastpath (A: set, C: replaced, D: cleared), lookup -- the first
    lookup's records are those of the old table, the second's of the new one."""
    import torch
    rng = np.random.default_rng(25)
    a, c, d = (mk_key(V, sport=s) for s in (11, 13, 14))
    tab = V.FlowTable(8)
    s = torch.cuda.Stream()
    tab.update(add=mk_flows(V, [a, c, d], [mk_entry(V, rng) for _ in range(3)], (1, 3, 4)), stream=s)
    fc, fd, fa, fc2 = mk_fp(rng, 3), mk_fp(rng, 4), mk_fp(rng, 1), mk_fp(rng, 33)
    assert tab.set_fastpath(np.array([c, d], V.TUPLE_DTYPE), np.array([fc, fd], V.FASTPATH_DTYPE), stream=s) == 0
    tu = dev(np.array([a, c, d], V.TUPLE_DTYPE))
    out = [[torch.full((3 * w,), 0xAB, dtype=torch.uint8, device="cuda") for w in (48, 1, 16)] for _ in range(2)]
    torch.cuda.synchronize()
    tab.lookup(tu, 3, out[0][0], out[0][1], stream=s, fastpath=out[0][2])
    assert tab.set_fastpath(np.array([a, c, d], V.TUPLE_DTYPE), np.array([fa, fc2, mk_fp(rng, 0)], V.FASTPATH_DTYPE), stream=s) == 0
    tab.lookup(tu, 3, out[1][0], out[1][1], stream=s, fastpath=out[1][2])
    s.synchronize()
    assert list(host(out[0][1])) == [HIT] * 3 and list(host(out[1][1])) == [HIT] * 3
    assert host(out[0][0]).tobytes() == host(out[1][0]).tobytes()   # the entries did not change
    assert host(out[0][2]).tobytes() == ZERO_FP + fc.tobytes() + fd.tobytes()
    assert host(out[1][2]).tobytes() == fa.tobytes() + fc2.tobytes() + ZERO_FP
    tab.close()


# ------------------------------------------------------------------------------------------
# 5. PNI
# ------------------------------------------------------------------------------------------
def test_pni_flow_forward(V, orc, rx, tmp_path):
    """flowtabSetFastpath and natFlowForwardFrames from plain C++ through the C ABI
    (tests/cpp/pni_flow_forward.cpp) on six frames of the end-to-end batch -- forwarded TCP and UDP,
    a flow without a Fastpath, the SYN, the unknown flow, the TTL-1 frame --: the bytes, status,
    verdicts and ports it must find are the expectation of the end-to-end test."""
    pick = [rx["idx"][nm] for nm in ("tcp4", "vlan_udp4", "udp6_nofp", "syn", "unknown", "ttl1")]
    n = len(pick)
    arena = np.zeros(n * STRIDE, np.uint8)
    offs = np.array([i * STRIDE + HEADROOM for i in range(n)], np.uint64)
    lens = rx["lens"][pick].copy()
    desc = rx["desc"][pick].copy()
    for j, i in enumerate(pick):
        o = int(rx["offs"][i])
        arena[int(offs[j]):int(offs[j]) + int(lens[j])] = rx["base"][o:o + int(lens[j])]
        if desc[j]["l3_ver"]:
            desc[j]["l3_off"] = int(desc[j]["l3_off"]) - o + int(offs[j])
    want_vd, want_rw, want_fp = rx["want_vd"][pick], rx["want_rw"][pick], rx["want_fp"][pick]
    nat, want_st = NV.expect(orc, arena, desc, want_rw, 1)
    want, want_port = F.l2_forward(nat, offs, lens, want_vd, want_st, want_fp)
    assert list(want_vd) == [HIT, HIT, HIT, PUNT, MISS, HIT] and [bool(p) for p in want_port] == [True, True, False, False, False, False]
    flows = rx["flows"]
    assert len(flows) < 16                                  # the program's table holds 16 flows
    fkeys = [k for k in rx["keys"] if kb(k) in rx["fps"]] + [mk_key(V, sport=7777)]   # the last is in no table
    frecs = [rx["fps"].get(kb(k), F.mk_fp(b"\x02" * 6, b"\x04" * 6, 9)) for k in fkeys]
    missing = 1
    assert len(fkeys) < 16
    vf = tmp_path / "pni_flow_forward_vectors.bin"
    vf.write_bytes(struct.pack("<IIII", len(arena), len(flows), n, len(fkeys)) + arena.tobytes() + offs.tobytes() + lens.tobytes() +
                   flows.tobytes() + np.array(fkeys, V.TUPLE_DTYPE).tobytes() + np.array(frecs, V.FASTPATH_DTYPE).tobytes() +
                   struct.pack("<I", missing) + want.tobytes() + want_st.tobytes() + want_vd.tobytes() + want_port.tobytes())
    exe = tmp_path / "pni_flow_forward"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp", "pni_flow_forward.cpp"), "-L", os.path.join(REPO, "vproxy_amd"),
                           "-lvpcsum", "-Wl,-rpath," + os.path.join(REPO, "vproxy_amd"), "-o", str(exe)])
    r = subprocess.run([str(exe), str(vf)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "pni flow forward ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
