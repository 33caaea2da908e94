"""The NAT flow table on the GPU (vpcsum_flowtab_*, vpcsum_flow_lookup_async,
vpcsum_ctx_nat_flow_frames): the expected lookup is a Python dict over oracle.flow_tuple's 38 key
bytes, the expected frames the oracle's NAT (natvec.expect / tcprwvec.expected) with the dict's
entry, or an all-zero entry on MISS / PUNT."""
import json
import os
import struct
import subprocess

import numpy as np
import pytest

import hsumvec as H
import natvec as NV
import tcprwvec as T
from oracle import oracle as O
from pcaputil import read_pcap

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(REPO, "tests", "golden")
MISS, HIT, PUNT = 0, 1, 2
KEY = 38


@pytest.fixture(scope="module")
def V():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vproxy_amd import vpcsum
    vpcsum.lib()
    return vpcsum


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).pin_memory().cuda()


# ------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------
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


def changed(V, k, byte=None, xor=0x01, **fields):
    """A copy of tuple k with one byte flipped and / or fields set (an address field: (position, value))."""
    m = np.array([k], V.TUPLE_DTYPE)
    if byte is not None:
        m.view(np.uint8)[byte] ^= xor
    for f, v in fields.items():
        if f in ("src", "dst"):
            m[f][0, v[0]] = v[1]
        else:
            m[f] = v
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


def tuples_of(V, frames):
    """oracle.flow_tuple of each frame as TUPLE_DTYPE records."""
    out = np.zeros(len(frames), V.TUPLE_DTYPE)
    for i, f in enumerate(frames):
        t = O.flow_tuple(f)
        for k in ("src", "dst", "sport", "dport"):
            out[k][i] = np.frombuffer(t[k], np.uint8)
        out["l3_ver"][i], out["l4_proto"][i], out["tcp_flags"][i] = t["l3_ver"], t["l4_proto"], t["tcp_flags"]
    return out


def model_lookup(V, table: dict, tuples):
    """(verdicts, entries) of the dict {38 key bytes: entry} for TUPLE_DTYPE tuples."""
    vd = np.zeros(len(tuples), np.uint8)
    rw = np.zeros(len(tuples), V.NAT_DTYPE)
    for i, t in enumerate(tuples):
        e = table.get(kb(t)) if int(t["l3_ver"]) != 0 and int(t["l4_proto"]) in (6, 17) else None
        if e is None:
            continue
        if int(t["l4_proto"]) == 6 and int(t["tcp_flags"]) & 0x07:
            vd[i] = PUNT
        else:
            vd[i], rw[i] = HIT, e
    return vd, rw


def gpu_lookup(V, tab, tuples, stream=None):
    """(verdicts, entries) from the kernel; the outputs start as 0xAB so that every row must be written."""
    import torch
    n = len(tuples)
    rw = torch.full((max(n, 1) * 48,), 0xAB, dtype=torch.uint8, device="cuda")
    vd = torch.full((max(n, 1),), 0xAB, dtype=torch.uint8, device="cuda")
    tu = dev(tuples) if n else torch.zeros(40, dtype=torch.uint8, device="cuda")
    tab.lookup(tu, n, rw, vd, stream)
    torch.cuda.synchronize()
    return vd.cpu().numpy()[:n], rw.cpu().numpy()[:n * 48].view(V.NAT_DTYPE), (rw, vd)


def check_lookup(V, tab, table, tuples):
    want_vd, want_rw = model_lookup(V, table, tuples)
    vd, rw, _ = gpu_lookup(V, tab, tuples)
    bad = np.flatnonzero(vd != want_vd)
    assert not len(bad), [(int(i), int(vd[i]), int(want_vd[i])) for i in bad[:8]]
    assert rw.tobytes() == want_rw.tobytes(), int(np.flatnonzero(rw.view(np.uint8) != want_rw.view(np.uint8))[0]) // 48
    return vd, rw


def keys_by_home(V, slots, want: dict, **kw):
    """Keys (varying the source port) whose home slots -- from vpcsum_flow_hash -- are those of
    `want` {home: how many}."""
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


# ------------------------------------------------------------------------------------------
# 1. the smallest table
# ------------------------------------------------------------------------------------------
def test_smallest_table_shared_home_wrap_and_partial_keys(V):
    """8 slots, 4 flows: two keys share home slot 7, so the second wraps to slot 0 -- both asserted
    from vpcsum_flow_hash --, an IPv6 key and the IPv4 key with the same leading address bytes and
    ports sit side by side.  Every key hits with its own entry; each key with one byte changed, at
    every one of the 38 key positions, misses (a partial compare would hit)."""
    rng = np.random.default_rng(1)
    tab = V.FlowTable(4)
    assert tab.info() == {"slots": 8, "flows": 0, "max_probe": 0}
    a, b = keys_by_home(V, 8, {7: 2})
    k6 = mk_key(V, ver=6, proto=17, src=bytes(range(1, 17)), dst=bytes(range(101, 117)), sport=53, dport=5353)
    k4 = mk_key(V, ver=4, proto=17, src=bytes(range(1, 5)), dst=bytes(range(101, 105)), sport=53, dport=5353)
    keys = [a, b, k6, k4]
    homes = [V.flow_hash(k) & 7 for k in keys]
    assert homes[0] == homes[1] == 7          # two share a home slot, the last one: the chain wraps 7 -> 0
    entries = [mk_entry(V, rng) for _ in keys]
    tab.update(add=mk_flows(V, keys, entries, range(100, 104)))
    info = tab.info()
    assert info["flows"] == 4 and info["max_probe"] >= 1
    table = {kb(k): e for k, e in zip(keys, entries)}
    tuples = []
    for k in keys:
        tuples.append(k)
        tuples += [changed(V, k, byte=pos) for pos in range(KEY)]
    # the IPv4 key as version 6 (the IPv6 key cut to its first 4 address bytes), and the IPv6 key as version 4
    tuples += [changed(V, k4, l3_ver=6), changed(V, k6, l3_ver=4)]
    tuples = np.array(tuples, V.TUPLE_DTYPE)
    vd, rw = check_lookup(V, tab, table, tuples)
    per = KEY + 1
    for i in range(4):
        assert vd[i * per] == HIT and rw[i * per].tobytes() == entries[i].tobytes()
        assert not vd[i * per + 1:(i + 1) * per].any(), (i, np.flatnonzero(vd[i * per + 1:(i + 1) * per]))
    assert not vd[4 * per:].any()
    tab.close()


# ------------------------------------------------------------------------------------------
# 2. erase inside a chain
# ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [0, 1], ids=["erase_first", "erase_middle"])
def test_erase_inside_a_chain(V, first):
    """Three keys with one home slot (a chain of three): erase the first or the middle one, then one
    more; the others still hit with their own entries, the erased ones miss, and info() reports the
    flows and the max_probe the chain must have after the backward shift."""
    rng = np.random.default_rng(2)
    tab = V.FlowTable(4)
    keys = keys_by_home(V, 8, {6: 3})   # slots 6, 7 and, wrapped, 0
    entries = [mk_entry(V, rng) for _ in keys]
    tab.update(add=mk_flows(V, keys, entries, (1, 2, 3)))
    assert tab.info() == {"slots": 8, "flows": 3, "max_probe": 2}
    table = {kb(k): e for k, e in zip(keys, entries)}
    tuples = np.array(keys, V.TUPLE_DTYPE)
    vd, _ = check_lookup(V, tab, table, tuples)
    assert list(vd) == [HIT] * 3
    tab.update(delete=np.array([keys[first]], V.TUPLE_DTYPE))
    del table[kb(keys[first])]
    vd, _ = check_lookup(V, tab, table, tuples)
    assert list(vd) == [MISS if i == first else HIT for i in range(3)]
    assert tab.info() == {"slots": 8, "flows": 2, "max_probe": 1}   # the two left lie at their home and next to it
    second = 1 - first   # then the other of the two
    tab.update(delete=np.array([keys[second], keys[first]], V.TUPLE_DTYPE))   # a key not there is no error
    del table[kb(keys[second])]
    vd, _ = check_lookup(V, tab, table, tuples)
    assert list(vd) == [MISS, MISS, HIT]
    assert tab.info() == {"slots": 8, "flows": 1, "max_probe": 0}
    tab.close()


# ------------------------------------------------------------------------------------------
# 3. batch edges
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def table64(V):
    """A 64-flow table (128 slots, full) of IPv4 / IPv6, TCP / UDP keys, and as many keys not in it."""
    rng = np.random.default_rng(3)
    keys, absent = [], []
    for i in range(128):
        v6 = i % 3 == 0
        k = mk_key(V, ver=6 if v6 else 4, proto=6 if i % 2 else 17, src=bytes(rng.integers(0, 256, 16 if v6 else 4, dtype=np.uint8)),
                   dst=bytes(rng.integers(0, 256, 16 if v6 else 4, dtype=np.uint8)), sport=int(rng.integers(1, 65536)),
                   dport=int(rng.integers(1, 65536)))
        (keys if i < 64 else absent).append(k)
    entries = [mk_entry(V, rng) for _ in keys]
    tab = V.FlowTable(64)
    tab.update(add=mk_flows(V, keys, entries, range(1000, 1064)))
    assert tab.info()["flows"] == 64 and tab.info()["slots"] == 128
    yield tab, keys, absent, {kb(k): e for k, e in zip(keys, entries)}
    tab.close()


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 63, 64, 65, 257])
def test_batch_edges(V, table64, n):
    """Batches around the team (8 packets per wave instruction), wave and workgroup sizes: all hits,
    all misses, alternating; the entry of a MISS row is 48 zero bytes, and nothing is written past
    row n."""
    tab, keys, absent, table = table64
    for kind in ("hit", "miss", "alternate"):
        tuples = np.array([(keys if kind == "hit" or (kind == "alternate" and i % 2 == 0) else absent)[(i * 7) % 64]
                           for i in range(n)], V.TUPLE_DTYPE)
        import torch
        big_rw = torch.full(((n + 2) * 48,), 0xCD, dtype=torch.uint8, device="cuda")
        big_vd = torch.full((n + 2,), 0xCD, dtype=torch.uint8, device="cuda")
        tu = dev(tuples) if n else torch.zeros(40, dtype=torch.uint8, device="cuda")
        tab.lookup(tu, n, big_rw, big_vd)
        torch.cuda.synchronize()
        vd, rw = big_vd.cpu().numpy(), big_rw.cpu().numpy()
        assert (vd[n:] == 0xCD).all() and (rw[n * 48:] == 0xCD).all(), kind
        want_vd, want_rw = model_lookup(V, table, tuples)
        assert np.array_equal(vd[:n], want_vd) and rw[:n * 48].tobytes() == want_rw.tobytes(), kind
        if n:
            assert {"hit": (want_vd == HIT).all(), "miss": (want_vd == MISS).all(),
                    "alternate": (want_vd[::2] == HIT).all() and (want_vd[1::2] == MISS).all()}[kind]
            assert not rw[:n * 48].reshape(n, 48)[want_vd == MISS].any()


# ------------------------------------------------------------------------------------------
# 4. the verdict rule
# ------------------------------------------------------------------------------------------
def test_verdict_rule(V, table64):
    """TCP tuples of a known flow with each of the 64 tcp_flags values: PUNT iff FIN | SYN | RST;
    UDP of a known flow: HIT whatever the flags byte; ICMP / ICMPv6 tuples with a known flow's
    addresses and ports, and the all-zero tuple of a refused frame: MISS."""
    tab, keys, _, table = table64
    tcp = next(k for k in keys if k["l4_proto"] == 6)
    udp = next(k for k in keys if k["l4_proto"] == 17)
    tuples = []
    for fl in range(64):
        tuples += [changed(V, k, tcp_flags=fl) for k in (tcp, udp)]
    for proto in (1, 58, 0, 47):
        tuples += [changed(V, k, l4_proto=proto) for k in (tcp, udp)]
    tuples += [np.zeros(1, V.TUPLE_DTYPE)[0], changed(V, tcp, l3_ver=0)]
    tuples = np.array(tuples, V.TUPLE_DTYPE)
    vd, rw = check_lookup(V, tab, table, tuples)
    for fl in range(64):
        assert vd[2 * fl] == (PUNT if fl & 7 else HIT), fl
        assert vd[2 * fl + 1] == HIT, fl
        assert rw[2 * fl + 1].tobytes() == table[kb(udp)].tobytes()
    assert not vd[128:].any()


# ------------------------------------------------------------------------------------------
# 5. stream order
# ------------------------------------------------------------------------------------------
def test_update_is_ordered_on_the_stream(V):
    """On one stream: lookup, update (erase A, insert B, replace C's entry), lookup -- the first
    lookup's results are those of the old table, the second's of the new one."""
    import torch
    rng = np.random.default_rng(5)
    a, b, c = (mk_key(V, sport=s) for s in (11, 12, 13))
    ea, eb, ec, ec2 = (mk_entry(V, rng) for _ in range(4))
    tab = V.FlowTable(8)
    s = torch.cuda.Stream()
    tab.update(add=mk_flows(V, [a, c], [ea, ec], (1, 3)), stream=s)
    tuples = np.array([a, b, c], V.TUPLE_DTYPE)
    tu = dev(tuples)
    torch.cuda.synchronize()
    out = [(torch.full((3 * 48,), 0xAB, dtype=torch.uint8, device="cuda"), torch.full((3,), 0xAB, dtype=torch.uint8, device="cuda"))
           for _ in range(2)]
    torch.cuda.synchronize()
    tab.lookup(tu, 3, out[0][0], out[0][1], stream=s)
    tab.update(delete=np.array([a], V.TUPLE_DTYPE), add=mk_flows(V, [b, c], [eb, ec2], (2, 33)), stream=s)
    tab.lookup(tu, 3, out[1][0], out[1][1], stream=s)
    s.synchronize()
    zero = bytes(48)
    assert list(out[0][1].cpu().numpy()) == [HIT, MISS, HIT]
    assert out[0][0].cpu().numpy().tobytes() == ea.tobytes() + zero + ec.tobytes()
    assert list(out[1][1].cpu().numpy()) == [MISS, HIT, HIT]
    assert out[1][0].cpu().numpy().tobytes() == zero + eb.tobytes() + ec2.tobytes()
    assert tab.info()["flows"] == 2
    tab.close()


# ------------------------------------------------------------------------------------------
# 6. touched
# ------------------------------------------------------------------------------------------
def test_collect_returns_the_hit_flows_once(V):
    """A batch hitting A and B (B twice), punting C and missing D: collect returns exactly the
    cookies of A and B, a second collect nothing.  cap too small: the count, nothing cleared.  A flow
    hit and then erased is not returned, nor is the flow inserted afterwards that takes over its id,
    until it is hit itself."""
    rng = np.random.default_rng(6)
    a, b, d, e = (mk_key(V, proto=17, sport=s) for s in (21, 22, 24, 25))
    c = mk_key(V, proto=6, sport=23)
    tab = V.FlowTable(4)
    tab.update(add=mk_flows(V, [a, b, c], [mk_entry(V, rng) for _ in range(3)], (0xA, 0xB, 0xC)))
    assert len(tab.collect()) == 0
    syn = changed(V, c, tcp_flags=0x02)
    vd, _, _ = gpu_lookup(V, tab, np.array([a, b, syn, d, b], V.TUPLE_DTYPE))
    assert list(vd) == [HIT, HIT, PUNT, MISS, HIT]
    assert tab.collect(cap=1) == (2, None)          # no room: nothing cleared
    assert tab.collect(cap=0) == (2, None)
    n, got = tab.collect(cap=2)
    assert n == 2 and sorted(got.tolist()) == [0xA, 0xB]
    assert len(tab.collect()) == 0
    # hit, then erased: gone with its mark; the id's next owner is not reported for it
    vd, _, _ = gpu_lookup(V, tab, np.array([a, c], V.TUPLE_DTYPE))
    assert list(vd) == [HIT, HIT]
    tab.update(delete=np.array([a], V.TUPLE_DTYPE))
    tab.update(add=mk_flows(V, [e], [mk_entry(V, rng)], (0xE,)))   # the table held 3 of 4: e takes a's id or a new one
    assert sorted(tab.collect().tolist()) == [0xC]
    tab.update(delete=np.array([c], V.TUPLE_DTYPE), add=mk_flows(V, [d], [mk_entry(V, rng)], (0xD,)))
    vd, _, _ = gpu_lookup(V, tab, np.array([c], V.TUPLE_DTYPE))
    assert list(vd) == [MISS] and len(tab.collect()) == 0
    # a full table: every id has been used, so the next flows take recycled ones
    tab.update(delete=np.array([b, d, e], V.TUPLE_DTYPE))
    assert tab.info()["flows"] == 0
    four = [mk_key(V, proto=17, sport=s) for s in (31, 32, 33, 34)]
    tab.update(add=mk_flows(V, four, [mk_entry(V, rng) for _ in four], (31, 32, 33, 34)))
    gpu_lookup(V, tab, np.array(four, V.TUPLE_DTYPE))
    tab.update(delete=np.array(four[:2], V.TUPLE_DTYPE))
    tab.update(add=mk_flows(V, [a, b], [mk_entry(V, rng) for _ in range(2)], (0xA, 0xB)))   # the two freed ids
    assert sorted(tab.collect().tolist()) == [33, 34]
    vd, _, _ = gpu_lookup(V, tab, np.array([a], V.TUPLE_DTYPE))
    assert list(vd) == [HIT] and tab.collect().tolist() == [0xA]
    tab.close()


# ------------------------------------------------------------------------------------------
# 7. end to end
# ------------------------------------------------------------------------------------------
STRIDE, HEADROOM = 2048, 384
_KEEP = []


def rx_frames(orc):
    """The batch's frames: the KAT Ethernet frames, the Ethernet pcap fixture's, 120 received frames
    with correct sums (IPv4 options, an IPv6 extension header, 802.1Q), two crafted ones (a TTL of 1,
    an ACK without options), and 1,000 fuzzed packets in Ethernet frames -- every 9th behind an
    802.1Q tag, every 31st with a non-IP EtherType, every 37th cut short; those above the chunk's
    room are cut to it (truncated: refused)."""
    rng = np.random.default_rng(7)
    kats = json.load(open(os.path.join(GOLD, "kat.json")))["kats"]
    frames = [bytes.fromhex(k["hex"]) for k in kats if k["layer"] == "ether"]
    lt, pkts = read_pcap(os.path.join(GOLD, "pcap", "cap-ether.pcap"))
    assert lt == 1
    frames += pkts
    frames += [f["frame"] for f in H.received(17, 120)]
    # crafted: UDP over IPv4 with TTL 1; TCP ACK over IPv4 without options
    udp = bytearray(H.with_sums(H.ether(rng, H._l3(rng, 4, H._udp(rng, 40), 17), 4, False)))
    udp[14 + 8] = 1
    special = {"ttl1": len(frames)}
    frames.append(H.with_sums(bytes(udp)))
    seg = H._tcp(rng, 30, False, None, 0)
    seg[13] = 0x10
    special["ack"] = len(frames)
    frames.append(H.with_sums(H.ether(rng, H._l3(rng, 4, seg, 6), 4, False)))
    special["ack2"] = len(frames)
    seg = H._tcp(rng, 12, False, None, 0)
    seg[13] = 0x18
    frames.append(H.with_sums(H.ether(rng, H._l3(rng, 6, seg, 6), 6, False)))
    a, d = orc.synth(1000, 9216, 14, O.SYNTH_FUZZ, O.SEED, 777)
    for i, r in enumerate(d):
        l3 = bytes(a[int(r["l3_off"]):int(r["l3_off"]) + int(r["l3_len"])])
        et = b"\x08\x00" if r["l3_ver"] == 4 else b"\x86\xdd"
        if i % 31 == 5:
            et = b"\x08\x06"
        f = bytes(rng.integers(0, 256, 12, dtype=np.uint8)) + (b"\x81\x00\x00\x07" if i % 9 == 4 else b"") + et + l3
        if i % 37 == 11:
            f = f[:int(rng.integers(1, 60))]
        frames.append(f[:STRIDE - HEADROOM])
    return frames, special


@pytest.fixture(scope="module")
def rx(V, orc):
    frames, special = rx_frames(orc)
    n = len(frames)
    raw = np.zeros(n * STRIDE + 8192, np.uint8)
    # page-locked and released several times below: kept for the life of the process, so that no
    # later test's array lands on addresses HIP has held as registered
    _KEEP.append(raw)
    skip = (-raw.ctypes.data) % 4096
    arena = raw[skip:skip + n * STRIDE + 4096]   # page-aligned, umem geometry: 2,048-B chunks, frame at +384
    assert arena.ctypes.data % 4096 == 0
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
    # the table: every other distinct TCP / UDP key, and the crafted frames' keys
    rng = np.random.default_rng(8)
    distinct = {}
    for t in tuples:
        if int(t["l3_ver"]) and int(t["l4_proto"]) in (6, 17):
            distinct.setdefault(kb(t), t)
    chosen = dict(list(distinct.items())[::2])
    for i in special.values():
        chosen[kb(tuples[i])] = tuples[i]
    table = {k: mk_entry(V, rng, mask=int(rng.integers(1, 64))) for k in chosen}
    sk = {name: kb(tuples[i]) for name, i in special.items()}
    table[sk["ttl1"]] = mk_entry(V, rng, mask=O.NAT_SRC | O.NAT_DEC_TTL)
    table[sk["ack"]] = mk_entry(V, rng, mask=O.NAT_SRC | O.NAT_DPORT)
    table[sk["ack2"]] = mk_entry(V, rng, mask=O.NAT_DST | O.NAT_SPORT)
    T.fill(table[sk["ack"]], T.SEQ_ADD | T.CLAMP_MSS, max_mss=1200, addend=-77)    # no SYN: no clamp
    T.fill(table[sk["ack2"]], T.SET_FLAGS | T.CLAMP_MSS, flags=0x12, max_mss=1200)  # a SYN-ACK built: no MSS option
    flows = mk_flows(V, [changed(V, t, tcp_flags=0) for t in chosen.values()], [table[k] for k in chosen], range(1, len(chosen) + 1))
    cookies = {k: c for k, c in zip(chosen, range(1, len(chosen) + 1))}
    want_vd, want_rw = model_lookup(V, table, tuples)
    counts = {v: int((want_vd == v).sum()) for v in (MISS, HIT, PUNT)}
    assert min(counts.values()) >= 20 and (desc["l3_ver"] == 0).sum() >= 40, counts
    assert len(flows) <= 1024 and n <= 4096
    want_hit = sorted({cookies[kb(t)] for t, v in zip(tuples, want_vd) if v == HIT})
    return dict(frames=frames, special=special, arena=arena, base=arena.copy(), offs=offs, lens=lens, desc=desc, flows=flows,
                want_vd=want_vd, want_rw=want_rw, want_hit=want_hit, n=n)


def _first_frame_diff(rx, got, want):
    k = int(np.flatnonzero(got != want)[0])
    i = k // STRIDE
    return f"byte {k}: frame {i} +{k - int(rx['offs'][i])} (verdict {rx['want_vd'][i]}, desc {rx['desc'][i]}): {got[k]:#x} != {want[k]:#x}"


@pytest.mark.parametrize("tcp", [False, True], ids=["nat", "tcp_rewrites"])
def test_nat_flow_frames_end_to_end(V, orc, rx, tcp):
    """Context.nat_flow_frames on an RX batch in a registered page-aligned arena at umem geometry,
    the table holding half of the frames' TCP / UDP flows.  Strict Java: every byte of the arena,
    every status and every verdict equals the oracle's NAT with the dict's entries (any input: the
    CHECKSUM_PARTIAL pcap frames too).  RFC 1624: the same on the frames whose stored sums the
    oracle verifies.  Frames with verdict MISS / PUNT or status S_BAD_DESC are untouched; the TTL-1
    frame answers S_BAD_DESC | S_TTL_EXPIRED; with VPCSUM_NAT_TCP_REWRITES the two TCP entries match
    tests/tcprwvec.py (sequence addend; a SYN-ACK built without an MSS option: S_MSS_ABSENT)."""
    n, arena, base, desc, sp = rx["n"], rx["arena"], rx["base"], rx["desc"], rx["special"]
    bit = V.NAT_TCP_REWRITES if tcp else 0
    if tcp:
        want, want_st = T.expected(orc, base, desc, rx["want_rw"])
    else:
        want, want_st = NV.expect(orc, base, desc, rx["want_rw"], 1)
    assert want_st[sp["ttl1"]] == O.S_BAD_DESC | O.S_TTL_EXPIRED and rx["want_vd"][sp["ttl1"]] == HIT
    assert rx["want_vd"][sp["ack"]] == HIT and rx["want_vd"][sp["ack2"]] == HIT
    if tcp:
        plain, _ = NV.expect(orc, base, desc, rx["want_rw"], 1)
        for name in ("ack", "ack2"):   # the TCP rewrites changed these frames beyond the plain NAT
            o = int(rx["offs"][sp[name]])
            assert not np.array_equal(want[o:o + STRIDE - HEADROOM], plain[o:o + STRIDE - HEADROOM]), name
        assert want_st[sp["ack"]] == O.S_DONE and want_st[sp["ack2"]] == O.S_DONE | T.S_MSS_ABSENT
    # untouched: MISS / PUNT verdicts and refused frames, in the expectation itself
    quiet = (rx["want_vd"] != HIT) | ((want_st & O.S_BAD_DESC) != 0)
    for i in np.flatnonzero(quiet):
        o = int(rx["offs"][i])
        assert np.array_equal(want[o:o + int(rx["lens"][i])], base[o:o + int(rx["lens"][i])]), i
    assert (want != base).any()
    # the frames whose stored sums verify (RFC 1624's premise), or that nothing is written to
    _, vst = orc.process(base, desc, O.MODE_VERIFY)
    sums_ok = np.array([(not d["flags"] & O.F_IP or s & O.S_IP_OK) and (not d["flags"] & O.F_L4 or s & O.S_L4_OK)
                        for d, s in zip(desc, vst)], bool)
    exact = quiet | sums_ok
    assert (exact & ~quiet).sum() >= 10
    ctx = V.Context(0, max_arena=1 << 16, max_pkts=n)
    tab = V.FlowTable(1024)
    tab.update(add=rx["flows"])
    ctx.register(arena)
    try:
        for mode in (V.NAT_STRICT_JAVA | bit, V.NAT_RFC1624 | bit):
            arena[:] = base
            st, vd = ctx.nat_flow_frames(tab, arena, rx["offs"], rx["lens"], mode)
            assert np.array_equal(vd, rx["want_vd"]), (hex(mode), np.flatnonzero(vd != rx["want_vd"])[:8])
            bad = np.flatnonzero(st != want_st)
            assert not len(bad), (hex(mode), [(int(i), hex(st[i]), hex(want_st[i])) for i in bad[:8]])
            if mode & V.NAT_STRICT_JAVA:
                assert np.array_equal(arena, want), (hex(mode), _first_frame_diff(rx, arena, want))
            else:
                got = arena.reshape(-1)[:n * STRIDE].reshape(n, STRIDE)
                w = want[:n * STRIDE].reshape(n, STRIDE)
                badf = np.flatnonzero((got != w).any(axis=1) & exact)
                assert not len(badf), (hex(mode), int(badf[0]), rx["desc"][badf[0]], int(np.flatnonzero(got[badf[0]] != w[badf[0]])[0]))
                assert np.array_equal(arena[n * STRIDE:], base[n * STRIDE:])
        # the flows hit (in either run), each once: the host's resetTimer list
        assert sorted(tab.collect().tolist()) == rx["want_hit"]
        assert len(tab.collect()) == 0
    finally:
        ctx.unregister(arena)
        tab.close()
        ctx.close()


# ------------------------------------------------------------------------------------------
# 8. refusals
# ------------------------------------------------------------------------------------------
def test_refusals_change_nothing(V, orc, rx):
    """An unregistered arena, more frames than max_pkts, a bad nat_mode: refused with a message, the
    frames as they were.  An update with one malformed flow among good ones -- each kind of §1 --
    or that would overfill the table: refused with a message, the table as it was."""
    n = 64
    arena, base, offs, lens = rx["arena"], rx["base"], rx["offs"][:n], rx["lens"][:n]
    arena[:] = base
    rng = np.random.default_rng(9)
    tab = V.FlowTable(4)
    good = [mk_key(V, sport=s) for s in (1, 2, 3)]
    entries = [mk_entry(V, rng) for _ in good]
    tab.update(add=mk_flows(V, good, entries, (1, 2, 3)))
    table = {kb(k): e for k, e in zip(good, entries)}
    ctx = V.Context(0, max_arena=1 << 16, max_pkts=n)
    with pytest.raises(V.VpcsumError, match="vpcsum_ctx_nat_flow_frames.*must be registered"):
        ctx.nat_flow_frames(tab, arena, offs, lens)
    ctx.register(arena)
    with pytest.raises(V.VpcsumError, match="vpcsum_ctx_nat_flow_frames.*65 frames > capacity 64"):
        ctx.nat_flow_frames(tab, arena, rx["offs"][:65], rx["lens"][:65])
    with pytest.raises(V.VpcsumError, match="bad nat_mode"):
        ctx.nat_flow_frames(tab, arena, offs, lens, 0x04)
    ctx.unregister(arena)
    ctx.close()
    assert np.array_equal(arena, base)
    new = mk_key(V, sport=9)
    bad = []
    for f, v in (("l4_proto", 1), ("l4_proto", 58), ("l3_ver", 0), ("l3_ver", 5), ("tcp_flags", 0x10), ("rsv", 1)):
        bad.append(changed(V, mk_key(V, sport=10), **{f: v}))
    for f in ("src", "dst"):
        for pos in (4, 15):
            bad.append(changed(V, mk_key(V, sport=10), **{f: (pos, 1)}))
    info = tab.info()
    probe = np.array(good + [new], V.TUPLE_DTYPE)
    for k in bad:
        with pytest.raises(V.VpcsumError, match="vpcsum_flowtab_update: flow 1: "):
            tab.update(delete=np.array([good[0]], V.TUPLE_DTYPE), add=mk_flows(V, [new, k], [entries[0]] * 2, (8, 9)))
    with pytest.raises(V.VpcsumError, match="the table is full: 5 flows > max_flows 4"):
        tab.update(add=mk_flows(V, [new, mk_key(V, sport=11)], [entries[0]] * 2, (8, 9)))
    assert tab.info() == info
    vd, _ = check_lookup(V, tab, table, probe)
    assert list(vd) == [HIT, HIT, HIT, MISS]
    # erase one and add two: fits
    tab.update(delete=np.array([good[0]], V.TUPLE_DTYPE), add=mk_flows(V, [new, mk_key(V, sport=11)], [entries[0]] * 2, (8, 9)))
    assert tab.info()["flows"] == 4
    tab.close()


def test_refuses_a_table_of_another_device(V, rx):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible")
    arena, base = rx["arena"], rx["base"]
    arena[:] = base
    tab = V.FlowTable(4, device=1)
    ctx = V.Context(0, max_arena=1 << 16, max_pkts=8)
    ctx.register(arena)
    with pytest.raises(V.VpcsumError, match="the flow table lives on device 1, the context on device 0"):
        ctx.nat_flow_frames(tab, arena, rx["offs"][:8], rx["lens"][:8])
    ctx.unregister(arena)
    ctx.close()
    tab.close()
    assert np.array_equal(arena, base)


# ------------------------------------------------------------------------------------------
# 9. PNI
# ------------------------------------------------------------------------------------------
def test_pni_flow(V, orc, tmp_path):
    """flowtabCreate -> flowtabUpdate -> natFlowFrames -> waitFor -> flowtabCollect -> flowtabClose
    from plain C++ (tests/cpp/pni_flow.cpp, built and run like pni_nat_tcp.cpp) on three frames: a
    hit, a punt (the flow's SYN) and a miss; the bytes, status, verdicts and cookie it must find come
    from here, computed with the oracle."""
    rng = np.random.default_rng(10)
    fs = []
    for flags, sport in ((0x10, 4000), (0x02, 4001), (0x10, 4002)):
        seg = H._tcp(rng, 24, False, None, 0)
        seg[0:2] = sport.to_bytes(2, "big")
        seg[13] = flags
        fs.append(H.with_sums(H.ether(rng, H._l3(rng, 4, seg, 6), 4, False)))
    n = 3
    arena = np.zeros(n * STRIDE, np.uint8)
    offs = np.array([i * STRIDE + HEADROOM for i in range(n)], np.uint64)
    lens = np.array([len(f) for f in fs], np.uint32)
    tuples = tuples_of(V, fs)
    desc = np.zeros(n, O.DESC_DTYPE)
    for i, f in enumerate(fs):
        arena[int(offs[i]):int(offs[i]) + len(f)] = np.frombuffer(f, np.uint8)
        info, _ = O.parse_ether(f)
        desc[i] = (int(offs[i]) + info.l3_off, info.l3_len, info.l4_off, info.ver, info.proto, O.desc_flags_for(info), 0)
    keys = [changed(V, tuples[0], tcp_flags=0), changed(V, tuples[1], tcp_flags=0)]
    entries = [mk_entry(V, rng, mask=0x0f), mk_entry(V, rng, mask=0x0f)]
    flows = mk_flows(V, keys, entries, (0x1111, 0x2222))
    want_vd, want_rw = model_lookup(V, {kb(k): e for k, e in zip(keys, entries)}, tuples)
    assert list(want_vd) == [HIT, PUNT, MISS]
    want, want_st = NV.expect(orc, arena, desc, want_rw, 1)
    assert list(want_st) == [O.S_DONE] * 3 and (want != arena).any()
    vf = tmp_path / "pni_flow_vectors.bin"
    vf.write_bytes(struct.pack("<II", len(arena), len(flows)) + arena.tobytes() + offs.tobytes() + lens.tobytes() +
                   flows.tobytes() + want.tobytes() + want_st.tobytes() + want_vd.tobytes() + struct.pack("<Q", 0x1111))
    exe = tmp_path / "pni_flow"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp", "pni_flow.cpp"), "-L", os.path.join(REPO, "vproxy_amd"),
                           "-lvpcsum", "-Wl,-rpath," + os.path.join(REPO, "vproxy_amd"), "-o", str(exe)])
    r = subprocess.run([str(exe), str(vf)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "pni flow ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
