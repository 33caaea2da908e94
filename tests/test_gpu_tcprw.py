"""TCP-header rewrites on the GPU NAT path (VPCSUM_NAT_TCP entries under VPCSUM_NAT_TCP_REWRITES):
sequence addend, flags and MSS clamp, byte-equal to the reference's setters and recompute
(tests/tcprwvec.py), through vpcsum_nat_async, the context and group submits and the PNI entry."""
import os
import struct
import subprocess

import numpy as np
import pytest

import tcprwvec as T
from oracle import oracle as O

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def V():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vproxy_amd import vpcsum
    vpcsum.lib()
    return vpcsum


@pytest.fixture(scope="module")
def vecs(orc):
    return T.crafted(orc)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().cuda()


def gpu_nat(V, arena_np, desc, rw, mode):
    import torch
    arena = dev(arena_np.copy())
    st = torch.zeros(len(desc), dtype=torch.uint8, device="cuda")
    V.nat(arena, V.desc_to_tensor(desc), dev(rw.view(np.uint8)), len(desc), st, mode)
    torch.cuda.synchronize()
    return arena.cpu().numpy(), st.cpu().numpy()


def modes(V):
    return (V.NAT_RFC1624 | V.NAT_TCP_REWRITES, V.NAT_STRICT_JAVA | V.NAT_TCP_REWRITES,
            V.NAT_RFC1624 | V.NAT_TCP_REWRITES | 0x100, V.NAT_STRICT_JAVA | V.NAT_TCP_REWRITES | 0x100)


def _first_diff(got, want, desc, vecs=None):
    k = int(np.flatnonzero(got != want)[0])
    for i, d in enumerate(desc):
        if int(d["l3_off"]) <= k < int(d["l3_off"]) + int(d["l3_len"]):
            return f"byte {k} (packet {i}{' ' + vecs[i]['name'] if vecs else ''}, L3+{k - int(d['l3_off'])}, " \
                   f"L4+{k - int(d['l3_off']) - int(d['l4_off'])}): {got[k]:#x} != {want[k]:#x}"
    return f"byte {k} outside every packet: {got[k]:#x} != {want[k]:#x}"


@pytest.mark.parametrize("pad", [0, 1, 2, 15, None], ids=["pad0", "pad1", "pad2", "pad15", "packed"])
def test_tcprw_crafted(V, orc, vecs, pad):
    """The crafted vectors (tcprwvec.crafted: option positions, values against maxMss, malformed
    options, flag / protocol interplay, sequence wraps, sums of 0x0000, headers beyond the wide
    window, refused packets) at one L3 padding, or packed back to back with gaps of 0..3 bytes:
    every byte of the arena and every status equal the reference's, in both modes, wide and byte
    kernels of the first pass."""
    arena, desc, rw = T.pack(vecs, pad)
    want, want_st = T.expected(orc, arena, desc, rw)
    by = {v["name"]: i for i, v in enumerate(vecs)}
    # the refused ones: untouched, status as without the TCP ops
    assert want_st[by["ttl_expired"]] == O.S_BAD_DESC | O.S_TTL_EXPIRED and want_st[by["outside_arena"]] == O.S_BAD_DESC
    o = int(desc[by["ttl_expired"]]["l3_off"])
    assert want[o:o + len(vecs[by["ttl_expired"]]["l3"])].tobytes() == vecs[by["ttl_expired"]]["l3"]
    assert [v["name"] for v, s in zip(vecs, want_st) if s & T.S_MSS_ABSENT] == [v["name"] for v in vecs if v["absent"]]
    for mode in modes(V):
        got, st = gpu_nat(V, arena, desc, rw, mode)
        bad = np.flatnonzero(st != want_st)
        assert not len(bad), (hex(mode), [(vecs[i]["name"], hex(st[i]), hex(want_st[i])) for i in bad])
        assert np.array_equal(got, want), (hex(mode), _first_diff(got, want, desc, vecs))


def _field_mask(size, desc, only):
    """True on the L4 checksum fields of the packets `only` marks, over `size` arena bytes."""
    m = np.zeros(size, bool)
    for d, k in zip(desc, only):
        if k and int(d["l4_proto"]) in O.L4_FIELD:
            f = int(d["l3_off"]) + int(d["l4_off"]) + O.L4_FIELD[int(d["l4_proto"])]
            m[f:f + 2] = True
    return m


def _assert_differs_only(got, want, allowed, desc, what):
    stray = (got != want) & ~allowed
    assert not stray.any(), (what, _first_diff(np.where(stray, got, want), want, desc))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_tcprw_batch(V, orc, n):
    """n received frames (hsumvec.received: SYNs with MSS above / below maxMss and without the
    option, other TCP, UDP; IPv4 options, IPv6 extension headers, 802.1Q), every TCP entry with
    random ops next to random NAT bits.  Strict mode: bytes and status equal the reference's.
    RFC 1624: the same, except the L4 sum field of a frame whose incoming sum was wrong.  Then with
    30% of the frames corrupted: strict still equal, RFC 1624 differs on corrupted frames only."""
    for corrupt in (0.0, 0.3):
        arena, desc, rw, bad = T.received_batch(n, corrupt=corrupt)
        want, want_st = T.expected(orc, arena, desc, rw)
        got, st = gpu_nat(V, arena, desc, rw, V.NAT_STRICT_JAVA | V.NAT_TCP_REWRITES)
        assert np.array_equal(st, want_st), corrupt
        assert np.array_equal(got, want), (corrupt, _first_diff(got, want, desc))
        got, st = gpu_nat(V, arena, desc, rw, V.NAT_RFC1624 | V.NAT_TCP_REWRITES)
        assert np.array_equal(st, want_st), corrupt
        _assert_differs_only(got, want, _field_mask(len(arena), desc, bad), desc, corrupt)
        if n == 257 and corrupt:
            assert (got != want).any()   # and there it does differ: the incoming sum was wrong


def test_tcprw_off_by_default(V, orc, vecs):
    """Without the mode bit the mask bit and rsv are ignored: the same entries give orc.nat_java's
    bytes and status (RFC 1624: but for the sum field of a frame that came in with a wrong sum)."""
    ra, rd, rrw, bad = T.received_batch(257)
    for arena, desc, rw, wrong in ((*T.pack(vecs, 2), np.zeros(len(vecs), bool)), (ra, rd, rrw, bad)):
        want = arena.copy()
        want_st = orc.nat_java(want, desc, rw)
        for mode in (V.NAT_RFC1624, V.NAT_STRICT_JAVA):
            got, st = gpu_nat(V, arena, desc, rw, mode)
            assert np.array_equal(st, want_st) and not (st & T.S_MSS_ABSENT).any(), mode
            allowed = _field_mask(len(arena), desc, wrong if mode == V.NAT_RFC1624 else np.zeros(len(desc), bool))
            _assert_differs_only(got, want, allowed, desc, mode)


def test_tcprw_refusals(V, orc, vecs):
    """The mode bit with the 16-byte entry formats, or without a status buffer, is refused with a
    message naming the reason; nothing is written."""
    import torch
    arena, desc, rw = T.pack(vecs[:4], 0)
    a = dev(arena)
    d = V.desc_to_tensor(desc)
    st = torch.zeros(len(desc), dtype=torch.uint8, device="cuda")
    r4 = dev(np.zeros(len(desc), O.NAT4_DTYPE).view(np.uint8))
    with pytest.raises(V.VpcsumError, match="vpcsum_nat4_async.*48-byte vpcsum_nat_t entries only"):
        V.nat4(a, d, r4, len(desc), st, V.NAT_TCP_REWRITES)
    rec = np.zeros(len(desc), V.NAT4R_DTYPE)
    rec["desc"] = desc
    with pytest.raises(V.VpcsumError, match="vpcsum_nat4r_async.*48-byte vpcsum_nat_t entries only"):
        V.nat4r(a, dev(rec.view(np.uint8)), len(desc), st, V.NAT_TCP_REWRITES)
    for mode in (V.NAT_TCP_REWRITES, V.NAT_TCP_REWRITES | V.NAT_STRICT_JAVA):
        with pytest.raises(V.VpcsumError, match="needs a status buffer"):
            V.nat(a, d, dev(rw.view(np.uint8)), len(desc), None, mode)
    with pytest.raises(V.VpcsumError, match="bad nat_mode"):
        V.nat(a, d, dev(rw.view(np.uint8)), len(desc), st, 0x04)
    torch.cuda.synchronize()
    assert np.array_equal(a.cpu().numpy(), arena)
    # the host submits: no status bytes, no way to see S_MSS_ABSENT
    host = arena.copy()
    ctx = V.Context(0, max_arena=1 << 16, max_pkts=16)
    grp = V.Group(devices=(0, 0), max_arena=1 << 16, max_pkts=16)
    with pytest.raises(V.VpcsumError, match="vpcsum_ctx_nat_submit.*needs a status buffer"):
        ctx.nat_submit(host, desc, rw, None, V.NAT_TCP_REWRITES)
    with pytest.raises(V.VpcsumError, match="needs a status buffer"):
        grp.nat_submit(host, desc, rw, None, V.NAT_TCP_REWRITES)
    with pytest.raises(V.VpcsumError, match="bad nat_mode"):
        ctx.nat_submit(host, desc, rw, np.zeros(len(desc), np.uint8), 0x04)
    grp.close()
    ctx.close()
    assert np.array_equal(host, arena)


@pytest.mark.parametrize("registered", [True, False], ids=["registered", "staged"])
def test_ctx_nat_submit_tcp(V, orc, vecs, registered):
    """vpcsum_ctx_nat_submit with the mode bit on host frames, zero-copy (registered arena) and
    staged (the TCP header is copied back, through L3 + 111 for the IPv6 vector; every caller byte
    after it stays), both modes; and the same through a group of two contexts on one device."""
    ca, cd, crw = T.pack(vecs, 14)
    ra, rd, rrw, bad = T.received_batch(65)
    keep = ~bad
    rd, rrw = rd[keep].copy(), rrw[keep]
    rd["l3_off"] += (len(ca) + 15) // 16 * 16 + 2048
    arena = np.concatenate([ca, np.zeros((len(ca) + 15) // 16 * 16 - len(ca) + 2048, np.uint8), ra, np.zeros(4096, np.uint8)])
    cd = cd.copy()
    cd["l3_off"][np.array([v["bad"] for v in vecs])] = len(arena) - 10   # still past the end of the joined arena
    desc, rw = np.concatenate([cd, rd]), np.concatenate([crw, rrw])
    want, want_st = T.expected(orc, arena, desc, rw)
    assert (want_st & T.S_MSS_ABSENT).any() and "ipv6_mss_at_l3_110" in [v["name"] for v in vecs]
    base = arena.copy()
    ctx = V.Context(0, max_arena=arena.nbytes, max_pkts=len(desc))
    grp = V.Group(devices=(0, 0), max_arena=arena.nbytes, max_pkts=len(desc))
    if registered:
        ctx.register(arena)
    for mode in (V.NAT_RFC1624 | V.NAT_TCP_REWRITES, V.NAT_STRICT_JAVA | V.NAT_TCP_REWRITES):
        a = arena if registered else base.copy()
        a[:] = base
        st = ctx.nat(a, desc, rw, mode)
        assert np.array_equal(st, want_st), hex(mode)
        assert np.array_equal(a, want), (hex(mode), _first_diff(a, want, desc))
    if registered:
        ctx.unregister(arena)
        grp.register(arena)
    for mode in (V.NAT_RFC1624 | V.NAT_TCP_REWRITES, V.NAT_STRICT_JAVA | V.NAT_TCP_REWRITES):
        a = arena if registered else base.copy()
        a[:] = base
        st = np.zeros(len(desc), np.uint8)
        grp.wait(grp.nat_submit(a, desc, rw, st, mode))
        assert np.array_equal(st, want_st), hex(mode)
        assert np.array_equal(a, want), (hex(mode), _first_diff(a, want, desc))
    grp.close()
    ctx.close()


def test_pni_nat_tcp(V, orc, vecs, tmp_path):
    """Java_io_vproxy_vpcsum_VPCsum_natSubmit with mode bit 2 from plain C++ (tests/cpp/
    pni_nat_tcp.cpp, built and run like capi_smoke) on three frames: a clamp, an absent and a SYN-ACK
    build; the bytes and status it must find come from here."""
    by = {v["name"]: v for v in vecs}
    three = [by["mss_after_1_nop"], by["no_options"], by["proxy_synack"]]
    arena, desc, rw = T.pack(three, 14)
    want, want_st = T.expected(orc, arena, desc, rw)
    assert list(want_st) == [O.S_DONE, O.S_DONE | T.S_MSS_ABSENT, O.S_DONE]
    vf = tmp_path / "pni_vectors.bin"
    vf.write_bytes(struct.pack("<I", len(arena)) + arena.tobytes() + desc.tobytes() + rw.tobytes() + want.tobytes() +
                   want_st.tobytes())
    exe = tmp_path / "pni_nat_tcp"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(REPO, "include"),
                           os.path.join(REPO, "tests", "cpp", "pni_nat_tcp.cpp"), "-L", os.path.join(REPO, "vproxy_amd"),
                           "-lvpcsum", "-Wl,-rpath," + os.path.join(REPO, "vproxy_amd"), "-o", str(exe)])
    r = subprocess.run([str(exe), str(vf)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "pni nat tcp ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
