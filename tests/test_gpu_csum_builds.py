"""Every checksum kernel build against the oracle, at the edges of K2's plan, tiers, units, loop and
sampled paths.

tests/csumbuilds.py names every compute variant id launch_csum accepts with the build it resolves
to (held against the compiled code object by tests/test_kernel_resources.py); tests/k2vec.py builds
the batch that hits the geometry by construction (held against the descriptors by
tests/test_k2_vectors_cpu.py).  Here every id runs that batch with non-temporal and with plain loads
-- compute, verify on valid and on wrong stored sums, write-back into guarded views, prefixes,
status views, missing out / status -- and the layouts that need a grid decision run on the builds
that take it: the unit loop's second trip, workgroup-sorted units, staged result words (the flush's
second round), staging in the window build, the dense window build, the two sides of the
buffer-addressing limit.  Every word, status byte and arena byte is compared with the oracle's
(k2vec.expect), bit for bit.
"""
import numpy as np
import pytest

import csumbuilds as CB
import k2vec as K
from oracle import oracle as O

pytestmark = pytest.mark.gpu

GUARD = 0xEE
OUT_GUARD = 0x6EEEEEEE
PREFIXES = (1, 63, 64, 65, 255, 256, 257)
THREADS = 8


@pytest.fixture(scope="module")
def V():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vproxy_amd import vpcsum
    vpcsum.lib()
    return vpcsum


@pytest.fixture(scope="module")
def cus(V):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _dev(a):
    """Host to device through pinned memory, as the other GPU tests copy."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().cuda()


def _host(t):
    """Device to host through pinned memory."""
    import torch
    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    h.copy_(t)
    torch.cuda.synchronize()
    return h.numpy().copy()


def _any(t) -> bool:
    """Whether any byte of a device tensor is set, the answer fetched through pinned memory."""
    return bool(_host(t.any().reshape(1))[0])


def _desc_dev(desc):
    return _dev(np.ascontiguousarray(desc).view(np.uint8).reshape(-1))


class Geo:
    """The geometry batch on the device (valid and wrong stored sums) and the oracle's answers,
    each computed once and never changed."""

    def __init__(self, orc):
        self.orc = orc
        self.b = K.batch()
        self.S = {"valid": self.b, "wrong": K.corrupted(self.b)}
        self.desc = _desc_dev(self.b["desc"])
        self.arena = {k: _dev(S["arena"]) for k, S in self.S.items()}
        self._want = {}

    def want(self, which, mode, n=None, write=False):
        key = (which, mode, n, write)
        if key not in self._want:
            S = self.S[which]
            self._want[key] = K.expect(self.orc, S["arena"], S["desc"], mode, n, write)
        return self._want[key]


@pytest.fixture(scope="module")
def geo(V, orc):
    return Geo(orc)


def _launch(V, arena, desc, n, mode, variant, plain, out=True, status=True, st_off=0, **kw):
    """One vpcsum_compute_async on the first n descriptors; out and status are views into buffers
    of guard values, checked afterwards.  Returns (out words | None, status bytes | None)."""
    import torch
    obuf = torch.full((n + 8,), OUT_GUARD, dtype=torch.int32, device="cuda")
    sbuf = torch.full((n + 8,), GUARD, dtype=torch.uint8, device="cuda")
    o = obuf[4:4 + n] if out else None
    s = sbuf[st_off:st_off + n] if status else None
    V.compute(arena, desc, n, o, s, mode, variant, plain_loads=plain, **kw)
    torch.cuda.synchronize()
    ob, sb = _host(obuf), _host(sbuf)
    keep_o = np.ones(n + 8, bool)
    keep_s = np.ones(n + 8, bool)
    if out:
        keep_o[4:4 + n] = False
    if status:
        keep_s[st_off:st_off + n] = False
    assert (ob[keep_o] == OUT_GUARD).all(), "words around (or instead of) out written"
    assert (sb[keep_s] == GUARD).all(), "bytes around (or instead of) status written"
    return (ob[4:4 + n].view(np.uint32) if out else None), (sb[st_off:st_off + n] if status else None)


def _diffs(S, what, got_out, got_st, want_out, want_st, build=None, arena_len=None) -> list:
    """Messages naming the first packet whose out word / status byte differs from the oracle's."""
    msgs = []
    if got_out is not None:
        msgs.append(K.first_diff(S, got_out, want_out[:len(got_out)], "out words", build, arena_len))
    if got_st is not None:
        msgs.append(K.first_diff(S, got_st, want_st[:len(got_st)], "status bytes", build, arena_len))
    return [f"{what}: {m}" for m in msgs if m]


def _compare(S, what, got_out, got_st, want_out, want_st, build=None, arena_len=None):
    msgs = _diffs(S, what, got_out, got_st, want_out, want_st, build, arena_len)
    if msgs:
        pytest.fail("\n".join(msgs))


def _check(V, geo, row, plain, which, mode, n=None, **kw):
    S = geo.S[which]
    n_run = S["n"] if n is None else n
    got = _launch(V, geo.arena[which], geo.desc, n_run, mode, row.id, plain, **kw)
    want_out, want_st, _ = geo.want(which, mode & O.MODE_VERIFY, n)
    what = f"{row.label} {'plain' if plain else 'nt'} loads, {which} sums, mode {mode:#x}, n {n_run}, {kw}"
    _compare(S, what, got[0], got[1], want_out, want_st, CB.build_of(row))


def _check_write(V, geo, row, plain, arena_off):
    """Write-back over the wrong-sums copy in a view at byte offset arena_off of a guarded buffer:
    the whole arena, out and status equal the oracle's, nothing outside the view is written.  A view
    that is not 16-B aligned goes to the team kernel (launch_d's fallback)."""
    import torch
    S = geo.S["wrong"]
    alen = len(S["arena"])
    abuf = torch.full((alen + 64,), GUARD, dtype=torch.uint8, device="cuda")
    arena = abuf[arena_off:arena_off + alen]
    arena.copy_(geo.arena["wrong"])
    assert arena.data_ptr() % 16 == arena_off % 16
    got = _launch(V, arena, geo.desc, S["n"], O.MODE_WRITE, row.id, plain)
    want_out, want_st, want_arena = geo.want("wrong", O.MODE_COMPUTE, None, True)
    what = f"{row.label} {'plain' if plain else 'nt'} loads, write, arena offset {arena_off}"
    _compare(S, what, got[0], got[1], want_out, want_st, CB.build_of(row))
    ab = _host(abuf)
    assert (ab[:arena_off] == GUARD).all() and (ab[arena_off + alen:] == GUARD).all(), f"{what}: bytes around the arena written"
    msg = K.first_arena_diff(S, ab[arena_off:arena_off + alen], want_arena)
    if msg:
        pytest.fail(f"{what}: {msg}")


@pytest.mark.parametrize("plain", [False, True], ids=["nt", "plain"])
@pytest.mark.parametrize("row", CB.ID_ROWS, ids=[r.label for r in CB.ID_ROWS])
def test_row_equals_oracle(V, geo, row, plain):
    """One id of launch_csum's switch with one load policy on the geometry batch: compute; verify on
    valid and on wrong stored sums; write-back with the arena a guarded view at byte offsets 0, 1
    and 9; the prefixes of n in PREFIXES (partial units and workgroups); the status a view at byte
    offsets 1..3; out or status missing."""
    _check(V, geo, row, plain, "valid", O.MODE_COMPUTE)
    _check(V, geo, row, plain, "valid", O.MODE_VERIFY)
    _check(V, geo, row, plain, "wrong", O.MODE_VERIFY)
    for arena_off in (0, 1, 9):
        _check_write(V, geo, row, plain, arena_off)
    for n in PREFIXES:
        _check(V, geo, row, plain, "wrong", O.MODE_VERIFY, n=n)
    for st_off in (1, 2, 3):
        _check(V, geo, row, plain, "wrong", O.MODE_VERIFY, st_off=st_off)
    _check(V, geo, row, plain, "wrong", O.MODE_VERIFY, out=False)
    _check(V, geo, row, plain, "wrong", O.MODE_VERIFY, status=False)
    _check(V, geo, row, plain, "valid", O.MODE_COMPUTE, status=False)


def test_id_sweep(V, geo):
    """Ids 0..255 with n = 1: exactly the table's ids run (and equal the oracle), every other is
    refused with VpcsumError and writes nothing."""
    want_out, want_st, _ = geo.want("valid", O.MODE_VERIFY, 1)
    ran = []
    for i in range(256):
        try:
            out, st = _launch(V, geo.arena["valid"], geo.desc, 1, O.MODE_VERIFY, i, False)
        except V.VpcsumError:
            continue
        assert out[0] == want_out[0] and st[0] == want_st[0], i
        ran.append(i)
    assert ran == CB.IDS


# ---- the unit loop's second trip ----

class Layout:
    """A layout of k2vec on the device, its oracle answers computed once (threads: the layouts are
    large, and none of them writes)."""

    def __init__(self, orc, L, arena_np):
        import torch
        self.L, self.orc = L, orc
        self.host_arena = arena_np
        self.desc = _desc_dev(L["desc"])
        self.arena = torch.zeros(L["arena_len"], dtype=torch.uint8, device="cuda")
        self.arena[:len(arena_np)].copy_(_dev(arena_np))
        self._want = {}

    def want(self, mode, write=False):
        if (mode, write) not in self._want:
            self._want[(mode, write)] = K.expect(self.orc, self.host_arena, self.L["desc"], mode, None, write,
                                                 threads=1 if write else THREADS)
        return self._want[(mode, write)]

    def diffs(self, V, variant, plain, mode, what, build=None, **kw) -> list:
        got = _launch(V, self.arena, self.desc, self.L["n"], mode, variant, plain, **kw)
        want_out, want_st, _ = self.want(mode & O.MODE_VERIFY)
        return _diffs(self.L, f"{what}: id {variant} {'plain' if plain else 'nt'} loads, mode {mode:#x}, n {self.L['n']}", got[0],
                      got[1], want_out, want_st, build, self.L["arena_len"])

    def check(self, V, *a, **kw):
        msgs = self.diffs(V, *a, **kw)
        if msgs:
            pytest.fail("\n".join(msgs))


@pytest.fixture(scope="module")
def trip2(V, orc, geo, cus):
    L = K.second_trip(geo.b, cus)
    return Layout(orc, L, geo.S["wrong"]["arena"])


@pytest.mark.parametrize("row", CB.second_trip_rows(), ids=[r.label for r in CB.second_trip_rows()])
def test_loop_second_trip(V, trip2, cus, row):
    """One workgroup per CU and cus * 256 + 256 + 65 packets cycling the geometry batch: the first
    workgroup's four waves and one more take a second trip through the unit loop (the prefetched
    descriptor, the slots rewritten), the last of them with one live lane.  One row per distinct
    (TEAM, U, TS, IL, DS, WGS) shape, compute and verify."""
    assert trip2.L["n"] == cus * 256 + 321
    for mode in (O.MODE_COMPUTE, O.MODE_VERIFY):
        trip2.check(V, row.id, False, mode, "second trip", CB.build_of(row), blocks_per_cu=1)


# ---- workgroup-sorted units ----

def test_sorted_units(V, orc, geo, cus):
    """Workgroup-sorted units (ids 0 and 84 on a batch the sample finds mixed) at the compositions of
    k2vec.sorted_compositions: compute, verify and write equal the oracle; ids 76 and 79 (per-wave
    units) run the same batch.  Every descriptor has a frame of its own, so the write is safe."""
    import torch
    L = K.sorted_units(geo.b, cus)
    lay = Layout(orc, L, L["arena"])
    front = lay.arena[:len(L["arena"])].clone()
    fails = []       # every id's first difference, not the first id's alone
    for variant, plain in ((0, False), (84, False), (76, False), (79, False), (84, True)):
        for mode in (O.MODE_COMPUTE, O.MODE_VERIFY):
            fails += lay.diffs(V, variant, plain, mode, "sorted units")
    assert not fails, f"{len(fails)} runs differ:\n" + "\n".join(fails)
    want_out, want_st, want_arena = lay.want(O.MODE_COMPUTE, True)
    for variant in (0, 84):
        out, st = _launch(V, lay.arena, lay.desc, L["n"], O.MODE_WRITE, variant, False)
        _compare(L, f"sorted units: id {variant} write", out, st, want_out, want_st, None, L["arena_len"])
        got = _host(lay.arena[:len(L["arena"])])
        msg = K.first_arena_diff(L, got, want_arena)
        assert msg is None, f"sorted units: id {variant} write: {msg}"
        assert not _any(lay.arena[len(L["arena"]):]), "bytes past the frames written"
        lay.arena[:len(L["arena"])].copy_(front)
    del lay, front
    torch.cuda.empty_cache()


# ---- staged result words ----

@pytest.fixture(scope="module")
def staged_arena(V, geo, cus):
    """One device arena for the three staged sizes: zeros, the wrong-sums geometry arena in front."""
    import torch
    a = torch.zeros(K.staged_sizes(cus)[2] * 1024, dtype=torch.uint8, device="cuda")
    a[:len(geo.b["arena"])].copy_(geo.arena["wrong"])
    yield a
    del a
    torch.cuda.empty_cache()


@pytest.mark.parametrize("k", [0, 1, 2], ids=["4W-1", "4W", "8W+5wg+37"])
def test_staged_result_words(V, orc, geo, cus, staged_arena, k):
    """The staging builds (ids 0, 84, 79) on a batch whose sample is all >= 1 KiB, at n = 4 W - 1 (not
    staged), 4 W (staged: 4 units per wave, one flush when the wave leaves) and 8 W + 256 * 5 + 37
    (a full flush at the 8th unit, then a 9th unit for 21 waves and an empty last flush for the
    others; a partial last unit), verify and compute, both load policies; id 76 as the unstaged
    build on the largest."""
    L = K.staged(geo.b, cus, k)
    arena = staged_arena[:L["arena_len"]]
    desc = _desc_dev(L["desc"])
    host = geo.S["wrong"]["arena"]
    want = {m: K.expect(orc, host, L["desc"], m, threads=THREADS) for m in (O.MODE_COMPUTE, O.MODE_VERIFY)}
    fails = []       # every build's first difference, not the first build's alone
    for variant in (0, 84, 79) + ((76,) if k == 2 else ()):
        for plain in (False, True):
            for mode in (O.MODE_VERIFY, O.MODE_COMPUTE):
                out, st = _launch(V, arena, desc, L["n"], mode, variant, plain, status=mode == O.MODE_VERIFY)
                fails += _diffs(L, f"staged n {L['n']}: id {variant} {'plain' if plain else 'nt'} loads, mode {mode:#x}", out, st,
                                want[mode][0], want[mode][1], None, L["arena_len"])
    assert not fails, f"{len(fails)} runs differ:\n" + "\n".join(fails)


# ---- staging in the window build, arenas at the buffer-addressing limit ----

def test_staged_window_build(V, orc, geo, cus):
    """K2StagedWin with staged result words: a slab of the geometry batch laid across the 2-GiB window
    line of an arena past 4 GiB, every unit's lanes alternating between the two windows (the
    leftover pass writes into the staging words), n = 4 W + 64 * 3 + 5 with the sample all >= 1 KiB;
    verify and write, both load policies.  The oracle runs on the slab."""
    import torch
    L = K.staged_window(geo.b, cus)
    big = torch.zeros(L["arena_len"], dtype=torch.uint8, device="cuda")
    slab = _dev(L["slab"])
    lo, hi = L["base"], L["base"] + len(L["slab"])
    big[lo:hi].copy_(slab)
    desc = _desc_dev(L["dev"])
    want_v = K.expect(orc, L["slab"], L["rel"], O.MODE_VERIFY, threads=THREADS)
    want_w = K.expect(orc, L["slab"], L["rel"], O.MODE_COMPUTE, None, True)
    for plain in (False, True):
        out, st = _launch(V, big, desc, L["n"], O.MODE_VERIFY, 0, plain)
        _compare(L, f"staged window build, {'plain' if plain else 'nt'} loads, verify", out, st, want_v[0], want_v[1], CB.K2_STAGED_WIN,
                 len(L["slab"]))
        out, st = _launch(V, big, desc, L["n"], O.MODE_WRITE, 0, plain)
        _compare(L, f"staged window build, {'plain' if plain else 'nt'} loads, write", out, st, want_w[0], want_w[1], CB.K2_STAGED_WIN,
                 len(L["slab"]))
        msg = K.first_arena_diff(L, _host(big[lo:hi]), want_w[2])
        assert msg is None, msg
        assert not _any(big[lo - (1 << 20):lo]) and not _any(big[hi:hi + (1 << 20)]), "bytes around the slab written"
        big[lo:hi].copy_(slab)
    del big
    torch.cuda.empty_cache()


def test_dense_window_build(V, orc, geo, cus):
    """K2DenseWin: id 0 takes it when an arena past 4 GiB holds at most 128 bytes per packet, that is
    from 2^25 packets on, which no other test has.  The staged window layout's first 101 units (a slab
    across the 2-GiB line, every unit's lanes alternating between the two windows) repeated over
    arena_len / 128 descriptors, built on the device; the oracle's answer for one period repeats
    likewise.  Verify with both load policies, then write."""
    import torch
    L = K.staged_window(geo.b, cus)
    arena_len = (4 << 30) + (128 << 10)
    n = arena_len // 128
    assert arena_len > CB.MAX_BUF_ARENA and arena_len <= n * 128 and n * 1024 > arena_len      # dense, no sample
    P = K.UNIT * 101
    rel, dev = np.ascontiguousarray(L["rel"][:P]), np.ascontiguousarray(L["dev"][:P])
    reps = -(-n // P)
    big = torch.zeros(arena_len, dtype=torch.uint8, device="cuda")
    slab = _dev(L["slab"])
    lo, hi = L["base"], L["base"] + len(L["slab"])
    big[lo:hi].copy_(slab)
    desc = _desc_dev(dev).repeat(reps)[:16 * n].contiguous()
    per = dict(L, desc=rel, idx=L["idx"][:P])
    want_v = K.expect(orc, L["slab"], rel, O.MODE_VERIFY)
    want_w = K.expect(orc, L["slab"], rel, O.MODE_COMPUTE, None, True)

    def check(what, got, want):
        for g, w, name in zip(got, want, ("out words", "status bytes")):
            full = np.tile(w, reps)[:n]
            bad = np.nonzero(g != full)[0]
            if len(bad):
                i = int(bad[0])
                pytest.fail(f"dense window build, {what}: {len(bad)} {name} differ, first at {i}: got {int(g[i]):#x}, oracle "
                            f"{int(full[i]):#x}: period {K.describe(per, i % P, CB.K2_DENSE_WIN, len(L['slab']))}")

    for plain in (False, True):
        check(f"{'plain' if plain else 'nt'} loads, verify", _launch(V, big, desc, n, O.MODE_VERIFY, 0, plain), want_v)
    check("write", _launch(V, big, desc, n, O.MODE_WRITE, 0, False), want_w)
    msg = K.first_arena_diff(per, _host(big[lo:hi]), want_w[2])
    assert msg is None, msg
    assert not _any(big[lo - (1 << 20):lo]) and not _any(big[hi:hi + (1 << 20)]), "bytes around the slab written"
    del big, desc
    torch.cuda.empty_cache()


@pytest.mark.parametrize("arena_len", [CB.MAX_BUF_ARENA, CB.MAX_BUF_ARENA + 16], ids=["0xFFFF0000", "0xFFFF0010"])
def test_arena_at_the_buffer_limit(V, orc, geo, arena_len):
    """The geometry batch at the end of an arena of exactly kMaxBufArena bytes (buffer addressing with
    the largest offsets, next to kOutOfRange) and of 16 bytes more (the window build, id 0's
    K2StagedWin), compute and write, both load policies; the 16 bytes more also on the staging
    build's id, which refuses such an arena."""
    import torch
    S = geo.S["wrong"]
    alen = len(S["arena"])
    base = (arena_len - alen) & ~15
    d = S["desc"].copy()
    d["l3_off"] += np.uint64(base)
    K.place_oob(d, S["oob"], arena_len)
    rel = S["desc"].copy()
    K.place_oob(rel, S["oob"], arena_len)            # out of range for the oracle's short arena too
    big = torch.zeros(arena_len, dtype=torch.uint8, device="cuda")
    big[base:base + alen].copy_(geo.arena["wrong"])
    desc = _desc_dev(d)
    L = dict(S, desc=rel)
    want = K.expect(orc, S["arena"], rel, O.MODE_VERIFY)
    want_w = K.expect(orc, S["arena"], rel, O.MODE_COMPUTE, None, True)
    build = CB.K2_STAGED if arena_len <= CB.MAX_BUF_ARENA else CB.K2_STAGED_WIN
    for plain in (False, True):
        what = f"arena of {arena_len:#x} bytes, {'plain' if plain else 'nt'} loads"
        out, st = _launch(V, big, desc, S["n"], O.MODE_VERIFY, 0, plain)
        _compare(L, what + ", verify", out, st, want[0], want[1], build)
        out, st = _launch(V, big, desc, S["n"], O.MODE_COMPUTE, 0, plain)
        _compare(L, what + ", compute", out, st, want[0], np.where(want[1] & O.S_BAD_DESC, O.S_BAD_DESC, O.S_DONE).astype(np.uint8),
                 build)
        out, st = _launch(V, big, desc, S["n"], O.MODE_WRITE, 0, plain)
        _compare(L, what + ", write", out, st, want_w[0], want_w[1], build)
        msg = K.first_arena_diff(L, _host(big[base:base + alen]), want_w[2])
        assert msg is None, f"{what}: {msg}"
        assert not _any(big[base - (1 << 20):base]) and not _any(big[base + alen:]), "bytes around the batch written"
        big[base:base + alen].copy_(geo.arena["wrong"])
    if arena_len > CB.MAX_BUF_ARENA:
        with pytest.raises(V.VpcsumError):
            _launch(V, big, desc, S["n"], O.MODE_COMPUTE, 84, False)
    del big
    torch.cuda.empty_cache()
