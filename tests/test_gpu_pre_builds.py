"""Every build of the pre-image flush kernel against the oracle, at the edges of its window, store
and loop geometry.

tests/prebuilds.py names one mode word per k_pre build of vproxy_amd/csrc/launch_modes.h and the
three run-time switches (held against the header by tests/test_lib_cpu.py); tests/prevec.py builds
the batch that hits the geometry by construction (held against the descriptors, and its expected
bytes against a pure-Python model, by tests/test_pre_vectors_cpu.py).  Here each build flushes that
batch through vpcsum_pre_async, and the whole arena, every out word and every status byte are
compared with Java's bytes from the reference-free oracle (orc.nat_java; the full recompute for the
header-sum packets), bit for bit.  The host context's three ways to a flush -- staged, in place, the
service grid -- take the same batch and the same comparison.
"""
import numpy as np
import pytest

import prebuilds as PB
import prevec as PV
from oracle import oracle as O

pytestmark = pytest.mark.gpu

PREFIXES = (1, 2, 3, 5, 63, 64, 65, 255, 257)
GUARD = PV.GUARD
OUT_GUARD_I32 = int(np.array(PV.OUT_GUARD, np.uint32).view(np.int32))


@pytest.fixture(scope="module")
def V():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vproxy_amd import vpcsum
    vpcsum.lib()
    return vpcsum


def _dev(a):
    """Host to device through pinned memory."""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).pin_memory().cuda()


def _host(t):
    """Device to host through pinned memory."""
    import torch
    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    h.copy_(t)
    torch.cuda.synchronize()
    return h.numpy().copy()


class Batch:
    """The geometry batch, its device-resident descriptors and entries per format, and the oracle's
    answer per (format, prefix length), each computed once and never changed."""

    def __init__(self, orc, b):
        self.orc, self.b = orc, b
        self._dev, self._want = {}, {}

    def tables(self, V, fmt):
        if fmt not in self._dev:
            self._dev[fmt] = (V.desc_to_tensor(self.b["desc"]), _dev(PV.entries(self.b["pre"], fmt)))
        return self._dev[fmt]

    def want(self, fmt, n=None):
        if (fmt, n) not in self._want:
            self._want[(fmt, n)] = PV.expect(self.b, self.orc, fmt, n)
        return self._want[(fmt, n)]


@pytest.fixture(scope="module")
def S(orc):
    return Batch(orc, PV.batch(orc))


def _run(V, S, fmt, mode, n, st_off=0, arena_off=0):
    """The first n packets of S through vpcsum_pre_async.  The arena is a view at byte offset
    arena_off into its allocation, the status one at st_off into a buffer of guard bytes, the out
    words start as guards; returns (arena, out, status) after checking that nothing outside the
    views was written."""
    import torch
    a = S.b["after"]
    abuf = torch.full((len(a) + 32,), GUARD, dtype=torch.uint8, device="cuda")
    arena = abuf[arena_off:arena_off + len(a)]
    arena.copy_(torch.from_numpy(a).pin_memory())
    assert arena.data_ptr() % 16 == arena_off
    sbuf = torch.full((n + 8,), GUARD, dtype=torch.uint8, device="cuda")
    st = sbuf[st_off:st_off + n]
    out = torch.full((n + 2,), OUT_GUARD_I32, dtype=torch.int32, device="cuda")
    desc, ent = S.tables(V, fmt)
    V.pre(arena, desc, ent, n, out, st, mode, pre_fmt=fmt)
    torch.cuda.synchronize()
    ab, sb, ob = _host(abuf), _host(sbuf), _host(out).view(np.uint32)
    assert (ab[:arena_off] == GUARD).all() and (ab[arena_off + len(a):] == GUARD).all(), "bytes around the arena written"
    assert (sb[:st_off] == GUARD).all() and (sb[st_off + n:] == GUARD).all(), "bytes around the status written"
    assert (ob[n:] == PV.OUT_GUARD).all(), "out words past the batch written"
    return ab[arena_off:arena_off + len(a)], ob[:n], sb[st_off:st_off + n]


def _check(V, S, build, switches, n=None, st_off=0, arena_off=0):
    n_run = len(S.b["desc"]) if n is None else n
    got, out, st = _run(V, S, build.fmt, build.word(switches=switches), n_run, st_off, arena_off)
    w = S.want(build.fmt, n)
    want = w["arena"] if "write" in switches else S.b["after"]
    what = f"{build.id} {'+'.join(switches) or 'compute'} n {n_run} status offset {st_off} arena offset {arena_off}"
    if not np.array_equal(got, want):
        pytest.fail(f"{what}: {PV.first_diff(S.b, got, want, build.fmt, build.ch, arena_off)}")
    for name, g, x in (("status", st, w["status"][:n_run]), ("out word", out, w["out"][:n_run])):
        if not np.array_equal(g, x):
            i = int(np.nonzero(g != x)[0][0])
            pytest.fail(f"{what}: {name} {int(g[i]):#x}, oracle {int(x[i]):#x}: {PV.describe(S.b, i, build.fmt, build.ch, arena_off)}")


@pytest.mark.parametrize("switches", PB.RUNS, ids=["+".join(s) or "compute" for s in PB.RUNS])
@pytest.mark.parametrize("build", PB.LIVE, ids=[b.id for b in PB.LIVE])
def test_build_equals_oracle(V, S, build, switches):
    """One build under one setting of its run-time switches -- WRITE; compute only (the arena stays
    as received, the out words are the same); WRITE on the byte path; WRITE with non-temporal stores
    -- on the geometry batch: the whole batch; its prefixes of n in PREFIXES (the batch tail: `p >=
    n` for a lane's second packet, the packed status store's last dword); the status a view at byte
    offsets 1..3 (the packed store's byte branch); the arena a view at byte offsets 1 and 9 (the
    kernel addresses by absolute address, so every r0 shifts).  Under the 16-B entries the IPv6 rows
    are refused (S_BAD_DESC, out 0) and untouched: the expectation holds them so."""
    _check(V, S, build, switches)
    for n in PREFIXES:
        _check(V, S, build, switches, n=n)
    for st_off in (1, 2, 3):
        _check(V, S, build, switches, st_off=st_off)
    for arena_off in (1, 9):
        _check(V, S, build, switches, arena_off=arena_off)


def test_fmt0_refuses_ipv6_untouched(S):
    """What the sweep's 16-B runs compare with: every IPv6 F_PRE row refused, its frame as received,
    and there are rows of that kind the 48-B entries flush."""
    e0, e1 = S.want(PB.FMT_PRE4), S.want(PB.FMT_PRE)
    d = S.b["desc"]
    v6 = (d["l3_ver"] == 6) & e0["act"]
    assert v6.sum() > 100 and (e0["status"][v6] == O.S_BAD_DESC).all() and (e0["out"][v6] == 0).all()
    assert e1["live"][v6].sum() > 100
    for i in np.nonzero(v6)[0]:
        o, ln = int(d[i]["l3_off"]), int(d[i]["l3_len"])
        assert np.array_equal(e0["arena"][o:o + ln], S.b["after"][o:o + ln])


@pytest.mark.parametrize("byte_path", [False, True], ids=["window", "byte_path"])
@pytest.mark.parametrize("build", PB.PROBES, ids=[b.id for b in PB.PROBES])
def test_probe_writes_the_stored_sums_back(V, S, build, byte_path):
    """The memory-pattern probes (16-B entries) in WRITE mode over the whole batch, and again with
    the byte-path bit: the stored sums are written back unchanged, so the arena is byte-identical to
    its input -- also for a packet that has no window (past it, or the byte-path bit) -- every
    accepted row reports S_DONE, every refused one S_BAD_DESC, the others' bytes are not touched."""
    sw = ("write", "byte_path") if byte_path else ("write",)
    n = len(S.b["desc"])
    got, out, st = _run(V, S, build.fmt, build.word(switches=sw), n)
    if not np.array_equal(got, S.b["after"]):
        pytest.fail(f"{build.id} {'+'.join(sw)}: {PV.first_diff(S.b, got, S.b['after'], build.fmt, build.ch)}")
    alen = len(S.b["after"])
    act = (S.b["desc"]["flags"] & O.F_PRE) != 0
    ok = np.array([PV.pre_desc_ok(d, alen, build.fmt) for d in S.b["desc"]]) & act
    want = np.where(ok, O.S_DONE, np.where(act, O.S_BAD_DESC, GUARD))
    bad = np.nonzero(st != want)[0]
    assert not len(bad), (build.id, hex(st[bad[0]]), PV.describe(S.b, int(bad[0]), build.fmt, build.ch))
    assert (out[~act] == PV.OUT_GUARD).all() and (out[act & ~ok] == 0).all()
    # the out words are the stored sums of the flagged fields
    d = S.b["desc"]
    for i in np.nonzero(ok)[0][::7]:
        o, l4o, fl = int(d[i]["l3_off"]), int(d[i]["l4_off"]), int(d[i]["flags"])
        f = o + l4o + O.L4_FIELD.get(int(d[i]["l4_proto"]), 0)
        a = S.b["after"]
        word = ((int(a[o + 10]) << 8 | int(a[o + 11])) if fl & O.F_IP else 0) | \
               ((int(a[f]) << 8 | int(a[f + 1])) << 16 if fl & O.F_L4 else 0)
        assert out[i] == word, PV.describe(S.b, int(i), build.fmt, build.ch)


# ---- the grid-stride loop's second trip ----

@pytest.fixture(scope="module")
def cus(V):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def strided(orc, cus):
    """2 * CUs * 256 + 65 packets in pre-image form, Java's answer computed once; one packet per
    lane takes a prefix (64-byte stride: no packet reaches into another's frame)."""
    return PV.strided(orc, 2 * cus * 256 + 65)


@pytest.mark.parametrize("fmt,w", PB.SECOND_TRIP, ids=[f"fmt{f}-w{w}" for f, w in PB.SECOND_TRIP])
def test_loop_second_trip(V, strided, cus, fmt, w):
    """One workgroup per CU and W * CUs * 256 + 65 packets of 28..60 bytes at a 64-byte stride: the
    grid covers W * CUs * 256 packets per trip, so the first 65 lanes' packets come from a second
    trip through the loop, the last of them alone in its wave.  Arena and status whole."""
    import torch
    build = PB.Build(fmt, w, 6, False)
    assert build in PB.BUILDS
    n = w * cus * 256 + 65
    arena = _dev(strided["after"][:64 * n])
    st = torch.full((n,), GUARD, dtype=torch.uint8, device="cuda")
    desc = V.desc_to_tensor(strided["desc"][:n])
    ent = _dev(PV.entries(strided["pre"][:n], fmt))
    V.pre(arena, desc, ent, n, None, st, build.word(wgs_per_cu=1, switches=("write",)), pre_fmt=fmt)
    torch.cuda.synchronize()
    got, st = _host(arena), _host(st)
    want, want_st = strided["want"][:64 * n], strided["status"][:n]
    bad = np.nonzero(st != want_st)[0]
    assert not len(bad), (build.id, int(bad[0]), hex(st[bad[0]]), hex(want_st[bad[0]]))
    bad = np.nonzero(got != want)[0]
    assert not len(bad), (build.id, f"byte {int(bad[0]) % 64} of packet {int(bad[0]) // 64} of {n}")
    assert (want_st[n - 65:] == O.S_DONE).sum() > 32 and not np.array_equal(got[-65 * 64:], strided["after"][64 * (n - 65):64 * n])


# ---- the host context ----

def _ctx_tables(S, fmt):
    """(descriptors, entries, expectation) for the host context, which sums the rows without F_PRE
    in full.  48-B entries: the batch as it is.  16-B entries: the IPv6 rows the 48-B entries would
    flush go the full path (F_PRE cleared: Java's bytes too), the other IPv6 rows carry no flags."""
    e1 = S.want(PB.FMT_PRE)
    d = S.b["desc"].copy()
    moved = np.zeros(len(d), bool)
    if fmt == PB.FMT_PRE4:
        v6 = d["l3_ver"] == 6
        moved = v6 & e1["live"]
        d["flags"][moved] &= 0xFF ^ O.F_PRE
        d["flags"][v6 & ~e1["live"]] = 0
    act = (d["flags"] & O.F_PRE) != 0
    return d, PV.entries_array(S.b["pre"], fmt), e1, act, moved


def _ctx_compare(S, fmt, arena, out, st, e1, act, moved, rows, what):
    """A context flush of the rows `rows`: the whole arena, and the status and out words of the
    F_PRE rows and the moved ones (the others' are the checksum kernel's)."""
    if not np.array_equal(arena, e1["arena"]):
        pytest.fail(f"{what}: {PV.first_diff(S.b, arena, e1['arena'], fmt, 6)}")
    mine = (act | moved)[rows]
    want_st = np.where(moved[rows], O.S_DONE, e1["status"][rows])
    bad = np.nonzero(mine & (st != want_st))[0]
    assert not len(bad), (what, hex(st[bad[0]]), PV.describe(S.b, int(np.arange(len(act))[rows][bad[0]]), fmt, 6))
    bad = np.nonzero(mine & (out != e1["out"][rows]))[0]
    assert not len(bad), (what, hex(out[bad[0]]), PV.describe(S.b, int(np.arange(len(act))[rows][bad[0]]), fmt, 6))


@pytest.mark.parametrize("fmt", [PB.FMT_PRE, PB.FMT_PRE4], ids=["48B", "16B"])
@pytest.mark.parametrize("registered", [False, True], ids=["staged", "in_place"])
def test_ctx_run_pre(V, S, registered, fmt):
    """The batch through vpcsum_ctx_submit_pre on a pageable arena (staged: batch_plan.h's
    pre_staged_len cuts each F_PRE packet to its header, or to the L4 header its record covers) and
    on a registered one (launched in place): the whole arena, and every F_PRE row's status and out
    word."""
    d, ent, e1, act, moved = _ctx_tables(S, fmt)
    arena = S.b["after"].copy()
    ctx = V.Context(0, max_arena=arena.nbytes + 4096, max_pkts=len(d))
    try:
        if registered:
            ctx.register(arena)
        out, st = ctx.run_pre(arena, d, ent, O.MODE_WRITE)
        assert ctx.stats()["service_batches"] == 0
        _ctx_compare(S, fmt, arena, out, st, e1, act, moved, slice(None), f"registered {registered} fmt {fmt}")
        # compute only: the frames stay, the same words
        arena[:] = S.b["after"]
        out2, st2 = ctx.run_pre(arena, d, ent, O.MODE_COMPUTE)
        assert np.array_equal(arena, S.b["after"])
        assert np.array_equal(out2[act | moved], out[act | moved]) and np.array_equal(st2[act | moved], st[act | moved])
    finally:
        ctx.close()


@pytest.mark.parametrize("fmt", [PB.FMT_PRE, PB.FMT_PRE4], ids=["48B", "16B"])
def test_ctx_service_slices(V, S, fmt):
    """The batch in consecutive slices of 1, 3, 37 and 512 frames with the service grid on
    (kernels.hip svc_pre_packet, one wave per frame, a window of 24 chunks: the svc384 rows sit at
    383 / 384 / 385): every slice goes through the grid, and after the last one the whole arena
    equals Java's."""
    d, ent, e1, act, moved = _ctx_tables(S, fmt)
    arena = S.b["after"].copy()
    alen = len(arena)
    ctx = V.Context(0, max_arena=arena.nbytes + 4096, max_pkts=len(d))
    try:
        ctx.register(arena)
        ctx.set_service(5000)
        lo = k = posted = 0
        while lo < len(d):
            hi = min(lo + (1, 3, 37, 512)[k % 4], len(d))
            rows = slice(lo, hi)
            out = np.full(hi - lo, PV.OUT_GUARD, np.uint32)
            st = np.full(hi - lo, GUARD, np.uint8)
            ctx.wait(ctx.submit_pre(arena, np.ascontiguousarray(d[rows]), np.ascontiguousarray(ent[rows]), out, st, O.MODE_WRITE))
            posted += any(int(x["l3_off"]) + int(x["l3_len"]) <= alen for x in d[rows])   # a slice with a frame in the umem
            mine = (act | moved)[rows]
            want_st = np.where(moved[rows], O.S_DONE, e1["status"][rows])
            bad = np.nonzero(mine & (st != want_st))[0]
            assert not len(bad), (lo, hi, hex(st[bad[0]]), PV.describe(S.b, lo + int(bad[0]), fmt, 6))
            bad = np.nonzero(mine & (out != e1["out"][rows]))[0]
            assert not len(bad), (lo, hi, hex(out[bad[0]]), PV.describe(S.b, lo + int(bad[0]), fmt, 6))
            lo, k = hi, k + 1
        assert k >= 16 and ctx.stats()["service_batches"] == posted == k
        if not np.array_equal(arena, e1["arena"]):
            pytest.fail(f"service fmt {fmt}: {PV.first_diff(S.b, arena, e1['arena'], fmt, 6)}")
    finally:
        ctx.close()
