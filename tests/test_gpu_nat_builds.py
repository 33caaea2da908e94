"""Every NAT rewrite kernel build against the oracle, at the edges of its window, store and loop
geometry.

tests/natbuilds.py names one nat_mode word per build of vproxy_amd/csrc/launch_modes.h (held
against the header by tests/test_lib_cpu.py); tests/natvec.py builds the batch that hits the
geometry by construction (held against the descriptors by tests/test_nat_vectors_cpu.py).  Here each
build rewrites that batch through its entry format's call -- vpcsum_nat4_async (16-B entries),
vpcsum_nat_async (48-B), vpcsum_nat4r_async (32-B records) -- and the whole arena and every status
byte are compared with orc.nat4_java / orc.nat_java, bit for bit.  A build runs in the mode it was
compiled for: RFC 1624 on the valid-sum batch, strict Java on that and on the wrong-sum copy.
"""
import numpy as np
import pytest

import natbuilds as NB
import natvec as NV
from oracle import oracle as O

pytestmark = pytest.mark.gpu

PREFIXES = (1, 2, 3, 5, 63, 64, 65, 255, 257)
GUARD = 0xEE
REFUSED = O.S_BAD_DESC | O.S_TTL_EXPIRED


@pytest.fixture(scope="module")
def V():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vproxy_amd import vpcsum
    vpcsum.lib()
    return vpcsum


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


class Batches:
    """A batch's device-resident descriptors and entries per format, and the oracle's answer per
    (format, prefix length), each computed once and never changed."""

    def __init__(self, orc, b):
        self.orc, self.b = orc, b
        self._dev, self._want = {}, {}

    def tables(self, V, fmt):
        if fmt not in self._dev:
            self._dev[fmt] = (V.desc_to_tensor(self.b["desc"]), _dev(NV.entries(self.b["desc"], self.b["rw"], fmt)))
        return self._dev[fmt]

    def want(self, fmt, n=None):
        fmt = 0 if fmt == 2 else fmt   # the records carry 16-B IPv4 entries
        if (fmt, n) not in self._want:
            self._want[(fmt, n)] = NV.expect(self.orc, self.b["arena"], self.b["desc"], self.b["rw"], fmt, n)
        return self._want[(fmt, n)]


@pytest.fixture(scope="module")
def valid(orc):
    return Batches(orc, NV.batch())


@pytest.fixture(scope="module")
def wrong(orc, valid):
    return Batches(orc, NV.corrupted(valid.b))


def _run(V, S, fmt, mode, n, st_off=0, arena_off=0):
    """The first n packets of S through format fmt's call.  The arena is a view at byte offset
    arena_off into its allocation, the status one at st_off into a buffer of guard bytes; both
    allocations are returned whole after checking that nothing outside the views was written."""
    import torch
    a = S.b["arena"]
    abuf = torch.full((len(a) + 32,), GUARD, dtype=torch.uint8, device="cuda")
    arena = abuf[arena_off:arena_off + len(a)]
    arena.copy_(torch.from_numpy(a).pin_memory())
    assert arena.data_ptr() % 16 == arena_off
    sbuf = torch.full((n + 8,), GUARD, dtype=torch.uint8, device="cuda")
    st = sbuf[st_off:st_off + n]
    desc, ent = S.tables(V, fmt)
    if fmt == NB.FMT_NAT4:
        V.nat4(arena, desc, ent, n, st, mode)
    elif fmt == NB.FMT_NAT:
        V.nat(arena, desc, ent, n, st, mode)
    else:
        V.nat4r(arena, ent, n, st, mode)
    torch.cuda.synchronize()
    ab, sb = _host(abuf), _host(sbuf)
    assert (ab[:arena_off] == GUARD).all() and (ab[arena_off + len(a):] == GUARD).all(), "bytes around the arena written"
    assert (sb[:st_off] == GUARD).all() and (sb[st_off + n:] == GUARD).all(), "bytes around the status written"
    return ab[arena_off:arena_off + len(a)], sb[st_off:st_off + n]


def _check(V, S, build, n=None, st_off=0, arena_off=0):
    n_run = len(S.b["desc"]) if n is None else n
    got, st = _run(V, S, build.fmt, build.word(), n_run, st_off, arena_off)
    want, want_st = S.want(build.fmt, n)
    what = f"{build.id} n {n_run} status offset {st_off} arena offset {arena_off}"
    if not np.array_equal(got, want):
        pytest.fail(f"{what}: {NV.first_diff(S.b, got, want, build.fmt, build.ch or 6, arena_off)}")
    if build.strict:   # the recompute pass's status: the refusals are the oracle's
        st, want_st = st & REFUSED, want_st & REFUSED
    if not np.array_equal(st, want_st):
        i = int(np.nonzero(st != want_st)[0][0])
        pytest.fail(f"{what}: status {st[i]:#x}, oracle {want_st[i]:#x}: {NV.describe(S.b, i, build.fmt, build.ch or 6, arena_off)}")


@pytest.mark.parametrize("build", NB.BUILDS, ids=[b.id for b in NB.BUILDS])
def test_build_equals_oracle(V, valid, wrong, build):
    """One build on the geometry batch: the whole batch; its prefixes of n in PREFIXES (the batch
    tail: `p >= n` for a lane's later packets, the packed status store's last dword); the status
    a view at byte offsets 1..3 (the packed store's byte branch); the arena a view at byte offsets 1
    and 9 (the kernels address by absolute address, so every r0 shifts).  Strict builds also take
    the wrong-sum copy: Java recomputes, RFC 1624 would not."""
    for S in (valid, wrong) if build.strict else (valid,):
        _check(V, S, build)
        for n in PREFIXES:
            _check(V, S, build, n=n)
        for st_off in (1, 2, 3):
            _check(V, S, build, st_off=st_off)
        for arena_off in (1, 9):
            _check(V, S, build, arena_off=arena_off)


# ---- the grid-stride loop's second trip ----

@pytest.fixture(scope="module")
def cus(V):
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def strided(orc, cus):
    """W * CUs * 256 + 65 packets at the largest W, its oracle answers per format computed once; a
    smaller W takes a prefix (64-byte stride: no packet reaches into another's frame)."""
    S = Batches(orc, NV.strided(4 * cus * 256 + 65))
    return S


@pytest.mark.parametrize("fmt", [NB.FMT_NAT4, NB.FMT_NAT], ids=["fmt0", "fmt1"])
@pytest.mark.parametrize("family,w", NB.SECOND_TRIP, ids=[f"{f}-w{w}" for f, w in NB.SECOND_TRIP])
def test_loop_second_trip(V, strided, cus, fmt, family, w):
    """One workgroup per CU and W * CUs * 256 + 65 packets of 28..60 bytes at a 64-byte stride: the
    grid covers W * CUs * 256 packets per trip, so the first 65 lanes' packets come from a second
    trip through the loop, the last of them alone in its wave.  RFC 1624; arena and status whole."""
    import torch
    build = NB.Build(family, fmt, False, w, 0 if family == "nat" else 6, 1)
    assert build in NB.BUILDS
    n = w * cus * 256 + 65
    want, want_st = strided.want(fmt)
    desc, ent = strided.tables(V, fmt)
    arena = _dev(strided.b["arena"][:64 * n])
    st = torch.full((n,), GUARD, dtype=torch.uint8, device="cuda")
    (V.nat4 if fmt == NB.FMT_NAT4 else V.nat)(arena, desc, ent, n, st, build.word(wgs_per_cu=1))
    torch.cuda.synchronize()
    got, st = _host(arena), _host(st)
    bad = np.nonzero(st != want_st[:n])[0]
    assert not len(bad), (build.id, int(bad[0]), hex(st[bad[0]]), hex(want_st[bad[0]]))
    bad = np.nonzero(got != want[:64 * n])[0]
    assert not len(bad), (build.id, f"byte {int(bad[0]) % 64} of packet {int(bad[0]) // 64} of {n}")
    assert (want_st[n - 65:n] == O.S_DONE).sum() > 32 and not np.array_equal(got[-65 * 64:], strided.b["arena"][64 * (n - 65):64 * n])
