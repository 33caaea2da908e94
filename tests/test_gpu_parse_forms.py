"""The frame parse in every form against the geometry batch (tests/parsevec.py, held to its edges by
tests/test_parse_vectors_cpu.py): k_parse_ether launched through the device API (plain, with flow
tuples, with header sums) and through the context's frame entries, and svc_frame_packet on the
service grid (verify, verify with header sums, egress, parse only).  Descriptors, status bytes,
tuples, header sums, out words and -- for egress -- the whole arena are compared byte for byte with
what the oracle's restatements give; every output starts as 0xAB and carries guard rows past n (two on
the host, a wave's worth on the device); the copies to and from the device go through pinned memory."""
import ctypes

import numpy as np
import pytest

import parsevec as PV
from oracle import oracle as O

pytestmark = pytest.mark.gpu

AB = 0xAB
GUARD_ROWS = 64    # device outputs: a wave's worth, so that a store past n by any lane of the last wave is seen
PREFIXES = (1, 63, 64, 65, 255, 256, 257)
SLICES = (1, 2, 3, 4, 5, 64, 511, 512)      # inline descriptors, one workgroup, a wave's worth, the largest
SERVICE_US = 20000
_KEEP = []   # page-locked once and kept for the life of the process


@pytest.fixture(scope="module")
def V():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from vproxy_amd import vpcsum
    vpcsum.lib()
    assert vpcsum.TUPLE_DTYPE == PV.TUPLE_DTYPE and vpcsum.HSUM_DTYPE == O.HSUM_DTYPE
    return vpcsum


@pytest.fixture(scope="module")
def B():
    return PV.batch()


def dev(a):
    """Host to device through pinned memory, as the other GPU tests copy (a copy first: the batch's
    arrays are read-only)."""
    import torch
    return torch.from_numpy(np.array(a).view(np.uint8).reshape(-1)).pin_memory().cuda()


def host(t):
    """Device to host through pinned memory."""
    import torch
    h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    h.copy_(t)
    torch.cuda.synchronize()
    return h.numpy().copy()


def rows(a, width):
    return np.ascontiguousarray(a).view(np.uint8).reshape(-1, width)


def same(got, want, B, what, lo=0):
    """got == want row by row (both as bytes); the first rows that differ are named by class and case."""
    g, w = rows(got, got.dtype.itemsize), rows(want, want.dtype.itemsize)
    assert g.shape == w.shape, (what, g.shape, w.shape)
    bad = np.flatnonzero((g != w).any(axis=1))
    assert not len(bad), (what, len(bad), [(int(i) + lo, B["cls"][i + lo], B["case"][i + lo], bytes(g[i]).hex(), bytes(w[i]).hex())
                                           for i in bad[:4]])


@pytest.fixture(scope="module")
def W(B, orc):
    """What the context's forms must give for the whole batch: the oracle's verify of the oracle's
    descriptors (refused frames: S_BAD_DESC, out 0), and its egress write-back with each frame's own
    flags (refused, or a flag that cannot be honoured: S_BAD_DESC, out 0, no byte written)."""
    acc = B["status"] == 0
    vout, vst = orc.process(B["arena"], B["desc"], O.MODE_VERIFY)
    vout[~acc], vst[~acc] = 0, O.S_BAD_DESC
    after = B["arena"].copy()
    eout, est = orc.process(after, PV.egress_desc(B), O.MODE_COMPUTE, write=True)
    eout[~B["eg_ok"]], est[~B["eg_ok"]] = 0, O.S_BAD_DESC
    assert (est[B["eg_ok"]] == O.S_DONE).all() and not np.array_equal(after, B["arena"])
    return dict(vout=vout, vst=vst, eout=eout, est=est, after=after)


# ------------------------------------------------------------------------------------------
# launched, device API
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def D(V, B):
    """The batch on the device: the arena at byte offsets 0, 1 and 9 of larger tensors (the physical
    residue of every frame differs from its offset), the frame table."""
    import torch
    views = {}
    for shift in (0, 1, 9):
        big = torch.full((B["arena"].nbytes + 64,), 0x5C, dtype=torch.uint8, device="cuda")
        assert big.data_ptr() % 16 == 0
        big[shift:shift + B["arena"].nbytes] = dev(B["arena"])
        views[shift] = (big, big[shift:shift + B["arena"].nbytes])
    torch.cuda.synchronize()
    return dict(views=views, off=dev(B["frame_off"]), len=dev(B["frame_len"]))


def launched(V, D, n, form, flags=O.F_IP | O.F_L4, status=True, shift=0, arena_len=None):
    """One launch of k_parse_ether through the device API: (desc, status, tuples, hsum) of the
    first n frames, each None where the form has none."""
    import torch
    arena = D["views"][shift][1]
    if arena_len is not None:
        arena = arena[:arena_len]
    d = torch.full(((n + GUARD_ROWS) * 16,), AB, dtype=torch.uint8, device="cuda")
    st = torch.full((n + GUARD_ROWS,), AB, dtype=torch.uint8, device="cuda")
    tu = hs = None
    if form == "tuples":   # based at a 4-byte, not 8-byte aligned address
        buf = torch.full(((n + GUARD_ROWS) * 40 + 16,), AB, dtype=torch.uint8, device="cuda")
        tu = buf[4:4 + (n + GUARD_ROWS) * 40]
        assert tu.data_ptr() % 8 == 4
    if form == "hsum":
        hs = torch.full(((n + GUARD_ROWS) * 8,), AB, dtype=torch.uint8, device="cuda")
    V.parse_ether(arena, D["off"], D["len"], n, d, st if status else None, flags=flags, tuples=tu, hsum=hs)
    torch.cuda.synchronize()
    d, st = host(d), host(st)
    assert (d[n * 16:] == AB).all() and (st[n:] == AB).all(), "a store past n"
    if not status:
        assert (st == AB).all()
    if tu is not None:
        assert (host(buf)[:4] == AB).all()
        tu = host(tu)
        assert (tu[n * 40:] == AB).all(), "a tuple stored past n"
        tu = tu[:n * 40].view(PV.TUPLE_DTYPE)
    if hs is not None:
        hs = host(hs)
        assert (hs[n * 8:] == AB).all(), "a header sum stored past n"
        hs = hs[:n * 8].view(O.HSUM_DTYPE)
    return d[:n * 16].view(O.DESC_DTYPE), st[:n] if status else None, tu, hs


def check_launched(B, got, n, want_desc=None, what=""):
    d, st, tu, hs = got
    same(d, (B["desc"] if want_desc is None else want_desc)[:n], B, f"{what} descriptors")
    if st is not None:
        same(st, B["status"][:n], B, f"{what} status")
    if tu is not None:
        same(tu, B["tuples"][:n], B, f"{what} tuples")
    if hs is not None:
        same(hs, B["hsum"][:n], B, f"{what} header sums")


@pytest.mark.parametrize("status", [True, False])
@pytest.mark.parametrize("flags", [0, O.F_IP, O.F_L4, O.F_IP | O.F_L4, O.F_L4P, O.F_IP | O.F_L4 | O.F_L4P])
def test_launched_plain(V, B, D, flags, status):
    n = len(B["cls"])
    check_launched(B, launched(V, D, n, "plain", flags, status), n, PV.ingress_desc(B, flags), f"flags {flags:#x}")


def test_launched_forms_agree(V, B, D):
    """Plain, with tuples and with header sums: each against the oracle, the descriptors of the three equal."""
    n = len(B["cls"])
    got = {form: launched(V, D, n, form) for form in ("plain", "tuples", "hsum")}
    for form, g in got.items():
        check_launched(B, g, n, what=form)
    assert got["plain"][0].tobytes() == got["tuples"][0].tobytes() == got["hsum"][0].tobytes()
    assert got["tuples"][2]["l3_ver"].any() and got["hsum"][3]["l2_len"].any()


@pytest.mark.parametrize("n", PREFIXES)
def test_launched_prefixes(V, B, D, n):
    """A batch that ends inside a wave, on one and just past one: the last, partial wave's tuple
    exchange and the guard rows past n."""
    for form in ("plain", "tuples", "hsum"):
        check_launched(B, launched(V, D, n, form), n, what=f"{form} n={n}")


@pytest.mark.parametrize("shift", [1, 9])
def test_launched_arena_views(V, B, D, shift):
    n = len(B["cls"])
    assert D["views"][shift][1].data_ptr() % 16 == shift
    for form in ("plain", "tuples", "hsum"):
        check_launched(B, launched(V, D, n, form, shift=shift), n, what=f"{form} arena +{shift}")
    big, view = D["views"][shift]
    got = host(big)
    assert (got[:shift] == 0x5C).all() and (got[shift + view.numel():] == 0x5C).all()
    assert np.array_equal(got[shift:shift + view.numel()], B["arena"])


@pytest.mark.parametrize("shift", [0, 9])
def test_launched_arena_ends_on_a_deep_frame(V, B, D, shift):
    """The arena cut behind the deep frame: o + L == arena_len for a frame whose headers reach byte 380."""
    n = B["cut_n"]
    for form in ("plain", "tuples", "hsum"):
        got = launched(V, D, n, form, shift=shift, arena_len=B["cut_len"])
        check_launched(B, got, n, what=f"{form} cut arena +{shift}")
        assert got[1][n - 1] == 0 and got[0][n - 1]["l4_off"] == 303
    # and cut one byte shorter the frame is refused
    got = launched(V, D, n, "tuples", shift=shift, arena_len=B["cut_len"] - 1)
    assert got[1][n - 1] == O.S_BAD_DESC and not rows(got[0][n - 1:], 16).any() and not rows(got[2][n - 1:], 40).any()
    same(got[0][:n - 1], B["desc"][:n - 1], B, "one byte shorter")


# ------------------------------------------------------------------------------------------
# the context: a registered arena, launched and on the service grid
# ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def C(V, B):
    """One context for the module, the batch's arena (page-aligned, so a frame's address residue
    is its offset's) registered once."""
    raw = np.zeros(B["arena"].nbytes + 8192, np.uint8)
    _KEEP.append(raw)
    skip = (-raw.ctypes.data) % 4096
    arena = raw[skip:skip + B["arena"].nbytes]
    arena[:] = B["arena"]
    assert arena.ctypes.data % 4096 == 0
    ctx = V.Context(0, max_arena=arena.nbytes, max_pkts=len(B["cls"]) + GUARD_ROWS)
    ctx.register(arena)
    yield dict(ctx=ctx, arena=arena)
    ctx.close()


def frames_call(V, C, B, form, lo, hi, arena=None, want_out=True):
    """One call of a context frame entry for frames [lo, hi): {out, st, desc, tu, hs} (those the form
    has), outputs prefilled with 0xAB and checked for two untouched guard rows."""
    ctx, arena = C["ctx"], C["arena"] if arena is None else arena
    n = hi - lo
    fo, fl = np.ascontiguousarray(B["frame_off"][lo:hi]), np.ascontiguousarray(B["frame_len"][lo:hi])
    ff = np.ascontiguousarray(B["fwant"][lo:hi])
    out, st = np.full(n + 2, 0xABABABAB, np.uint32), np.full(n + 2, AB, np.uint8)
    desc, tu, hs = np.full((n + 2) * 16, AB, np.uint8), np.full((n + 2) * 40, AB, np.uint8), np.full((n + 2) * 8, AB, np.uint8)
    t = ctypes.c_uint64()
    L, a = V.lib(), (ctx.h, arena.ctypes.data, arena.nbytes, fo.ctypes.data, fl.ctypes.data)
    po = out.ctypes.data if want_out else None
    if form == "verify":
        rc = L.vpcsum_ctx_verify_frames(*a, n, po, st.ctypes.data, ctypes.byref(t))
    elif form == "verify_hsum":
        rc = L.vpcsum_ctx_verify_frames_hsum(*a, n, po, st.ctypes.data, hs.ctypes.data, ctypes.byref(t))
    elif form == "parse":
        rc = L.vpcsum_ctx_parse_frames(*a, n, desc.ctypes.data, st.ctypes.data, tu.ctypes.data, ctypes.byref(t))
    else:
        rc = L.vpcsum_ctx_egress_frames(*a, ff.ctypes.data, n, po, st.ctypes.data, ctypes.byref(t))
    V._check(rc, form)
    ctx.wait(t.value)
    assert (out[n:] == 0xABABABAB).all() and (st[n:] == AB).all() and (desc[n * 16:] == AB).all() and \
        (tu[n * 40:] == AB).all() and (hs[n * 8:] == AB).all(), f"{form}: a result stored past n"
    r = dict(st=st[:n])
    if form != "parse":
        if want_out:
            r["out"] = out[:n]
        else:
            assert (out == 0xABABABAB).all()
    if form == "verify_hsum":
        r["hs"] = hs[:n * 8].view(O.HSUM_DTYPE)
    if form == "parse":
        r["desc"], r["tu"] = desc[:n * 16].view(O.DESC_DTYPE), tu[:n * 40].view(PV.TUPLE_DTYPE)
    return r


def walk(V, C, B, form, sizes, want_out=True):
    """The whole batch through one form in consecutive calls of the given sizes (cycled); the
    results joined, and the number of calls."""
    n, lo, k, parts = len(B["cls"]), 0, 0, []
    while lo < n:
        hi = min(lo + sizes[k % len(sizes)], n)
        parts.append(frames_call(V, C, B, form, lo, hi, want_out=want_out))
        lo, k = hi, k + 1
    return {key: np.concatenate([p[key] for p in parts]) for key in parts[0]}, k


def check_form(B, W, form, r, lo=0, hi=None, what=""):
    hi = len(B["cls"]) if hi is None else hi
    what = f"{what} {form}"
    if form in ("verify", "verify_hsum"):
        same(r["st"], W["vst"][lo:hi], B, f"{what} status", lo)
        if "out" in r:
            same(r["out"], W["vout"][lo:hi], B, f"{what} out", lo)
        if form == "verify_hsum":
            same(r["hs"], B["hsum"][lo:hi], B, f"{what} header sums", lo)
    elif form == "parse":
        same(r["desc"], B["desc"][lo:hi], B, f"{what} descriptors", lo)
        same(r["st"], B["status"][lo:hi], B, f"{what} status", lo)
        same(r["tu"], B["tuples"][lo:hi], B, f"{what} tuples", lo)
    else:
        same(r["st"], W["est"][lo:hi], B, f"{what} status", lo)
        same(r["out"], W["eout"][lo:hi], B, f"{what} out", lo)


def arena_is(got, want, B, what):
    """The arena `got` equals `want` byte for byte; the first frame that differs is named."""
    if np.array_equal(got, want):
        return
    k = int(np.flatnonzero(got != want)[0])
    idx = np.flatnonzero(B["inb"])
    offs = B["frame_off"][idx].astype(np.int64)
    order = np.argsort(offs, kind="stable")
    j = int(idx[order[max(int(np.searchsorted(offs[order], k, side="right")) - 1, 0)]])
    raise AssertionError((what, f"byte {k}: {got[k]:#x} != {want[k]:#x}", j, B["cls"][j], B["case"][j]))


FORMS = [("verify", True), ("verify", False), ("verify_hsum", False), ("parse", True), ("egress", True)]


@pytest.fixture(scope="module")
def ref(V, C, B):
    """ref(form, want_out): the form launched -- one call of the whole batch with the service off --
    as (results, the arena afterwards); run once per module.  What the service grid's results must
    equal byte for byte."""
    done = {}

    def get(form, want_out):
        if (form, want_out) not in done:
            ctx = C["ctx"]
            ctx.set_service(0)
            before = ctx.stats()["service_batches"]
            C["arena"][:] = B["arena"]
            r = frames_call(V, C, B, form, 0, len(B["cls"]), want_out=want_out)
            assert ctx.stats()["service_batches"] == before
            done[form, want_out] = (r, C["arena"].copy())
            C["arena"][:] = B["arena"]
        return done[form, want_out]
    return get


@pytest.mark.parametrize("form,want_out", FORMS)
def test_ctx_launched(B, W, ref, form, want_out):
    """Each frame entry launched (the whole batch is past the service grid's 512): against the
    oracle, and the arena afterwards the oracle's write-back (egress) or untouched."""
    r, after = ref(form, want_out)
    check_form(B, W, form, r, what="launched")
    arena_is(after, W["after"] if form == "egress" else B["arena"], B, f"launched {form}")


@pytest.mark.parametrize("form,want_out", FORMS)
def test_ctx_service_slices(V, C, B, W, ref, form, want_out):
    """The whole batch through the service grid in calls of 1, 2, 3 (the inline descriptors), 4 (one
    workgroup), 5, 64, 511 and 512 frames: every call is a service batch, the results equal the
    oracle's and the launched ones, and after an egress walk the whole arena is the oracle's
    write-back -- refused frames and every guard byte untouched."""
    ctx = C["ctx"]
    launched_r, _ = ref(form, want_out)
    C["arena"][:] = B["arena"]
    ctx.set_service(SERVICE_US)
    try:
        before = ctx.stats()["service_batches"]
        r, calls = walk(V, C, B, form, SLICES, want_out)
        assert ctx.stats()["service_batches"] == before + calls and calls >= 3 * len(SLICES)
        check_form(B, W, form, r, what="service")
        for key, v in launched_r.items():
            assert r[key].tobytes() == v.tobytes(), (form, key)
        arena_is(C["arena"], W["after"] if form == "egress" else B["arena"], B, f"service {form}")
    finally:
        ctx.set_service(0)
        C["arena"][:] = B["arena"]


def test_ctx_service_sizes_shifted(V, C, B, W):
    """The same walk with the slice sizes in another order, so that other frames meet the inline
    slots, the one-workgroup batches and the 511 / 512 edge; parse only."""
    ctx = C["ctx"]
    ctx.set_service(SERVICE_US)
    try:
        for sizes in ((512, 511, 4, 3, 2, 1, 64, 5), (3, 512, 1, 511, 2, 4)):
            before = ctx.stats()["service_batches"]
            r, calls = walk(V, C, B, "parse", sizes)
            assert ctx.stats()["service_batches"] == before + calls
            check_form(B, W, "parse", r, what=f"service {sizes[:2]}")
    finally:
        ctx.set_service(0)
    arena_is(C["arena"], B["arena"], B, "parse")


@pytest.mark.parametrize("form", ["verify", "verify_hsum", "parse", "egress"])
def test_ctx_513_frames_are_launched(V, C, B, W, form):
    """512 frames are the service grid's largest batch; 513 are launched.  Same frames, same results."""
    ctx = C["ctx"]
    lo = 64 * 22 + 1000          # past the bounds waves, inside rules@r
    C["arena"][:] = B["arena"]
    ctx.set_service(SERVICE_US)
    try:
        s0 = ctx.stats()["service_batches"]
        a = frames_call(V, C, B, form, lo, lo + 512)
        assert ctx.stats()["service_batches"] == s0 + 1
        C["arena"][:] = B["arena"]
        b = frames_call(V, C, B, form, lo, lo + 513)
        assert ctx.stats()["service_batches"] == s0 + 1
        check_form(B, W, form, a, lo, lo + 512, "512")
        check_form(B, W, form, b, lo, lo + 513, "513")
        for key in a:
            assert a[key].tobytes() == b[key][:512].tobytes(), key
    finally:
        ctx.set_service(0)
        C["arena"][:] = B["arena"]


def test_ctx_service_forms_back_to_back(V, C, B, W):
    """Consecutive service batches of different forms reuse the aux buffer (header sums, then
    descriptors and tuples) and the inline slots: verify then parse, egress then verify, over deep
    and bounds frames, in batches of 3 (inline) and 200."""
    ctx = C["ctx"]
    deep = B["cls"].index("deep")
    C["arena"][:] = B["arena"]
    ctx.set_service(SERVICE_US)
    try:
        s0, calls, written = ctx.stats()["service_batches"], 0, 0
        for lo, m in ((0, 3), (0, 200), (deep, 3), (deep + 7, 200), (len(B["cls"]) - 200, 200)):
            for first, second in (("verify_hsum", "parse"), ("parse", "verify_hsum"), ("verify", "parse")):
                a = frames_call(V, C, B, first, lo, lo + m, want_out=first == "verify")
                b = frames_call(V, C, B, second, lo + 1, lo + m)      # a batch of its own, one frame on
                check_form(B, W, first, a, lo, lo + m, "first")
                check_form(B, W, second, b, lo + 1, lo + m, "second")
                calls += 2
            # egress writes the frames; the verify behind it sees the written sums
            e = frames_call(V, C, B, "egress", lo, lo + m)
            check_form(B, W, "egress", e, lo, lo + m, "egress first")
            v = frames_call(V, C, B, "verify", lo, lo + m)
            calls += 2
            ok = B["eg_ok"][lo:lo + m]
            fl = PV.egress_desc(B)["flags"][lo:lo + m]
            want_ok = np.where(fl & O.F_IP, O.S_IP_OK, 0) | np.where(fl & O.F_L4, O.S_L4_OK, 0)
            full = ok & ((fl & O.F_L4P) == 0) & (fl == B["desc"]["flags"][lo:lo + m])   # every sum the verify checks was written
            assert ((v["st"][full] & (O.S_IP_OK | O.S_L4_OK)) == want_ok[full]).all()
            written += int(full.sum())
            C["arena"][:] = B["arena"]
        assert ctx.stats()["service_batches"] == s0 + calls and written > 100
    finally:
        ctx.set_service(0)
        C["arena"][:] = B["arena"]


@pytest.mark.parametrize("service", [False, True])
def test_ctx_arena_ends_on_a_deep_frame(V, C, B, W, service):
    """The arena cut behind the deep frame (a view of the registered range): its last frame ends on
    the arena's last byte, parsed, verified with its header sum and written, launched and on the
    service grid."""
    ctx, n = C["ctx"], B["cut_n"]
    cut = C["arena"][:B["cut_len"]]
    lo = n - 100 if service else 0
    C["arena"][:] = B["arena"]
    ctx.set_service(SERVICE_US if service else 0)
    try:
        s0 = ctx.stats()["service_batches"]
        for form in ("parse", "verify_hsum", "verify", "egress"):
            r = frames_call(V, C, B, form, lo, n, arena=cut)
            check_form(B, W, form, r, lo, n, f"cut arena, service {service}")
            assert r["st"][-1] != O.S_BAD_DESC
        assert ctx.stats()["service_batches"] == s0 + (4 if service else 0)
        want = W["after"].copy()
        if lo:     # the frames before lo were not in the flush
            want[:int(B["frame_off"][lo])] = B["arena"][:int(B["frame_off"][lo])]
        want[B["cut_len"]:] = B["arena"][B["cut_len"]:]
        arena_is(C["arena"], want, B, "cut arena")
        C["arena"][:] = B["arena"]
        r = frames_call(V, C, B, "parse", n - 1, n, arena=C["arena"][:B["cut_len"] - 1])     # one byte shorter: refused
        assert r["st"][0] == O.S_BAD_DESC and not rows(r["desc"], 16).any() and not rows(r["tu"], 40).any()
    finally:
        ctx.set_service(0)
        C["arena"][:] = B["arena"]
