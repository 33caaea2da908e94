"""tests/k2vec.py held to its own claims without a GPU: every class of the geometry batch is there
for every K2 build of tests/csumbuilds.py, the C oracle and the pure-Python restatement agree on
every packet of it, the wrong-sums copy changes what it says, and the layouts for the loop and the
sampled paths meet the conditions the kernel's grid decisions need (kernels.hip k2_run: the sample,
`stage`, `wg`)."""
from collections import Counter

import numpy as np
import pytest

import csumbuilds as CB
import k2vec as K
from oracle import oracle as O

CUS = (256, 304)   # the MI355X's CU count and another one


@pytest.fixture(scope="module")
def b():
    return K.batch()


@pytest.fixture(scope="module")
def wrong(b):
    return K.corrupted(b)


@pytest.mark.parametrize("build", CB.K2_BUILDS, ids=[f"{x.team}x{x.u}-s{x.ts}x{x.us}" + "".join(
    t for t, on in (("-il", x.il), ("-rot", x.rot), ("-sf", x.sf), ("-wt", x.wt), ("-ds", x.ds), ("-win", x.win), ("-wgs", x.wgs)) if on)
    for x in CB.K2_BUILDS])
def test_check_classes(b, build):
    counts = K.check_classes(b, build)
    assert b["n"] % K.UNIT == 0 and counts["refused"] == 95 and counts["end16"] == 64


def test_plan_keys_cover_the_table(b):
    """Every K2 build's every cost class occurs in the batch, and the builds' shapes that
    second_trip runs are all the distinct ones."""
    for build in CB.K2_BUILDS:
        assert {p.key for p in K.plans(b, build)} == K.possible_keys(build), build
    shapes = {CB.build_of(r).shape for r in CB.ID_ROWS if r.family == "k2"}
    assert {CB.build_of(r).shape for r in CB.second_trip_rows()} == shapes and len(CB.second_trip_rows()) == len(shapes)


def test_oracle_equals_pure_python(orc, b, wrong):
    """On every live packet of the batch (and of its wrong-sums copy) the C oracle's words equal
    oracle.pure_process; raw ranges equal oracle.csum."""
    for S in (b, wrong):
        out, st, _ = K.expect(orc, S["arena"], S["desc"], O.MODE_COMPUTE)
        live = 0
        for i, d in enumerate(S["desc"]):
            p = K.plan(d, CB.DEFAULT_BUILD, len(S["arena"]))
            assert (st[i] == O.S_BAD_DESC) == p.bad, K.describe(S, i)
            if p.bad:
                assert out[i] == 0
                continue
            off, ln, fl = int(d["l3_off"]), int(d["l3_len"]), int(d["flags"])
            l3 = S["arena"][off:off + ln].tobytes()
            if p.raw:
                want = O.csum(l3)
            elif fl & O.F_PRE:
                want = 0
            else:
                ipc, l4c = O.pure_process(l3, O.L3Info(0, ln, int(d["l4_off"]), int(d["l3_ver"]), int(d["l4_proto"])), fl)
                want = ipc | (l4c << 16)
            assert out[i] == want and st[i] == O.S_DONE, K.describe(S, i)
            live += 1
        assert live > 5000


def test_valid_batch_verifies(orc, b):
    """The batch's stored sums are valid: verify finds every field it checks OK."""
    out, st, _ = K.expect(orc, b["arena"], b["desc"], O.MODE_VERIFY)
    P = K.plans(b, CB.DEFAULT_BUILD)
    for i, p in enumerate(P):
        if not p.bad and not p.raw:
            assert bool(st[i] & O.S_IP_OK) == p.do_ip and bool(st[i] & O.S_L4_OK) == p.do_l4, K.describe(b, i)
            assert not st[i] & O.S_UDP_NOCSUM
    # and writing changes nothing: the stored values are the computed ones
    _, _, after = K.expect(orc, b["arena"], b["desc"], O.MODE_COMPUTE, write=True)
    assert np.array_equal(after, b["arena"])


def test_corrupted_changes_what_it_says(orc, b, wrong):
    out0, st0, _ = K.expect(orc, b["arena"], b["desc"], O.MODE_VERIFY)
    out, st, _ = K.expect(orc, wrong["arena"], wrong["desc"], O.MODE_VERIFY)
    out0, st0, out, st = (x.astype(np.int64) for x in (out0, st0, out, st))
    kinds = wrong["kinds"]
    seen = Counter(kinds.values())
    assert set(seen) == set(K.CORRUPTIONS) and min(seen.values()) >= 20, seen
    P = K.plans(b, CB.DEFAULT_BUILD)
    for i in range(b["n"]):
        kind = kinds.get(i)
        if kind is None:
            assert out[i] == out0[i] and st[i] == st0[i], K.describe(b, i)
        elif kind == "ip":        # the IP field alone: not part of any sum
            assert out[i] == out0[i] and st[i] == st0[i] & ~O.S_IP_OK and st0[i] & O.S_IP_OK
        elif kind == "l4":        # the L4 field alone
            assert out[i] == out0[i] and st[i] & ~O.S_UDP_NOCSUM == st0[i] & ~O.S_L4_OK and st0[i] & O.S_L4_OK
        elif kind == "payload":   # the L4 sum moves, the stored field does not
            assert out[i] >> 16 != out0[i] >> 16 and out[i] & 0xFFFF == out0[i] & 0xFFFF and not st[i] & O.S_L4_OK
            assert st[i] & O.S_IP_OK == st0[i] & O.S_IP_OK
        elif kind == "udp0":
            assert out[i] == out0[i] and st[i] & O.S_UDP_NOCSUM and not st[i] & O.S_L4_OK
        else:                     # udp_zero: computes to 0, Java stores 0xffff, and that is what is stored
            assert out[i] >> 16 == 0xFFFF and st[i] & O.S_L4_OK and not st[i] & O.S_UDP_NOCSUM
    # a write over the wrong-sums copy repairs every field and changes nothing else
    _, _, after = K.expect(orc, wrong["arena"], wrong["desc"], O.MODE_COMPUTE, write=True)
    diff = np.nonzero(after != wrong["arena"])[0]
    assert len(diff) >= sum(seen[k] for k in ("ip", "l4", "payload", "udp0"))
    _, st2, _ = K.expect(orc, after, wrong["desc"], O.MODE_VERIFY)
    for i, p in enumerate(P):
        if not p.bad and not p.raw and not p.psonly:
            assert bool(st2[i] & O.S_IP_OK) == p.do_ip and bool(st2[i] & O.S_L4_OK) == p.do_l4, K.describe(b, i)


@pytest.mark.parametrize("cus", CUS)
def test_second_trip_layout(b, cus):
    L = K.second_trip(b, cus)
    assert L["n"] == cus * 256 + 256 + 65 == len(L["desc"]) and (cus * 256) % L["cycle"] != 0
    # the second trip's packets are not the first trip's: lane k of trip 2 differs from lane k of trip 1
    d = L["desc"]
    assert not np.array_equal(d[:321], d[cus * 256:cus * 256 + 321])
    assert int(d["l3_len"].max()) < 65535
    for i, kind in b["oob"].items():
        assert K.plan(b["desc"][i], CB.DEFAULT_BUILD, L["arena_len"]).bad


def _sample_lens(L):
    return L["desc"]["l3_len"][K.sampled(L["n"])].astype(int)


@pytest.mark.parametrize("cus", CUS)
def test_sorted_units_layout(b, cus):
    """The sample finds the batch mixed (not every packet of it at least 1 KiB, more than one sample
    class), the grid is the launch grid and larger than the low-concurrency one, the arena fits its
    n * 1024 bytes, and the composed workgroups are what their names say."""
    L = K.sorted_units(b, cus)
    n, d = L["n"], L["desc"]
    assert n == 2 * cus * 256 + 256 * L["G"] + 37 == len(d) and len(L["arena"]) <= L["arena_len"] == n * 1024
    assert -(-n // 256) > 2 * cus and -(-n // 256) <= 12 * cus       # sample taken; one unit per workgroup
    lens = _sample_lens(L)
    assert (lens < 1024).any() and len({K.sample_class(int(x)) for x in lens}) >= 2
    # frames of their own: no two live descriptors share a byte
    P = [K.plan(x, CB.DEFAULT_BUILD, L["arena_len"]) for x in d[:256 * L["G"]]]
    live = np.array([not p.bad and p.nch > 0 for p in P] + [False] * 0)
    off = d["l3_off"][:256 * L["G"]].astype(np.int64)[live]
    end = off + d["l3_len"][:256 * L["G"]].astype(np.int64)[live]
    order = np.argsort(off)
    assert np.all(off[order][1:] >= end[order][:-1])
    keys = np.array([p.key for p in P]).reshape(L["G"], 256)
    name = {c: g for g, c in enumerate(L["names"])}
    small = lambda g: int((keys[g] <= 1).sum())
    assert set(keys[name["one_large"]]) == {3} and set(keys[name["all_small"]]) == {1} and set(keys[name["all_bad"]]) == {0}
    for k in K.SORTED_NSMALL:
        g = name[f"n_small/{k}"]
        assert small(g) == k and set(keys[g][keys[g] > 1]) == {3}, k
    g = name["one_wave_class"]
    waves = keys[g].reshape(4, 64)
    assert [int((w == 4).sum() > 0) for w in waves] == [0, 0, 1, 0]
    for nit in range(1, 6):
        for r in range(8):
            g = name[f"tier/{nit}/{r}"]
            size = 256 - small(g)
            assert -(-size // 8) == nit and size % 8 == r and 15 not in keys[g], (nit, r)
    assert 15 in keys[name["slow_present"]] and 15 not in keys[name["slow_absent"]]
    assert set(keys[name["every_key"]]) == K.possible_keys(CB.DEFAULT_BUILD)
    # the tail: three waves of the last workgroup lie past the batch
    assert n % 256 == 37
    oob = K._oob_of(b, L["idx"])
    assert len(oob) > 100 and all(K.plan(d[j], CB.DEFAULT_BUILD, L["arena_len"]).bad for j in oob)


@pytest.mark.parametrize("cus", CUS)
def test_staged_layouts(b, cus):
    """Every sampled descriptor at least 1 KiB (the low-concurrency grid), the arena n * 1024 bytes,
    and the units per wave: below 4 W no staging; at 4 W exactly 4 units in every wave; at 8 W + 256
    * 5 + 37 some waves take a 9th unit after the full flush of kEsUnits = 8 and the others stop at 8
    (an empty last flush)."""
    W = 2 * cus * 256
    sizes = K.staged_sizes(cus)
    assert sizes == (4 * W - 1, 4 * W, 8 * W + 1317)
    for k, n in enumerate(sizes):
        L = K.staged(b, cus, k)
        assert L["n"] == n == len(L["desc"]) and L["arena_len"] == n * 1024 >= len(L["arena"])
        assert (_sample_lens(L) >= 1024).all()
        lens = L["desc"]["l3_len"].astype(int)
        assert (lens < 64).any() and (L["desc"]["flags"] & O.F_RAW).any()
        assert sum(K.plan(x, CB.DEFAULT_BUILD, L["arena_len"]).bad for x in L["desc"][:6200]) > 300
        assert (n // 4 >= W) == (k > 0)                              # k2_run's `stage`
        assert -(-n // 256) > 2 * cus                                 # the launch grid above the low one
    per = [K.units_per_wave(n, W) for n in sizes]
    waves = W // 64
    assert per[0] == {4: waves} and per[1] == {4: waves}
    assert per[2] == {9: 21, 8: waves - 21} and CB.ES_UNITS == 8
    assert sizes[0] % 64 == 63 and sizes[2] % 64 == 37               # partial last units


@pytest.mark.parametrize("cus", CUS)
def test_staged_window_layout(b, cus):
    L = K.staged_window(b, cus)
    W = 2 * cus * 256
    n = L["n"]
    assert n == 4 * W + 64 * 3 + 5 and L["arena_len"] == max(n * 1024, (4 << 30) + (128 << 10)) > CB.MAX_BUF_ARENA
    assert len(L["slab"]) <= 128 << 10 and L["base"] % 16 == 0
    assert L["base"] < L["line"] < L["base"] + len(L["slab"]) and L["base"] + len(L["slab"]) <= L["arena_len"]
    off = L["dev"]["l3_off"].astype(np.int64)
    assert np.array_equal(off - L["base"], L["rel"]["l3_off"].astype(np.int64))
    side = off >= L["line"]
    full = side[:n - n % 64].reshape(-1, 64)
    assert not full[:, 0].any() and (full.sum(axis=1) >= 31).all()  # every unit: lane 0 below, half above (pend != 0)
    assert (L["dev"]["l3_len"][K.sampled(n)] >= 1024).all()
    assert n // 4 >= W and K.units_per_wave(n, W)[5] == 4            # staged; four waves take a fifth unit
    # some packet that starts below the line reaches across it
    end = off + L["dev"]["l3_len"].astype(np.int64)
    assert ((off < L["line"]) & (end > L["line"])).any()
    # in range for the oracle (slab) exactly when in range for the device (arena)
    for d_rel, d_dev in zip(L["rel"][:512], L["dev"][:512]):
        assert K.plan(d_rel, CB.DEFAULT_BUILD, len(L["slab"])).bad == K.plan(d_dev, CB.DEFAULT_BUILD, L["arena_len"]).bad
