"""The NAT geometry vectors (tests/natvec.py), the parts that need no GPU: every class the GPU sweep
(tests/test_gpu_nat_builds.py) relies on is in the batch, recomputed from the descriptors, and the
C oracle the sweep compares with equals the pure-Python restatement of the rule on these vectors."""
import numpy as np
import pytest

import natvec as NV
from oracle import oracle as O


@pytest.fixture(scope="module")
def batch():
    return NV.batch()


def test_every_class_is_in_the_batch(batch, orc):
    """r0, need, wend and the tail recomputed from the descriptors: the 4- and 6-chunk window limits
    from both sides, waves with no / one / every packet past the second quad round's threshold,
    every kind of packet on every lane mod 4 of one wave, the three packet ends at every tail packed
    back to back, the sum edges and the masks."""
    size = NV.check_classes(batch, orc)
    assert size and all(size.values()), size
    n = len(batch["desc"])
    assert n > 257 and n % NV.WAVE, "the batch ends in a partial wave past the largest prefix the sweep takes"
    # which packets a window-limit or a store-width mistake would touch (the mutation check of the sweep)
    at_limit = {(fmt, ch): sum(1 for d in batch["desc"] if NV.geometry(d, len(batch["arena"]), fmt, ch)[3] == 16 * ch)
                for fmt, ch in ((0, 4), (0, 6), (1, 6))}
    assert at_limit[(0, 4)] >= 12 and at_limit[(1, 6)] >= 12 and at_limit[(0, 6)] == 0, at_limit
    ends = [i for i, d in enumerate(batch["desc"])
            if (g := NV.geometry(d, len(batch["arena"]), 1, 6))[3] and g[4] and g[3] == g[1] + int(d["l3_len"])]
    assert len(ends) >= 40, "window packets ending right after their L4 field on a tail of 1..3"


def test_wrong_sum_copy_differs_only_in_sums(batch):
    bad = NV.corrupted(batch)
    diff = np.nonzero(bad["arena"] != batch["arena"])[0]
    assert len(diff) > len(batch["desc"])
    allowed = set()
    for d in batch["desc"]:
        o, l4o, proto = int(d["l3_off"]), int(d["l4_off"]), int(d["l4_proto"])
        if o + int(d["l3_len"]) > len(batch["arena"]):
            continue
        allowed |= {o + 10, o + l4o + O.L4_FIELD[proto] + 1}
    assert set(diff.tolist()) <= allowed


@pytest.mark.parametrize("wrong", [False, True])
def test_c_oracle_equals_pure_restatement(batch, orc, wrong):
    """orc.nat_java / orc.nat4_java against oracle.nat_java_pure, packet by packet, on the valid
    and the wrong-sum batch: bytes and status; refused descriptors untouched."""
    b = NV.corrupted(batch) if wrong else batch
    arena, desc, rw = b["arena"], b["desc"], b["rw"]
    for fmt in (0, 1):
        want, st = NV.expect(orc, arena, desc, rw, fmt)
        pure = arena.copy()
        for i, d in enumerate(desc):
            ok = NV.desc_ok(d, len(arena), fmt)
            if not ok:
                assert st[i] == O.S_BAD_DESC, NV.describe(b, i, fmt, 6)
                continue
            o, ln = int(d["l3_off"]), int(d["l3_len"])
            l3 = bytearray(arena[o:o + ln].tobytes())
            s = O.nat_java_pure(l3, int(d["l3_ver"]), int(d["l4_proto"]), ln, int(d["l4_off"]), rw[i])
            assert s == st[i], NV.describe(b, i, fmt, 6)
            if s != O.S_DONE:
                assert bytes(l3) == arena[o:o + ln].tobytes()
            pure[o:o + ln] = np.frombuffer(bytes(l3), np.uint8)
        assert np.array_equal(pure, want), NV.first_diff(b, pure, want, fmt, 6)
        assert set(np.unique(st)) == {O.S_DONE, O.S_BAD_DESC, O.S_BAD_DESC | O.S_TTL_EXPIRED}


def test_strided_batch_has_valid_sums():
    """natvec.strided's numpy arithmetic against tcprwvec.l3_sums, packet by packet: valid IPv4
    header and L4 sums (but the UDP fields it zeroed), 28..60 bytes, every protocol, with and
    without an L4 field."""
    import tcprwvec as T
    s = NV.strided(1500)
    arena, desc = s["arena"], s["desc"]
    seen = set()
    for d in desc:
        o, ln, proto = int(d["l3_off"]), int(d["l3_len"]), int(d["l4_proto"])
        assert o % 64 == 0 and 28 <= ln <= 60 and d["l4_off"] == 20 and d["l3_ver"] == 4
        l3 = bytearray(arena[o:o + ln].tobytes())
        field = NV.l4sum(4, proto, ln, 20)
        zero = proto == 17 and l3[26:28] == b"\x00\x00"
        seen.add((proto, field, zero))
        want = T.l3_sums(l3, 4, proto, 20)
        if zero:
            want[26:28] = b"\x00\x00"
        assert want == l3, (o, ln, proto)
    assert seen == {(6, True, False), (6, False, False), (17, True, False), (17, True, True), (1, True, False)}
    assert set(desc["l3_len"]) == set(range(28, 61))


def test_prefix_expectations_are_prefixes(batch, orc):
    """The packets do not overlap, so the first n packets' rewrites are the whole batch's on those
    packets and nothing else (what the sweep's batch-tail cases compare with)."""
    arena, desc, rw = batch["arena"], batch["desc"], batch["rw"]
    full, st = NV.expect(orc, arena, desc, rw, 1)
    for n in (1, 65, 257):
        want, s = NV.expect(orc, arena, desc, rw, 1, n)
        assert np.array_equal(s, st[:n])
        mine = np.zeros(len(arena), bool)
        for d in desc[:n]:
            o = int(d["l3_off"])
            if o + int(d["l3_len"]) <= len(arena):
                mine[o:o + int(d["l3_len"])] = True
        assert np.array_equal(want[mine], full[mine]) and np.array_equal(want[~mine], arena[~mine])
