"""The pre-image geometry vectors (tests/prevec.py), the parts that need no GPU: every class the GPU
sweep (tests/test_gpu_pre_builds.py) relies on is in the batch, recomputed from the descriptors and
entries, and the expected bytes the sweep compares with -- Java's, from the C oracle -- equal a
pure-Python restatement of the kernel's arithmetic (pre_common.h:pre_sums) on every live packet."""
import numpy as np
import pytest

import natvec as NV
import prevec as PV
from oracle import oracle as O
from test_pre_cpu import _fold, _ld16, _words, rfc1624_from_pre


@pytest.fixture(scope="module")
def batch(orc):
    return PV.batch(orc)


def test_every_class_is_in_the_batch(batch):
    """act, ok, r0, need, wend and the second-round test recomputed from the descriptors and entries:
    every class count is the number built, both window limits are hit from both sides for 4- and
    6-chunk windows, the service grid's 383 / 384 / 385 triple, all 16 quad patterns, every kind of
    row on every lane mod 4."""
    size = PV.check_classes(batch)
    assert size and all(size.values()), size
    n = len(batch["desc"])
    assert n > 257 and n % NV.WAVE, "the batch ends in a partial wave past the largest prefix the sweep takes"
    alen = len(batch["after"])
    # which packets a `need` without the header-sum length would cut short (the sweep's mutation check)
    cut = [i for i in range(n) if PV.is_hsum(batch["pre"][i]) and PV.geometry(batch["desc"][i], batch["pre"][i], alen, 1, 6).wend
           and PV.hsum_hlen(batch["pre"][i]) > 20]
    assert len(cut) >= 200
    # ... and the packed frames do not overlap: a packet's expectation is its own
    spans = sorted((int(d["l3_off"]), int(d["l3_len"])) for d in batch["desc"] if int(d["l3_off"]) + int(d["l3_len"]) <= alen)
    assert all(o + ln <= o2 for (o, ln), (o2, _) in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] == alen


def model_sums(l3: bytes, d, entry):
    """(ip sum | None, L4 sum | None) of one live F_PRE packet as pre_common.h:pre_sums computes
    them: the IPv4 header summed in full; the L4 sum by RFC 1624 eqn. 3 from the stored field --
    test_pre_cpu.rfc1624_from_pre for a pre-image, for a header-sum record ~m = the complement of the
    recorded header sum, m' = the same words now, folded end-around -- and a UDP stored 0 summed in
    full."""
    fl, ver, proto, l4o, ln = int(d["flags"]), int(d["l3_ver"]), int(d["l4_proto"]), int(d["l4_off"]), int(d["l3_len"])
    ipc = l4c = None
    if fl & O.F_IP:
        ipc = 0xFFFF - _fold(sum(w for k, w in enumerate(_words(l3[:l4o])) if k != 5))
    if fl & O.F_L4:
        d0 = d.copy()
        d0["l3_off"] = 0
        hc = _ld16(l3, l4o + O.L4_FIELD[proto])
        if proto == 17 and hc == 0:
            l4c = O.l4_csum(l3, ln, l4o, ver, proto)
        elif PV.is_hsum(entry):
            rec = np.frombuffer(PV._raw(entry)[:8].tobytes(), O.HSUM_DTYPE)[0]
            now = _fold(sum(_words(O.hdr_words(l3, ver, l4o, int(rec["hlen"]), proto))))
            l4c = ~_fold((~hc & 0xFFFF) + _fold((~int(rec["sum"]) & 0xFFFF) + now)) & 0xFFFF
            l4c = 0xFFFF if proto == 17 and l4c == 0 else l4c
        else:
            l4c = rfc1624_from_pre(np.frombuffer(l3, np.uint8), d0, entry)
    return ipc, l4c


@pytest.mark.parametrize("fmt", [0, 1])
def test_model_equals_expected_bytes(batch, orc, fmt):
    """Every live packet of every class, none left out: the frame the flush receives with the
    model's sums in its two fields is the expected frame; every other byte of the expected arena is
    the received arena's.  Status and out words follow the rows' kinds."""
    e = PV.expect(batch, orc, fmt)
    desc, pre, after = batch["desc"], batch["pre"], batch["after"]
    model = after.copy()
    full = hs = 0
    for i in np.nonzero(e["live"])[0]:
        d = desc[i]
        o, ln, l4o = int(d["l3_off"]), int(d["l3_len"]), int(d["l4_off"])
        l3 = bytearray(after[o:o + ln].tobytes())
        ipc, l4c = model_sums(bytes(l3), d, pre[i])
        word = 0
        if ipc is not None:
            l3[10:12] = ipc.to_bytes(2, "big")
            word |= ipc
        if l4c is not None:
            f = l4o + O.L4_FIELD[int(d["l4_proto"])]
            full += d["l4_proto"] == 17 and l3[f:f + 2] == b"\x00\x00"
            hs += PV.is_hsum(pre[i])
            l3[f:f + 2] = l4c.to_bytes(2, "big")
            word |= l4c << 16
        assert bytes(l3) == e["arena"][o:o + ln].tobytes(), PV.describe(batch, i, fmt, 6)
        assert word == e["out"][i], PV.describe(batch, i, fmt, 6)
        model[o:o + ln] = np.frombuffer(bytes(l3), np.uint8)
    assert np.array_equal(model, e["arena"]), PV.first_diff(batch, model, e["arena"], fmt, 6)
    assert full >= 10 and hs >= (400 if fmt else 350), (full, hs)
    act, live = e["act"], e["live"]
    assert np.all(e["status"][live] == O.S_DONE) and np.all(e["status"][act & ~live] == O.S_BAD_DESC)
    assert np.all(e["status"][~act] == PV.GUARD) and np.all(e["out"][~act] == PV.OUT_GUARD) and np.all(e["out"][act & ~live] == 0)
    assert live.sum() > 1000 and (act & ~live).sum() >= 100 and (~act).sum() >= 200


def test_formats_agree_on_ipv4(batch, orc):
    """The 16-B entries' expectation is the 48-B entries' with the IPv6 rows refused and untouched."""
    e0, e1 = PV.expect(batch, orc, 0), PV.expect(batch, orc, 1)
    desc = batch["desc"]
    v6 = desc["l3_ver"] == 6
    assert np.array_equal(e0["live"][~v6], e1["live"][~v6]) and not e0["live"][v6].any() and e1["live"][v6].sum() > 100
    assert np.array_equal(e0["out"][~v6], e1["out"][~v6])
    for i in np.nonzero(v6)[0]:
        o = int(desc[i]["l3_off"])
        if o + int(desc[i]["l3_len"]) <= len(batch["after"]):
            assert np.array_equal(e0["arena"][o:o + int(desc[i]["l3_len"])], batch["after"][o:o + int(desc[i]["l3_len"])])


def test_prefix_expectations_are_prefixes(batch, orc):
    """The first n packets' flush is the whole batch's on those packets and nothing else."""
    full = PV.expect(batch, orc, 1)
    desc, after = batch["desc"], batch["after"]
    for n in (1, 65, 257):
        e = PV.expect(batch, orc, 1, n)
        assert np.array_equal(e["status"][:n], full["status"][:n]) and np.all(e["status"][n:] == PV.GUARD)
        assert np.array_equal(e["out"][:n], full["out"][:n]) and np.all(e["out"][n:] == PV.OUT_GUARD)
        mine = np.zeros(len(after), bool)
        for d in desc[:n]:
            o = int(d["l3_off"])
            if o + int(d["l3_len"]) <= len(after):
                mine[o:o + int(d["l3_len"])] = True
        assert np.array_equal(e["arena"][mine], full["arena"][mine]) and np.array_equal(e["arena"][~mine], after[~mine])


def test_entry_tables(batch):
    """The 16-B table keeps a pre-image's IPv4 fields and a header-sum record's 8 bytes and mask."""
    pre = batch["pre"]
    e4, e48 = PV.entries_array(pre, 0), PV.entries_array(pre, 1)
    assert e4.dtype == O.NAT4_DTYPE and e48.dtype == O.NAT_DTYPE and len(e4) == len(e48) == len(pre)
    raw4, raw48 = e4.view(np.uint8).reshape(-1, 16), e48.view(np.uint8).reshape(-1, 48)
    hs = (pre["mask"] & O.PRE_HSUM) != 0
    assert hs.sum() > 400 and np.array_equal(raw4[hs, :8], raw48[hs, :8]) and np.all(raw4[hs, 12] == O.PRE_HSUM)
    assert not raw4[hs, 8:12].any() and not raw4[hs, 13:].any()
    assert np.array_equal(raw4[~hs, :4], raw48[~hs, :4]) and np.array_equal(raw4[~hs, 4:8], raw48[~hs, 16:20])
    assert np.array_equal(raw4[~hs, 8:12], raw48[~hs, 32:36]) and np.array_equal(raw4[~hs, 12], raw48[~hs, 36])


def test_strided_pre_images(orc):
    """prevec.strided's numpy pre-images equal vswitch.record_pre_image's, packet by packet; its
    expectation is Java's on the rows it flags, the received frame elsewhere."""
    s = PV.strided(orc, 1500)
    want = PV.pre_images(s["before"], s["desc"], s["rw"])
    assert np.array_equal(s["pre"].view(np.uint8), want.view(np.uint8))
    flagged = s["desc"]["flags"] != 0
    assert 1000 < flagged.sum() < 1500 and np.all((s["desc"]["flags"][flagged] & O.F_PRE) != 0)
    A, W = s["after"].reshape(-1, 64), s["want"].reshape(-1, 64)
    assert np.array_equal(A[~flagged], W[~flagged]) and (A[flagged] != W[flagged]).any(axis=1).sum() > 900
