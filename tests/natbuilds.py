"""One canonical nat_mode tuning word per NAT rewrite kernel build (test infrastructure: tests/ only).

vproxy_amd/csrc/launch_modes.h lists the builds (natq_exists, natw_exists, the byte kernel per
format) and decodes a nat_mode word into one of them (nat_build).  The table below names every
non-probe build once per entry format, with a word put together from the named fields of
launch_modes.h's nat_bits.  tests/test_lib_cpu.py holds it against the header on the CPU: each word
resolves to the build it stands next to, and the table is exactly the header's list -- a build
added there without a word here fails without a GPU.  tests/test_gpu_nat_builds.py runs every
entry against the oracle.
"""
from __future__ import annotations

from collections import namedtuple

# nat_bits of launch_modes.h, as (lowest bit, bits) / single bits
STRICT_JAVA = 1 << 0            # VPCSUM_NAT_STRICT_JAVA (include/vpcsum.h)
BYTE_PATH = 1 << 8              # kBytePath: the byte-access kernel k_nat
PKTS_PER_LANE = (12, 3)         # kPktsPerLane: log2(packets per lane) + 1
CHUNKS = (16, 2)                # kChunks: 1: 6-chunk windows, 2: 4-chunk windows
WGS_PER_CU = (18, 5)            # kWgsPerCu: the grid's workgroups per CU
LANE_LAYOUT = 1 << 23           # kLaneLayout: k_natw instead of the quads k_natq
OCCUPANCY = (24, 2)             # kOccupancy: 1: 6, 2: 8 waves per SIMD asked of k_natq

PKTS_SEL = {1: 1, 2: 2, 4: 3}   # packets per lane -> selector
CHUNKS_SEL = {6: 1, 4: 2}       # window chunks -> selector
OCC_SEL = {1: 0, 6: 1, 8: 2}    # waves per EU -> selector

FMT_NAT4, FMT_NAT, FMT_NAT4R = 0, 1, 2   # vpcsum_nat4_t, vpcsum_nat_t, vpcsum_nat4_rec_t
FAMILIES = ("nat", "natw", "natq")       # NatFamily Byte, Lane, Quad: k_nat, k_natw, k_natq


def _put(field, v: int) -> int:
    lo, bits = field
    assert 0 <= v < (1 << bits)
    return v << lo


def word(family: str, strict: bool = False, w: int = 1, ch: int = 6, wpe: int = 1, wgs_per_cu: int = 0) -> int:
    """The nat_mode word of a build, field by field (the mode bit STRICT_JAVA included)."""
    m = (STRICT_JAVA if strict else 0) | _put(PKTS_PER_LANE, PKTS_SEL[w]) | _put(WGS_PER_CU, wgs_per_cu)
    if family == "nat":
        return m | BYTE_PATH
    m |= _put(CHUNKS, CHUNKS_SEL[ch])
    if family == "natw":
        return m | LANE_LAYOUT
    return m | _put(OCCUPANCY, OCC_SEL[wpe])


class Build(namedtuple("Build", "family fmt strict w ch wpe")):
    """(family, fmt, strict, w, ch, wpe) as launch_modes.h's NatBuild has them; the byte kernel: w 1,
    ch 0, wpe 1."""

    @property
    def id(self) -> str:
        return f"{self.family}-fmt{self.fmt}-{'strict' if self.strict else 'rfc'}-w{self.w}-ch{self.ch}-wpe{self.wpe}"

    def word(self, wgs_per_cu: int = 0) -> int:
        return word(self.family, self.strict, self.w, self.ch or 6, self.wpe, wgs_per_cu)

    @property
    def key(self) -> tuple:
        """The tuple tests/cpp/launch_modes_test.cpp prints for this build."""
        return (FAMILIES.index(self.family), self.fmt, int(self.strict), self.w, self.ch, self.wpe)


def _table():
    t = []
    for fmt in (FMT_NAT4, FMT_NAT, FMT_NAT4R):
        for strict in ((False,) if fmt == FMT_NAT4R else (False, True)):   # records: RFC 1624 only
            t.append(Build("nat", fmt, strict, 1, 0, 1))
            for w in (1, 2, 4):
                t.append(Build("natw", fmt, strict, w, 6, 1))
            if fmt == FMT_NAT4 and not strict:   # the lane layout's 4-chunk windows
                t += [Build("natw", fmt, strict, w, 4, 1) for w in (2, 4)]
            for w in (1, 2):
                for ch in ((6,) if fmt == FMT_NAT else (6, 4)):   # 48-B entries: 6-chunk windows only
                    t += [Build("natq", fmt, strict, w, ch, wpe) for wpe in (1, 6, 8)]
    return t


BUILDS = _table()
COUNT_BY_FMT = {FMT_NAT4: 34, FMT_NAT: 20, FMT_NAT4R: 16}   # launch_modes.h today: 70 builds

# the loop's second trip: one build per kernel family and packets-per-lane value
SECOND_TRIP = [("nat", 1), ("natw", 1), ("natw", 2), ("natw", 4), ("natq", 1), ("natq", 2)]
