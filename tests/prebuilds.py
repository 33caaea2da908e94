"""One canonical pre-image `mode` tuning word per k_pre build (test infrastructure: tests/ only).

vproxy_amd/csrc/launch_modes.h lists the builds of the pre-image flush kernel (pre_exists) and
decodes a vpcsum_pre_async mode word into one of them and its three run-time switches (pre_build).
The table below names every build once per entry format, with a word put together from the named
fields of launch_modes.h's pre_bits, as tests/natbuilds.py does for the NAT rewrite kernels.
tests/test_lib_cpu.py holds it against the header on the CPU: each word resolves to the build it
stands next to, and the table is exactly the header's list -- a build added there without a word
here fails without a GPU.  tests/test_gpu_pre_builds.py runs every entry against the oracle.
"""
from __future__ import annotations

from collections import namedtuple

# pre_bits of launch_modes.h, as (lowest bit, bits) / single bits
MODE_WRITE = 1 << 4             # VPCSUM_MODE_WRITE (include/vpcsum.h): the sums into the frames
BYTE_PATH = 1 << 8              # kBytePath: byte accesses on the frames
PKTS_PER_LANE = (12, 2)         # kPktsPerLane: 2: two packets per lane, else one
CHUNKS = (16, 2)                # kChunks: 2: 4-chunk windows (16-B entries only)
WGS_PER_CU = (18, 5)            # kWgsPerCu: the grid's workgroups per CU
PROBE = 1 << 23                 # kProbe: the memory-pattern probe (16-B entries only)
NT_STORE = 1 << 24              # kNtStore: non-temporal field stores

PKTS_SEL = {1: 1, 2: 2}         # packets per lane -> selector
CHUNKS_SEL = {6: 1, 4: 2}       # window chunks -> selector

FMT_PRE4, FMT_PRE = 0, 1        # vpcsum_pre4_t (16 B, IPv4), vpcsum_pre_t (48 B)

# the run-time switches of every build (PreBuild write / byte_path / nt_store): an axis of their own
SWITCHES = {"write": MODE_WRITE, "byte_path": BYTE_PATH, "nt_store": NT_STORE}


def _put(field, v: int) -> int:
    lo, bits = field
    assert 0 <= v < (1 << bits)
    return v << lo


def word(w: int = 1, ch: int = 6, probe: bool = False, wgs_per_cu: int = 0, switches=()) -> int:
    """The mode word of a build, field by field, with the named run-time switches on."""
    m = _put(PKTS_PER_LANE, PKTS_SEL[w]) | _put(CHUNKS, CHUNKS_SEL[ch]) | _put(WGS_PER_CU, wgs_per_cu)
    m |= PROBE if probe else 0
    for s in switches:
        m |= SWITCHES[s]
    return m


class Build(namedtuple("Build", "fmt w ch probe")):
    """(fmt, w, ch, probe) as launch_modes.h's PreBuild has them."""

    @property
    def id(self) -> str:
        return f"pre-fmt{self.fmt}-w{self.w}-ch{self.ch}" + ("-probe" if self.probe else "")

    def word(self, wgs_per_cu: int = 0, switches=()) -> int:
        return word(self.w, self.ch, self.probe, wgs_per_cu, switches)

    @property
    def key(self) -> tuple:
        """The tuple tests/cpp/launch_modes_test.cpp prints for this build."""
        return (self.fmt, self.w, self.ch, int(self.probe))


def _table():
    t = []
    for fmt in (FMT_PRE4, FMT_PRE):
        for w in (1, 2):
            for ch in ((6, 4) if fmt == FMT_PRE4 else (6,)):   # 4-chunk windows: 16-B entries only
                t.append(Build(fmt, w, ch, False))
    t += [Build(FMT_PRE4, 2, ch, True) for ch in (6, 4)]        # the probes: 16-B entries, 2 packets
    return t


BUILDS = _table()
LIVE = [b for b in BUILDS if not b.probe]
PROBES = [b for b in BUILDS if b.probe]
COUNT_BY_FMT = {FMT_PRE4: 6, FMT_PRE: 2}   # launch_modes.h today: 8 builds

# the switch settings each non-probe build runs under (test_gpu_pre_builds.py)
RUNS = (("write",), (), ("write", "byte_path"), ("write", "nt_store"))

# the loop's second trip: packets per lane, both formats
SECOND_TRIP = [(fmt, w) for fmt in (FMT_PRE4, FMT_PRE) for w in (1, 2)]
