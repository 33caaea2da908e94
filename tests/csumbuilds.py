"""One row per checksum kernel build that launch_csum (vproxy_amd/csrc/kernels.hip) can run (test
infrastructure: tests/ only).

launch_csum's switch takes a compute variant id (launch_modes.h csum_tune: bits 8..12 and 24..26 of
the compute mode word) and runs a team kernel build (k_csum<TEAM, U, VERIFY, NT, PRED>) or a K2
build (k_csum_d<TEAM, U, TS, US, VERIFY, NT, WPE, IL, ROT, SF, WT, DS, WIN, WGS>); VERIFY and NT are
picked per batch (the mode's VERIFY bit, the kPlainLoads bit).  The table below names every id of
the switch once with the template arguments it resolves to, and the four builds ids 0 / 70 pick
between by the arena (K2Dense, K2Staged, K2DenseWin, K2StagedWin) as rows without an id.
tests/test_kernel_resources.py holds the table against the compiled code object on the CPU: the
k_csum_d and k_csum kernels in it are exactly the table's distinct builds x VERIFY x NT (a K2 row
also instantiates its team fallback, launch_d's k_csum<TEAM, U> for arenas it cannot address).
tests/test_gpu_csum_builds.py runs every row against the oracle.
"""
from __future__ import annotations

from collections import namedtuple

# csum_bits of launch_modes.h, as (lowest bit, bits) / single bits
VARIANT_LO = (8, 5)             # kVariantLo: variant id bits 0..4
PLAIN_LOADS = 1 << 13           # kPlainLoads: NT = false
NO_ADAPT = 1 << 14              # kNoAdapt: no sampled low-concurrency / dense-frame grid
WGS_PER_CU = (16, 8)            # kWgsPerCu: the grid's workgroups per CU
VARIANT_HI = (24, 3)            # kVariantHi: variant id bits 5..7

# kernels.hip: kDefaultTeam, kDefaultUnroll, kSmallTeam, kSmallUnroll, kDefaultRot, kEsUnits
DEFAULT_TEAM, DEFAULT_UNROLL, SMALL_TEAM, SMALL_UNROLL, DEFAULT_ROT, ES_UNITS = 8, 6, 2, 2, -9, 8
MAX_BUF_ARENA = 0xFFFF0000      # device_common.h kMaxBufArena


def _put(field, v: int) -> int:
    lo, bits = field
    assert 0 <= v < (1 << bits)
    return v << lo


def word(variant: int = 0, plain_loads: bool = False, no_adapt: bool = False, wgs_per_cu: int = 0) -> int:
    """The tuning fields of a compute mode word, field by field (the VERIFY / WRITE bits are the
    caller's)."""
    return _put(VARIANT_LO, variant & 0x1F) | _put(VARIANT_HI, variant >> 5) | (PLAIN_LOADS if plain_loads else 0) | \
        (NO_ADAPT if no_adapt else 0) | _put(WGS_PER_CU, wgs_per_cu)


class K2(namedtuple("K2", "team u ts us wpe il rot sf wt ds win wgs")):
    """k2_run's template arguments as K2Build spells them (VERIFY and NT left to the batch)."""

    def kernel(self, verify: bool, nt: bool) -> tuple:
        """k_csum_d's template argument list for this build."""
        return (self.team, self.u, self.ts, self.us, verify, nt, self.wpe, self.il, self.rot, self.sf, self.wt, self.ds,
                self.win, self.wgs)

    @property
    def shape(self) -> tuple:
        return (self.team, self.u, self.ts, self.il, self.ds, self.wgs)


class Team(namedtuple("Team", "team u pred")):
    """k_csum's template arguments but VERIFY and NT."""

    def kernel(self, verify: bool, nt: bool) -> tuple:
        return (self.team, self.u, verify, nt, self.pred)


def k2(team, u, ts=0, us=1, wpe=1, il=0, rot=0, sf=False, wt=False, ds=False, win=False, wgs=False) -> K2:
    return K2(team, u, ts, us, wpe, il, rot, sf, wt, ds, win, wgs)


def k2_default(sf, wt, ds, win, wgs) -> K2:
    """K2Default<SF, WT, DS, WIN, WGS>"""
    return K2(DEFAULT_TEAM, DEFAULT_UNROLL, SMALL_TEAM, SMALL_UNROLL, 1, 0, DEFAULT_ROT, sf, wt, ds, win, wgs)


K2_DENSE = k2_default(True, False, False, False, False)
K2_STAGED = k2_default(True, False, True, False, True)
K2_DENSE_WIN = k2_default(True, False, False, True, False)
K2_STAGED_WIN = k2_default(True, False, True, True, False)
K2_NO_WINDOW_UNITS = k2_default(False, False, False, False, False)
K2_STAGED_UNSORTED = k2_default(True, False, True, False, False)
K2_WT_AB = k2_default(True, True, False, False, False)


class Row(namedtuple("Row", "id name family build")):
    """id None: a build ids 0 / 70 dispatch to; build None: an id that dispatches by the arena."""

    @property
    def label(self) -> str:
        return f"{'x' if self.id is None else self.id}-{self.name}"

    def word(self, plain_loads: bool = False, no_adapt: bool = False, wgs_per_cu: int = 0) -> int:
        return word(self.id, plain_loads, no_adapt, wgs_per_cu)


def _table():
    t = [Row(0, "default", "k2", None)]
    for i, (team, u) in {2: (4, 4), 3: (8, 4), 4: (16, 8), 5: (32, 4), 6: (64, 4), 7: (4, 8), 8: (8, 6), 9: (8, 12),
                         10: (16, 4), 11: (8, 8)}.items():
        t.append(Row(i, f"team{team}x{u}", "team", Team(team, u, False)))
    t.append(Row(12, "zerocopy64x4", "zerocopy", Team(64, 4, True)))
    for i, b in {40: k2(8, 6), 41: k2(4, 12), 43: k2(16, 6), 45: k2(2, 12), 46: k2(8, 6, 2, 4), 47: k2(8, 6, 1, 4),
                 48: k2(8, 8, 2, 4), 49: k2(8, 6, 4, 4), 50: k2(8, 6, 2, 2), 54: k2(8, 4, 2, 2), 58: k2(8, 12, 2, 2),
                 62: k2(8, 6, 2, 2, 1, 1), 66: k2(8, 6, 2, 2, 1, 0, 1)}.items():
        t.append(Row(i, f"k2-{b.team}x{b.u}-s{b.ts}x{b.us}-il{b.il}-rot{b.rot}", "k2", b))
    t += [Row(70, "default70", "k2", None),
          Row(72, "K2NoWindowUnits", "k2", K2_NO_WINDOW_UNITS),
          Row(74, "K2WtAB", "k2", K2_WT_AB),
          Row(76, "K2NoStaging", "k2", K2_DENSE),
          Row(78, "team8x6-ab", "team", Team(DEFAULT_TEAM, DEFAULT_UNROLL, False)),
          Row(79, "K2StagedUnsorted", "k2", K2_STAGED_UNSORTED),
          Row(84, "K2Staged", "k2", K2_STAGED),
          Row(None, "K2Dense", "k2", K2_DENSE),
          Row(None, "K2Staged", "k2", K2_STAGED),
          Row(None, "K2DenseWin", "k2", K2_DENSE_WIN),
          Row(None, "K2StagedWin", "k2", K2_STAGED_WIN)]
    return t


ROWS = _table()
IDS = sorted(r.id for r in ROWS if r.id is not None)
ID_ROWS = [r for r in ROWS if r.id is not None]
K2_BUILDS = sorted({r.build for r in ROWS if r.family == "k2" and r.build is not None})
# what ids 0 / 70 run on a 16-B aligned arena of at most MAX_BUF_ARENA bytes that is not dense
DEFAULT_BUILD = K2_STAGED


def build_of(row: Row) -> K2 | Team:
    """The build a row runs on the tests' geometry batch (not dense, below 4 GiB, aligned)."""
    return DEFAULT_BUILD if row.build is None else row.build


def team_builds() -> set:
    """Every k_csum build: the team rows, and launch_d's fallback of each K2 row."""
    s = {r.build for r in ROWS if r.family in ("team", "zerocopy")}
    return s | {Team(b.team, b.u, False) for b in K2_BUILDS}


def kernel_set() -> tuple[set, set]:
    """(k_csum_d argument lists, k_csum argument lists) of the builds x VERIFY x NT."""
    vn = [(v, n) for v in (False, True) for n in (False, True)]
    return ({b.kernel(v, n) for b in K2_BUILDS for v, n in vn}, {b.kernel(v, n) for b in team_builds() for v, n in vn})


# one row per distinct (TEAM, U, TS, IL, DS, WGS) among the rows with an id: the loop's second trip
def second_trip_rows() -> list:
    seen, rows = set(), []
    for r in ID_ROWS:
        b = build_of(r)
        if r.family == "k2" and b.shape not in seen:
            seen.add(b.shape)
            rows.append(r)
    return rows
