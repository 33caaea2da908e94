// launch_modes.h -- the internal tuning fields of the three mode words the C ABI takes (compute
// `mode`, `nat_mode`, pre-image `mode`), decoded once into the kernel build and grid shape the
// launchers run.  The one place that knows the bit layouts: api.cpp refuses what the accept masks
// below leave out, the launchers (kernels.hip, nat.hip) take the decoded structs and test no bit.
// None of these fields is part of the stable ABI (vpcsum.h documents VERIFY / WRITE and the two
// NAT mode bits only).  Pure host arithmetic, no HIP: tests/cpp/launch_modes_test.cpp compares it
// with a transcription of the ladders it replaced, with plain g++ under the sanitizers.
#pragma once
#include <stdint.h>

#include <initializer_list>
#include <type_traits>

#include "vpcsum.h"

namespace vpcsum {

// `bits` bits of a mode word from bit `lo` up
struct ModeField {
    int lo, bits;
    constexpr uint32_t mask() const { return ((1u << bits) - 1u) << lo; }
    constexpr uint32_t get(uint32_t word) const { return (word >> lo) & ((1u << bits) - 1u); }
    constexpr uint32_t put(uint32_t v) const { return (v << lo) & mask(); }
};
// no bit of a word has two meanings
constexpr bool disjoint(std::initializer_list<uint32_t> masks) {
    uint32_t seen = 0;
    for (uint32_t m : masks) {
        if (seen & m) return false;
        seen |= m;
    }
    return true;
}

constexpr int kNatChunks = 6;     // 16-B chunks of the NAT / pre-image kernels' window: 96 B
constexpr int kNatWideLog2 = 1;   // packets per lane and iteration of k_natw / k_natq: 2
// NAT and pre-image grids: 24 workgroups per CU (4 resident at 101 VGPRs, so the grid-stride loop
// starts in six dispatch rounds): +2.6% over 8 on 10M C5 packets, 12 and 16 in between
// (profiles/r03e_nat_grid/)
constexpr uint32_t kNatWgsPerCu = 24;

// ---- compute mode (vpcsum_compute_async) -------------------------------------------------------
namespace csum_bits {
constexpr ModeField kVariantLo{8, 5};    // kernel variant id, bits 0..4 (launch_csum's switch; 0: default)
constexpr uint32_t kPlainLoads = 1u << 13;   // plain (temporal) loads instead of non-temporal ones
constexpr uint32_t kNoAdapt = 1u << 14;      // K2 without the sampled low-concurrency and dense-frame grids
constexpr ModeField kWgsPerCu{16, 8};    // grid: workgroups per CU (0: each launcher's default)
constexpr ModeField kVariantHi{24, 3};   // kernel variant id, bits 5..7
constexpr uint32_t kIgnored = 0xeeu;     // bits 1..3 and 5..7: let through, read by nobody
static_assert(disjoint({VPCSUM_MODE_VERIFY, VPCSUM_MODE_WRITE, kIgnored, kVariantLo.mask(), kPlainLoads, kNoAdapt,
                        kWgsPerCu.mask(), kVariantHi.mask()}), "compute mode fields overlap");
}  // namespace csum_bits
constexpr uint32_t kCsumModeAccept = VPCSUM_MODE_VERIFY | VPCSUM_MODE_WRITE | csum_bits::kIgnored |
                                     csum_bits::kVariantLo.mask() | csum_bits::kPlainLoads | csum_bits::kNoAdapt |
                                     csum_bits::kWgsPerCu.mask() | csum_bits::kVariantHi.mask();

struct CsumTune {
    int variant = 0;           // launch_csum's kernel variant id, 0..255
    bool nt = true;            // non-temporal packet loads
    bool adapt = true;         // K2 picks its grid by packet size (low-concurrency sample, dense frames)
    uint32_t wgs_per_cu = 0;   // 0: the launcher's own grid
};
constexpr CsumTune csum_tune(uint32_t mode) {
    using namespace csum_bits;
    return {(int)(kVariantLo.get(mode) | (kVariantHi.get(mode) << kVariantLo.bits)), !(mode & kPlainLoads),
            !(mode & kNoAdapt), kWgsPerCu.get(mode)};
}

// ---- nat_mode (vpcsum_nat*_async, VPCSUM_NAT_PROBE_TUNE) ---------------------------------------
namespace nat_bits {
constexpr uint32_t kBytePath = 1u << 8;    // the byte-access kernel (k_nat)
constexpr ModeField kPktsPerLane{12, 3};   // log2(packets per lane) + 1; 0: kNatWideLog2; above 3: as 3
constexpr ModeField kChunks{16, 2};        // window chunks; 1: 6, 2: 4 (not for 48-B entries), else kNatChunks
constexpr ModeField kWgsPerCu{18, 5};      // grid: workgroups per CU (0: kNatWgsPerCu)
constexpr uint32_t kLaneLayout = 1u << 23; // the lane layout (k_natw) instead of quads (k_natq)
constexpr ModeField kOccupancy{24, 2};     // k_natq's forced occupancy; 1: 6, 2: 8 waves per SIMD (tuning
                                           // shapes that may spill, tests/test_kernel_resources.py exempts
                                           // them); 0 and 3: the default
static_assert(disjoint({VPCSUM_NAT_STRICT_JAVA, VPCSUM_NAT_TCP_REWRITES, kBytePath, kPktsPerLane.mask(), kChunks.mask(),
                        kWgsPerCu.mask(), kLaneLayout, kOccupancy.mask()}), "nat_mode fields overlap");
}  // namespace nat_bits
constexpr uint32_t kNatModeAccept = VPCSUM_NAT_STRICT_JAVA | VPCSUM_NAT_TCP_REWRITES | nat_bits::kBytePath |
                                    nat_bits::kPktsPerLane.mask() | nat_bits::kChunks.mask() |
                                    nat_bits::kWgsPerCu.mask() | nat_bits::kLaneLayout | nat_bits::kOccupancy.mask();
// the context's NAT batches (vpcsum_ctx_nat_submit) take the byte path as their only tuning bit
constexpr uint32_t kNatCtxModeAccept = VPCSUM_NAT_STRICT_JAVA | VPCSUM_NAT_TCP_REWRITES | nat_bits::kBytePath;

enum class NatFamily : int { Byte, Lane, Quad };   // k_nat, k_natw, k_natq
// One NAT kernel build and its grid shape.  fmt 0: vpcsum_nat4_t entries, 1: vpcsum_nat_t, 2:
// vpcsum_nat4_rec_t records.  The byte kernel is built per format only: it takes `strict` as an
// argument and has no window (w 1, ch 0).
struct NatBuild {
    NatFamily family;
    int fmt;
    bool strict;           // VPCSUM_NAT_STRICT_JAVA: rewrite only, store Java's dirty flags
    int w;                 // packets per lane and iteration
    int ch;                // window chunks
    int wpe;               // amdgpu_waves_per_eu of k_natq (1: the compiler's own)
    bool probe;            // the memory operations without the rewrite (tooling)
    uint32_t wgs_per_cu;   // nat_grid's cap
    int wl2;               // nat_grid's log2(packets per lane): as asked for, also where w was clamped
};

// Which builds exist (the launchers instantiate these and no others): what a request outside them
// resolves to is nat_build's / nat_probe_build's / pre_build's business.
//   quads: 1 or 2 packets per lane; 4-chunk windows except for 48-B entries; records know no
//   strict mode; any of the three occupancies.  Probes: 2 packets, RFC 1624, default occupancy,
//   4-chunk windows for 16-B entries only.
constexpr bool natq_exists(int fmt, bool strict, int w, int ch, int wpe, bool probe) {
    if (fmt < 0 || fmt > 2 || (ch != 4 && ch != kNatChunks) || (wpe != 1 && wpe != 6 && wpe != 8)) return false;
    if (probe) return !strict && w == 2 && wpe == 1 && (ch == kNatChunks || fmt == 0);
    return (w == 1 || w == 2) && !(strict && fmt == 2) && !(ch == 4 && fmt == 1);
}
//   lane layout: 1, 2 or 4 packets per lane at the default window; 4-chunk windows only for 16-B
//   entries in RFC 1624 mode, at 2 or 4 packets.  Probes: 2 packets, RFC 1624, entries only.
constexpr bool natw_exists(int fmt, bool strict, int w, int ch, bool probe) {
    if (fmt < 0 || fmt > 2 || (ch != 4 && ch != kNatChunks)) return false;
    if (probe) return !strict && w == 2 && fmt != 2 && (ch == kNatChunks || fmt == 0);
    if (ch == 4) return fmt == 0 && !strict && (w == 2 || w == 4);
    return (w == 1 || w == 2 || w == 4) && !(strict && fmt == 2);
}

constexpr NatBuild nat_build(uint32_t nat_mode, int fmt) {
    using namespace nat_bits;
    const uint32_t wsel = kPktsPerLane.get(nat_mode);
    const int wl2 = wsel ? (wsel > 3 ? 2 : (int)wsel - 1) : kNatWideLog2;
    const uint32_t wgs = kWgsPerCu.get(nat_mode) ? kWgsPerCu.get(nat_mode) : kNatWgsPerCu;
    const bool strict = (nat_mode & VPCSUM_NAT_STRICT_JAVA) && fmt != 2;   // records: RFC 1624 only
    const bool ch4 = kChunks.get(nat_mode) == 2 && fmt != 1;
    if (nat_mode & kBytePath) return {NatFamily::Byte, fmt, strict, 1, 0, 1, false, wgs, wl2};
    if (nat_mode & kLaneLayout) {
        // 4-chunk windows: 16-B entries in RFC 1624 mode only, and not at 1 packet per lane (runs at 2)
        if (ch4 && fmt == 0 && !strict) return {NatFamily::Lane, fmt, strict, wl2 == 2 ? 4 : 2, 4, 1, false, wgs, wl2};
        return {NatFamily::Lane, fmt, strict, 1 << wl2, kNatChunks, 1, false, wgs, wl2};
    }
    const uint32_t occ = kOccupancy.get(nat_mode);
    // k_natq takes 1 or 2 packets per lane: a request for 4 runs at 2
    return {NatFamily::Quad, fmt, strict, wl2 == 0 ? 1 : 2, ch4 ? 4 : kNatChunks, occ == 1 ? 6 : occ == 2 ? 8 : 1,
            false, wgs, wl2};
}

// The pattern probes (vpcsum_nat4_pattern_probe_async, vpcsum_nat4r_pattern_probe_async) take the
// layout, window and grid fields of a nat_mode word from VPCSUM_NAT_PROBE_TUNE, to price the shapes
// launch_nat can take.  The lane layout has no probe for records: it runs the 48-B entries' one.
constexpr NatBuild nat_probe_build(uint32_t tune, int fmt) {
    using namespace nat_bits;
    const bool lane = (tune & kLaneLayout) != 0;
    const uint32_t wgs = kWgsPerCu.get(tune) ? kWgsPerCu.get(tune) : kNatWgsPerCu;
    return {lane ? NatFamily::Lane : NatFamily::Quad, lane && fmt == 2 ? 1 : fmt, false, 1 << kNatWideLog2,
            kChunks.get(tune) == 2 && fmt == 0 ? 4 : kNatChunks, 1, true, wgs, kNatWideLog2};
}

// ---- pre-image mode (vpcsum_pre_async) ---------------------------------------------------------
namespace pre_bits {
constexpr uint32_t kBytePath = 1u << 8;    // byte accesses on the frames
constexpr ModeField kPktsPerLane{12, 2};   // 2: two packets per lane; else one (C5 +0.9% over two,
                                           // profiles/r05d_presweep.json)
constexpr ModeField kChunks{16, 2};        // 2: 4-chunk windows (16-B entries only)
constexpr ModeField kWgsPerCu{18, 5};      // grid: workgroups per CU (0: kNatWgsPerCu)
constexpr uint32_t kProbe = 1u << 23;      // the memory-pattern probe (16-B entries only): the same loads
                                           // and stores, the stored sums written back unchanged
constexpr uint32_t kNtStore = 1u << 24;    // non-temporal field stores (A/B)
static_assert(disjoint({VPCSUM_MODE_WRITE, kBytePath, kPktsPerLane.mask(), kChunks.mask(), kWgsPerCu.mask(), kProbe,
                        kNtStore}), "pre-image mode fields overlap");
}  // namespace pre_bits
constexpr uint32_t kPreModeAccept = VPCSUM_MODE_WRITE | pre_bits::kBytePath | pre_bits::kPktsPerLane.mask() |
                                    pre_bits::kChunks.mask() | pre_bits::kWgsPerCu.mask() | pre_bits::kProbe |
                                    pre_bits::kNtStore;

// One k_pre build, its three run-time switches and its grid shape.  fmt 0: vpcsum_pre4_t, 1: vpcsum_pre_t.
struct PreBuild {
    int fmt;
    int w;                 // packets per lane
    int ch;                // window chunks
    bool probe;
    int write;             // VPCSUM_MODE_WRITE: the sums into the frames
    int byte_path;
    int nt_store;
    uint32_t wgs_per_cu;   // nat_grid's cap
    int wl2;               // nat_grid's log2(packets per lane): as asked for, the probe runs at 2 regardless
};
// 1 or 2 packets per lane; 4-chunk windows and the probe (2 packets) for 16-B entries only
constexpr bool pre_exists(int fmt, int w, int ch, bool probe) {
    if (fmt < 0 || fmt > 1 || (w != 1 && w != 2) || (ch != 4 && ch != kNatChunks)) return false;
    return fmt == 0 ? (!probe || w == 2) : (!probe && ch == kNatChunks);
}
constexpr PreBuild pre_build(uint32_t mode, int fmt) {
    using namespace pre_bits;
    const int wl2 = kPktsPerLane.get(mode) == 2 ? 1 : 0;
    const bool probe = (mode & kProbe) && fmt == 0;
    return {fmt, probe ? 2 : 1 << wl2, kChunks.get(mode) == 2 && fmt == 0 ? 4 : kNatChunks, probe,
            (mode & VPCSUM_MODE_WRITE) ? 1 : 0, (mode & kBytePath) ? 1 : 0, (mode & kNtStore) ? 1 : 0,
            kWgsPerCu.get(mode) ? kWgsPerCu.get(mode) : kNatWgsPerCu, wl2};
}

// ---- run-time values to template arguments -----------------------------------------------------
// dispatch(f, v1, Among<T1, ...>{}, v2, Among<T2, ...>{}, ...) returns f(std::integral_constant<T1, v1>{},
// std::integral_constant<T2, v2>{}, ...), or false when a value is not among its candidates.  f is
// instantiated for the whole cross product: a launcher guards its kernel with `if constexpr
// (..._exists(...))` and returns false otherwise, so that only the builds listed above are compiled
// and a build outside them is an error, not a launch that did not happen.
template <class T, T... Vs>
struct Among {};
using AmongBool = Among<bool, false, true>;

template <class F>
bool dispatch(F&& f) {
    return f();
}
template <class F, class T, T... Vs, class... Rest>
bool dispatch(F&& f, T v, Among<T, Vs...>, Rest... rest) {
    return ((v == Vs && dispatch([&](auto... cs) { return f(std::integral_constant<T, Vs>{}, cs...); }, rest...)) || ...);
}
// the candidates of the NAT and pre-image kernels' template arguments
using NatFmts = Among<int, 0, 1, 2>;
using PreFmts = Among<int, 0, 1>;
using NatwPkts = Among<int, 1, 2, 4>;
using NatqPkts = Among<int, 1, 2>;
using NatWindows = Among<int, 4, kNatChunks>;
using NatqOccupancies = Among<int, 1, 6, 8>;

}  // namespace vpcsum
