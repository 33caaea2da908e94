// The mode-word decoders of vproxy_amd/csrc/launch_modes.h against the launch ladders they replaced.
// spec_* below transcribe those ladders (launch_nat, launch_nat_probe, launch_pre, nat_chunks_sel,
// nat_wgs_per_cu of nat.hip, team_from_mode and the grid arithmetic of api.cpp, launch_csum's bit
// tests) as they stood, hex literals and all: they are the specification, launch_modes.h the code
// under test.  Every combination of the bits a decoder reads is compared, then the builds the
// decoders can reach against the builds the launchers instantiate (*_exists over the dispatchers'
// candidate lists).  Stand-alone, plain g++ under ASan / UBSan; prints the build counts, which
// tests/test_lib_cpu.py compares with the kernels in the code object.
//
// `launch_modes_test builds [FMT:WORD ...]` instead lists the NAT rewrite builds the launchers
// instantiate (probes left out) and the build nat_build() resolves each given nat_mode word to, for
// tests/test_lib_cpu.py to hold tests/natbuilds.py against.  `launch_modes_test prebuilds [FMT:WORD ...]`
// does the same for the k_pre builds (probes included) and pre_build(), for tests/prebuilds.py.
#include <errno.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <set>
#include <string>
#include <tuple>
#include <vector>

#include "launch_modes.h"

using namespace vpcsum;

static int g_fail = 0;
#define CHECK(c, ...)                                                  \
    do {                                                               \
        if (!(c)) {                                                    \
            if (g_fail++ < 20) {                                       \
                printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #c);     \
                printf(__VA_ARGS__);                                   \
                printf("\n");                                          \
            }                                                          \
        }                                                              \
    } while (0)

// family (0 byte, 1 lane, 2 quad), FMT, STRICT, W, CH, WPE, PROBE.  The byte kernel has neither W,
// CH nor WPE: 1, 0, 1 by launch_modes.h's convention; its STRICT is the argument it is launched with.
using Build = std::tuple<int, int, int, int, int, int, int>;
struct Spec {
    Build b;
    int wl2;
    uint32_t wgs;
};
constexpr int kCh = 6;   // the parent's kNatChunks

static int spec_chunks_sel(uint32_t nat_mode, int fmt) {
    const uint32_t c = (nat_mode >> 16) & 3u;
    if (c == 1) return 6;
    if (c == 2 && fmt != 1) return 4;
    return kCh;
}
static uint32_t spec_wgs_per_cu(uint32_t nat_mode) {
    const uint32_t w = (nat_mode >> 18) & 31u;
    return w ? w : 24u;
}

static Spec spec_nat(uint32_t nat_mode, int fmt) {
    const bool strict = (nat_mode & 0x01u) != 0;
    const int wsel = (int)((nat_mode >> 12) & 7u);
    const int wl2 = wsel ? (wsel - 1 > 2 ? 2 : wsel - 1) : 1;
    const int ch = spec_chunks_sel(nat_mode, fmt);
    const bool wide = !(nat_mode & 0x100u);
    const bool quad = (nat_mode & 0x800000u) == 0;
    Build b;
    if (wide && quad) {
        const uint32_t wpe_sel = (nat_mode >> 24) & 3u;
        const int wpe = wpe_sel == 1 ? 6 : wpe_sel == 2 ? 8 : 1;
        const int w = wl2 == 0 ? 1 : 2;
        if (fmt == 2) b = Build{2, 2, 0, w, ch == 4 ? 4 : kCh, wpe, 0};
        else if (fmt == 0 && ch == 4) b = Build{2, 0, strict, w, 4, wpe, 0};
        else if (fmt == 0) b = Build{2, 0, strict, w, kCh, wpe, 0};
        else b = Build{2, 1, strict, w, kCh, wpe, 0};
    } else if (wide) {
        const int w = wl2 == 0 ? 1 : wl2 == 1 ? 2 : 4;
        if (fmt == 2) b = Build{1, 2, 0, w, kCh, 1, 0};
        else if (fmt == 0 && !strict && ch == 4) b = Build{1, 0, 0, wl2 == 2 ? 4 : 2, 4, 1, 0};
        else if (fmt == 0) b = Build{1, 0, strict, w, kCh, 1, 0};
        else b = Build{1, 1, strict, w, kCh, 1, 0};
    } else if (fmt == 2) {
        b = Build{0, 2, 0, 1, 0, 1, 0};
    } else if (fmt == 0) {
        b = Build{0, 0, strict ? 1 : 0, 1, 0, 1, 0};
    } else {
        b = Build{0, 1, strict ? 1 : 0, 1, 0, 1, 0};
    }
    return {b, wl2, spec_wgs_per_cu(nat_mode)};
}

static Spec spec_nat_probe(uint32_t tune, int fmt) {
    Build b;
    if (!(tune & 0x800000u)) {
        if (fmt == 2) b = Build{2, 2, 0, 2, kCh, 1, 1};
        else if (fmt == 0 && spec_chunks_sel(tune, 0) == 4) b = Build{2, 0, 0, 2, 4, 1, 1};
        else if (fmt == 0) b = Build{2, 0, 0, 2, kCh, 1, 1};
        else b = Build{2, 1, 0, 2, kCh, 1, 1};
    } else if (fmt == 0 && spec_chunks_sel(tune, 0) == 4)
        b = Build{1, 0, 0, 2, 4, 1, 1};
    else if (fmt == 0)
        b = Build{1, 0, 0, 2, kCh, 1, 1};
    else
        b = Build{1, 1, 0, 2, kCh, 1, 1};
    return {b, 1, spec_wgs_per_cu(tune)};
}

// FMT, W, CH, PROBE
using PreKey = std::tuple<int, int, int, int>;
struct PreSpec {
    PreKey b;
    int write, byte_path, nt_store, wl2;
    uint32_t wgs;
};
static PreSpec spec_pre(uint32_t mode, int fmt) {
    const int write = (mode & 0x10u) ? 1 : 0;
    const int byte_path = (mode & 0x100u) ? 1 : 0;
    const int w1 = ((mode >> 12) & 3u) != 2;
    const bool ch4 = ((mode >> 16) & 3u) == 2 && fmt == 0;
    const bool probe = (mode & 0x800000u) != 0 && fmt == 0;
    const int nt_store = (mode & 0x1000000u) ? 1 : 0;
    PreKey b;
    if (probe) {
        b = ch4 ? PreKey{0, 2, 4, 1} : PreKey{0, 2, kCh, 1};
    } else if (fmt == 0) {
        if (ch4) b = w1 ? PreKey{0, 1, 4, 0} : PreKey{0, 2, 4, 0};
        else b = w1 ? PreKey{0, 1, kCh, 0} : PreKey{0, 2, kCh, 0};
    } else {
        b = w1 ? PreKey{1, 1, kCh, 0} : PreKey{1, 2, kCh, 0};
    }
    return {b, write, byte_path, nt_store, w1 ? 0 : 1, spec_wgs_per_cu(mode)};
}

static Build key(const NatBuild& b) {
    return Build{(int)b.family, b.fmt, b.strict, b.w, b.ch, b.wpe, b.probe};
}
// the kernel a build names: the byte kernel takes `strict` as an argument
static Build kernel_of(Build b) {
    if (std::get<0>(b) == 0) std::get<2>(b) = 0;
    return b;
}

// every word with bits only from `bits`
static std::vector<uint32_t> words_over(std::initializer_list<int> bits) {
    std::vector<uint32_t> pos;
    for (int b : bits) pos.push_back(1u << b);
    std::vector<uint32_t> out;
    for (uint32_t i = 0; i < (1u << pos.size()); ++i) {
        uint32_t w = 0;
        for (size_t k = 0; k < pos.size(); ++k)
            if (i & (1u << k)) w |= pos[k];
        out.push_back(w);
    }
    return out;
}

template <class T, T... Vs>
static std::vector<int> values(Among<T, Vs...>) {
    return {(int)Vs...};
}

// "exists F FMT STRICT W CH WPE" per non-probe build, then "resolves FMT WORD F FMT STRICT W CH WPE"
// per argument.  The byte kernel takes `strict` as an argument: it has a strict build where
// nat_build hands a strict request on to it.
static int list_builds(int argc, char** argv) {
    auto print = [](const char* what, const NatBuild& b) {
        printf("%s %d %d %d %d %d %d\n", what, (int)b.family, b.fmt, (int)b.strict, b.w, b.ch, b.wpe);
    };
    for (int f : values(NatFmts{}))
        for (int s : values(AmongBool{})) {
            const NatBuild byte = nat_build(nat_bits::kBytePath | (s ? VPCSUM_NAT_STRICT_JAVA : 0u), f);
            if (byte.family == NatFamily::Byte && byte.strict == (s != 0) && !byte.probe) print("exists", byte);
            for (int c : values(NatWindows{})) {
                for (int w : values(NatwPkts{}))
                    if (natw_exists(f, s, w, c, false)) print("exists", NatBuild{NatFamily::Lane, f, s != 0, w, c, 1, false, 0, 0});
                for (int w : values(NatqPkts{}))
                    for (int o : values(NatqOccupancies{}))
                        if (natq_exists(f, s, w, c, o, false))
                            print("exists", NatBuild{NatFamily::Quad, f, s != 0, w, c, o, false, 0, 0});
            }
        }
    for (int i = 2; i < argc; ++i) {
        char* end = nullptr;
        errno = 0;
        const long fmt = strtol(argv[i], &end, 0);
        if (errno || end == argv[i] || *end != ':' || fmt < 0 || fmt > 2) {
            printf("bad argument %s\n", argv[i]);
            return 2;
        }
        const char* ws = end + 1;
        const unsigned long word = strtoul(ws, &end, 0);
        if (errno || end == ws || *end || word > 0xfffffffful || (word & ~(unsigned long)kNatModeAccept)) {
            printf("bad argument %s\n", argv[i]);
            return 2;
        }
        char what[48];
        snprintf(what, sizeof what, "resolves %ld 0x%lx", fmt, word);
        print(what, nat_build((uint32_t)word, (int)fmt));
    }
    printf("builds ok\n");
    return 0;
}

// "exists FMT W CH PROBE" per k_pre build (pre_exists over the dispatcher's candidates), then
// "resolves FMT WORD FMT W CH PROBE WRITE BYTE_PATH NT_STORE" per argument (pre_build).
static int list_pre_builds(int argc, char** argv) {
    for (int f : values(PreFmts{}))
        for (int w : values(NatqPkts{}))
            for (int c : values(NatWindows{}))
                for (int p : values(AmongBool{}))
                    if (pre_exists(f, w, c, p != 0)) printf("exists %d %d %d %d\n", f, w, c, p);
    for (int i = 2; i < argc; ++i) {
        char* end = nullptr;
        errno = 0;
        const long fmt = strtol(argv[i], &end, 0);
        if (errno || end == argv[i] || *end != ':' || fmt < 0 || fmt > 1) {
            printf("bad argument %s\n", argv[i]);
            return 2;
        }
        const char* ws = end + 1;
        const unsigned long word = strtoul(ws, &end, 0);
        if (errno || end == ws || *end || word > 0xfffffffful || (word & ~(unsigned long)kPreModeAccept)) {
            printf("bad argument %s\n", argv[i]);
            return 2;
        }
        const PreBuild b = pre_build((uint32_t)word, (int)fmt);
        printf("resolves %ld 0x%lx %d %d %d %d %d %d %d\n", fmt, word, b.fmt, b.w, b.ch, (int)b.probe, b.write, b.byte_path,
               b.nt_store);
    }
    printf("prebuilds ok\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc > 1) {
        if (argv[1] == std::string("builds")) return list_builds(argc, argv);
        if (argv[1] == std::string("prebuilds")) return list_pre_builds(argc, argv);
        printf("usage: %s [builds | prebuilds [FMT:WORD ...]]\n", argv[0]);
        return 2;
    }
    // the accept masks, bit for bit the literals api.cpp held
    CHECK(kCsumModeAccept == (0x07ff7fffu | 0x11u), "0x%x", kCsumModeAccept);
    CHECK(kNatModeAccept == (0x03u | 0x100u | 0x7000u | 0x3ff0000u), "0x%x", kNatModeAccept);
    CHECK(kNatCtxModeAccept == (0x03u | 0x100u), "0x%x", kNatCtxModeAccept);
    CHECK(kPreModeAccept == (0x10u | 0x100u | 0x3000u | 0x1ff0000u), "0x%x", kPreModeAccept);

    // nat_mode: strict, TCP rewrites, byte path, packets per lane, chunks, layout, occupancy
    std::set<Build> nat_reached;
    for (uint32_t m : words_over({0, 1, 8, 12, 13, 14, 16, 17, 23, 24, 25})) {
        CHECK(!(m & ~kNatModeAccept), "0x%x", m);
        for (int fmt = 0; fmt < 3; ++fmt) {
            const Spec s = spec_nat(m, fmt);
            const NatBuild b = nat_build(m, fmt);
            CHECK(key(b) == s.b && b.wl2 == s.wl2 && b.wgs_per_cu == s.wgs, "nat_mode 0x%x fmt %d", m, fmt);
            nat_reached.insert(kernel_of(key(b)));
            const Spec ps = spec_nat_probe(m, fmt);
            const NatBuild pb = nat_probe_build(m, fmt);
            CHECK(key(pb) == ps.b && pb.wl2 == ps.wl2 && pb.wgs_per_cu == ps.wgs, "probe tune 0x%x fmt %d", m, fmt);
            nat_reached.insert(kernel_of(key(pb)));
        }
    }
    // workgroups per CU: every value, 0 the default, next to the fields around it
    for (uint32_t w = 0; w < 32; ++w)
        for (uint32_t around : {0u, 0x20000u, 0x800000u, 0x820000u})
            for (int fmt = 0; fmt < 3; ++fmt) {
                const uint32_t m = (w << 18) | around;
                CHECK(nat_build(m, fmt).wgs_per_cu == (w ? w : 24u), "nat wgs %u", w);
                CHECK(nat_probe_build(m, fmt).wgs_per_cu == (w ? w : 24u), "probe wgs %u", w);
                CHECK(key(nat_build(m, fmt)) == spec_nat(m, fmt).b, "nat wgs %u changes the build", w);
                if (fmt < 2) {
                    CHECK(pre_build(m, fmt).wgs_per_cu == (w ? w : 24u), "pre wgs %u", w);
                    CHECK(pre_build(m, fmt).wgs_per_cu == spec_pre(m, fmt).wgs, "pre wgs %u", w);
                }
            }

    // pre-image mode: write, byte path, packets per lane, chunks, probe, non-temporal stores
    std::set<PreKey> pre_reached;
    for (uint32_t m : words_over({4, 8, 12, 13, 16, 17, 23, 24})) {
        CHECK(!(m & ~kPreModeAccept), "0x%x", m);
        for (int fmt = 0; fmt < 2; ++fmt) {
            const PreSpec s = spec_pre(m, fmt);
            const PreBuild b = pre_build(m, fmt);
            CHECK((PreKey{b.fmt, b.w, b.ch, b.probe} == s.b) && b.write == s.write && b.byte_path == s.byte_path &&
                      b.nt_store == s.nt_store && b.wl2 == s.wl2 && b.wgs_per_cu == s.wgs,
                  "pre mode 0x%x fmt %d", m, fmt);
            pre_reached.insert(PreKey{b.fmt, b.w, b.ch, b.probe});
        }
    }

    // compute mode: variant id, plain loads, no adaptive grid; workgroups per CU
    for (uint32_t m : words_over({8, 9, 10, 11, 12, 13, 14, 24, 25, 26})) {
        CHECK(!(m & ~kCsumModeAccept), "0x%x", m);
        const CsumTune t = csum_tune(m);
        const int variant = (int)(((m >> 8) & 0x1f) | (((m >> 24) & 0x7) << 5));
        CHECK(t.variant == variant && t.nt == ((m & 0x2000u) == 0) && t.adapt == ((m & 0x4000u) == 0) && t.wgs_per_cu == 0,
              "mode 0x%x", m);
    }
    for (uint32_t w = 0; w < 256; ++w)
        for (uint32_t around : {0u, 0x0100ff00u | 0x6000u, 0x07000000u}) {
            const CsumTune t = csum_tune((w << 16) | around);
            CHECK(t.wgs_per_cu == w && t.variant == csum_tune(around).variant, "csum wgs %u", w);   // 0: the launcher's own grid
        }
    const CsumTune dflt;   // what the internal call sites pass: launch_csum(..., 0, 0) before
    const CsumTune zero = csum_tune(0);
    CHECK(dflt.variant == 0 && dflt.nt && dflt.adapt && dflt.wgs_per_cu == 0, "default CsumTune");
    CHECK(zero.variant == 0 && zero.nt && zero.adapt && zero.wgs_per_cu == 0, "csum_tune(0)");
    // the ignored bits change nothing
    CHECK(csum_tune(0xeeu | 0x11u).variant == 0 && csum_tune(0xffu).nt && csum_tune(0xffu).adapt, "ignored bits");

    // the builds the launchers instantiate: *_exists over the dispatchers' candidates (and the byte
    // kernel per format) -- exactly the builds the decoders reach
    std::set<Build> nat_built;
    for (int f : values(NatFmts{})) nat_built.insert(Build{0, f, 0, 1, 0, 1, 0});
    for (int f : values(NatFmts{}))
        for (int s : values(AmongBool{}))
            for (int p : values(AmongBool{}))
                for (int c : values(NatWindows{})) {
                    for (int w : values(NatwPkts{}))
                        if (natw_exists(f, s, w, c, p)) nat_built.insert(Build{1, f, s, w, c, 1, p});
                    for (int w : values(NatqPkts{}))
                        for (int o : values(NatqOccupancies{}))
                            if (natq_exists(f, s, w, c, o, p)) nat_built.insert(Build{2, f, s, w, c, o, p});
                }
    std::set<PreKey> pre_built;
    for (int f : values(PreFmts{}))
        for (int w : values(NatqPkts{}))
            for (int c : values(NatWindows{}))
                for (int p : values(AmongBool{}))
                    if (pre_exists(f, w, c, p)) pre_built.insert(PreKey{f, w, c, p});
    CHECK(nat_built == nat_reached, "NAT builds: %zu instantiated, %zu reachable", nat_built.size(), nat_reached.size());
    CHECK(pre_built == pre_reached, "pre-image builds: %zu instantiated, %zu reachable", pre_built.size(), pre_reached.size());

    // dispatch: the chosen candidates reach f as constants, a value outside them is refused
    int got = 0;
    CHECK(dispatch([&](auto A, auto B) { got = A * 10 + (B ? 1 : 0); return true; }, 4, NatWindows{}, true, AmongBool{}) &&
              got == 41, "dispatch");
    CHECK(!dispatch([&](auto) { got = -1; return true; }, 5, NatWindows{}) && got == 41, "dispatch refuses");
    CHECK(!dispatch([&](auto A) { return natq_exists(A, false, 4, 6, 1, false); }, 0, NatFmts{}), "dispatch passes f's refusal on");

    printf("nat builds %zu pre builds %zu\n", nat_reached.size(), pre_reached.size());
    if (g_fail) {
        printf("%d checks failed\n", g_fail);
        return 1;
    }
    printf("launch_modes ok\n");
    return 0;
}
