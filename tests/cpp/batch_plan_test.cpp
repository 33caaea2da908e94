// batch_plan_test.cpp -- the host arithmetic of vproxy_amd/csrc/batch_plan.h under ASan / UBSan
// (tests/test_lib_cpu.py builds and runs it; nothing of the library is linked).  Every buffer is
// allocated at its exact size, so a read or write past one is an error; expected values are listed
// by hand or recomputed here with arithmetic of the test's own.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <random>
#include <vector>

#include "batch_plan.h"

using namespace vpcsum;

static int g_fail = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            if (++g_fail > 20) exit(1);                                          \
        }                                                                        \
    } while (0)

static vpcsum_desc_t mk(uint64_t off, uint16_t len, uint16_t l4_off = 20, uint8_t ver = 4, uint8_t proto = 6,
                        uint8_t flags = VPCSUM_F_L4) {
    vpcsum_desc_t d;
    memset(&d, 0, sizeof(d));
    d.l3_off = off;
    d.l3_len = len;
    d.l4_off = l4_off;
    d.l3_ver = ver;
    d.l4_proto = proto;
    d.flags = flags;
    return d;
}

static uint64_t floor16(uint64_t x) { return x / 16 * 16; }
static uint64_t ceil16(uint64_t x) { return (x + 15) / 16 * 16; }

static void span_is(const std::vector<vpcsum_desc_t>& d, uint64_t arena_len, uint64_t lo, uint64_t hi, uint64_t used) {
    std::unique_ptr<vpcsum_desc_t[]> exact(new vpcsum_desc_t[d.size()]);
    for (size_t i = 0; i < d.size(); ++i) exact[i] = d[i];
    const BatchSpan s = batch_span(exact.get(), (uint32_t)d.size(), arena_len);
    CHECK(s.lo == lo);
    CHECK(s.hi == hi);
    CHECK(s.used == used);
}

static void test_span() {
    span_is({}, 1000, 0, 0, 0);
    span_is({mk(1001, 0), mk(990, 11), mk(UINT64_MAX, 1), mk(0, 1001)}, 1000, 0, 0, 0);   // all outside
    const uint64_t offs[5] = {0, 1, 14, 15, 16};
    const uint64_t los[5] = {0, 0, 0, 0, 16};
    for (int k = 0; k < 5; ++k) span_is({mk(offs[k], 60)}, 1000, los[k], offs[k] + 60, 76);
    span_is({mk(900, 103)}, 1003, 896, 1003, 119);       // ends exactly at an arena_len that is no multiple of 16
    span_is({mk(37, 0)}, 1000, 32, 37, 16);              // l3_len = 0
    span_is({mk(1000, 0)}, 1000, 992, 1000, 16);         // l3_off == arena_len (an empty packet fits)
    span_is({mk(1000, 1)}, 1000, 0, 0, 0);
    span_is({mk(1001, 0)}, 1000, 0, 0, 0);               // l3_off = arena_len + 1
    // several packets, one outside: min / max over the ones inside only
    span_is({mk(500, 40), mk(990, 20), mk(49, 100), mk(300, 7)}, 1000, 48, 540, 56 + 116 + 23);
    CHECK(desc_in_arena(mk(0, 0), 0) && !desc_in_arena(mk(0, 1), 0) && desc_in_arena(mk(3, 5), 8) && !desc_in_arena(mk(4, 5), 8));
}

static void test_l4_field() {
    CHECK(l4_field_host(6) == 16);
    CHECK(l4_field_host(17) == 6);
    CHECK(l4_field_host(1) == 2);
    CHECK(l4_field_host(58) == 2);
    CHECK(l4_field_host(0) == -1);
}

struct TakeFrom {
    const uint32_t* v;
    uint32_t operator()(uint32_t i, const vpcsum_desc_t&) const { return v[i]; }
};

static void test_gather_random() {
    std::mt19937_64 rng(0x6a7468);
    int refused = 0, accepted = 0, outside = 0;
    for (int it = 0; it < 4000; ++it) {
        const uint64_t arena_len = 1 + rng() % 700;
        const uint32_t n = (uint32_t)(rng() % 6);
        std::unique_ptr<uint8_t[]> arena(new uint8_t[arena_len]);
        for (uint64_t k = 0; k < arena_len; ++k) arena[k] = (uint8_t)rng();
        std::unique_ptr<vpcsum_desc_t[]> in(new vpcsum_desc_t[n]), out(new vpcsum_desc_t[n]);
        std::vector<uint32_t> take(n);
        const bool whole = rng() & 1;
        for (uint32_t i = 0; i < n; ++i) {
            const uint64_t off = rng() % (arena_len + 3);
            const uint64_t room = off <= arena_len ? arena_len - off : 0;
            uint16_t len = (uint16_t)(rng() % (room + 1));
            if (rng() % 8 == 0) len = (uint16_t)(room + 1 + rng() % 4);   // sticks out of the arena
            in[i] = mk(off, len, (uint16_t)(rng() % 64), rng() & 1 ? 4 : 6, (uint8_t)rng(), (uint8_t)rng());
            take[i] = whole ? len : (uint32_t)(rng() % (len + 1u));
        }
        // the staging need, block by block, with the test's own arithmetic
        uint64_t need = 0, pos = 0;
        for (uint32_t i = 0; i < n; ++i) {
            if (in[i].l3_off > arena_len || in[i].l3_off + in[i].l3_len > arena_len) continue;
            uint64_t end = ceil16(in[i].l3_off + take[i]);
            if (end > arena_len) end = arena_len;
            const uint64_t bytes = end - floor16(in[i].l3_off);
            need = pos + bytes > need ? pos + bytes : need;
            pos += ceil16(bytes);
        }
        const uint64_t capacity = rng() % 4 == 0 ? rng() % (need + 1) : need + rng() % 3;
        std::unique_ptr<uint8_t[]> stage(new uint8_t[capacity]);
        const int64_t got = whole ? gather_blocks(arena.get(), arena_len, in.get(), n, out.get(), stage.get(), capacity)
                                  : gather_blocks(arena.get(), arena_len, in.get(), n, out.get(), stage.get(), capacity,
                                                  TakeFrom{take.data()});
        if (capacity < need) {
            CHECK(got == -1);
            ++refused;
            continue;
        }
        ++accepted;
        CHECK(got == (int64_t)pos);
        CHECK(got % 16 == 0);
        for (uint32_t i = 0; i < n; ++i) {
            const vpcsum_desc_t &a = in[i], &b = out[i];
            CHECK(b.l4_off == a.l4_off && b.l3_ver == a.l3_ver && b.l4_proto == a.l4_proto && b.flags == a.flags && b.rsv == a.rsv);
            if (a.l3_off > arena_len || a.l3_off + a.l3_len > arena_len) {
                CHECK(b.l3_off == UINT64_MAX && b.l3_len == a.l3_len);
                ++outside;
                continue;
            }
            CHECK(b.l3_off % 16 == a.l3_off % 16);
            CHECK(b.l3_len == take[i]);
            CHECK(b.l3_off + take[i] <= capacity);
            for (uint32_t k = 0; k < take[i]; ++k) CHECK(stage[b.l3_off + k] == arena[a.l3_off + k]);
            CHECK(ceil16(b.l3_off + take[i]) <= (uint64_t)got);
            for (uint32_t j = 0; j < i; ++j) {   // 16-B blocks of different packets do not overlap
                if (in[j].l3_off > arena_len || in[j].l3_off + in[j].l3_len > arena_len) continue;
                const uint64_t lo = std::max(floor16(b.l3_off), floor16(out[j].l3_off));
                const uint64_t hi = std::min(ceil16(b.l3_off + take[i]), ceil16(out[j].l3_off + take[j]));
                CHECK(lo >= hi);
            }
        }
    }
    CHECK(refused > 100 && accepted > 1000 && outside > 100);
}

static void test_gather_capacity() {
    // three packets in a 16-B-multiple arena: 2 + 3 + 1 blocks
    const uint64_t arena_len = 256;
    std::unique_ptr<uint8_t[]> arena(new uint8_t[arena_len]);
    for (uint64_t k = 0; k < arena_len; ++k) arena[k] = (uint8_t)(k * 7 + 1);
    std::unique_ptr<vpcsum_desc_t[]> in(new vpcsum_desc_t[4]), out(new vpcsum_desc_t[4]);
    in[0] = mk(10, 20);     // [0, 32)
    in[1] = mk(100, 30);    // [96, 144)
    in[2] = mk(300, 4);     // outside
    in[3] = mk(240, 16);    // [240, 256)
    const uint64_t need = 32 + 48 + 16;
    std::unique_ptr<uint8_t[]> exact(new uint8_t[need]), shorter(new uint8_t[need - 16]);
    CHECK(gather_blocks(arena.get(), arena_len, in.get(), 4, out.get(), shorter.get(), need - 16) == -1);
    CHECK(gather_blocks(arena.get(), arena_len, in.get(), 4, out.get(), exact.get(), need) == (int64_t)need);
    CHECK(out[0].l3_off == 10 && out[1].l3_off == 32 + 4 && out[2].l3_off == UINT64_MAX && out[3].l3_off == 80);
    CHECK(memcmp(exact.get() + 36, arena.get() + 100, 30) == 0);
    CHECK(gather_blocks(arena.get(), arena_len, in.get(), 0, out.get(), exact.get(), 0) == 0);
}

static void test_header_extents() {
    std::unique_ptr<uint8_t[]> arena(new uint8_t[2048]);
    memset(arena.get(), 0xAB, 2048);
    uint8_t pre[sizeof(vpcsum_pre_t)], pre4[sizeof(vpcsum_pre4_t)];
    memset(pre, 0, sizeof(pre));
    memset(pre4, 0, sizeof(pre4));
    const uint8_t PF = VPCSUM_F_L4 | VPCSUM_F_PRE;
    bool cut = false;
    // IPv4 / TCP: through the checksum field at L4 + 16
    vpcsum_desc_t tcp = mk(100, 1500, 20, 4, 6, PF);
    CHECK(nat_header_end(tcp) == 38);
    CHECK(pre_staged_len(arena.get(), tcp, pre, VPCSUM_PRE_FMT_PRE, &cut) == 38 && cut);
    CHECK(pre_staged_len(arena.get(), tcp, pre4, VPCSUM_PRE_FMT_PRE4, &cut) == 38 && cut);
    // IPv4 (IHL 6) / UDP: the field at L4 + 6
    vpcsum_desc_t udp = mk(64, 200, 24, 4, 17, PF);
    CHECK(nat_header_end(udp) == 32);
    CHECK(pre_staged_len(arena.get(), udp, pre, VPCSUM_PRE_FMT_PRE, &cut) == 32 && cut);
    // IPv6 / ICMPv6: the field at L4 + 2
    vpcsum_desc_t icmp6 = mk(7, 100, 40, 6, 58, PF);
    CHECK(nat_header_end(icmp6) == 44);
    CHECK(pre_staged_len(arena.get(), icmp6, pre, VPCSUM_PRE_FMT_PRE, &cut) == 44 && cut);
    // a segment too short to hold the field: the L3 header alone goes back; staged in full
    vpcsum_desc_t shrt = mk(100, 37, 20, 4, 6, PF);
    CHECK(nat_header_end(shrt) == 20);
    CHECK(pre_staged_len(arena.get(), shrt, pre, VPCSUM_PRE_FMT_PRE, &cut) == 37 && !cut);
    CHECK(nat_header_end(mk(100, 38, 20, 4, 6, PF)) == 38);
    CHECK(nat_header_end(mk(100, 10, 20, 4, 47, PF)) == 10);      // never past the packet
    CHECK(nat_header_end(mk(100, 300, 40, 6, 47, PF)) == 40);     // no L4 sum: the IPv6 header
    // at the very end of an exact-size arena: the field is the last thing read
    vpcsum_desc_t last = mk(2048 - 38, 38, 20, 4, 6, PF);
    CHECK(pre_staged_len(arena.get(), last, pre, VPCSUM_PRE_FMT_PRE, &cut) == 38 && cut);
    // UDP with a stored zero sum is summed in full
    arena[64 + 24 + 6] = 0;
    arena[64 + 24 + 7] = 0;
    CHECK(pre_staged_len(arena.get(), udp, pre, VPCSUM_PRE_FMT_PRE, &cut) == 200 && !cut);
    arena[64 + 24 + 7] = 1;
    CHECK(pre_staged_len(arena.get(), udp, pre, VPCSUM_PRE_FMT_PRE, &cut) == 32 && cut);
    // not F_PRE, or no L4 sum: all of it
    CHECK(pre_staged_len(arena.get(), mk(100, 1500, 20, 4, 6, VPCSUM_F_L4), pre, VPCSUM_PRE_FMT_PRE, &cut) == 1500 && !cut);
    CHECK(pre_staged_len(arena.get(), mk(100, 1500, 20, 4, 47, PF), pre, VPCSUM_PRE_FMT_PRE, &cut) == 1500 && !cut);
    // a header-sum entry: through the L4 header it covers (TCP with options, 32 B), both formats
    vpcsum_hsum_t hs;
    memset(&hs, 0, sizeof(hs));
    hs.hlen = 32;
    memcpy(pre, &hs, sizeof(hs));
    memcpy(pre4, &hs, sizeof(hs));
    pre[36] = VPCSUM_PRE_HSUM;     // vpcsum_pre_t.mask
    pre4[12] = VPCSUM_PRE_HSUM;    // vpcsum_pre4_t.mask
    CHECK(pre_staged_len(arena.get(), tcp, pre, VPCSUM_PRE_FMT_PRE, &cut) == 52 && cut);
    CHECK(pre_staged_len(arena.get(), tcp, pre4, VPCSUM_PRE_FMT_PRE4, &cut) == 52 && cut);
    CHECK(pre_staged_len(arena.get(), mk(100, 50, 20, 4, 6, PF), pre, VPCSUM_PRE_FMT_PRE, &cut) == 50 && cut);   // never past the packet
    pre[36] = 0;                   // the same bytes without the bit are addresses: hlen is not read
    CHECK(pre_staged_len(arena.get(), tcp, pre, VPCSUM_PRE_FMT_PRE, &cut) == 38 && cut);
    hs.hlen = 8;                   // UDP's 8-B header ends with its checksum field
    memcpy(pre4, &hs, sizeof(hs));
    CHECK(pre_staged_len(arena.get(), udp, pre4, VPCSUM_PRE_FMT_PRE4, &cut) == 32 && cut);
}

// An exact-size copy of a byte list: reading or writing past it is a sanitizer error
static std::unique_ptr<uint8_t[]> exact_bytes(const std::vector<uint8_t>& v) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[v.size()]);
    memcpy(p.get(), v.data(), v.size());
    return p;
}

static void test_place_checksums() {
    // seven packets in a 200-byte arena filled with 0xEE; out word 0xAABBCCDD: L4 sum AA BB, IP sum CC DD
    const uint64_t arena_len = 200;
    std::vector<uint8_t> before(arena_len, 0xEE);
    const uint8_t BAD = VPCSUM_S_BAD_DESC, OK = VPCSUM_S_DONE;
    std::unique_ptr<vpcsum_desc_t[]> d(new vpcsum_desc_t[7]);
    std::unique_ptr<uint32_t[]> out(new uint32_t[7]);
    std::unique_ptr<uint8_t[]> st(new uint8_t[7]);
    d[0] = mk(0, 20, 20, 4, 6, VPCSUM_F_IP | VPCSUM_F_L4);    // refused, first: untouched
    d[1] = mk(20, 20, 20, 4, 6, VPCSUM_F_IP);                 // IP only
    d[2] = mk(40, 28, 20, 4, 17, VPCSUM_F_L4);                // L4 only (UDP: field at L4 + 6)
    d[3] = mk(70, 40, 20, 4, 6, VPCSUM_F_IP | VPCSUM_F_L4);   // both (TCP: field at L4 + 16)
    d[4] = mk(110, 44, 40, 6, 58, VPCSUM_F_L4P);              // F_L4P (ICMPv6: field at L4 + 2)
    d[5] = mk(156, 24, 20, 4, 47, VPCSUM_F_IP | VPCSUM_F_L4); // no checksum field in the protocol: IP only
    d[6] = mk(180, 20, 0, 4, 1, VPCSUM_F_IP | VPCSUM_F_L4);   // refused, last (ends at the arena's end): untouched
    for (int i = 0; i < 7; ++i) { out[i] = 0xAABBCCDDu + 0x01010101u * (uint32_t)i; st[i] = OK; }
    st[0] = BAD;
    st[6] = BAD | OK;
    std::vector<uint8_t> want = before;
    want[20 + 10] = 0xCD; want[20 + 11] = 0xDE;                                   // out[1] = AB BC CD DE
    want[40 + 20 + 6] = 0xAC; want[40 + 20 + 7] = 0xBD;                           // out[2] = AC BD CE DF
    want[70 + 10] = 0xCF; want[70 + 11] = 0xE0; want[70 + 36] = 0xAD; want[70 + 37] = 0xBE;   // out[3] = AD BE CF E0
    want[110 + 42] = 0xAE; want[110 + 43] = 0xBF;                                 // out[4] = AE BF D0 E1
    want[156 + 10] = 0xD1; want[156 + 11] = 0xE2;                                 // out[5] = AF C0 D1 E2
    std::unique_ptr<uint8_t[]> arena = exact_bytes(before);
    place_checksums(arena.get(), d.get(), out.get(), st.get(), 7);
    CHECK(memcmp(arena.get(), want.data(), arena_len) == 0);
    // a refused packet's descriptor is not trusted: one far outside the arena is skipped, first and last
    d[0] = mk(UINT64_MAX - 5, 20, 20, 4, 6, VPCSUM_F_IP | VPCSUM_F_L4);
    d[6] = mk(1ull << 40, 20, 65000, 4, 6, VPCSUM_F_IP | VPCSUM_F_L4);
    arena = exact_bytes(before);
    place_checksums(arena.get(), d.get(), out.get(), st.get(), 7);
    CHECK(memcmp(arena.get(), want.data(), arena_len) == 0);
    place_checksums(nullptr, nullptr, nullptr, nullptr, 0);   // an empty batch touches nothing
}

static void test_return_nat_headers() {
    // the caller's arena: 0x11 everywhere; the staging (gather_blocks' layout): byte k holds 0x80 + k
    const uint64_t arena_len = 300;
    std::vector<uint8_t> before(arena_len, 0x11), stage_v(160);
    for (size_t k = 0; k < stage_v.size(); ++k) stage_v[k] = (uint8_t)(0x80 + k);
    std::unique_ptr<vpcsum_desc_t[]> d(new vpcsum_desc_t[4]), sd(new vpcsum_desc_t[4]);
    std::unique_ptr<uint8_t[]> st(new uint8_t[4]);
    d[0] = mk(5, 100, 20, 4, 6);      // IPv4 / TCP, 80-B segment: 38 B back, 80 B (L4 + 60) with the TCP rewrites
    d[1] = mk(120, 40, 20, 4, 17);    // IPv4 / UDP: 28 B back either way
    d[2] = mk(170, 50, 20, 4, 6);     // refused: neither read nor written
    d[3] = mk(250, 50, 20, 4, 6);     // IPv4 / TCP ending at the arena's end, 30-B segment: 38 B, or all 50
    for (int i = 0; i < 4; ++i) { sd[i] = d[i]; st[i] = VPCSUM_S_DONE; }
    sd[0].l3_off = 5;      // staged [0, 112): needs stage[5, 85)
    sd[1].l3_off = 112 + 8;   // needs stage[120, 148)
    sd[2].l3_off = UINT64_MAX;
    sd[3].l3_off = 10;     // (the test's own layout: overlaps packet 0's blocks, the copy is what is checked) stage[10, 60)
    st[2] = VPCSUM_S_BAD_DESC;
    for (int tcp = 0; tcp < 2; ++tcp) {
        std::vector<uint8_t> want = before;
        const uint32_t len0 = tcp ? 80 : 38, len3 = tcp ? 50 : 38;
        for (uint32_t k = 0; k < len0; ++k) want[5 + k] = (uint8_t)(0x80 + 5 + k);
        for (uint32_t k = 0; k < 28; ++k) want[120 + k] = (uint8_t)(0x80 + 120 + k);
        for (uint32_t k = 0; k < len3; ++k) want[250 + k] = (uint8_t)(0x80 + 10 + k);
        std::unique_ptr<uint8_t[]> arena = exact_bytes(before);
        // the staging at the exact size the copies need: through byte 148 (packet 1's 28 B)
        stage_v.resize(148);
        const std::unique_ptr<uint8_t[]> stage = exact_bytes(stage_v);
        return_nat_headers(arena.get(), d.get(), stage.get(), sd.get(), st.get(), 4, tcp != 0);
        CHECK(memcmp(arena.get(), want.data(), arena_len) == 0);
    }
    CHECK(nat_tcp_header_end(d[0]) == 80 && nat_tcp_header_end(d[1]) == 28 && nat_tcp_header_end(d[3]) == 50);
    CHECK(nat_tcp_header_end(mk(0, 39, 20, 4, 6)) == 38);   // 19 B of TCP header: no TCP rewrite ran, the plain extent
    return_nat_headers(nullptr, nullptr, nullptr, nullptr, nullptr, 0, true);
}

int main() {
    test_place_checksums();
    test_return_nat_headers();
    test_span();
    test_l4_field();
    test_gather_random();
    test_gather_capacity();
    test_header_extents();
    if (g_fail) {
        fprintf(stderr, "batch_plan: %d checks failed\n", g_fail);
        return 1;
    }
    printf("batch_plan ok\n");
    return 0;
}
