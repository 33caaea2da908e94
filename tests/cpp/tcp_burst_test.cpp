// tcp_burst_test.cpp -- the host-checkable rules of the TCP send bursts (vproxy_amd/csrc/tcp_burst.h:
// the 9-ary search, the cut, the whole-burst refusals, the staged source's span and rebase) in a
// stand-alone program under ASan / UBSan (tests/test_tcp_burst_cpu.py builds and runs it; nothing of
// the library is linked).  Every table lives in a heap block of its exact size, so a probe past
// n_bursts is an error of the run, not of a CHECK.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <utility>
#include <vector>

#include "tcp_burst.h"

using namespace vpcsum;

static int g_fail = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            if (++g_fail > 20) exit(1);                                          \
        }                                                                        \
    } while (0)

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint64_t rnd() {
    g_rng ^= g_rng << 13; g_rng ^= g_rng >> 7; g_rng ^= g_rng << 17;
    return g_rng;
}

static vpcsum_tcphdr_t mk_hdr(int ver, int l2, int rsv = 0) {
    vpcsum_tcphdr_t h;
    memset(&h, 0, sizeof(h));
    h.l2_len = (uint8_t)l2;
    h.l3_ver = (uint8_t)ver;
    h.ttl = 64;
    h.rsv[1] = (uint8_t)rsv;
    return h;
}

static vpcsum_tcpburst_t mk_burst(uint64_t data_off, uint32_t data_len, uint32_t mss, uint32_t first, uint32_t seq = 0,
                                  uint32_t hdr = 0) {
    vpcsum_tcpburst_t b;
    memset(&b, 0, sizeof(b));
    b.data_off = data_off; b.data_len = data_len; b.seq = seq; b.hdr = hdr; b.first = first;
    b.mss = (uint16_t)mss; b.flags = 0x18;
    b.count = (data_len && !mss) ? 0u : tcp_burst_count(data_len, mss);
    return b;
}

// an exact-size heap copy of a table
static std::unique_ptr<vpcsum_tcpburst_t[]> heap(const std::vector<vpcsum_tcpburst_t>& v) {
    std::unique_ptr<vpcsum_tcpburst_t[]> p(new vpcsum_tcpburst_t[v.size()]);
    std::copy(v.begin(), v.end(), p.get());
    return p;
}

// One frame of a one-burst call, IPv4 + Ethernet template unless told otherwise
static bool one(const vpcsum_tcpburst_t& b, uint32_t j, uint64_t frame_off, uint32_t frame_cap, uint64_t dst_len, uint64_t src_len,
                vpcsum_tcpseg_t* seg, const vpcsum_tcphdr_t* hdrs = nullptr, uint32_t n_hdr = 1) {
    static const vpcsum_tcphdr_t v4 = mk_hdr(4, 14);
    std::unique_ptr<vpcsum_tcpburst_t[]> t(new vpcsum_tcpburst_t[1]);
    t[0] = b;
    return tcp_burst_frame(hdrs ? hdrs : &v4, n_hdr, t.get(), 1, frame_off, j, frame_cap, dst_len, src_len, seg);
}

static void check_layout() {
    vpcsum_tcpburst_t r = mk_burst(0x0102030405060708ull, 0x11121314u, 0x2122, 0x31323334u, 0x41424344u, 0x51525354u);
    r.flags = 0x3f; r.rsv = 0x7a; r.count = 0x61626364u;
    uint32_t w[8];
    memcpy(w, &r, 32);
    const TcpBurst a = tcp_burst_unpack(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]), b = tcp_burst_fields(r);
    CHECK(a.data_off == r.data_off && a.data_len == r.data_len && a.seq == r.seq && a.hdr == r.hdr && a.first == r.first);
    CHECK(a.mss == r.mss && a.flags == r.flags && a.rsv == r.rsv && a.count == r.count);
    CHECK(b.data_off == a.data_off && b.data_len == a.data_len && b.seq == a.seq && b.hdr == a.hdr && b.first == a.first &&
          b.mss == a.mss && b.flags == a.flags && b.rsv == a.rsv && b.count == a.count);
}

static void check_cut() {
    vpcsum_tcpseg_t s;
    const uint64_t big = 1ull << 40;
    // data_len mss - 1, mss, mss + 1, 2 mss, 2 mss + 1: counts and the last piece
    for (uint32_t mss : {1u, 7u, 536u, 1460u, 65495u}) {
        for (uint32_t d : {1u, mss - 1, mss, mss + 1, 2 * mss, 2 * mss + 1, 45 * mss, 45 * mss + 1}) {
            if (!d) continue;
            const vpcsum_tcpburst_t b = mk_burst(100, d, mss, 5, 0xfffffc18u);   // 2^32 - 1000: seq wraps inside
            const uint32_t cnt = (d + mss - 1) / mss;
            CHECK(b.count == cnt);
            uint64_t covered = 0;
            for (uint32_t k = 0; k < cnt; ++k) {
                CHECK(one(b, 5 + k, 4096ull * k, 1u << 17, big, 100 + (uint64_t)d, &s));
                CHECK(s.data_off == 100 + (uint64_t)k * mss && s.seq == (uint32_t)(0xfffffc18u + k * mss));
                CHECK(s.data_len == (k + 1 < cnt ? mss : d - (cnt - 1) * mss) && s.flags == 0x18 && s.rsv == 0 && s.hdr == 0);
                CHECK(s.frame_off == 4096ull * k && s.frame_cap == 1u << 17);
                covered += s.data_len;
            }
            CHECK(covered == d);
            CHECK(!one(b, 4, 0, 1u << 17, big, 100 + (uint64_t)d, &s));         // before the burst
            CHECK(!one(b, 5 + cnt, 0, 1u << 17, big, 100 + (uint64_t)d, &s));   // past its count
        }
    }
    // a burst without payload: one frame, mss not read
    for (uint32_t mss : {0u, 1460u}) {
        vpcsum_tcpburst_t b = mk_burst(77, 0, mss, 0, 9);
        b.flags = 0x11;
        CHECK(b.count == 1 && one(b, 0, 10, 54, 64, 77, &s) && s.data_len == 0 && s.seq == 9 && s.flags == 0x11 && s.data_off == 77);
        CHECK(!one(b, 1, 10, 54, 64, 77, &s));
        CHECK(!one(b, 0, 10, 54, 64, 76, &s));    // data_off > src_len, even without payload
    }
    // data_len up to 2^32 - 1 with mss 1 and 65535 (IPv6: the length field takes 65535 - 20)
    {
        const uint32_t d = 0xffffffffu;
        const vpcsum_tcpburst_t b1 = mk_burst(0, d, 1, 0, 0x80000000u);
        CHECK(b1.count == d);
        for (uint32_t k : {0u, 1u, 0x7fffffffu, 0x80000000u, d - 1}) {
            CHECK(one(b1, k, 0, 55, 1u << 20, d, &s) && s.data_len == 1 && s.data_off == k && s.seq == (uint32_t)(0x80000000u + k));
        }
        CHECK(!one(b1, 0, 0, 55, 1u << 20, (uint64_t)d - 1, &s));   // the source ends one byte early
        const vpcsum_tcpburst_t b2 = mk_burst(3, d, 65535, 0);
        CHECK(b2.count == 65537);
        CHECK(!one(b2, 0, 0, 1u << 17, 1u << 20, 3 + (uint64_t)d, &s));   // 40 + 65535 > 65535
        const vpcsum_tcpburst_t b3 = mk_burst(3, d, 65495, 0);
        const uint32_t c3 = (uint32_t)(((uint64_t)d + 65494) / 65495);
        CHECK(b3.count == c3);
        CHECK(one(b3, c3 - 1, 0, 1u << 17, 1u << 20, 3 + (uint64_t)d, &s));
        CHECK(s.data_off == 3 + (uint64_t)(c3 - 1) * 65495 && s.data_len == d - (c3 - 1) * 65495u && s.data_off + s.data_len == 3 + (uint64_t)d);
        CHECK(one(b3, 0, 0, 1u << 17, 1u << 20, 3 + (uint64_t)d, &s) && s.data_len == 65495);
    }
}

static void check_refusals() {
    vpcsum_tcpseg_t s;
    const vpcsum_tcphdr_t hs[6] = {mk_hdr(4, 14), mk_hdr(6, 0), mk_hdr(5, 14), mk_hdr(4, 18), mk_hdr(4, 14, 1), mk_hdr(6, 14)};
    auto ok = [&](vpcsum_tcpburst_t b, uint32_t j = 0, uint64_t fo = 0, uint32_t cap = 1u << 17, uint64_t dl = 1ull << 40,
                  uint64_t sl = 1ull << 40, uint32_t n_hdr = 6) { return one(b, j, fo, cap, dl, sl, &s, hs, n_hdr); };
    // hdr, the template
    CHECK(ok(mk_burst(0, 10, 5, 0, 0, 5)) && !ok(mk_burst(0, 10, 5, 0, 0, 6)) && !ok(mk_burst(0, 10, 5, 0, 0, 0xffffffffu)));
    CHECK(!ok(mk_burst(0, 10, 5, 0), 0, 0, 1u << 17, 1ull << 40, 1ull << 40, 0));   // n_hdr 0
    CHECK(ok(mk_burst(0, 10, 5, 0, 0, 1)) && !ok(mk_burst(0, 10, 5, 0, 0, 2)) && !ok(mk_burst(0, 10, 5, 0, 0, 3)) &&
          !ok(mk_burst(0, 10, 5, 0, 0, 4)));
    // flags, rsv
    vpcsum_tcpburst_t b = mk_burst(0, 10, 5, 0);
    b.flags = 0x3f; CHECK(ok(b));
    b.flags = 0x40; CHECK(!ok(b));
    b.flags = 0x80; CHECK(!ok(b));
    b.flags = 0x18; b.rsv = 1; CHECK(!ok(b));
    // mss 0 with payload, whatever the count says
    b = mk_burst(0, 10, 0, 0);
    for (uint32_t c : {0u, 1u, 10u}) { b.count = c; CHECK(!ok(b)); }
    // count
    b = mk_burst(0, 11, 5, 0);
    CHECK(b.count == 3 && ok(b) && ok(b, 2));
    b.count = 2; CHECK(!ok(b) && !ok(b, 1));
    b.count = 4; CHECK(!ok(b) && !ok(b, 3));
    b = mk_burst(0, 0, 5, 0);
    b.count = 0; CHECK(!ok(b));
    b.count = 2; CHECK(!ok(b) && !ok(b, 1));
    // the longest frame's length field: IPv4 40 + 65495, IPv6 20 + 65515
    CHECK(ok(mk_burst(0, 70000, 65495, 0)) && !ok(mk_burst(0, 70000, 65496, 0)) && ok(mk_burst(0, 65495, 65535, 0)) &&
          !ok(mk_burst(0, 65496, 65535, 0)));
    CHECK(ok(mk_burst(0, 70000, 65515, 0, 0, 1)) && !ok(mk_burst(0, 70000, 65516, 0, 0, 1)));
    // frame_cap against the longest frame, also for the burst's shorter last frame
    CHECK(ok(mk_burst(0, 101, 100, 0), 1, 0, 154) && !ok(mk_burst(0, 101, 100, 0), 1, 0, 153) && !ok(mk_burst(0, 101, 100, 0), 0, 0, 153));
    CHECK(ok(mk_burst(0, 0, 0, 0), 0, 0, 54) && !ok(mk_burst(0, 0, 0, 0), 0, 0, 53) && ok(mk_burst(0, 0, 0, 0, 0, 5), 0, 0, 74));
    // the source range, without wrapping
    CHECK(ok(mk_burst(90, 10, 4, 0), 2, 0, 1u << 17, 1ull << 40, 100) && !ok(mk_burst(91, 10, 4, 0), 0, 0, 1u << 17, 1ull << 40, 100));
    CHECK(!ok(mk_burst(UINT64_MAX - 3, 10, 4, 0), 0, 0, 1u << 17, 1ull << 40, UINT64_MAX));
    CHECK(ok(mk_burst(UINT64_MAX - 10, 10, 4, 0), 2, 0, 1u << 17, 1ull << 40, UINT64_MAX) && s.data_off == UINT64_MAX - 2 && s.data_len == 2);
    CHECK(!ok(mk_burst(UINT64_MAX, 1, 1, 0), 0, 0, 1u << 17, 1ull << 40, UINT64_MAX - 1));
    // a single frame's destination: its siblings are built
    b = mk_burst(0, 300, 100, 0);
    CHECK(ok(b, 0, 1000 - 154, 154, 1000) && !ok(b, 1, 1000 - 153, 154, 1000) && ok(b, 2, 0, 154, 1000));
    CHECK(!ok(b, 1, UINT64_MAX - 20, 154, UINT64_MAX) && ok(b, 1, UINT64_MAX - 154, 154, UINT64_MAX) && !ok(b, 1, 1001, 154, 1000));
    // no bursts at all
    CHECK(!tcp_burst_frame(hs, 6, nullptr, 0, 0, 0, 1u << 17, 1ull << 40, 1ull << 40, &s));
}

// the count a sorted table's frame must get: bursts with first <= j
static uint32_t linear_count(const std::vector<vpcsum_tcpburst_t>& t, uint32_t j) {
    uint32_t c = 0;
    while (c < t.size() && t[c].first <= j) ++c;
    return c;
}

static void check_search_sorted() {
    for (uint32_t n : {0u, 1u, 2u, 7u, 8u, 9u, 10u, 63u, 64u, 65u, 80u, 81u, 82u, 513u, 729u, 730u, 4096u}) {
        for (int shape = 0; shape < 3; ++shape) {
            std::vector<vpcsum_tcpburst_t> t;
            uint32_t next = shape == 2 ? 3 : 0;   // shape 2: frames before the first burst
            for (uint32_t i = 0; i < n; ++i) {
                const uint32_t cnt = shape == 0 ? 1 : (uint32_t)(rnd() % 5);   // shape 1, 2: equal `first`s (count 0 steps) too
                t.push_back(mk_burst(0, 0, 0, next));
                next += cnt;
            }
            const auto p = heap(t);
            for (uint32_t j = 0; j < next + 3; ++j) CHECK(tcp_burst_find(p.get(), n, j) == linear_count(t, j));
            CHECK(tcp_burst_find(p.get(), n, UINT32_MAX) == n);
        }
    }
    // the steps: 4 for 4,096 bursts, 6 for 131,072
    const std::pair<uint32_t, int> sizes[] = {{4096u, 4}, {131072u, 6}, {1u << 28, 9}};
    for (const auto& [n, steps] : sizes) {
        for (uint32_t j : {0u, n / 3, n - 1}) {
            uint32_t lo = 0, hi = n;
            int k = 0;
            while (lo < hi) {   // first[b] = b, never stored: the bits from the pivots themselves
                uint32_t bits = 0;
                for (uint32_t i = 0; i < 8; ++i) {
                    const uint32_t pv = tcp_burst_pivot(lo, hi, i);
                    CHECK(pv >= lo && pv < hi);
                    if (pv <= j) bits |= 1u << i;
                }
                tcp_burst_narrow(lo, hi, bits);
                ++k;
            }
            CHECK(lo == j + 1 && k <= steps + 1);
        }
    }
}

// Random tables -- sorted, unsorted, overlapping, gappy, with bad records among them: whatever the
// search lands on, an accepted frame lies inside the destination and inside ITS burst's source range,
// and that burst names the frame.
static void check_random_tables() {
    const vpcsum_tcphdr_t hs[3] = {mk_hdr(4, 14), mk_hdr(6, 0), mk_hdr(7, 0)};
    uint32_t accepted = 0, refused = 0;
    for (int round = 0; round < 400; ++round) {
        const uint32_t n = (uint32_t)(rnd() % 70), n_frames = 1 + (uint32_t)(rnd() % 200);
        const uint64_t src_len = 1 + rnd() % 100000, dst_len = 1 + rnd() % 400000;
        const uint32_t frame_cap = 54 + (uint32_t)(rnd() % 1600);
        const int kind = round % 4;   // 0 sorted and tight, 1 gappy, 2 overlapping, 3 shuffled
        std::vector<vpcsum_tcpburst_t> t;
        uint32_t next = 0;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t mss = 1 + (uint32_t)(rnd() % 1500);
            const uint32_t d = (rnd() % 8 == 0) ? 0 : (uint32_t)(rnd() % (6 * mss));
            vpcsum_tcpburst_t b = mk_burst(rnd() % (src_len + 50), d, mss, next, (uint32_t)rnd(), (uint32_t)(rnd() % 4));
            if (rnd() % 16 == 0) b.count += 1;
            if (rnd() % 32 == 0) b.data_off = UINT64_MAX - rnd() % 64;
            if (rnd() % 32 == 0) b.flags = 0x58;
            t.push_back(b);
            next += kind == 1 ? b.count + (uint32_t)(rnd() % 3) : kind == 2 ? (uint32_t)(rnd() % (b.count + 1)) : b.count;
        }
        if (kind == 3)
            for (size_t i = t.size(); i > 1; --i) std::swap(t[i - 1], t[rnd() % i]);
        const auto p = heap(t);
        for (uint32_t j = 0; j < n_frames; ++j) {
            const uint64_t fo = rnd() % 8 == 0 ? UINT64_MAX - rnd() % 2000 : rnd() % (dst_len + 100);
            vpcsum_tcpseg_t s;
            uint32_t bi = UINT32_MAX;
            if (!tcp_burst_frame(hs, 3, p.get(), n, fo, j, frame_cap, dst_len, src_len, &s, &bi)) {
                ++refused;
                continue;
            }
            ++accepted;
            CHECK(bi < n);
            const vpcsum_tcpburst_t& b = t[bi];
            CHECK(j >= b.first && j - b.first < b.count && b.hdr < 2);
            const uint32_t L = (b.hdr == 0 ? 54u : 60u) + s.data_len;
            CHECK(s.frame_off == fo && fo <= dst_len && L <= dst_len - fo && L <= frame_cap);
            CHECK(b.data_off <= src_len && b.data_len <= src_len - b.data_off);
            CHECK(s.data_off >= b.data_off && s.data_off - b.data_off <= b.data_len && s.data_len <= b.data_len - (s.data_off - b.data_off));
            CHECK(s.data_off - b.data_off == (uint64_t)(j - b.first) * b.mss || b.data_len == 0);
            if (kind == 0) CHECK(bi + 1 == linear_count(t, j));
        }
    }
    CHECK(accepted > 2000 && refused > 2000);
}

static void check_span_and_rebase() {
    const uint64_t src_len = 1000;
    std::vector<vpcsum_tcpburst_t> t = {mk_burst(300, 100, 10, 0), mk_burst(950, 51, 10, 10),   // ends past the source: not staged
                                        mk_burst(120, 0, 10, 16), mk_burst(200, 50, 10, 17), mk_burst(UINT64_MAX - 4, 10, 10, 22),
                                        mk_burst(990, 10, 10, 23), mk_burst(1001, 0, 0, 24)};
    auto p = heap(t);
    TcpPayloadSpan sp;
    CHECK(tcp_burst_payload_span(p.get(), (uint32_t)t.size(), src_len, 800, &sp) && sp.lo == 200 && sp.len == 800);
    CHECK(!tcp_burst_payload_span(p.get(), (uint32_t)t.size(), src_len, 799, &sp) && sp.len == 800);
    CHECK(tcp_burst_payload_span(p.get(), 3, src_len, 100, &sp) && sp.lo == 300 && sp.len == 100);
    CHECK(tcp_burst_payload_span(p.get() + 1, 2, src_len, 0, &sp) && sp.len == 0);   // nothing to stage
    CHECK(tcp_burst_payload_span(p.get(), 0, src_len, 0, &sp) && sp.len == 0);
    tcp_burst_rebase_payloads(p.get(), (uint32_t)t.size(), src_len, 200);
    CHECK(p[0].data_off == 100 && p[1].data_off == UINT64_MAX && p[2].data_off == 0 && p[3].data_off == 0 && p[4].data_off == UINT64_MAX &&
          p[5].data_off == 790 && p[6].data_off == UINT64_MAX);
    for (size_t i = 0; i < t.size(); ++i) {
        t[i].data_off = p[i].data_off;
        CHECK(memcmp(&t[i], &p[i], 32) == 0);   // nothing but data_off changed
    }
    // against the staged span, the accepted bursts are the accepted bursts of the source
    const vpcsum_tcphdr_t h = mk_hdr(4, 14);
    vpcsum_tcpseg_t s;
    const bool want[7] = {true, false, true, true, false, true, false};
    for (uint32_t i = 0; i < 7; ++i)
        CHECK(tcp_burst_frame(&h, 1, p.get(), 7, 0, p[i].first, 1u << 17, 1u << 20, 800, &s) == want[i]);
}

int main() {
    check_layout();
    check_cut();
    check_refusals();
    check_search_sorted();
    check_random_tables();
    check_span_and_rebase();
    if (g_fail) {
        fprintf(stderr, "tcp_burst: %d checks failed\n", g_fail);
        return 1;
    }
    printf("tcp_burst ok\n");
    return 0;
}
