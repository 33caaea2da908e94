// icmp_rules_test.cpp -- the host-checkable rules of the ICMP replies (vproxy_amd/csrc/icmp_reply.h)
// in a stand-alone program under ASan / UBSan (tests/test_icmp_cpu.py builds and runs it; nothing of
// the library is linked).  The lengths M and L of the three kinds, q at its three cases (l3_len below,
// at and above l4_off + 64) and at l3_len == l4_off, every refusal at the value that is accepted and
// at the first that is not (offsets near 2^64 included: nothing wraps), the one type byte read only
// when nothing else refuses the record, and the header words with both sums against a byte-wise
// restatement of the field list of include/vpcsum.h with byte-wise RFC 1071 sums -- the all-zero echo
// (0xffff) and the echo whose words sum to 0xffff (0x0000) among them.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "icmp_reply.h"

using namespace vpcsum;

static int g_fail = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            if (++g_fail > 20) exit(1);                                          \
        }                                                                        \
    } while (0)

// Utils.calculateChecksum over bytes: big-endian words, end-around carry (an integer 0 stays 0),
// complemented
static uint32_t csum_bytes(const std::vector<uint8_t>& b) {
    uint64_t s = 0;
    for (size_t i = 0; i < b.size(); i += 2) s += ((uint32_t)b[i] << 8) | (i + 1 < b.size() ? b[i + 1] : 0u);
    while (s >> 16) s = (s & 0xffff) + (s >> 16);
    return (uint32_t)(0xffff - s);
}

static vpcsum_icmphdr_t mk_hdr(int ver, int l2) {
    vpcsum_icmphdr_t h;
    memset(&h, 0, sizeof(h));
    for (int i = 0; i < 6; ++i) h.eth_dst[i] = (uint8_t)(0xa0 + i), h.eth_src[i] = (uint8_t)(0xb0 + i);
    h.l2_len = (uint8_t)l2;
    h.l3_ver = (uint8_t)ver;
    h.tos = 0xb8;
    h.ttl = 64;
    for (int i = 0; i < 16; ++i) h.src[i] = (uint8_t)(0x11 + i), h.dst[i] = (uint8_t)(0x91 + 3 * i);
    h.ident[0] = 0x37; h.ident[1] = 0xbd;
    h.frag[0] = 0x40; h.frag[1] = 0x00;
    return h;
}

static vpcsum_desc_t mk_desc(uint64_t l3_off, uint32_t l3_len, uint32_t l4_off, int ver, int proto, int flags) {
    vpcsum_desc_t d;
    memset(&d, 0, sizeof(d));
    d.l3_off = l3_off;
    d.l3_len = (uint16_t)l3_len;
    d.l4_off = (uint16_t)l4_off;
    d.l3_ver = (uint8_t)ver;
    d.l4_proto = (uint8_t)proto;
    d.flags = (uint8_t)flags;
    return d;
}

static vpcsum_icmprp_t mk_rp(uint64_t frame_off, int kind, uint32_t hdr, uint32_t cap) {
    vpcsum_icmprp_t r;
    memset(&r, 0, sizeof(r));
    r.frame_off = frame_off;
    r.hdr = hdr;
    r.frame_cap = cap;
    r.kind = (uint8_t)kind;
    return r;
}

// the whole rule with a fixed type byte; counts the reads of it
static int g_type_reads = 0;
static bool plan(const vpcsum_desc_t& d, const vpcsum_icmprp_t& r, const vpcsum_icmphdr_t* hdrs, uint32_t n_hdr, uint64_t arena_len,
                 uint64_t dst_len, uint8_t type, IcmpReplyPlan* p) {
    return icmp_reply_plan(d, r, hdrs, n_hdr, arena_len, dst_len, [&](uint64_t) { ++g_type_reads; return type; }, p);
}

static void test_lengths_and_refusals() {
    const vpcsum_icmphdr_t hdrs[] = {mk_hdr(4, 14), mk_hdr(6, 0), mk_hdr(5, 14), mk_hdr(4, 13), mk_hdr(4, 14), mk_hdr(4, 14),
                                     mk_hdr(6, 14), mk_hdr(4, 14)};
    vpcsum_icmphdr_t hs[8];
    memcpy(hs, hdrs, sizeof(hs));
    hs[4].rsv[1] = 1;         // template rsv
    hs[5].ack[3] = 1;         // a TCP-only byte
    hs[6].window[0] = 1;
    hs[7].dport[1] = 1;       // ports must be 0 too
    const uint64_t big = 1ull << 40;
    const int F4 = VPCSUM_F_L4 | VPCSUM_F_IP, F6 = VPCSUM_F_L4;
    IcmpReplyPlan p;

    // echo: M = seg_len, L = l2 + (20 | 40) + M; IP options and extension headers are not carried over
    CHECK(plan(mk_desc(100, 20 + 64, 20, 4, 1, F4), mk_rp(0, VPCSUM_ICMP_ECHO_REPLY, 0, 1000), hs, 8, big, big, 8, &p) &&
          p.M == 64 && p.L == 14 + 20 + 64 && p.q == 0);
    CHECK(plan(mk_desc(100, 24 + 9, 24, 4, 1, F4), mk_rp(0, VPCSUM_ICMP_ECHO_REPLY, 0, 1000), hs, 8, big, big, 8, &p) &&
          p.M == 9 && p.L == 14 + 20 + 9);
    CHECK(plan(mk_desc(100, 48 + 8, 48, 6, 58, F6), mk_rp(0, VPCSUM_ICMP_ECHO_REPLY, 1, 1000), hs, 8, big, big, 128, &p) &&
          p.M == 8 && p.L == 40 + 8);
    CHECK(plan(mk_desc(100, 65535, 20, 4, 1, F4), mk_rp(0, VPCSUM_ICMP_ECHO_REPLY, 0, 70000), hs, 8, big, big, 8, &p) &&
          p.M == 65515 && p.L == 14 + 20 + 65515);
    // the errors: q = min(l3_len, l4_off + 64) -- l3_len below, at and above l4_off + 64, and a packet that is all header
    const struct { uint32_t l3_len, l4_off, q; int ver; uint32_t hdr; } qs[] = {
        {83, 20, 83, 4, 0}, {84, 20, 84, 4, 0}, {85, 20, 84, 4, 0}, {1500, 20, 84, 4, 0}, {20, 20, 20, 4, 0}, {60, 60, 60, 4, 0},
        {1500, 60, 124, 4, 0}, {1500, 24, 88, 4, 0}, {103, 40, 103, 6, 1}, {104, 40, 104, 6, 1}, {105, 40, 104, 6, 1},
        {40, 40, 40, 6, 1}, {1500, 48, 112, 6, 1}, {65535, 40, 104, 6, 1}};
    for (const auto& c : qs) {
        for (int kind : {VPCSUM_ICMP_PORT_UNREACH, VPCSUM_ICMP_TIME_EXCEEDED}) {
            CHECK(icmp_reply_quote_len(c.l3_len, c.l4_off) == c.q);
            const bool ok = plan(mk_desc(7, c.l3_len, c.l4_off, c.ver, 17, c.ver == 4 ? F4 : F6), mk_rp(0, kind, c.hdr, 1000), hs, 8, big, big, 0, &p);
            CHECK(ok && p.q == c.q && p.M == 8 + c.q && p.L == (c.ver == 4 ? 14 + 20 : 40) + 8 + c.q);
        }
    }

    const vpcsum_desc_t e4 = mk_desc(100, 84, 20, 4, 1, F4), e6 = mk_desc(100, 104, 40, 6, 58, F6), u4 = mk_desc(100, 84, 20, 4, 17, F4);
    auto echo4 = [&](const vpcsum_desc_t& d, vpcsum_icmprp_t r, uint8_t type = 8, uint64_t arena_len = 1ull << 40, uint64_t dst_len = 1ull << 40,
                     uint32_t n_hdr = 8) { return plan(d, r, hs, n_hdr, arena_len, dst_len, type, &p); };
    const vpcsum_icmprp_t r0 = mk_rp(0, VPCSUM_ICMP_ECHO_REPLY, 0, 1000);
    CHECK(echo4(e4, r0));
    // the record's own words
    CHECK(!echo4(e4, mk_rp(0, VPCSUM_ICMP_ECHO_REPLY, 8, 1000)) && !echo4(e4, mk_rp(0, VPCSUM_ICMP_ECHO_REPLY, 0xffffffffu, 1000)));
    CHECK(!echo4(e4, r0, 8, big, big, 0));
    CHECK(!echo4(e4, mk_rp(0, 0, 0, 1000)) && !echo4(e4, mk_rp(0, 4, 0, 1000)) && !echo4(e4, mk_rp(0, 255, 0, 1000)));
    for (int k = 0; k < 7; ++k) {
        vpcsum_icmprp_t r = r0;
        r.rsv[k] = 0x80;
        CHECK(!echo4(e4, r));
    }
    // the template, and its version against the descriptor's
    for (uint32_t h = 2; h < 8; ++h) CHECK(!echo4(e4, mk_rp(0, VPCSUM_ICMP_ECHO_REPLY, h, 1000)));
    CHECK(!echo4(e4, mk_rp(0, VPCSUM_ICMP_ECHO_REPLY, 1, 1000)) && !echo4(e6, r0, 128));
    CHECK(echo4(e6, mk_rp(0, VPCSUM_ICMP_ECHO_REPLY, 1, 1000), 128));
    // the descriptor
    CHECK(!echo4(mk_desc(100, 84, 20, 5, 1, F4), r0));
    for (int fl : {VPCSUM_F_L4P, VPCSUM_F_RAW, VPCSUM_F_PRE})
        for (int kind = 1; kind <= 3; ++kind) CHECK(!echo4(mk_desc(100, 84, 20, 4, kind == 1 ? 1 : 17, F4 | fl), mk_rp(0, kind, 0, 1000)));
    CHECK(!echo4(mk_desc(100, 104, 40, 6, 58, F6 | VPCSUM_F_IP), mk_rp(0, VPCSUM_ICMP_ECHO_REPLY, 1, 1000), 128));
    CHECK(!echo4(mk_desc(100, 84, 88, 4, 17, F4), mk_rp(0, VPCSUM_ICMP_TIME_EXCEEDED, 0, 1000)));          // l4_off > l3_len
    CHECK(!echo4(mk_desc(100, 84, 16, 4, 17, F4), mk_rp(0, VPCSUM_ICMP_TIME_EXCEEDED, 0, 1000)));
    CHECK(!echo4(mk_desc(100, 84, 22, 4, 17, F4), mk_rp(0, VPCSUM_ICMP_TIME_EXCEEDED, 0, 1000)));
    CHECK(!echo4(mk_desc(100, 84, 39, 6, 17, F6), mk_rp(0, VPCSUM_ICMP_TIME_EXCEEDED, 1, 1000)));
    CHECK(echo4(e4, r0, 8, 184) && !echo4(e4, r0, 8, 183));                                              // the arena's end
    CHECK(!echo4(mk_desc(UINT64_MAX - 8, 84, 20, 4, 1, F4), r0, 8, 184) && !echo4(mk_desc(UINT64_MAX, 84, 20, 4, 1, F4), r0));
    // the destination: the chunk's room, the arena's end, no wrap
    CHECK(echo4(e4, mk_rp(0, VPCSUM_ICMP_ECHO_REPLY, 0, 98)) && !echo4(e4, mk_rp(0, VPCSUM_ICMP_ECHO_REPLY, 0, 97)));
    CHECK(echo4(e4, mk_rp(902, VPCSUM_ICMP_ECHO_REPLY, 0, 1000), 8, big, 1000) && !echo4(e4, mk_rp(903, VPCSUM_ICMP_ECHO_REPLY, 0, 1000), 8, big, 1000));
    CHECK(!echo4(e4, mk_rp(UINT64_MAX, VPCSUM_ICMP_ECHO_REPLY, 0, 1000), 8, big, 1000) &&
          !echo4(e4, mk_rp(UINT64_MAX - 97, VPCSUM_ICMP_ECHO_REPLY, 0, 1000), 8, big, UINT64_MAX));
    CHECK(echo4(e4, mk_rp(UINT64_MAX - 98, VPCSUM_ICMP_ECHO_REPLY, 0, 1000), 8, big, UINT64_MAX));
    // echo's own
    CHECK(!echo4(mk_desc(100, 84, 20, 4, 1, VPCSUM_F_IP), r0));                                          // no F_L4
    CHECK(!echo4(mk_desc(100, 84, 20, 4, 58, F4), r0, 128) && !echo4(mk_desc(100, 104, 40, 6, 1, F6), mk_rp(0, 1, 1, 1000), 8));
    CHECK(!echo4(mk_desc(100, 84, 20, 4, 17, F4), r0));
    CHECK(echo4(mk_desc(100, 28, 20, 4, 1, F4), r0) && !echo4(mk_desc(100, 27, 20, 4, 1, F4), r0));      // seg_len 8 / 7
    CHECK(!echo4(e4, r0, 0) && !echo4(e4, r0, 128) && !echo4(e6, mk_rp(0, 1, 1, 1000), 8) && !echo4(e6, mk_rp(0, 1, 1, 1000), 129));
    // port unreachable: UDP only
    CHECK(echo4(u4, mk_rp(0, VPCSUM_ICMP_PORT_UNREACH, 0, 1000)) && !echo4(e4, mk_rp(0, VPCSUM_ICMP_PORT_UNREACH, 0, 1000)) &&
          !echo4(mk_desc(100, 84, 20, 4, 6, F4), mk_rp(0, VPCSUM_ICMP_PORT_UNREACH, 0, 1000)));
    // time exceeded: any packet, any flags but the three; NS / NA refused
    CHECK(echo4(mk_desc(100, 84, 20, 4, 6, 0), mk_rp(0, VPCSUM_ICMP_TIME_EXCEEDED, 0, 1000)) &&
          echo4(mk_desc(100, 84, 20, 4, 99, F4), mk_rp(0, VPCSUM_ICMP_TIME_EXCEEDED, 0, 1000)));
    const vpcsum_icmprp_t t6 = mk_rp(0, VPCSUM_ICMP_TIME_EXCEEDED, 1, 1000);
    CHECK(echo4(e6, t6, 128) && !echo4(e6, t6, 135) && !echo4(e6, t6, 136) && echo4(e6, t6, 134) && echo4(e6, t6, 137));
    CHECK(echo4(mk_desc(100, 104, 40, 6, 17, F6), t6, 135));                                             // not ICMPv6: the byte is a port's
    CHECK(echo4(mk_desc(100, 84, 20, 4, 1, F4), mk_rp(0, VPCSUM_ICMP_TIME_EXCEEDED, 0, 1000), 135));     // ICMPv4 has no NDP
    CHECK(!echo4(mk_desc(100, 41, 40, 6, 58, 0), t6, 135));
    // the type byte: read once for an accepted echo, never for a record something else refuses, never
    // for an error that does not ask, never for an empty ICMPv6 segment
    g_type_reads = 0;
    CHECK(echo4(e4, r0) && g_type_reads == 1);
    CHECK(!echo4(e4, mk_rp(0, VPCSUM_ICMP_ECHO_REPLY, 0, 97)) && !echo4(e4, r0, 8, 183) && !echo4(e4, mk_rp(0, 1, 9, 1000)) && g_type_reads == 1);
    CHECK(echo4(u4, mk_rp(0, VPCSUM_ICMP_PORT_UNREACH, 0, 1000)) && echo4(u4, mk_rp(0, VPCSUM_ICMP_TIME_EXCEEDED, 0, 1000)) && g_type_reads == 1);
    CHECK(echo4(mk_desc(100, 40, 40, 6, 58, 0), t6, 135) && g_type_reads == 1);
    CHECK(echo4(e6, t6, 1) && g_type_reads == 2);
}

// the reply's bytes from the field list, byte by byte: `body` is what follows type | code | sum
static std::vector<uint8_t> want_frame(const vpcsum_icmphdr_t& h, int kind, const std::vector<uint8_t>& body, uint32_t* ipc, uint32_t* l4c) {
    const bool v4 = h.l3_ver == 4;
    const uint32_t M = 4 + (uint32_t)body.size();
    static const uint8_t tc[3][2][2] = {{{129, 0}, {0, 0}}, {{1, 4}, {3, 3}}, {{3, 0}, {11, 0}}};
    std::vector<uint8_t> eth, ip, ph, msg = {tc[kind - 1][v4][0], tc[kind - 1][v4][1], 0, 0};
    msg.insert(msg.end(), body.begin(), body.end());
    if (h.l2_len == 14) {
        eth.insert(eth.end(), h.eth_dst, h.eth_dst + 6);
        eth.insert(eth.end(), h.eth_src, h.eth_src + 6);
        eth.push_back(v4 ? 0x08 : 0x86);
        eth.push_back(v4 ? 0x00 : 0xdd);
    }
    if (v4) {
        const uint32_t tl = 20 + M;
        ip = {0x45, h.tos, (uint8_t)(tl >> 8), (uint8_t)tl, h.ident[0], h.ident[1], h.frag[0], h.frag[1], h.ttl, 1, 0, 0};
        ip.insert(ip.end(), h.src, h.src + 4);
        ip.insert(ip.end(), h.dst, h.dst + 4);
        *ipc = csum_bytes(ip);
        ip[10] = (uint8_t)(*ipc >> 8);
        ip[11] = (uint8_t)*ipc;
    } else {
        ip = {(uint8_t)(0x60 | (h.tos >> 4)), (uint8_t)(h.tos << 4), 0, 0, (uint8_t)(M >> 8), (uint8_t)M, 58, h.ttl};
        ip.insert(ip.end(), h.src, h.src + 16);
        ip.insert(ip.end(), h.dst, h.dst + 16);
        *ipc = 0;
        ph.insert(ph.end(), h.src, h.src + 16);
        ph.insert(ph.end(), h.dst, h.dst + 16);
        ph.push_back((uint8_t)(M >> 24)); ph.push_back((uint8_t)(M >> 16)); ph.push_back((uint8_t)(M >> 8)); ph.push_back((uint8_t)M);
        ph.push_back(0); ph.push_back(0); ph.push_back(0); ph.push_back(58);
    }
    std::vector<uint8_t> all = ph;
    all.insert(all.end(), msg.begin(), msg.end());
    *l4c = csum_bytes(all);
    msg[2] = (uint8_t)(*l4c >> 8);
    msg[3] = (uint8_t)*l4c;
    std::vector<uint8_t> f = eth;
    f.insert(f.end(), ip.begin(), ip.end());
    f.insert(f.end(), msg.begin(), msg.end());
    return f;
}

// the kernel's arithmetic on the host: the body's folded little-endian sum, then the words
static std::vector<uint8_t> got_header(const vpcsum_icmphdr_t& h, int kind, const std::vector<uint8_t>& body, uint32_t* ipc, uint32_t* l4c) {
    uint32_t t[16];
    tcp_build_template_words(h, t);
    CHECK(icmp_reply_hdr_ok(t));
    const bool v4 = tb_l3_ver(t) == 4;
    const uint32_t M = 4 + (uint32_t)body.size();
    uint64_t s = 0;   // bytes 4.. of the message start on an even byte of it
    for (size_t i = 0; i < body.size(); ++i) s += (uint64_t)body[i] << (8 * (i & 1));
    IcmpReplyWords w;
    icmp_reply_words(t, (uint32_t)kind, M, w);
    const uint32_t ip_field = v4 ? 0xffffu - tb_fold64(icmp_reply_ip_header_sum(w)) : 0u;
    const uint32_t l4_field = icmp_reply_l4_field(tb_fold64(icmp_reply_l4_header_sum(t, w, M) + tb_fold64(s)));
    icmp_reply_set_sums(w, v4, ip_field, l4_field);
    *ipc = tb_bswap16(ip_field);
    *l4c = tb_bswap16(l4_field);
    uint8_t out[kIcmpReplyMaxHeader];
    const uint32_t n = icmp_reply_header_bytes(w, t, out);
    CHECK(n == tb_header_len(t, kIcmpHeader) && n + M - kIcmpHeader == icmp_reply_frame_len(t, M));
    return std::vector<uint8_t>(out, out + n);
}

static void test_words() {
    uint32_t x = 12345;
    auto rnd = [&]() { x = x * 1664525u + 1013904223u; return (uint8_t)(x >> 24); };
    for (int ver : {4, 6})
        for (int l2 : {0, 14})
            for (int kind = 1; kind <= 3; ++kind)
                for (uint32_t blen : {4u, 5u, 7u, 24u, 61u, 128u, 1468u}) {
                    const vpcsum_icmphdr_t h = mk_hdr(ver, l2);
                    std::vector<uint8_t> body(blen);
                    for (auto& b : body) b = rnd();
                    if (kind != VPCSUM_ICMP_ECHO_REPLY) body[0] = body[1] = body[2] = body[3] = 0;   // the unused dword
                    uint32_t wi, wl, gi, gl;
                    const std::vector<uint8_t> want = want_frame(h, kind, body, &wi, &wl);
                    const std::vector<uint8_t> got = got_header(h, kind, body, &gi, &gl);
                    CHECK(wi == gi && wl == gl);
                    // an echo's bytes 4..7 are the request's: the words leave them 0
                    const size_t cmp = got.size() - (kind == VPCSUM_ICMP_ECHO_REPLY ? 4 : 0);
                    CHECK(got.size() <= want.size() && memcmp(got.data(), want.data(), cmp) == 0);
                }
    // the all-zero IPv4 echo stores 0xffff; bytes 4..7 = ff ff 00 00 (the words sum to 0xffff) store 0x0000
    vpcsum_icmphdr_t h = mk_hdr(4, 14);
    uint32_t wi, wl, gi, gl;
    std::vector<uint8_t> z(60, 0);
    want_frame(h, VPCSUM_ICMP_ECHO_REPLY, z, &wi, &wl);
    got_header(h, VPCSUM_ICMP_ECHO_REPLY, z, &gi, &gl);
    CHECK(wl == 0xffff && gl == 0xffff);
    z[0] = z[1] = 0xff;
    want_frame(h, VPCSUM_ICMP_ECHO_REPLY, z, &wi, &wl);
    got_header(h, VPCSUM_ICMP_ECHO_REPLY, z, &gi, &gl);
    CHECK(wl == 0 && gl == 0);
}

int main() {
    test_lengths_and_refusals();
    test_words();
    if (g_fail) {
        fprintf(stderr, "%d checks failed\n", g_fail);
        return 1;
    }
    printf("icmp_rules ok\n");
    return 0;
}
