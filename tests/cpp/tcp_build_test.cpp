// tcp_build_test.cpp -- the host-checkable rules of the TCP segment build (vproxy_amd/csrc/tcp_build.h:
// refusals, L, the header words the kernel stores) in a stand-alone program under ASan / UBSan
// (tests/test_tcp_build_cpu.py builds and runs it; nothing of the library is linked).
//
// argv: <frame hex> <seq> <flags> -- a reference Ethernet / IPv4 / TCP frame without options and the
// two record fields that are not in a template; the template is read out of the frame's own
// header bytes here, the header rebuilt from it and compared byte for byte, sums included (the
// payload's share of the TCP sum is added from the frame's bytes).  The frame comes from the test's
// fixture file: no reference bytes are written in this source.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <vector>

#include "tcp_build.h"

using namespace vpcsum;

static int g_fail = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            if (++g_fail > 20) exit(1);                                          \
        }                                                                        \
    } while (0)

static vpcsum_tcphdr_t mk_hdr(int ver, int l2) {
    vpcsum_tcphdr_t h;
    memset(&h, 0, sizeof(h));
    for (int i = 0; i < 6; ++i) { h.eth_dst[i] = (uint8_t)(0xa0 + i); h.eth_src[i] = (uint8_t)(0xb0 + i); }
    h.l2_len = (uint8_t)l2;
    h.l3_ver = (uint8_t)ver;
    h.tos = 0x5c;
    h.ttl = 64;
    for (int i = 0; i < 16; ++i) { h.src[i] = (uint8_t)(0x10 + i); h.dst[i] = (uint8_t)(0x30 + i); }
    h.sport[0] = 0x12; h.sport[1] = 0x34; h.dport[0] = 0x00; h.dport[1] = 0x50;
    h.ack[0] = 0xde; h.ack[1] = 0xad; h.ack[2] = 0xbe; h.ack[3] = 0xef;
    h.window[0] = 0x7f; h.window[1] = 0xff;
    h.ident[0] = 0xab; h.ident[1] = 0xcd; h.frag[0] = 0x40; h.frag[1] = 0x00;
    return h;
}

// The header as the kernel writes it, payload-less sums included, at its exact size
static std::vector<uint8_t> header_of(const vpcsum_tcphdr_t& h, uint32_t seq, uint32_t data_len, uint32_t flags,
                                      uint64_t payload_sum_le = 0) {
    uint32_t t[16];
    tcp_build_template_words(h, t);
    TcpBuildWords w;
    tcp_build_words(t, seq, data_len, flags, w);
    const bool v4 = tb_l3_ver(t) == 4;
    const uint32_t ipf = v4 ? 0xffffu - tb_fold64(tcp_build_ip_header_sum(w)) : 0u;
    const uint32_t l4f = 0xffffu - tb_fold64(tcp_build_l4_header_sum(t, w, data_len) + payload_sum_le);
    tcp_build_set_sums(w, v4, ipf, l4f);
    std::unique_ptr<uint8_t[]> buf(new uint8_t[tcp_build_header_len(t)]);   // exact size: an overrun is an error
    const uint32_t n = tcp_build_header_bytes(w, t, buf.get());
    CHECK(n == tcp_build_header_len(t));
    return std::vector<uint8_t>(buf.get(), buf.get() + n);
}

static uint32_t be16(const uint8_t* p) { return ((uint32_t)p[0] << 8) | p[1]; }

// RFC 1071 over bytes, big-endian words, folded: the plain reading the words' sums must equal
static uint32_t csum_be(const std::vector<uint8_t>& b) {
    uint64_t s = 0;
    for (size_t i = 0; i + 1 < b.size(); i += 2) s += be16(&b[i]);
    if (b.size() & 1) s += (uint32_t)b.back() << 8;
    while (s >> 16) s = (s & 0xffff) + (s >> 16);
    return 0xffffu - (uint32_t)s;
}

static void check_layout(int ver, int l2) {
    const vpcsum_tcphdr_t h = mk_hdr(ver, l2);
    uint32_t t[16];
    tcp_build_template_words(h, t);
    CHECK(tcp_build_hdr_ok(t));
    const uint32_t iplen = ver == 4 ? 20 : 40, H = (uint32_t)l2 + iplen + 20;
    CHECK(tcp_build_header_len(t) == H && H <= kTcpBuildMaxHeader);
    CHECK(tcp_build_frame_len(t, 0) == H && tcp_build_frame_len(t, 1460) == H + 1460);
    const uint32_t seq = 0x01020304u, d = 517, flags = 0x18;
    const std::vector<uint8_t> b = header_of(h, seq, d, flags);
    CHECK(b.size() == H);
    const uint8_t* ip = b.data() + l2;
    if (l2) {
        CHECK(memcmp(b.data(), h.eth_dst, 6) == 0 && memcmp(b.data() + 6, h.eth_src, 6) == 0);
        CHECK(be16(b.data() + 12) == (ver == 4 ? 0x0800u : 0x86ddu));
    }
    if (ver == 4) {
        CHECK(ip[0] == 0x45 && ip[1] == h.tos && be16(ip + 2) == 40 + d);
        CHECK(memcmp(ip + 4, h.ident, 2) == 0 && memcmp(ip + 6, h.frag, 2) == 0 && ip[8] == h.ttl && ip[9] == 6);
        CHECK(memcmp(ip + 12, h.src, 4) == 0 && memcmp(ip + 16, h.dst, 4) == 0);
        std::vector<uint8_t> z(ip, ip + 20);
        z[10] = z[11] = 0;
        CHECK(be16(ip + 10) == csum_be(z));
    } else {
        CHECK(ip[0] == (0x60 | (h.tos >> 4)) && ip[1] == (uint8_t)(h.tos << 4) && ip[2] == 0 && ip[3] == 0);
        CHECK(be16(ip + 4) == 20 + d && ip[6] == 6 && ip[7] == h.ttl);
        CHECK(memcmp(ip + 8, h.src, 16) == 0 && memcmp(ip + 24, h.dst, 16) == 0);
    }
    const uint8_t* tcp = ip + iplen;
    CHECK(memcmp(tcp, h.sport, 2) == 0 && memcmp(tcp + 2, h.dport, 2) == 0);
    CHECK(tcp[4] == 1 && tcp[5] == 2 && tcp[6] == 3 && tcp[7] == 4 && memcmp(tcp + 8, h.ack, 4) == 0);
    CHECK(tcp[12] == 0x50 && tcp[13] == flags && memcmp(tcp + 14, h.window, 2) == 0 && tcp[18] == 0 && tcp[19] == 0);
    // the TCP field of a segment whose payload sums to 0: pseudo-header ‖ header, by the plain reading
    std::vector<uint8_t> ps;
    if (ver == 4) { ps.insert(ps.end(), h.src, h.src + 4); ps.insert(ps.end(), h.dst, h.dst + 4); }
    else { ps.insert(ps.end(), h.src, h.src + 16); ps.insert(ps.end(), h.dst, h.dst + 16); }
    ps.push_back(0); ps.push_back(6); ps.push_back((uint8_t)((20 + d) >> 8)); ps.push_back((uint8_t)(20 + d));
    ps.insert(ps.end(), tcp, tcp + 16); ps.push_back(0); ps.push_back(0); ps.push_back(0); ps.push_back(0);
    CHECK(be16(tcp + 16) == csum_be(ps));
}

struct Rec {
    uint64_t frame_off, data_off;
    uint32_t frame_cap, data_len;
};

static bool fits(const vpcsum_tcphdr_t& h, const Rec& r, uint64_t dst_len, uint64_t src_len) {
    uint32_t t[16];
    tcp_build_template_words(h, t);
    return tcp_build_hdr_ok(t) && tcp_build_fits(t, r.frame_off, r.data_off, r.frame_cap, r.data_len, dst_len, src_len);
}

static void check_refusals() {
    // the record's own words
    CHECK(tcp_build_seg_ok(2, 3, 0x3f, 0) && !tcp_build_seg_ok(3, 3, 0x18, 0) && !tcp_build_seg_ok(0, 0, 0x18, 0));
    CHECK(!tcp_build_seg_ok(0, 1, 0x40, 0) && !tcp_build_seg_ok(0, 1, 0x80, 0) && !tcp_build_seg_ok(0, 1, 0x18, 1));
    CHECK(tcp_build_seg_ok(0xfffffffeu, 0xffffffffu, 0, 0) && !tcp_build_seg_ok(0xffffffffu, 0xffffffffu, 0, 0));
    // the template
    for (int ver = 0; ver < 256; ++ver)
        for (int l2 : {0, 1, 13, 14, 15, 18, 255}) {
            vpcsum_tcphdr_t h = mk_hdr(ver, l2);
            uint32_t t[16];
            tcp_build_template_words(h, t);
            CHECK(tcp_build_hdr_ok(t) == ((ver == 4 || ver == 6) && (l2 == 0 || l2 == 14)));
        }
    for (int k = 0; k < 2; ++k) {
        vpcsum_tcphdr_t h = mk_hdr(4, 14);
        h.rsv[k] = 1;
        uint32_t t[16];
        tcp_build_template_words(h, t);
        CHECK(!tcp_build_hdr_ok(t));
    }
    const vpcsum_tcphdr_t v4 = mk_hdr(4, 14), v6 = mk_hdr(6, 0), v4n = mk_hdr(4, 0), v6e = mk_hdr(6, 14);
    const uint64_t big = 1ull << 40;
    // the room at frame_off
    CHECK(fits(v4, {0, 0, 54 + 100, 100}, big, big) && !fits(v4, {0, 0, 54 + 99, 100}, big, big));
    CHECK(fits(v6, {0, 0, 60, 0}, big, big) && !fits(v6, {0, 0, 59, 0}, big, big));
    CHECK(fits(v6e, {0, 0, 74, 0}, big, big) && !fits(v6e, {0, 0, 73, 0}, big, big));
    // the length fields
    CHECK(fits(v4, {0, 0, 1u << 20, 65495}, big, big) && !fits(v4, {0, 0, 1u << 20, 65496}, big, big));
    CHECK(fits(v4n, {0, 0, 1u << 20, 65495}, big, big) && !fits(v4n, {0, 0, 1u << 20, 65535}, big, big));
    CHECK(fits(v6, {0, 0, 1u << 20, 65515}, big, big) && !fits(v6, {0, 0, 1u << 20, 65516}, big, big));
    // the destination: a frame ending exactly at dst_len, one byte past it, starting past it
    CHECK(fits(v4, {1000 - 154, 0, 154, 100}, 1000, big) && !fits(v4, {1000 - 153, 0, 154, 100}, 1000, big));
    CHECK(!fits(v4, {1001, 0, 154, 100}, 1000, big) && !fits(v4, {0, 0, 154, 100}, 153, big));
    CHECK(fits(v4, {0, 0, 54, 0}, 54, 0) && !fits(v4, {0, 0, 54, 0}, 53, 0));
    // the source: a payload ending exactly at src_len, one past it, starting past it; an empty payload at the end
    CHECK(fits(v4, {0, 900, 154, 100}, big, 1000) && !fits(v4, {0, 901, 154, 100}, big, 1000));
    CHECK(fits(v4, {0, 1000, 54, 0}, big, 1000) && !fits(v4, {0, 1001, 54, 0}, big, 1000));
    // offsets near 2^64: the sums would wrap to small numbers
    const uint64_t top = ~0ull;
    CHECK(!fits(v4, {top, 0, 154, 100}, big, big) && !fits(v4, {top - 153, 0, 154, 100}, big, big));
    CHECK(!fits(v4, {top - 100, 0, 154, 100}, top, big));            // frame_off + L wraps past dst_len = 2^64 - 1
    CHECK(fits(v4, {top - 154, 0, 154, 100}, top, big));             // ends exactly at dst_len
    CHECK(!fits(v4, {0, top, 154, 100}, big, big) && !fits(v4, {0, top - 50, 154, 100}, big, top));
    CHECK(fits(v4, {0, top - 100, 154, 100}, big, top) && !fits(v4, {0, top - 99, 154, 100}, big, top));
    CHECK(!fits(v4, {0, top, 54, 0}, big, top - 1) && fits(v4, {0, top, 54, 0}, big, top));
}

// The payload span of a staged source and the records rebased to it, over an exact-size copy of the
// records; `want`: the data_off each record must have afterwards.
struct Pay {
    uint64_t data_off;
    uint16_t data_len;
};
static void span_is(const std::vector<Pay>& recs, uint64_t src_len, uint64_t capacity, bool fits, uint64_t lo, uint64_t len,
                    const std::vector<uint64_t>& want) {
    std::unique_ptr<vpcsum_tcpseg_t[]> seg(new vpcsum_tcpseg_t[recs.size()]);
    for (size_t i = 0; i < recs.size(); ++i) {
        memset(&seg[i], 0, sizeof(seg[i]));
        seg[i].frame_off = 1000 * i;
        seg[i].seq = 7;
        seg[i].data_off = recs[i].data_off;
        seg[i].data_len = recs[i].data_len;
    }
    TcpPayloadSpan sp = {99, 99};
    CHECK(tcp_build_payload_span(seg.get(), (uint32_t)recs.size(), src_len, capacity, &sp) == fits);
    CHECK(sp.lo == lo && sp.len == len);
    tcp_build_rebase_payloads(seg.get(), (uint32_t)recs.size(), src_len, sp.lo);
    for (size_t i = 0; i < recs.size(); ++i) {
        CHECK(seg[i].data_off == want[i]);
        CHECK(seg[i].data_len == recs[i].data_len && seg[i].frame_off == 1000 * i && seg[i].seq == 7);   // nothing else moves
    }
}

static void check_payload_span() {
    const uint64_t top = ~0ull, big = 1ull << 40, out = UINT64_MAX;
    span_is({}, 1000, big, true, 0, 0, {});
    span_is({{300, 50}}, 1000, big, true, 300, 50, {0});                        // a single record
    span_is({{300, 0}}, 1000, big, true, 0, 0, {0});                            // data_len == 0: reads nothing
    span_is({{1000, 0}}, 1000, big, true, 0, 0, {0});                           // data_off == src_len, empty: accepted
    span_is({{1000, 1}}, 1000, big, true, 0, 0, {out});                         // data_off == src_len, one byte: outside
    span_is({{1001, 0}}, 1000, big, true, 0, 0, {out});                         // data_off > src_len: outside even when empty
    span_is({{990, 11}}, 1000, big, true, 0, 0, {out});                         // one byte past the end
    span_is({{990, 10}}, 1000, big, true, 990, 10, {0});                        // ends exactly at src_len
    // data_off + data_len wraps past 2^64 to a small number: refused, and no part of the span
    span_is({{top - 4, 10}, {100, 20}}, 1000, big, true, 100, 20, {out, 0});
    span_is({{top, 1}}, top, big, true, 0, 0, {out});
    span_is({{top - 4, 10}, {top - 4, 4}}, top, big, true, top - 4, 4, {out, 0});   // inside the source, 10 > the 4 bytes left
    span_is({{top - 10, 10}}, top, big, true, top - 10, 10, {0});               // ends exactly at src_len = 2^64 - 1
    // several: the span is over the accepted, non-empty ones; empty and refused ones do not widen it
    span_is({{500, 100}, {5, 0}, {200, 50}, {2000, 8}, {950, 50}, {999, 2}}, 1000, big, true, 200, 800,
            {300, 0, 0, out, 750, out});
    span_is({{2000, 8}, {1000, 1}, {top, 65535}}, 1000, big, true, 0, 0, {out, out, out});   // all refused: span 0
    span_is({{2000, 8}}, 1000, 0, true, 0, 0, {out});                           // span 0 fits a capacity of 0
    // the staging's room: exactly at capacity, one byte over (the span is still reported)
    span_is({{100, 60}, {300, 100}}, 1000, 300, true, 100, 300, {0, 200});
    span_is({{100, 60}, {300, 100}}, 1000, 299, false, 100, 300, {0, 200});
    span_is({{0, 1}}, 1, 1, true, 0, 1, {0});
    span_is({{0, 1}}, 1, 0, false, 0, 1, {0});
}

static std::vector<uint8_t> unhex(const char* s) {
    std::vector<uint8_t> b;
    const size_t n = strlen(s);
    for (size_t i = 0; i + 1 < n; i += 2) {
        unsigned v = 0;
        if (sscanf(s + i, "%2x", &v) != 1) { fprintf(stderr, "bad hex\n"); exit(2); }
        b.push_back((uint8_t)v);
    }
    return b;
}

// The reference frame: its template read out of its own header, rebuilt, compared
static void check_reference(const char* hex, uint32_t seq, uint32_t flags) {
    const std::vector<uint8_t> f = unhex(hex);
    CHECK(f.size() > 54 && f[12] == 0x08 && f[13] == 0x00 && f[14] == 0x45 && f[23] == 6 && f[46] == 0x50);
    vpcsum_tcphdr_t h;
    memset(&h, 0, sizeof(h));
    memcpy(h.eth_dst, &f[0], 6);
    memcpy(h.eth_src, &f[6], 6);
    h.l2_len = 14;
    h.l3_ver = 4;
    h.tos = f[15];
    h.ttl = f[22];
    memcpy(h.ident, &f[18], 2);
    memcpy(h.frag, &f[20], 2);
    memcpy(h.src, &f[26], 4);
    memcpy(h.dst, &f[30], 4);
    memcpy(h.sport, &f[34], 2);
    memcpy(h.dport, &f[36], 2);
    memcpy(h.ack, &f[42], 4);
    memcpy(h.window, &f[48], 2);
    const uint32_t total = be16(&f[16]), d = total - 40;
    CHECK(14 + total == f.size());
    // the payload's sum in the words' domain: little-endian 16-bit words from the payload's first byte
    uint64_t ps = 0;
    for (uint32_t i = 0; i < d; ++i) ps += (uint64_t)f[54 + i] << (8 * (i & 1));
    const std::vector<uint8_t> b = header_of(h, seq, d, flags, ps);
    CHECK(b.size() == 54);
    for (size_t i = 0; i < b.size() && i < f.size(); ++i)
        if (b[i] != f[i]) {
            fprintf(stderr, "reference frame: header byte %zu: built %02x, frame %02x\n", i, b[i], f[i]);
            ++g_fail;
        }
    uint32_t t[16];
    tcp_build_template_words(h, t);
    CHECK(tcp_build_frame_len(t, d) == f.size());
    printf("reference header %zu bytes, ip sum %04x, tcp sum %04x\n", b.size(), be16(&b[24]), be16(&b[50]));
}

int main(int argc, char** argv) {
    static_assert(sizeof(vpcsum_tcphdr_t) == 64 && sizeof(vpcsum_tcpseg_t) == 32, "layouts");
    for (int ver : {4, 6})
        for (int l2 : {0, 14}) check_layout(ver, l2);
    check_refusals();
    check_payload_span();
    if (argc == 4) check_reference(argv[1], (uint32_t)strtoul(argv[2], nullptr, 0), (uint32_t)strtoul(argv[3], nullptr, 0));
    if (g_fail) return 1;
    printf("tcp_build ok%s\n", argc == 4 ? " (with the reference frame)" : "");
    return 0;
}
